/*
 * streamparse.h -- the field-order logic of the reference-side binding (integration/gpucommon.h), free of Mitsuba's headers:
 * it takes the bytes `InstanceManager::serialize` produced for a BSDF, a delta / environment / sky luminaire or a sphere and fills
 * the parameter blocks of include/mtsgpu.h.  gpucommon.h produces the bytes (MemoryStream) and calls in here; the CPU tests
 * (tests/test_stream_parsers.py) produce them with an independent writer that follows each class's serialize() and compare
 * the blocks with what the library's own flattener builds for the same scene description, bit for bit.
 *
 * Wire format (src/libcore/serialization.cpp:72-85, src/libcore/stream.cpp): host byte order; an object reference is a uint32
 * id -- 0 for NULL, a known id for an object written before, otherwise a new id followed by the NUL-terminated class name
 * (stream.cpp:214-216, :391-402) and the object's serialize().  Float is `FloatT` (float with SINGLE_PRECISION).  A Spectrum is
 * SPECTRUM_SAMPLES = 3 Floats (spectrum.h:144-146, :438-440), a Point / Vector 3 Floats (point.h:264-268), a Matrix4x4 16 Floats
 * row major (matrix.h:74-76, :387-389), a Transform its matrix and its inverse (transform.h:40-43, :304-307), a BSphere centre +
 * radius (bsphere.h:40-43, :121-124), a bool one byte (stream.h:192, :279).
 */
#ifndef MTSGPU_STREAMPARSE_H
#define MTSGPU_STREAMPARSE_H

#include <mtsgpu.h>
#include <mtsgpu_mask.h>
#include <mtsgpu_snow.h>
#include <mtsgpu_cloth.h>
#include <mtsgpu_cylinder.h>
#include <mtsgpu_spot.h>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>
#include <stdint.h>

namespace mtsgpu_stream {

template <typename FloatT> struct Matrix44 { FloatT m[4][4]; };
template <typename FloatT> struct Xform { Matrix44<FloatT> fwd, inv; };      /* Transform: m_transform, m_invTransform */

/* A cursor over the bytes of a MemoryStream.  Reading past the end or an unexpected field sets `error` (first one wins) and
 * makes every later read return zeros; callers check ok() once at the end, as SLog(EError) would have thrown. */
template <typename FloatT> class ByteReader {
public:
	ByteReader(const uint8_t *data, size_t size) : m_data(data), m_size(size), m_pos(0) { }
	bool ok() const { return m_error.empty(); }
	const std::string &error() const { return m_error; }
	void fail(const std::string &what) { if (m_error.empty()) m_error = what; }
	size_t pos() const { return m_pos; }
	size_t size() const { return m_size; }
	void setPos(size_t p) { if (p > m_size) fail("seek beyond the end of the stream"); else m_pos = p; }

	uint32_t readUInt() { uint32_t v = 0; raw(&v, 4); return v; }                      /* stream.cpp:275-281 */
	int32_t readInt() { int32_t v = 0; raw(&v, 4); return v; }
	uint64_t readSize() { uint64_t v = 0; raw(&v, 8); return v; }                       /* stream.h:267: readULong */
	bool readBool() { uint8_t v = 0; raw(&v, 1); return v != 0; }                     /* stream.h:279 */
	FloatT readFloat() { FloatT v = 0; raw(&v, sizeof(FloatT)); return v; }
	std::string readString() {                                                        /* stream.cpp:391-402 */
		std::string s;
		while (ok()) {
			char c = 0; raw(&c, 1);
			if (c == 0) break;
			s += c;
		}
		return s;
	}
	void readSpectrum(float rgb[3]) {                                                 /* rgbOf(): toLinearRGB is the identity for 3 samples */
		for (int i = 0; i < 3; ++i) rgb[i] = (float) readFloat();
	}
	void readVec3(FloatT v[3]) { for (int i = 0; i < 3; ++i) v[i] = readFloat(); }
	Matrix44<FloatT> readMatrix() {
		Matrix44<FloatT> m;
		for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) m.m[i][j] = readFloat();
		return m;
	}
	Xform<FloatT> readTransform() { Xform<FloatT> t; t.fwd = readMatrix(); t.inv = readMatrix(); return t; }
private:
	void raw(void *dst, size_t n) {
		if (!ok()) { memset(dst, 0, n); return; }
		if (m_pos + n > m_size) { fail("unexpected end of the serialized stream"); memset(dst, 0, n); return; }
		memcpy(dst, m_data + m_pos, n); m_pos += n;
	}
	const uint8_t *m_data; size_t m_size, m_pos;
	std::string m_error;
};

template <typename FloatT> inline void copy3x3(float *dst, const Matrix44<FloatT> &m) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) dst[3 * i + j] = (float) m.m[i][j];
}
template <typename FloatT> inline void copy3x4(float *dst, const Matrix44<FloatT> &m) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) dst[4 * i + j] = (float) m.m[i][j];
}

/* ------------------------------------------------------------------------------------------------------------------
 * BSDFs.  What <BSDF class>::serialize wrote -- the only access to the plugins' private parameters.  BSDFs have no parent
 * (BSDF::setParent is empty, bsdf.cpp:55-57) and their only children are textures.
 * ---------------------------------------------------------------------------------------------------------------- */
/* First float of texture slot `slot` (0, 1) of BSDF type `type` inside its parameter block, -1 = the type has no such slot: the
 * table of include/mtsgpu.h (mtsgpu_set_vertex_colors), for callers that write a slot's floats after parsing. */
inline int bsdfSlotOffset(uint32_t type, int slot) {
	static const int table[MTSGPU_BSDF_NTYPES][2] = { { 0, -1 }, { 2, 5 }, { 7, -1 }, { 5, 8 }, { 0, -1 }, { 5, 8 }, { 4, 7 }, { 0, -1 }, { 7, 10 }, { -1, -1 } };
	type &= 0xFFu;
	return (type < (uint32_t) MTSGPU_BSDF_NTYPES && (slot == 0 || slot == 1)) ? table[type][slot] : -1;
}

/* What LDRTexture::serialize wrote (src/textures/ldrtexture.cpp:210-228), as far as a parser without an image decoder can go:
 * the fields, and where the bytes of the encoded file lie in the stream the caller handed over.  wrapMode is translated to
 * MTSGPU_WRAP_* (MIPMap::EWrapMode numbers repeat, black, white, clamp: mipmap.h:32-37). */
struct LdrTexture {
	int32_t texture;             /* index of the texture's descriptor in the caller's mtsgpu_uv_texture list */
	std::string filename;
	float gamma;                 /* -1: sRGB */
	int32_t format;              /* Bitmap::EFileFormat */
	int32_t filterType;          /* MIPMap::EFilterType: always ENone = 2 here, the others are refused */
	uint32_t wrapMode;           /* MTSGPU_WRAP_* */
	float maxAnisotropy;
	size_t offset; uint32_t size;      /* the encoded file: bytes [offset, offset + size) of the stream */
};

template <typename FloatT> class BSDFStream {
public:
	BSDFStream(const uint8_t *data, size_t size) : r(data, size) {
		if (!openObject(m_className)) r.fail("cannot read back the parameters of a BSDF");
		/* BSDF::serialize (bsdf.cpp:50-53): ConfigurableObject::serialize = the parent (none), then m_name */
		skipReference(); r.readString();
	}
	const std::string &className() const { return m_className; }
	/* a texture child: [id][class name][Texture::serialize = parent reference][ConstantSpectrumTexture: the value]
	 * (src/librender/texture.cpp:39-41, :89-93).  Anything but a constant needs computePartials + MIPMap: out of scope --
	 * except `VertexColors` (src/textures/vertexcolors.cpp), see readSpectrumTexture. */
	void readConstantTexture(const char *what, float rgb[3]) { readSpectrumTexture(what, rgb, -1); }
	/* The texture of slot `slot` (0, 1: the texture-typed spectrum slots of include/mtsgpu.h) of the BSDF the reader stands on.
	 * A `VertexColors` instance writes nothing of its own (vertexcolors.cpp:37-39: Texture::serialize, the parent reference);
	 * its slot is reported in colorSlots() and the block receives (1, 1, 1), the texture's getAverage() / getMaximum()
	 * (:49-55), from which Phong::configure and Ward::configure derived the weights that follow in the stream.  One
	 * VertexColors instance in two slots arrives as a bare id the second time: refused, like every shared instance whose
	 * fields are out of reach.  slot < 0: a slot that cannot take colours. */
	/* A `Checkerboard` or `GridTexture` instance (src/textures/checkerboard.cpp:42-46, gridtexture.cpp:44-49) writes
	 * Texture2D::serialize (texture.cpp:67-71: Texture::serialize, then uvOffset and uvScale, two Floats each), brightColor,
	 * darkColor and, the grid, lineWidth.  A caller that called takeUvTextures() receives the descriptor in its list and the
	 * list index in slotTextures(); the block receives the texture's getAverage(), darkColor * .5f (sic) or brightColor, which is
	 * what Phong::configure and Ward::configure read.  Every other caller is refused as before.  A shared instance is refused. */
	void readSpectrumTexture(const char *what, float rgb[3], int slot) {
		const uint32_t id = r.readUInt();
		if (id != 0 && m_values.count(id)) { memcpy(rgb, m_values[id].v, sizeof(float) * 3); return; }      /* one texture shared by two slots */
		if (id == 0) { r.fail(std::string(what) + " of " + m_className + " is missing"); return; }
		if (m_colorIds.count(id)) { r.fail(std::string(what) + " of " + m_className + " is a VertexColors instance shared with another slot: shared instances are not supported"); return; }
		if (m_uvTexIds.count(id)) { r.fail(std::string(what) + " of " + m_className + " is a " + m_uvTexIds[id] + " instance shared with another slot: shared instances are not supported"); return; }
		m_seen.insert(id);
		const std::string cls = r.readString();
		if ((cls == "Checkerboard" || cls == "GridTexture") && slot >= 0 && m_uvTextures) {
			skipReference();
			mtsgpu_uv_texture t;
			memset(&t, 0, sizeof(t));
			t.kind = cls == "GridTexture" ? MTSGPU_TEX_GRID : MTSGPU_TEX_CHECKERBOARD;
			t.uoffset = (float) r.readFloat(); t.voffset = (float) r.readFloat();                /* Point2 m_uvOffset */
			t.uscale = (float) r.readFloat(); t.vscale = (float) r.readFloat();                  /* Vector2 m_uvScale */
			r.readSpectrum(t.bright); r.readSpectrum(t.dark);
			if (t.kind == MTSGPU_TEX_GRID) t.line_width = (float) r.readFloat();
			if (!r.ok()) return;
			for (int k = 0; k < 3; ++k) rgb[k] = t.kind == MTSGPU_TEX_GRID ? t.bright[k] : t.dark[k] * .5f;      /* getAverage() */
			m_slotTextures[slot] = (int32_t) m_uvTextures->size();
			m_uvTextures->push_back(t);
			m_uvTexIds[id] = cls;
			return;
		}
		if (cls == "LDRTexture" && slot >= 0 && m_uvTextures && m_bitmaps) {
			/* Texture2D::serialize, filename, gamma, format, filterType, wrapMode, maxAnisotropy, a uint32 size and that many
			 * bytes of the encoded file.  Nothing is decoded here: the block's slot stays (0, 0, 0) until the caller, who has
			 * the decoder, writes the texture's getAverage() there. */
			skipReference();
			mtsgpu_uv_texture t;
			memset(&t, 0, sizeof(t));
			t.kind = MTSGPU_TEX_BITMAP;
			t.uoffset = (float) r.readFloat(); t.voffset = (float) r.readFloat();
			t.uscale = (float) r.readFloat(); t.vscale = (float) r.readFloat();
			LdrTexture b;
			b.texture = (int32_t) m_uvTextures->size();
			b.filename = r.readString();
			b.gamma = (float) r.readFloat();
			b.format = r.readInt();
			b.filterType = r.readInt();
			const uint32_t wrap = r.readUInt();
			b.maxAnisotropy = (float) r.readFloat();
			b.size = r.readUInt();
			b.offset = r.pos();
			b.wrapMode = 0;
			if (!r.ok()) return;
			if (b.filterType != 2) {                                                             /* MIPMap::ENone */
				const char *filter = b.filterType == 0 ? "ewa" : b.filterType == 1 ? "trilinear" : "unknown";
				r.fail(std::string(what) + " of " + m_className + " is an LDRTexture with filterType \"" + filter + "\": a filtered lookup needs ray "
				       "differentials (the uv partials of every hit), which this path does not trace; set filterType to \"none\" for the unfiltered texel");
				return;
			}
			static const uint32_t wrapOf[4] = { MTSGPU_WRAP_REPEAT, MTSGPU_WRAP_BLACK, MTSGPU_WRAP_WHITE, MTSGPU_WRAP_CLAMP };
			if (wrap > 3) { r.fail(std::string(what) + " of " + m_className + " is an LDRTexture with unknown wrap mode " + std::to_string((unsigned long long) wrap)); return; }
			b.wrapMode = wrapOf[wrap];
			if (b.size > r.size() - b.offset) {
				r.fail(std::string(what) + " of " + m_className + " is an LDRTexture whose encoded file (" + std::to_string((unsigned long long) b.size) + " bytes) is truncated");
				return;
			}
			r.setPos(b.offset + b.size);
			rgb[0] = rgb[1] = rgb[2] = 0.0f;
			m_slotTextures[slot] = b.texture;
			m_uvTextures->push_back(t);
			m_bitmaps->push_back(b);
			m_uvTexIds[id] = cls;
			return;
		}
		if (cls == "VertexColors" && slot >= 0) {
			skipReference();
			rgb[0] = rgb[1] = rgb[2] = 1.0f;
			m_colorSlots |= 1u << slot;
			m_colorIds.insert(id);
			return;
		}
		if (cls != "ConstantSpectrumTexture") {                                                 /* consttexture.h:28-60 */
			r.fail(std::string(what) + " of " + m_className + " is a " + cls + "; only constant reflectances are supported");
			return;
		}
		skipReference();
		r.readSpectrum(rgb);
		memcpy(m_values[id].v, rgb, sizeof(float) * 3);
	}
	/* the slots of the block read since the last resetColorSlots() that hold a VertexColors texture (bit s = slot s) */
	uint32_t colorSlots() const { return m_colorSlots; }
	void resetColorSlots() { m_colorSlots = 0; m_slotTextures[0] = m_slotTextures[1] = -1; }
	/* the list that receives the Checkerboard / GridTexture descriptors (what mtsgpu_set_uv_textures takes as `textures`);
	 * without it these classes are refused like every non-constant texture */
	void takeUvTextures(std::vector<mtsgpu_uv_texture> *list) { m_uvTextures = list; }
	/* the list that receives one LdrTexture per unfiltered LDRTexture met (next to takeUvTextures, which receives its
	 * descriptor); without it the class is refused like every non-constant texture */
	void takeBitmaps(std::vector<LdrTexture> *list) { m_bitmaps = list; }
	/* per slot of the block read since the last resetColorSlots(): the index of its texture in that list, or -1 */
	const int32_t *slotTextures() const { return m_slotTextures; }
	bool hasSlotTexture() const { return m_slotTextures[0] >= 0 || m_slotTextures[1] >= 0; }
	/* The opacity of the Mask the reader stands on (mask.cpp:47-52: BSDF::serialize, then the opacity texture instance, then the
	 * nested BSDF instance) -> one mtsgpu_bsdf_mask.  A ConstantSpectrumTexture becomes MTSGPU_MASK_CONSTANT; a Checkerboard, a
	 * GridTexture or an unfiltered LDRTexture becomes MTSGPU_MASK_TEXTURE through the lists of takeUvTextures / takeBitmaps, with
	 * the texture's getAverage() in `opacity` (an LDRTexture: left 0 for the caller, who has the decoder).  VertexColors is
	 * refused: there is no mask kind for it. */
	void readMaskOpacity(mtsgpu_bsdf_mask &m) {
		resetColorSlots();
		memset(&m, 0, sizeof(m));
		readSpectrumTexture("opacity", m.opacity, 0);
		if (r.ok() && m_colorSlots) r.fail("opacity of Mask is a VertexColors texture: vertex colours as opacity are not supported");
		m.kind = m_slotTextures[0] >= 0 ? MTSGPU_MASK_TEXTURE : MTSGPU_MASK_CONSTANT;
		m.texture = m_slotTextures[0];
		resetColorSlots();
	}
	/* a ConstantFloatTexture child (roughglass' alpha): [id][class name][Texture::serialize][the value] (texture.cpp:95-103) */
	FloatT readConstantFloatTexture(const char *what) {
		const uint32_t id = r.readUInt();
		if (id == 0 || m_seen.count(id)) { r.fail(std::string(what) + " of " + m_className + " is missing or shared"); return 0; }
		m_seen.insert(id);
		const std::string cls = r.readString();
		if (cls == "VertexColors") { r.fail(std::string(what) + " of " + m_className + " is a VertexColors texture: vertex colours are a spectrum, this slot takes a float texture; not supported"); return 0; }
		if (cls == "Checkerboard" || cls == "GridTexture" || cls == "LDRTexture") { r.fail(std::string(what) + " of " + m_className + " is a " + cls + " texture: uv textures are supported in spectrum slots only, this slot takes a float texture; not supported"); return 0; }
		if (cls != "ConstantFloatTexture") { r.fail(std::string(what) + " of " + m_className + " is a " + cls + "; only constant values are supported"); return 0; }
		skipReference();
		return r.readFloat();
	}
	/* the nested BRDF of a `twosided` adapter or of a composite: positions the reader on its fields */
	void enterNestedBSDF() {
		const std::string outer = m_className;
		if (!r.ok()) return;
		if (!openObject(m_className)) {
			r.fail(outer == "TwoSidedBRDF" ? "twosided BRDF without a nested BRDF" : outer + ": a nested BSDF is missing or was written before (shared instances are not supported)");
			return;
		}
		skipReference(); r.readString();
	}
	ByteReader<FloatT> r;
private:
	struct RGB { float v[3]; };
	bool openObject(std::string &cls) {
		const uint32_t id = r.readUInt();
		if (id == 0 || m_seen.count(id)) return false;
		m_seen.insert(id);
		cls = r.readString();
		return true;
	}
	void skipReference() {
		const uint32_t id = r.readUInt();
		if (id != 0 && !m_seen.count(id)) r.fail("unexpected nested object in the serialized form of " + m_className);
	}
	std::set<uint32_t> m_seen, m_colorIds;
	std::map<uint32_t, std::string> m_uvTexIds;
	std::vector<mtsgpu_uv_texture> *m_uvTextures = NULL;
	std::vector<LdrTexture> *m_bitmaps = NULL;
	int32_t m_slotTextures[2] = { -1, -1 };
	uint32_t m_colorSlots = 0;
	std::map<uint32_t, RGB> m_values;
	std::string m_className;
};

/* The fields of the class the reader stands on (after BSDF::serialize's own), for every class with ONE parameter block.
 * slots (optional): the mask of the block's texture slots that hold a VertexColors texture (bit s = slot s of the table in
 * include/mtsgpu.h; Mirror keeps a plain Spectrum, mirror.cpp:51-55, and can have none). */
template <typename FloatT> inline void parseBSDFFields(BSDFStream<FloatT> &rd, uint32_t flags, uint32_t *type, float *P, uint32_t *slots = NULL) {
	const std::string cls = rd.className();
	rd.resetColorSlots();
	if (cls == "Lambertian") {                                               /* lambertian.cpp:137-141 */
		*type = MTSGPU_BSDF_LAMBERTIAN | flags;
		rd.readSpectrumTexture("reflectance", P, 0);
	} else if (cls == "Dielectric") {                                        /* dielectric.cpp:88-95 */
		*type = MTSGPU_BSDF_DIELECTRIC | flags;
		P[0] = (float) rd.r.readFloat(); P[1] = (float) rd.r.readFloat();
		rd.readSpectrumTexture("specularReflectance", P + 2, 0);
		rd.readSpectrumTexture("specularTransmittance", P + 5, 1);
	} else if (cls == "RoughMetal") {                                        /* roughmetal.cpp:169-176 */
		*type = MTSGPU_BSDF_ROUGHMETAL | flags;
		rd.readSpectrumTexture("specularReflectance", P + 7, 0);
		P[0] = (float) rd.r.readFloat();
		rd.r.readSpectrum(P + 1); rd.r.readSpectrum(P + 4);                  /* m_ior, m_k */
	} else if (cls == "Microfacet") {                                        /* microfacet.cpp:283-293 */
		*type = MTSGPU_BSDF_MICROFACET | flags;
		rd.readSpectrumTexture("diffuseReflectance", P + 5, 0);
		rd.readSpectrumTexture("specularReflectance", P + 8, 1);
		for (int k = 0; k < 5; ++k) P[k] = (float) rd.r.readFloat();         /* alphaB, kd, ks, intIOR, extIOR */
	} else if (cls == "Mirror") {                                            /* mirror.cpp:51-55 */
		*type = MTSGPU_BSDF_MIRROR | flags;
		rd.r.readSpectrum(P);
	} else if (cls == "Phong") {                                             /* phong.cpp:246-256 (values after configure()) */
		*type = MTSGPU_BSDF_PHONG | flags;
		rd.readSpectrumTexture("diffuseReflectance", P + 5, 0);
		rd.readSpectrumTexture("specularReflectance", P + 8, 1);
		for (int k = 0; k < 5; ++k) P[k] = (float) rd.r.readFloat();         /* exponent, kd, ks, specular / diffuse sampling weight */
	} else if (cls == "RoughGlass") {                                        /* roughglass.cpp:735-744 */
		*type = MTSGPU_BSDF_ROUGHGLASS | flags;
		P[0] = (float) rd.r.readInt();                                       /* EBeckmann 0, EPhong 1, EGGX 2 (:84-91) = the ABI's codes */
		P[1] = (float) rd.readConstantFloatTexture("alpha");                 /* phong: already the exponent (:130-136) */
		rd.readSpectrumTexture("specularReflectance", P + 4, 0);
		rd.readSpectrumTexture("specularTransmittance", P + 7, 1);
		P[2] = (float) rd.r.readFloat(); P[3] = (float) rd.r.readFloat();    /* intIOR, extIOR */
	} else if (cls == "DiffuseTransmitter") {                                /* difftrans.cpp:142-146 */
		*type = MTSGPU_BSDF_DIFFTRANS | flags;
		rd.readSpectrumTexture("transmittance", P, 0);
	} else if (cls == "Ward") {                                              /* ward.cpp:299-311 (values after configure()) */
		*type = MTSGPU_BSDF_WARD | flags;
		const uint32_t model = rd.r.readUInt();                              /* EWard 0, EWardDuer 1, EBalanced 2 (:45-52) = the ABI's codes */
		if (model > 2 && rd.r.ok()) rd.r.fail("Ward: unknown model type");
		P[0] = (float) model;
		rd.readSpectrumTexture("diffuseReflectance", P + 7, 0);
		rd.readSpectrumTexture("specularReflectance", P + 10, 1);
		for (int k = 1; k <= 6; ++k) P[k] = (float) rd.r.readFloat();        /* alphaX, alphaY, kd, ks, specular / diffuse sampling weight */
	} else {
		rd.r.fail("BSDF class " + cls + " is not on this path (lambertian, dielectric, roughmetal, microfacet, mirror, phong, "
		          "roughglass, difftrans, ward, composite and the twosided adapter are)");
	}
	if (slots) *slots = rd.colorSlots();
	else if (rd.colorSlots() && rd.r.ok()) rd.r.fail(cls + " holds a VertexColors texture: the caller does not take colour slots");
}

/* One BSDF instance -> its type word (MTSGPU_BSDF_* | MTSGPU_BSDF_TWOSIDED) and parameter block P[MTSGPU_BSDF_NPARAMS]
 * (zeroed by the caller).  Returns false with `err` set for classes and textures that are not on this path, and for a
 * Composite, which is more than one block: parseBSDFTable reads those. */
template <typename FloatT> inline bool parseBSDF(const uint8_t *data, size_t size, uint32_t *type, float *P, std::string *err, uint32_t *slots = NULL) {
	BSDFStream<FloatT> rd(data, size);
	uint32_t flags = 0;
	if (rd.className() == "TwoSidedBRDF") {                                  /* twosided.cpp:52-56: the nested BRDF follows */
		flags |= MTSGPU_BSDF_TWOSIDED;
		rd.enterNestedBSDF();
	}
	if (rd.className() == "Composite") rd.r.fail("a Composite BSDF fills several table entries: read it with parseBSDFTable");
	else parseBSDFFields(rd, flags, type, P, slots);
	if (!rd.r.ok()) { if (err) *err = rd.r.error() + " (while reading a " + rd.className() + ")"; return false; }
	return true;
}

/* One BSDF instance -> entries appended to a BSDF table (types[i], params[16 i ..]); returns the index of the instance's
 * own entry, or -1 with `err` set.  Every class but Composite appends one entry.  Composite::serialize (composite.cpp:81-89)
 * writes the child count (a size_t: 64 bits, stream.h:180) and then, per child, its weight and the nested BSDF instance;
 * the children are appended first, in their order, then the composite with the block of include/mtsgpu.h: [0] n,
 * [1..n] weights, [1+n..2n] the children's table indices as floats.  What the device cannot run is refused here with the
 * reason: more than MTSGPU_COMPOSITE_MAX children or none, a negative weight (composite.cpp:45-46), a nested composite, a
 * delta child (dielectric, mirror), a child instance that was written before (a bare id: its fields are not in reach). */
/* colorSlots (optional): one mask per appended entry, next to `types` (what mtsgpu_set_vertex_colors takes as
 * bsdf_color_slots).  A composite child with a coloured slot is refused with the child's number, as the library refuses it. */
/* uvTextures + slotTextures (optional, both or neither): the Checkerboard / GridTexture descriptors met are appended to
 * uvTextures, and slotTextures receives two entries per appended table entry, the index of the slot's texture in uvTextures
 * or -1 (what mtsgpu_set_uv_textures takes as `textures` and `bsdf_slot_texture`).  A composite child with a textured slot
 * is refused with the child's number.  Without them a Checkerboard or GridTexture is refused like any other texture. */
/* bitmaps (optional, with uvTextures and slotTextures): one LdrTexture per LDRTexture with filterType none, whose descriptor
 * (kind MTSGPU_TEX_BITMAP) goes to uvTextures; offset counts from `data`.  The slot's floats in the block are left 0: the
 * caller decodes the file and writes getAverage() there.  Without the list an LDRTexture is refused like any other texture. */
/* masks (optional): one mtsgpu_bsdf_mask per appended entry, next to `types` (what mtsgpu_set_uv_masked_textures takes as
 * bsdf_mask).  With the list an outermost Mask (mask.cpp) is opened: its opacity is read (readMaskOpacity), its nested BSDF is
 * entered like a twosided child, and the instance's own entry receives the mask; every other entry receives MTSGPU_MASK_NONE.
 * Refused with the reason: a Mask inside a Mask, under TwoSidedBRDF (twosided.cpp:71-73 refuses that child too), around a
 * Composite or as a composite's child, and a VertexColors opacity.  Without the list a Mask is refused like every class that is
 * not on this path. */
/* snow (optional) + wiscombeConfigure: one mtsgpu_bsdf_snow per appended entry, next to `types` (what mtsgpu_set_snow_bsdfs
 * takes).  With the list a Wiscombe (wiscombe.cpp:172-179: g, depth, w0, sigmaT after BSDF::serialize's own fields) becomes a
 * Lambertian entry whose block is zero, with the record wiscombeConfigure -- the library's mtsgpu_wiscombe_configure -- makes
 * of the four fields; twosided(Wiscombe) sets the bit; every other entry receives MTSGPU_SNOW_NONE.  Refused with the reason: a
 * Wiscombe whose derived values are not finite, under a Mask or as a composite's child, and every HanrahanKrueger: its stream
 * holds the size multiplier and the two sigmas alone (hanrahan-krueger.cpp:225-230), not g, the two indices, the two factors
 * and the flag.  Without the list both are refused like every class that is not on this path. */
typedef int (*WiscombeConfigure)(const float raw[8], mtsgpu_bsdf_snow *out);
inline std::string hkRefusal() {
	return "HanrahanKrueger: its stream holds only sizeMultiplier, sigmaA and sigmaS (hanrahan-krueger.cpp:225-230) and its unserialising "
	       "constructor reads nothing, so g, etaInt, etaExt, ssFactor, drFactor and diffuseReflectance are out of reach: the BRDF is served "
	       "through the C ABI (mtsgpu_hk_configure, mtsgpu_set_snow_bsdfs) only";
}
/* cloth (optional): the weaves of the IrawanClothBRDFs and one weave index per appended entry, -1 without one (what
 * mtsgpu_set_cloth_bsdfs takes once ClothTable::fill has set the pointers).  With it an IrawanClothBRDF -- after BSDF::serialize's own
 * fields WeavePattern::serialize (irawan.h:191-211: the name, alpha, beta, ss, hWidth, warpArea, weftArea, tileWidth, tileHeight,
 * the four d*UmaxOverD*, fineness, period, the pattern array of tileWidth * tileHeight words, writeSize of the yarn count, per yarn
 * type, psi, umax, kappa, width, length, centerU, centerV and the two Spectrums), then repeatU, repeatV, kdMultiplier,
 * ksMultiplier (irawan.cpp:265-273) -- becomes a Lambertian entry whose block is zero, with its weave; twosided(Irawan) sets the
 * bit.  Refused with the reason: under a Mask, as a composite's child, a tile dimension of zero or above 32768 (the library's
 * limit).  What the library checks of a weave (mtsgpu_cloth.h) it checks when the table is handed over.  Without the list the
 * class is refused like every class that is not on this path. */
struct ClothWeave {
	mtsgpu_weave w;                      /* pattern and yarns are NULL until ClothTable::fill */
	std::string name;
	std::vector<uint32_t> pattern;
	std::vector<mtsgpu_yarn> yarns;
};
struct ClothTable {
	std::vector<ClothWeave> weaves;
	std::vector<int32_t> bsdfWeave;
	bool any() const { return !weaves.empty(); }
	/* the array mtsgpu_set_cloth_bsdfs takes: valid while this table is neither changed nor destroyed */
	void fill(std::vector<mtsgpu_weave> &out) {
		out.resize(weaves.size());
		for (size_t k = 0; k < weaves.size(); ++k) {
			weaves[k].w.n_pattern = (uint32_t) weaves[k].pattern.size(); weaves[k].w.n_yarns = (uint32_t) weaves[k].yarns.size();
			weaves[k].w.pattern = weaves[k].pattern.empty() ? NULL : &weaves[k].pattern[0];
			weaves[k].w.yarns = weaves[k].yarns.empty() ? NULL : &weaves[k].yarns[0];
			out[k] = weaves[k].w;
		}
	}
};
template <typename FloatT> inline int parseBSDFTable(const uint8_t *data, size_t size, std::vector<uint32_t> &types, std::vector<float> &params,
                                                     std::string *err, std::vector<uint32_t> *colorSlots = NULL,
                                                     std::vector<mtsgpu_uv_texture> *uvTextures = NULL, std::vector<int32_t> *slotTextures = NULL,
                                                     std::vector<LdrTexture> *bitmaps = NULL, std::vector<mtsgpu_bsdf_mask> *masks = NULL,
                                                     std::vector<mtsgpu_bsdf_snow> *snow = NULL, WiscombeConfigure wiscombeConfigure = NULL,
                                                     ClothTable *cloth = NULL) {
	BSDFStream<FloatT> rd(data, size);
	const size_t firstWeave = cloth ? cloth->weaves.size() : 0;
	mtsgpu_bsdf_snow noSnow;
	memset(&noSnow, 0, sizeof(noSnow)); noSnow.kind = MTSGPU_SNOW_NONE;
	const size_t first = types.size(), firstTex = uvTextures ? uvTextures->size() : 0, firstBmp = bitmaps ? bitmaps->size() : 0;
	if (uvTextures && slotTextures) rd.takeUvTextures(uvTextures);
	if (uvTextures && slotTextures && bitmaps) rd.takeBitmaps(bitmaps);
	mtsgpu_bsdf_mask none, mask;
	memset(&none, 0, sizeof(none)); none.kind = MTSGPU_MASK_NONE; none.texture = -1;
	mask = none;
	if (masks && rd.className() == "Mask") {
		rd.readMaskOpacity(mask);
		rd.enterNestedBSDF();
		if (rd.r.ok() && rd.className() == "Mask") rd.r.fail("a Mask inside a Mask: nested masks are not supported");
	}
	uint32_t flags = 0;
	if (rd.r.ok() && rd.className() == "TwoSidedBRDF") {
		flags |= MTSGPU_BSDF_TWOSIDED; rd.enterNestedBSDF();
		if (masks && rd.r.ok() && rd.className() == "Mask")
			rd.r.fail("a Mask under TwoSidedBRDF: the mask transmits, and the adapter takes no child with a transmission component (twosided.cpp:71-73)");
	}
	int own = -1;
	if (!rd.r.ok()) {
		/* the mask or an adapter could not be opened */
	} else if (rd.className() == "Composite" && mask.kind != MTSGPU_MASK_NONE) {
		rd.r.fail("a Mask around a Composite is not supported");
	} else if (snow && rd.className() == "HanrahanKrueger") {
		rd.r.fail(hkRefusal());
	} else if (snow && rd.className() == "Wiscombe") {
		float raw[8];
		raw[0] = (float) rd.r.readFloat(); raw[1] = (float) rd.r.readFloat();            /* m_g, m_depth */
		rd.r.readSpectrum(raw + 2); rd.r.readSpectrum(raw + 5);                          /* m_w0, m_sigmaT */
		mtsgpu_bsdf_snow record = noSnow;
		if (!rd.r.ok()) {
			/* truncated */
		} else if (mask.kind != MTSGPU_MASK_NONE) {
			rd.r.fail("a Mask around a Wiscombe is not supported");
		} else if (!wiscombeConfigure) {
			rd.r.fail("Wiscombe: the caller gave a snow list without mtsgpu_wiscombe_configure");
		} else if (wiscombeConfigure(raw, &record) != MTSGPU_OK) {
			rd.r.fail("Wiscombe: configure() leaves a derived value that is not finite (g = " + std::to_string(raw[0]) + ", w0 = " + std::to_string(raw[2])
			          + " " + std::to_string(raw[3]) + " " + std::to_string(raw[4]) + ")");
		}
		types.push_back(MTSGPU_BSDF_LAMBERTIAN | flags); params.insert(params.end(), MTSGPU_BSDF_NPARAMS, 0.0f);
		if (colorSlots) colorSlots->push_back(0u);
		if (slotTextures) slotTextures->insert(slotTextures->end(), 2, (int32_t) -1);
		if (masks) masks->push_back(none);
		snow->push_back(record);
		if (cloth) cloth->bsdfWeave.push_back(-1);
		own = (int) types.size() - 1;
	} else if (cloth && rd.className() == "IrawanClothBRDF") {
		ClothWeave cw;
		memset(&cw.w, 0, sizeof(cw.w));
		mtsgpu_weave &w = cw.w;
		cw.name = rd.r.readString();
		w.alpha = (float) rd.r.readFloat(); w.beta = (float) rd.r.readFloat(); w.ss = (float) rd.r.readFloat(); w.hWidth = (float) rd.r.readFloat();
		w.warpArea = (float) rd.r.readFloat(); w.weftArea = (float) rd.r.readFloat();
		w.tileWidth = rd.r.readUInt(); w.tileHeight = rd.r.readUInt();
		w.dWarpUmaxOverDWarp = (float) rd.r.readFloat(); w.dWarpUmaxOverDWeft = (float) rd.r.readFloat();
		w.dWeftUmaxOverDWarp = (float) rd.r.readFloat(); w.dWeftUmaxOverDWeft = (float) rd.r.readFloat();
		w.fineness = (float) rd.r.readFloat(); w.period = (float) rd.r.readFloat();
		if (rd.r.ok() && (w.tileWidth == 0 || w.tileHeight == 0 || w.tileWidth > 32768u || w.tileHeight > 32768u))
			rd.r.fail("IrawanClothBRDF: tile of " + std::to_string(w.tileWidth) + " x " + std::to_string(w.tileHeight) + ": a dimension is zero or above 32768");
		for (uint64_t i = 0, n = (uint64_t) w.tileWidth * w.tileHeight; i < n && rd.r.ok(); ++i) cw.pattern.push_back(rd.r.readUInt());
		const uint64_t nYarns = rd.r.ok() ? rd.r.readSize() : 0;
		for (uint64_t i = 0; i < nYarns && rd.r.ok(); ++i) {
			mtsgpu_yarn y;
			y.type = (uint32_t) rd.r.readInt();
			y.psi = (float) rd.r.readFloat(); y.umax = (float) rd.r.readFloat(); y.kappa = (float) rd.r.readFloat();
			y.width = (float) rd.r.readFloat(); y.length = (float) rd.r.readFloat();
			y.centerU = (float) rd.r.readFloat(); y.centerV = (float) rd.r.readFloat();
			rd.r.readSpectrum(y.kd); rd.r.readSpectrum(y.ks);
			cw.yarns.push_back(y);
		}
		w.repeatU = (float) rd.r.readFloat(); w.repeatV = (float) rd.r.readFloat();
		w.kdMultiplier = (float) rd.r.readFloat(); w.ksMultiplier = (float) rd.r.readFloat();
		if (rd.r.ok() && mask.kind != MTSGPU_MASK_NONE) rd.r.fail("a Mask around an IrawanClothBRDF is not supported");
		types.push_back(MTSGPU_BSDF_LAMBERTIAN | flags); params.insert(params.end(), MTSGPU_BSDF_NPARAMS, 0.0f);
		if (colorSlots) colorSlots->push_back(0u);
		if (slotTextures) slotTextures->insert(slotTextures->end(), 2, (int32_t) -1);
		if (masks) masks->push_back(none);
		if (snow) snow->push_back(noSnow);
		cloth->bsdfWeave.push_back((int32_t) cloth->weaves.size());
		cloth->weaves.push_back(cw);
		own = (int) types.size() - 1;
	} else if (rd.className() != "Composite") {
		types.push_back(0); params.insert(params.end(), MTSGPU_BSDF_NPARAMS, 0.0f);
		uint32_t slots = 0;
		parseBSDFFields(rd, flags, &types.back(), &params[params.size() - MTSGPU_BSDF_NPARAMS], colorSlots ? &slots : NULL);
		if (colorSlots) colorSlots->push_back(slots);
		if (slotTextures) slotTextures->insert(slotTextures->end(), rd.slotTextures(), rd.slotTextures() + 2);
		if (masks) masks->push_back(mask);
		if (snow) snow->push_back(noSnow);
		if (cloth) cloth->bsdfWeave.push_back(-1);
		own = (int) types.size() - 1;
	} else {
		const uint64_t n = rd.r.readSize();
		if (rd.r.ok() && (n < 1 || n > MTSGPU_COMPOSITE_MAX))
			rd.r.fail("a Composite with " + std::to_string((unsigned long long) n) + " children: between 1 and " + std::to_string(MTSGPU_COMPOSITE_MAX) + " are supported");
		float block[MTSGPU_BSDF_NPARAMS] = { 0 };
		block[0] = (float) n;
		for (uint64_t i = 0; i < n && rd.r.ok(); ++i) {
			const float w = (float) rd.r.readFloat();
			if (rd.r.ok() && !(w >= 0.0f)) rd.r.fail("Composite: invalid BRDF weight (composite.cpp:45-46)");
			block[1 + i] = w;
			rd.enterNestedBSDF();                                            /* fails on NULL and on an instance written before */
			uint32_t childFlags = 0;
			if (rd.r.ok() && rd.className() == "TwoSidedBRDF") { childFlags |= MTSGPU_BSDF_TWOSIDED; rd.enterNestedBSDF(); }
			if (!rd.r.ok()) break;
			if (rd.className() == "Composite") { rd.r.fail("Composite: nested composites are not supported"); break; }
			if (masks && rd.className() == "Mask") { rd.r.fail("Composite: child " + std::to_string((unsigned long long) i) + " is a Mask: a mask is the outermost adapter, not supported as a composite's child"); break; }
			if (cloth && rd.className() == "IrawanClothBRDF") {
				rd.r.fail("Composite: child " + std::to_string((unsigned long long) i) + " is an IrawanClothBRDF: the composite's loop would run its entry as a Lambertian, not supported"); break;
			}
			if (snow && (rd.className() == "Wiscombe" || rd.className() == "HanrahanKrueger")) {
				rd.r.fail("Composite: child " + std::to_string((unsigned long long) i) + " is a " + rd.className() + ": the composite's loop would run its entry as a Lambertian, not supported"); break;
			}
			if (rd.className() == "Dielectric" || rd.className() == "Mirror") {
				rd.r.fail("Composite: child " + rd.className() + " is a delta BSDF (a composite would need fDelta / pdfDelta): not supported"); break;
			}
			types.push_back(0); params.insert(params.end(), MTSGPU_BSDF_NPARAMS, 0.0f);
			uint32_t slots = 0;
			parseBSDFFields(rd, childFlags, &types.back(), &params[params.size() - MTSGPU_BSDF_NPARAMS], &slots);
			if (colorSlots) colorSlots->push_back(0u);
			if (slotTextures) slotTextures->insert(slotTextures->end(), 2, (int32_t) -1);
			if (masks) masks->push_back(none);
			if (snow) snow->push_back(noSnow);
			if (cloth) cloth->bsdfWeave.push_back(-1);
			if (rd.r.ok() && rd.hasSlotTexture()) { rd.r.fail("Composite: child " + std::to_string((unsigned long long) i) + " (" + rd.className() + ") has a uv texture: a composite's children keep constant parameters, not supported"); break; }
			if (rd.r.ok() && slots) { rd.r.fail("Composite: child " + std::to_string((unsigned long long) i) + " (" + rd.className() + ") takes vertex colours: a composite's children keep constant parameters, not supported"); break; }
			block[1 + n + i] = (float) (types.size() - 1);
		}
		if (rd.r.ok()) {
			types.push_back(MTSGPU_BSDF_COMPOSITE | flags);
			if (colorSlots) colorSlots->push_back(0u);
			if (slotTextures) slotTextures->insert(slotTextures->end(), 2, (int32_t) -1);
			if (masks) masks->push_back(none);
			if (snow) snow->push_back(noSnow);
			if (cloth) cloth->bsdfWeave.push_back(-1);
			params.insert(params.end(), block, block + MTSGPU_BSDF_NPARAMS);
			own = (int) types.size() - 1;
		}
	}
	if (!rd.r.ok()) {
		types.resize(first); params.resize(first * MTSGPU_BSDF_NPARAMS);
		if (colorSlots) colorSlots->resize(first);
		if (slotTextures) slotTextures->resize(2 * first);
		if (masks) masks->resize(first);
		if (snow) snow->resize(first);
		if (cloth) { cloth->bsdfWeave.resize(first); cloth->weaves.resize(firstWeave); }
		if (uvTextures) uvTextures->resize(firstTex);
		if (bitmaps) bitmaps->resize(firstBmp);
		if (err) *err = rd.r.error() + " (while reading a " + rd.className() + ")";
		return -1;
	}
	return own;
}

/* ------------------------------------------------------------------------------------------------------------------
 * Scene-level objects (delta luminaires, the environment map, spheres) serialized with their parent taken off
 * (gpucommon.h: serializedDetached): [id]["<class>"][parent = 0][the class's fields]
 * ---------------------------------------------------------------------------------------------------------------- */
template <typename FloatT> inline void openDetached(ByteReader<FloatT> &r, const char *expectedClass) {
	r.readUInt();
	const std::string cls = r.readString();
	if (r.ok() && cls != expectedClass) r.fail(std::string("expected a ") + expectedClass + ", found a " + cls);
	if (r.readUInt() != 0 && r.ok()) r.fail(std::string(expectedClass) + " still has a parent");            /* ConfigurableObject(Stream *), properties.cpp:346-349 */
}
/* Luminaire(Stream *, InstanceManager *) (src/librender/luminaire.cpp:42-51): medium, sampling weight, type, intersectable,
 * worldToLuminaire, name */
template <typename FloatT> inline Xform<FloatT> readLuminaireBase(ByteReader<FloatT> &r) {
	if (r.readUInt() != 0 && r.ok()) r.fail("luminaires inside participating media are not on this path");
	r.readFloat(); r.readInt(); r.readBool();
	const Xform<FloatT> worldToLuminaire = r.readTransform();
	r.readString();
	return worldToLuminaire;
}

/* DirectionalLuminaire (directional.cpp:57-63): direction, intensity, disk origin, disk radius (after preprocess, :65-72) */
template <typename FloatT> inline bool parseDirectional(const uint8_t *data, size_t size, float *P, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "DirectionalLuminaire");
	readLuminaireBase(r);
	FloatT dir[3], origin[3];
	r.readVec3(dir);
	r.readSpectrum(P);
	r.readVec3(origin); (void) origin;
	P[6] = (float) r.readFloat();
	P[3] = (float) dir[0]; P[4] = (float) dir[1]; P[5] = (float) dir[2];
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	return true;
}

/* SpotLuminaire (spot.cpp:63-70): texture, intensity, beam width, cutoff angle; configure() (:56-62) derives the rest */
template <typename FloatT> inline bool parseSpot(const uint8_t *data, size_t size, float *P, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "SpotLuminaire");
	const Xform<FloatT> w2l = readLuminaireBase(r);
	{	/* m_texture: only the default constant 1 is on this path (spot.cpp:42-43, :96-102) */
		r.readUInt();
		if (r.readString() != "ConstantSpectrumTexture" && r.ok()) r.fail("projection textures of spot luminaires are not on this path");
		r.readUInt();                                                        /* Texture::serialize: its parent (the luminaire: a known id, or none) */
		float tex[3]; r.readSpectrum(tex);
		if (r.ok() && (tex[0] != 1.0f || tex[1] != 1.0f || tex[2] != 1.0f)) r.fail("projection textures of spot luminaires are not on this path");
	}
	r.readSpectrum(P);
	const FloatT beamWidth = r.readFloat(), cutoffAngle = r.readFloat();
	/* m_luminaireToWorld(Point(0, 0, 0)) (transform.h:133-149): the translation column, divided by w unless it is 1 */
	FloatT x = w2l.inv.m[0][3], y = w2l.inv.m[1][3], z = w2l.inv.m[2][3];
	const FloatT w = w2l.inv.m[3][3];
	if (w != (FloatT) 1) { const FloatT rc = (FloatT) 1 / w; x *= rc; y *= rc; z *= rc; }
	P[3] = (float) x; P[4] = (float) y; P[5] = (float) z;
	P[6] = (float) std::cos(beamWidth); P[7] = (float) std::cos(cutoffAngle);
	P[8] = (float) cutoffAngle; P[9] = (float) ((FloatT) 1 / (cutoffAngle - beamWidth));
	copy3x3(P + 10, w2l.fwd);
	P[19] = (float) beamWidth;
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	return true;
}

/* The projection texture of a spot luminaire, as parseSpotTextured found it.  present = false: a ConstantSpectrumTexture, which
 * falloffCurve never evaluates whatever its value (spot.cpp:95: only another class is looked up; the constant enters getPower
 * alone, which is not on this path) -- the luminaire is the plain spot.  Otherwise tex is the descriptor mtsgpu_set_spot_textures
 * takes and bilinear its filter flag; for an LDRTexture (isBitmap) ldr says where the encoded file lies, ldr.texture = 0. */
struct SpotTexture {
	bool present, isBitmap;
	mtsgpu_uv_texture tex;
	uint32_t bilinear;
	LdrTexture ldr;
};
/* SpotLuminaire with any texture this path serves (spot.cpp:63-70): parseSpot's block, and the nested texture instance read the
 * way the BSDF slots read theirs -- Checkerboard, GridTexture (Texture2D::serialize, brightColor, darkColor, the grid's lineWidth)
 * and LDRTexture with its encoded-file span (ldrtexture.cpp:210-228).  A luminaire lookup has no uv partials (spot.cpp:97), so
 * LDRTexture::getValue is MIPMap::triangle(0, u, v) for every filter type: none (2) is the nearest texel, ewa (0) and trilinear (1)
 * the bilinear lookup on level 0; all three are accepted here and translated to the flag.  ExrTexture, VertexColors and every
 * other class are refused by name. */
template <typename FloatT> inline bool parseSpotTextured(const uint8_t *data, size_t size, float *P, SpotTexture *tex, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "SpotLuminaire");
	const Xform<FloatT> w2l = readLuminaireBase(r);
	SpotTexture t;
	t.present = t.isBitmap = false; t.bilinear = 0;
	memset(&t.tex, 0, sizeof(t.tex));
	t.ldr.texture = 0; t.ldr.gamma = 0; t.ldr.format = 0; t.ldr.filterType = 2; t.ldr.wrapMode = 0; t.ldr.maxAnisotropy = 0; t.ldr.offset = 0; t.ldr.size = 0;
	{
		if (r.readUInt() == 0 && r.ok()) r.fail("the texture of the SpotLuminaire is missing");
		const std::string cls = r.readString();
		r.readUInt();                                                        /* Texture::serialize: its parent (the luminaire: a known id, or none) */
		if (!r.ok()) {
		} else if (cls == "ConstantSpectrumTexture") {
			float c[3]; r.readSpectrum(c);
		} else if (cls == "Checkerboard" || cls == "GridTexture") {
			t.present = true;
			t.tex.kind = cls == "GridTexture" ? MTSGPU_TEX_GRID : MTSGPU_TEX_CHECKERBOARD;
			t.tex.uoffset = (float) r.readFloat(); t.tex.voffset = (float) r.readFloat();              /* Point2 m_uvOffset */
			t.tex.uscale = (float) r.readFloat(); t.tex.vscale = (float) r.readFloat();                /* Vector2 m_uvScale */
			r.readSpectrum(t.tex.bright); r.readSpectrum(t.tex.dark);
			if (t.tex.kind == MTSGPU_TEX_GRID) t.tex.line_width = (float) r.readFloat();
		} else if (cls == "LDRTexture") {
			t.present = t.isBitmap = true;
			t.tex.kind = MTSGPU_TEX_BITMAP;
			t.tex.uoffset = (float) r.readFloat(); t.tex.voffset = (float) r.readFloat();
			t.tex.uscale = (float) r.readFloat(); t.tex.vscale = (float) r.readFloat();
			t.ldr.filename = r.readString();
			t.ldr.gamma = (float) r.readFloat();
			t.ldr.format = r.readInt();
			t.ldr.filterType = r.readInt();
			const uint32_t wrap = r.readUInt();
			t.ldr.maxAnisotropy = (float) r.readFloat();
			t.ldr.size = r.readUInt();
			t.ldr.offset = r.pos();
			static const uint32_t wrapOf[4] = { MTSGPU_WRAP_REPEAT, MTSGPU_WRAP_BLACK, MTSGPU_WRAP_WHITE, MTSGPU_WRAP_CLAMP };
			if (!r.ok()) {
			} else if (t.ldr.filterType < 0 || t.ldr.filterType > 2) {
				r.fail("the texture of the SpotLuminaire is an LDRTexture with unknown filter type " + std::to_string((long long) t.ldr.filterType));
			} else if (wrap > 3) {
				r.fail("the texture of the SpotLuminaire is an LDRTexture with unknown wrap mode " + std::to_string((unsigned long long) wrap));
			} else if (t.ldr.size > r.size() - t.ldr.offset) {
				r.fail("the texture of the SpotLuminaire is an LDRTexture whose encoded file (" + std::to_string((unsigned long long) t.ldr.size) + " bytes) is truncated");
			} else {
				t.ldr.wrapMode = wrapOf[wrap];
				t.bilinear = t.ldr.filterType == 2 ? 0u : 1u;                   /* MIPMap::ENone = 2; EEWA = 0, ETrilinear = 1 */
				r.setPos(t.ldr.offset + t.ldr.size);
			}
		} else {
			r.fail("the texture of the SpotLuminaire is a " + cls + ": projection textures are a Checkerboard, a GridTexture or an LDRTexture on this path"
			       + (cls == "ExrTexture" || cls == "VertexColors" ? " (this class is out of scope)" : ""));
		}
	}
	r.readSpectrum(P);
	const FloatT beamWidth = r.readFloat(), cutoffAngle = r.readFloat();
	/* m_luminaireToWorld(Point(0, 0, 0)) (transform.h:133-149): the translation column, divided by w unless it is 1 */
	FloatT x = w2l.inv.m[0][3], y = w2l.inv.m[1][3], z = w2l.inv.m[2][3];
	const FloatT w = w2l.inv.m[3][3];
	if (w != (FloatT) 1) { const FloatT rc = (FloatT) 1 / w; x *= rc; y *= rc; z *= rc; }
	P[3] = (float) x; P[4] = (float) y; P[5] = (float) z;
	P[6] = (float) std::cos(beamWidth); P[7] = (float) std::cos(cutoffAngle);
	P[8] = (float) cutoffAngle; P[9] = (float) ((FloatT) 1 / (cutoffAngle - beamWidth));
	copy3x3(P + 10, w2l.fwd);
	P[19] = (float) beamWidth;
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	if (tex) *tex = t;
	return true;
}

/* CollimatedBeamLuminaire (collimated.cpp:47-51): intensity, radius */
template <typename FloatT> inline bool parseCollimated(const uint8_t *data, size_t size, float *P, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "CollimatedBeamLuminaire");
	const Xform<FloatT> w2l = readLuminaireBase(r);
	r.readSpectrum(P);
	P[3] = (float) r.readFloat();
	copy3x4(P + 4, w2l.fwd);
	copy3x4(P + 16, w2l.inv);
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	return true;
}

/* EnvMapLuminaire (envmap.cpp:79-93): intensity scale, path, bounding sphere (after preprocess, :112-126), then the size and
 * the bytes of the EXR file.  Fills the parameter block and tells where the bitmap's bytes are; decoding them needs Mitsuba's
 * Bitmap / MIPMap and stays in gpucommon.h */
template <typename FloatT> inline bool parseEnvMapHeader(const uint8_t *data, size_t size, float *P, size_t *exrOffset, uint32_t *exrSize, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "EnvMapLuminaire");
	const Xform<FloatT> w2l = readLuminaireBase(r);
	P[0] = (float) r.readFloat();                                            /* m_intensityScale */
	r.readString();                                                          /* m_path */
	FloatT c[3]; r.readVec3(c);
	P[3] = (float) c[0]; P[4] = (float) c[1]; P[5] = (float) c[2]; P[6] = (float) r.readFloat();
	copy3x3(P + 7, w2l.fwd); copy3x3(P + 16, w2l.inv);
	*exrSize = r.readUInt();
	*exrOffset = r.pos();
	if (r.ok() && r.pos() + *exrSize > r.size()) r.fail("the environment map's bitmap is truncated");
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	return true;
}

/* SkyLuminaire (sky.cpp:121-133): Luminaire::serialize's fields, then skyScale, turbidity, thetaS, phiS, aConst .. eConst and
 * clipBelowHorizon (a bool: one byte).  Fills [0..2] and [7..22] of the block; the bounding sphere [3..6] is not serialized
 * (preprocess() takes it from the scene, sky.cpp:221-227) and is the caller's.  What configure() derives from these
 * (:139-179) is mtsgpu_sky_configure(). */
template <typename FloatT> inline bool parseSky(const uint8_t *data, size_t size, float *P, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "SkyLuminaire");
	const Xform<FloatT> w2l = readLuminaireBase(r);                          /* m_worldToLuminaire lives in the base class */
	P[0] = (float) r.readFloat(); P[1] = (float) r.readFloat();              /* m_skyScale, m_turbidity */
	P[16] = (float) r.readFloat(); P[17] = (float) r.readFloat();            /* m_thetaS, m_phiS */
	for (int k = 0; k < 5; ++k) P[18 + k] = (float) r.readFloat();           /* m_aConst .. m_eConst */
	P[2] = r.readBool() ? 1.0f : 0.0f;                                       /* m_clipBelowHorizon */
	copy3x3(P + 7, w2l.fwd);
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	return true;
}

/* Sphere (sphere.cpp:72-78) behind Shape::serialize (shape.cpp:130-138), whose nested BSDF / luminaire are skipped by seeking
 * from the END, where the sphere's own fields have a fixed size: objectToWorld, radius, centre, inverted */
template <typename FloatT> inline bool parseSphere(const uint8_t *data, size_t size, float *SP, std::string *err) {
	ByteReader<FloatT> r(data, size);
	openDetached(r, "Sphere");
	const size_t tail = 2 * 16 * sizeof(FloatT) + sizeof(FloatT) + 3 * sizeof(FloatT) + 1;
	if (r.ok() && size < tail + r.pos()) r.fail("the serialized sphere is too short");
	if (r.ok()) r.setPos(size - tail);
	const Xform<FloatT> o2w = r.readTransform();
	const FloatT radius = r.readFloat();
	FloatT c[3]; r.readVec3(c);
	const bool inverted = r.readBool();
	SP[0] = (float) c[0]; SP[1] = (float) c[1]; SP[2] = (float) c[2]; SP[3] = (float) radius;
	SP[4] = inverted ? 1.0f : 0.0f;
	copy3x3(SP + 5, o2w.fwd); copy3x3(SP + 14, o2w.inv);
	const FloatT pi = (FloatT) 3.14159265358979323846;                       /* Mitsuba's M_PI has Float's precision (constants.h:38-53) */
	SP[23] = (float) (1 / (4 * pi * radius * radius));                       /* m_invSurfaceArea (sphere.cpp:59, :69) */
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	return true;
}

/* Cylinder (cylinder.cpp:75-80) behind Shape::serialize (shape.cpp:130-138), whose nested BSDF / luminaire are skipped by seeking
 * from the END like parseSphere: the tail is a Transform (matrix and inverse), radius and length.  Then the unserialising
 * constructor's own derivation (cylinder.cpp:66-73): worldToObject = objectToWorld.inverse(), which swaps the two matrices
 * (transform.h:61-63), and m_invSurfaceArea.  D = the derived block of include/mtsgpu_cylinder.h (MTSGPU_CYLINDER_NDERIVED floats).
 * isLuminaire: what shape->isLuminaire() says; a cylinder with an area luminaire is refused here with the library's reason
 * (the nested luminaire cannot be seen from the end of the stream) */
template <typename FloatT> inline bool parseCylinder(const uint8_t *data, size_t size, bool isLuminaire, float *D, std::string *err) {
	if (isLuminaire) {
		if (err) *err = "a cylinder cannot carry an area luminaire: Cylinder has no pdfArea, and Shape::pdfArea raises an error on the first "
		                "BSDF-sampled hit (shape.cpp:174-178), so the reference cannot render it either";
		return false;
	}
	ByteReader<FloatT> r(data, size);
	openDetached(r, "Cylinder");
	const size_t tail = 2 * 16 * sizeof(FloatT) + 2 * sizeof(FloatT);
	if (r.ok() && size < tail + r.pos()) r.fail("the serialized cylinder is too short");
	if (r.ok()) r.setPos(size - tail);
	const Xform<FloatT> o2w = r.readTransform();
	const FloatT radius = r.readFloat();
	const FloatT length = r.readFloat();
	copy3x4(D, o2w.fwd); copy3x4(D + 12, o2w.inv);
	D[24] = (float) radius; D[25] = (float) length;
	const FloatT pi = (FloatT) 3.14159265358979323846;                       /* Mitsuba's M_PI has Float's precision (constants.h:38-53) */
	D[26] = (float) (1 / (2 * pi * radius * length));                        /* m_invSurfaceArea (cylinder.cpp:72) */
	D[27] = 0.0f;
	if (!r.ok()) { if (err) *err = r.error(); return false; }
	for (int j = 0; j < 4; ++j)
		if (o2w.fwd.m[3][j] != (FloatT) (j == 3 ? 1 : 0) || o2w.inv.m[3][j] != (FloatT) (j == 3 ? 1 : 0)) {
			if (err) *err = "the serialized cylinder's transform is not affine";
			return false;
		}
	return true;
}

} /* namespace mtsgpu_stream */

#endif /* MTSGPU_STREAMPARSE_H */
