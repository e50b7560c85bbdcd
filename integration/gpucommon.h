/*
 * gpucommon.h -- shared by the two reference-side bindings of libmtsgpu's C ABI (include/mtsgpu.h): the Mitsuba 0.2.1
 * integrator plugins `gpupath` (integration/gpupath.cpp, in place of src/integrators/path) and `gpudirect`
 * (integration/gpudirect.cpp, in place of src/integrators/direct).  A Mitsuba plugin exports ONE class
 * (MTS_EXPORT_PLUGIN, cobject.h:79-87), so each integrator is its own .cpp / .so and what they share lives here:
 *
 *   FlatScene        Scene / ShapeKDTree / TriMesh / Sphere / BSDFs / luminaires  ->  mtsgpu_scene
 *   GPURenderDriver  Integrator::render: upload, camera, sampler, film filter, the device group's render, and the film
 *                    handed back as ImageBlocks (Film::putImageBlock + RenderQueue::signalWorkEnd,
 *                    src/librender/renderproc.cpp:123-130)
 *
 * NOT compiled in this repository's image (Mitsuba's headers need Boost, include/mitsuba/core/util.h:22); every call
 * into Mitsuba is annotated with the file:line of the declaration it relies on.
 *
 * What of a Mitsuba scene reaches the GPU (everything else stops with an error message that names the class):
 *   shapes      every TriMesh (obj, ply, serialized, ...: TriMesh accessors), `sphere`, `cylinder` (a plain Lambertian on it, no luminaire)
 *   BSDFs       lambertian, dielectric, roughmetal, microfacet, mirror, phong, roughglass, difftrans, ward (anisotropic on
 *               spheres and on meshes with texture coordinates, whose vertex tangents travel along), twosided(any of them), composite(up to 7 of the non-delta ones, each with or without twosided);
 *               constant reflectances only (textures need uv partials and a MIPMap lookup per hit: out of scope)
 *   luminaires  area (on meshes and spheres), constant, point, spot (with a checkerboard, grid or ldrtexture projection texture; a filtered bitmap needs power-of-two sides), directional, collimated, envmap
 *   cameras     perspective (pinhole and thin lens), orthographic
 *   samplers    independent, ldsampler, stratified (keyed forms), halton, hammersley
 *   films       any (the result goes back as ImageBlocks); reconstruction filter = the film's own TabulatedFilter
 * Private members that block more: Texture2D bitmaps (BitmapTexture::m_mipmap has no accessor); every shape
 * other than TriMesh / Sphere / Cylinder (not implemented by the library, not blocked by access), media and
 * subsurface integrators (path.cpp ignores media, :31-34).
 */
#ifndef MTSGPU_GPUCOMMON_H
#define MTSGPU_GPUCOMMON_H

#include <mitsuba/render/scene.h>
#include <mitsuba/render/renderproc.h>
#include <mitsuba/render/renderjob.h>
#include <mitsuba/render/imageblock.h>
#include <mitsuba/render/triaccel.h>
#include <mitsuba/render/texture.h>
#include <mitsuba/render/mipmap.h>
#include <mitsuba/core/bitmap.h>
#include <mitsuba/core/mstream.h>
#include <mitsuba/core/plugin.h>
#include <mitsuba/core/sched.h>
#include <mtsgpu.h>
#include <mtsgpu_mask.h>
#include <mtsgpu_snow.h>
#include <mtsgpu_cloth.h>
#include <mtsgpu_cylinder.h>
#include "streamparse.h"
#include <sstream>
#include <cstdlib>

MTS_NAMESPACE_BEGIN

namespace {

/* ImageBlock keeps its alpha channel protected and has no setter (include/mitsuba/render/imageblock.h:277-297) */
class FilmBlock : public ImageBlock {
public:
	/* statistics: per-pixel variance and sample count, the test-case mode (renderproc.cpp:44-50) */
	FilmBlock(const Vector2i &maxSize, bool statistics = false) : ImageBlock(maxSize, 0, true, true, false, statistics) { }   /* imageblock.h:64-66 */
	inline void setAlpha(size_t idx, Float a) { alpha[idx] = a; }
};

inline void rgbOf(const Spectrum &s, float *out) {
	Float r, g, b;
	s.toLinearRGB(r, g, b);                      /* SPECTRUM_SAMPLES == 3: the identity (spectrum.h) */
	out[0] = (float) r; out[1] = (float) g; out[2] = (float) b;
}

inline void copyMatrix(float *dst, const Matrix4x4 &m) {
	for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) dst[4 * i + j] = (float) m.m[i][j];     /* matrix layout: transform.h */
}

/* The private parameters of BSDFs, delta / environment luminaires and spheres are read back from what the object's own
 * serialize() writes: the object goes through InstanceManager::serialize into memory (wire format,
 * src/libcore/serialization.cpp:72-85: a new object is [id][class name][its serialize()], a known one just [id], NULL is [0])
 * and the bytes are taken apart by integration/streamparse.h, which follows the field order of each class's serialize() and is
 * tested on bytes without Mitsuba (tests/test_stream_parsers.py).  Nothing is re-instantiated.
 *
 * BSDFs are serialized as they stand: they have no parent (BSDF::setParent is empty, bsdf.cpp:55-57) and their only children
 * are textures. */
inline ref<MemoryStream> serializedBSDF(const BSDF *bsdf) {
	ref<MemoryStream> stream = new MemoryStream();                            /* include/mitsuba/core/mstream.h:40 */
	ref<InstanceManager> writer = new InstanceManager();
	writer->serialize(stream, bsdf);
	return stream;
}

/* A scene-level object (a delta luminaire, the environment map, a sphere): these plugins live in their .cpp files and keep
 * every parameter private.  ConfigurableObject::serialize (properties.cpp:358-363) starts with the PARENT, which for such an
 * object is the Scene: serializing it as it stands would drag the whole scene along.  The parent pointer is public API
 * (getParent / setParent, cobject.h:40-46, properties.cpp:351-353: a plain store), so it is taken off for the duration of the
 * call and put back; render() runs on the RenderJob thread before any worker touches the scene. */
inline ref<MemoryStream> serializedDetached(ConfigurableObject *obj) {
	ConfigurableObject *parent = obj->getParent();
	obj->setParent(NULL);
	ref<MemoryStream> stream = new MemoryStream();
	ref<InstanceManager> writer = new InstanceManager();
	try {
		writer->serialize(stream, obj);                                        /* serialization.cpp:72-85: [id][class name][serialize()] */
	} catch (...) {
		obj->setParent(parent);
		throw;
	}
	obj->setParent(parent);
	return stream;
}

inline void copy3x3(float *dst, const Matrix4x4 &m) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) dst[3 * i + j] = (float) m.m[i][j];
}
inline void copy3x4(float *dst, const Matrix4x4 &m) {
	for (int i = 0; i < 3; ++i) for (int j = 0; j < 4; ++j) dst[4 * i + j] = (float) m.m[i][j];
}

/* ------------------------------------------------------------------------------------------------------------
 * FlatScene: Scene + ShapeKDTree + TriMesh + BSDF / luminaire parameter blocks -> mtsgpu_scene
 * ---------------------------------------------------------------------------------------------------------- */
struct FlatScene {
	mtsgpu_scene sc;
	std::vector<float> vtxPos, vtxNrm, shapeParams, bsdfParams, lumParams, lumInvArea, lumTriCdf, lumSelCdf, lumSelPdf;
	std::vector<float> envPixels, envPdf, envCdf;
	std::vector<uint32_t> triIdx, shapeTriOffset, shapeFlags, shapeType, kdNodes, kdIndices, triaccel, bsdfType, lumType, lumCdfOffset;
	std::vector<int32_t> shapeBsdf, shapeLum, lumShape;
	std::map<const BSDF *, int> bsdfIndex;
	/* per-vertex colours (TriMesh::getVertexColors, trimesh.h:121-126) in the order of vtxPos, one flag per shape, and per BSDF
	 * table entry the mask of its slots that hold a `vertexcolors` texture: what mtsgpu_group_set_vertex_colors takes */
	std::vector<float> vtxCol;
	std::vector<uint32_t> shapeHasColors, bsdfColorSlots;
	bool anyColors, anyColorSlots;
	/* texture coordinates (TriMesh::getVertexTexcoords, trimesh.h) in the order of vtxPos, one flag per shape, the
	 * Checkerboard / GridTexture instances of the BSDFs and per BSDF table entry the texture of its two slots (-1 = none):
	 * what mtsgpu_group_set_uv_textures takes */
	std::vector<float> vtxUv;
	std::vector<uint32_t> shapeHasUv;
	std::vector<mtsgpu_uv_texture> uvTextures;
	std::vector<int32_t> bsdfSlotTexture;
	bool anyUv;
	/* the `ldrtexture` instances with filterType none among them: what the stream says about each, its texels as
	 * LDRTexture::initializeFrom leaves them (mtsgpu_ldr_texels over Mitsuba's own decoder), and its size -- what
	 * mtsgpu_group_set_uv_bitmap_textures takes on top */
	std::vector<mtsgpu_stream::LdrTexture> ldrTextures;
	std::vector<std::vector<float> > ldrTexels;
	std::vector<uint32_t> ldrWidth, ldrHeight;
	/* per BSDF table entry the opacity of the `mask` adapter around it (none, a constant, one of uvTextures): what
	 * mtsgpu_group_set_uv_masked_textures takes on top */
	std::vector<mtsgpu_bsdf_mask> bsdfMasks;
	/* per BSDF table entry the snow record of a `wiscombe` in place of it (none: MTSGPU_SNOW_NONE): what
	 * mtsgpu_group_set_snow_bsdfs takes */
	std::vector<mtsgpu_bsdf_snow> bsdfSnow;
	/* after upload() and the colour and texture calls: hands the snow table over when a BSDF has a record */
	int setSnowBsdfs(mtsgpu_group *group) const {
		for (size_t b = 0; b < bsdfSnow.size(); ++b)
			if (bsdfSnow[b].kind != MTSGPU_SNOW_NONE) return mtsgpu_group_set_snow_bsdfs(group, ptr(bsdfSnow));
		return MTSGPU_OK;
	}
	/* the weaves of the `irawan` BSDFs and per BSDF table entry its weave (none: -1): what mtsgpu_group_set_cloth_bsdfs takes.  A
	 * cloth mesh has its tangents from Mitsuba itself: IrawanClothBRDF is EAnisotropic, so TriMesh::configure computed them */
	mtsgpu_stream::ClothTable cloth;
	/* after upload(), the colour and texture calls and setSnowBsdfs(): hands the cloth table over when a BSDF has a weave.  The
	 * cloth kernels read its.uv, so a scene whose texture call had nothing to hand over (no uv texture, no mask) first hands the
	 * texcoords of its meshes over alone; a sphere's its.uv comes from the hit point and needs none */
	int setClothBsdfs(mtsgpu_group *group) {
		if (!cloth.any()) return MTSGPU_OK;
		bool anyMask = false;
		for (size_t b = 0; b < bsdfMasks.size(); ++b) if (bsdfMasks[b].kind != MTSGPU_MASK_NONE) anyMask = true;
		if (uvTextures.empty() && !anyMask && anyUv) {
			const int rc = mtsgpu_group_set_uv_textures(group, ptr(vtxUv), ptr(shapeHasUv), 0, NULL, NULL);
			if (rc != MTSGPU_OK) return rc;
		}
		std::vector<mtsgpu_weave> weaves;
		cloth.fill(weaves);
		return mtsgpu_group_set_cloth_bsdfs(group, (uint32_t) weaves.size(), ptr(weaves), ptr(cloth.bsdfWeave));
	}
	/* vertex tangents (TriMesh::getVertexTangents, trimesh.h:136-140: TriMesh::configure computes them for a mesh whose BSDF is
	 * anisotropic, trimesh.cpp:288-290): dpdu in the order of vtxPos, one flag per shape -- what
	 * mtsgpu_group_upload_scene_tangents takes */
	std::vector<float> vtxDpdu;
	std::vector<uint32_t> shapeHasTangents;
	bool anyTangents;
	/* the derived blocks of the cylinders, [n_shapes][MTSGPU_CYLINDER_NDERIVED] with zero rows for the other shapes: what
	 * mtsgpu_group_upload_scene_cylinders takes */
	std::vector<float> cylinders;
	bool anyCylinders;

	/* the scene, with the tangents when a mesh has some; an anisotropic BSDF on a mesh that has vertex normals but no
	 * tangents (no texture coordinates: Mitsuba has stopped with an error long before) is refused by the library */
	int upload(mtsgpu_group *group) const {
		/* a scene with a cylinder takes the upload that carries the derived blocks (include/mtsgpu_cylinder.h) */
		if (anyCylinders)
			return mtsgpu_group_upload_scene_cylinders(group, &sc, anyTangents ? ptr(vtxDpdu) : NULL, anyTangents ? ptr(shapeHasTangents) : NULL, ptr(cylinders));
		if (!anyTangents) return mtsgpu_group_upload_scene(group, &sc);
		return mtsgpu_group_upload_scene_tangents(group, &sc, ptr(vtxDpdu), ptr(shapeHasTangents));
	}

	/* after upload() and setVertexColors: hands the textures over when a BSDF slot holds one (a mesh
	 * without texcoords is then shaded with uv = (0, 0), as in the reference) */
	int setUvTextures(mtsgpu_group *group) const {
		bool anyMask = false;
		for (size_t b = 0; b < bsdfMasks.size(); ++b) if (bsdfMasks[b].kind != MTSGPU_MASK_NONE) anyMask = true;
		if (uvTextures.empty() && !anyMask) return MTSGPU_OK;
		if (ldrTextures.empty() && !anyMask)      /* no bitmap: the call such a scene has always taken */
			return mtsgpu_group_set_uv_textures(group, anyUv ? ptr(vtxUv) : NULL, anyUv ? ptr(shapeHasUv) : NULL, (uint32_t) uvTextures.size(),
				&uvTextures[0], ptr(bsdfSlotTexture));
		std::vector<mtsgpu_bitmap> bitmaps(ldrTextures.size());
		std::vector<int32_t> textureBitmap(uvTextures.size(), -1);
		for (size_t k = 0; k < ldrTextures.size(); ++k) {
			bitmaps[k].width = ldrWidth[k]; bitmaps[k].height = ldrHeight[k];
			bitmaps[k].wrap_mode = ldrTextures[k].wrapMode; bitmaps[k].reserved = 0;
			bitmaps[k].texels = &ldrTexels[k][0];
			textureBitmap[ldrTextures[k].texture] = (int32_t) k;
		}
		if (anyMask)      /* a masked BSDF: the call that keeps textures and texcoords for the masks too */
			return mtsgpu_group_set_uv_masked_textures(group, anyUv ? ptr(vtxUv) : NULL, anyUv ? ptr(shapeHasUv) : NULL, (uint32_t) uvTextures.size(),
				ptr(uvTextures), ptr(bsdfSlotTexture), (uint32_t) bitmaps.size(), ptr(bitmaps), ptr(textureBitmap), ptr(bsdfMasks));
		return mtsgpu_group_set_uv_bitmap_textures(group, anyUv ? ptr(vtxUv) : NULL, anyUv ? ptr(shapeHasUv) : NULL, (uint32_t) uvTextures.size(),
			&uvTextures[0], ptr(bsdfSlotTexture), (uint32_t) bitmaps.size(), &bitmaps[0], &textureBitmap[0]);
	}

	/* the projection textures of the spot luminaires (spot.cpp:95-101): one descriptor, filter flag and -- for an `ldrtexture` --
	 * decoded bitmap per textured spot, and per luminaire its texture (-1 = none): what mtsgpu_group_set_spot_textures takes */
	std::vector<mtsgpu_uv_texture> spotTextures;
	std::vector<uint32_t> spotBilinear, spotWrap, spotWidth, spotHeight;
	std::vector<int32_t> spotTextureBitmap, lumTexture;
	std::vector<std::vector<float> > spotTexels;
	/* after upload() and every BSDF-side call (the library refuses a textured spot beside masks, snow and cloth, by name) */
	int setSpotTextures(mtsgpu_group *group) const {
		if (spotTextures.empty()) return MTSGPU_OK;
		std::vector<mtsgpu_bitmap> bitmaps(spotTexels.size());
		for (size_t k = 0; k < spotTexels.size(); ++k) {
			bitmaps[k].width = spotWidth[k]; bitmaps[k].height = spotHeight[k];
			bitmaps[k].wrap_mode = spotWrap[k]; bitmaps[k].reserved = 0;
			bitmaps[k].texels = &spotTexels[k][0];
		}
		std::vector<int32_t> perLum(lumTexture);      /* (filled up to the last textured spot: the luminaires after it have none) */
		perLum.resize(lumType.size(), -1);
		return mtsgpu_group_set_spot_textures(group, (uint32_t) spotTextures.size(), ptr(spotTextures), (uint32_t) bitmaps.size(), ptr(bitmaps),
			ptr(spotTextureBitmap), ptr(spotBilinear), ptr(perLum));
	}

	/* after upload(): hands the colours over when a mesh has some or a BSDF slot asks for them (then the
	 * library refuses a coloured slot on a shape without colours, where the reference would read an its.color nobody wrote) */
	int setVertexColors(mtsgpu_group *group) const {
		if (!anyColors && !anyColorSlots) return MTSGPU_OK;
		return mtsgpu_group_set_vertex_colors(group, anyColors ? ptr(vtxCol) : NULL, anyColors ? ptr(shapeHasColors) : NULL, ptr(bsdfColorSlots));
	}

	FlatScene(const Scene *scene) : anyColors(false), anyColorSlots(false), anyUv(false), anyTangents(false), anyCylinders(false) {
		memset(&sc, 0, sizeof(sc));
		sc.abi_version = MTSGPU_ABI_VERSION;
		const ShapeKDTree *kd = scene->getKDTree();                                   /* scene.h:498 */
		const std::vector<const Shape *> &shapes = kd->getShapes();                   /* skdtree.h:83: m_shapes order */
		const std::vector<Luminaire *> &lums = scene->getLuminaires();                /* scene.h:519 */

		/* --- luminaires first (shapes refer to them by index), Scene::m_luminaires order --- */
		std::map<const Luminaire *, int> lumIndex;
		lumParams.assign((size_t) MTSGPU_LUM_NPARAMS * lums.size(), 0.0f);
		lumShape.assign(lums.size(), -1); lumInvArea.assign(lums.size(), 0.0f);
		sc.background_lum = -1;
		for (size_t l = 0; l < lums.size(); ++l) {
			Luminaire *lum = lums[l];                                                 /* non-const: serializedDetached takes the parent off and puts it back */
			lumIndex[lum] = (int) l;
			float *P = &lumParams[(size_t) MTSGPU_LUM_NPARAMS * l];
			const std::string cls = lum->getClass()->getName();
			std::string err;
			/* area, constant and point luminaires hand their stored values out through the public evaluation interface
			 * unchanged; the others keep them private and are read back from serialize() (serializedDetached + streamparse.h) */
			if (cls == "AreaLuminaire") {
				lumType.push_back(MTSGPU_LUM_AREA);
				ShapeSamplingRecord sRec; sRec.n = Normal(0, 0, 1);
				rgbOf(lum->Le(sRec, Vector(0, 0, 1)), P);                           /* area.cpp:62-66: m_intensity when dot(d, n) > 0 */
			} else if (cls == "ConstantLuminaire") {
				lumType.push_back(MTSGPU_LUM_CONSTANT);
				rgbOf(lum->Le(Ray(Point(0, 0, 0), Vector(0, 0, 1), 0.0f)), P);      /* constant.cpp: Le(ray) = m_intensity */
				/* m_bsphere as ConstantLuminaire::preprocess derives it (constant.cpp:49-63) */
				BSphere bs = scene->getBSphere();                                   /* scene.h:273 */
				bs.radius *= 1.01f;
				if (scene->getCamera()) {
					const BSphere old = bs;
					bs.expandBy(scene->getCamera()->getPosition());                 /* bsphere.h; camera.h:83 */
					if (old != bs) bs.radius *= 1.01f;
				}
				P[3] = (float) bs.center.x; P[4] = (float) bs.center.y; P[5] = (float) bs.center.z; P[6] = (float) bs.radius;
				sc.background_lum = (int32_t) l;
			} else if (cls == "PointLuminaire") {
				lumType.push_back(MTSGPU_LUM_POINT);
				/* the public emission interface returns both stored values as they are (point.cpp:71-77) */
				EmissionRecord eRec;
				lum->sampleEmission(eRec, Point2(0.5f, 0.5f), Point2(0.5f, 0.5f));
				rgbOf(eRec.value, P);
				P[3] = (float) eRec.sRec.p.x; P[4] = (float) eRec.sRec.p.y; P[5] = (float) eRec.sRec.p.z;
			} else if (cls == "DirectionalLuminaire") {
				lumType.push_back(MTSGPU_LUM_DIRECTIONAL);
				ref<MemoryStream> st = serializedDetached(lum);                     /* directional.cpp:57-63; m_diskRadius after preprocess (:65-72) */
				if (!mtsgpu_stream::parseDirectional<Float>(st->getData(), st->getSize(), P, &err)) SLog(EError, "gpupath: %s", err.c_str());
			} else if (cls == "SpotLuminaire") {
				lumType.push_back(MTSGPU_LUM_SPOT);
				ref<MemoryStream> st = serializedDetached(lum);                     /* spot.cpp:63-70, configure() :56-62 */
				mtsgpu_stream::SpotTexture tex;
				if (!mtsgpu_stream::parseSpotTextured<Float>(st->getData(), st->getSize(), P, &tex, &err)) SLog(EError, "gpupath: %s", err.c_str());
				if (tex.present) {
					lumTexture.resize(lumType.size(), -1);
					lumTexture.back() = (int32_t) spotTextures.size();
					spotTextures.push_back(tex.tex);
					spotBilinear.push_back(tex.bilinear);
					spotTextureBitmap.push_back(-1);
					if (tex.isBitmap) {      /* the encoded file through Mitsuba's decoder and mtsgpu_ldr_texels, as decodeLdrTexture does it */
						ref<MemoryStream> file = new MemoryStream(tex.ldr.size);
						file->write(st->getData() + tex.ldr.offset, tex.ldr.size);
						file->setPos(0);
						ref<Bitmap> bitmap = new Bitmap(static_cast<Bitmap::EFileFormat>(tex.ldr.format), file);
						const uint32_t bw = (uint32_t) bitmap->getWidth(), bh = (uint32_t) bitmap->getHeight();
						std::vector<float> texels(3 * (size_t) bw * bh);
						if (bw == 0 || bh == 0 || mtsgpu_ldr_texels(bitmap->getBitsPerPixel(), bw, bh, bitmap->getData(), tex.ldr.gamma, &texels[0]) != MTSGPU_OK)
							SLog(EError, "gpupath: texture \"%s\": %s", tex.ldr.filename.c_str(), (bw == 0 || bh == 0) ? "empty bitmap" : mtsgpu_last_error(NULL));
						spotTextureBitmap.back() = (int32_t) spotTexels.size();
						spotTexels.push_back(texels); spotWidth.push_back(bw); spotHeight.push_back(bh); spotWrap.push_back(tex.ldr.wrapMode);
					}
				}
			} else if (cls == "CollimatedBeamLuminaire") {
				lumType.push_back(MTSGPU_LUM_COLLIMATED);
				ref<MemoryStream> st = serializedDetached(lum);                     /* collimated.cpp:47-51 */
				if (!mtsgpu_stream::parseCollimated<Float>(st->getData(), st->getSize(), P, &err)) SLog(EError, "gpupath: %s", err.c_str());
			} else if (cls == "EnvMapLuminaire") {
				lumType.push_back(MTSGPU_LUM_ENVMAP);
				if (sc.background_lum >= 0) SLog(EError, "gpupath: more than one background luminaire");
				sc.background_lum = (int32_t) l;
				readEnvMap(lum, P);
			} else if (cls == "SkyLuminaire") {
				lumType.push_back(MTSGPU_LUM_SKY);
				if (sc.background_lum >= 0) SLog(EError, "gpupath: more than one background luminaire");
				sc.background_lum = (int32_t) l;
				ref<MemoryStream> st = serializedDetached(lum);                     /* sky.cpp:121-133 */
				if (!mtsgpu_stream::parseSky<Float>(st->getData(), st->getSize(), P, &err)) SLog(EError, "gpupath: %s", err.c_str());
				/* SkyLuminaire::preprocess (sky.cpp:221-227): the scene's bounding sphere x 1.01f, not grown to hold the camera */
				BSphere bs = scene->getBSphere();
				bs.radius *= 1.01f;
				P[3] = (float) bs.center.x; P[4] = (float) bs.center.y; P[5] = (float) bs.center.z; P[6] = (float) bs.radius;
			} else {
				SLog(EError, "gpupath: luminaire class %s is not on this path (area, constant, point, spot, directional, collimated, "
					"envmap and sky are)", cls.c_str());
			}
		}

		/* --- shapes: primitive index space = concatenation in m_shapes order (skdtree.cpp:43-65) --- */
		shapeTriOffset.push_back(0);
		for (size_t s = 0; s < shapes.size(); ++s) {
			const Shape *shape = shapes[s];
			const bool isMesh = shape->getClass()->derivesFrom(MTS_CLASS(TriMesh));   /* skdtree.cpp:46-57 */
			shapeBsdf.push_back(bsdfOf(shape->getBSDF()));                            /* shape.h:385; NULL = not an occluder */
			shapeLum.push_back(shape->isLuminaire() ? lumIndex[shape->getLuminaire()] : -1);   /* shape.h:329-340 */
			shapeParams.insert(shapeParams.end(), MTSGPU_SHAPE_NPARAMS, 0.0f);
			cylinders.insert(cylinders.end(), MTSGPU_CYLINDER_NDERIVED, 0.0f);
			if (isMesh) {
				const TriMesh *mesh = static_cast<const TriMesh *>(shape);
				const uint32_t base = (uint32_t) (vtxPos.size() / 3);
				const Point *pos = mesh->getVertexPositions(); const Normal *nrm = mesh->getVertexNormals();   /* trimesh.h:110,115 */
				const Spectrum *col = mesh->hasVertexColors() ? mesh->getVertexColors() : NULL;               /* trimesh.h:121-126 */
				shapeHasColors.push_back(col ? 1u : 0u);
				if (col) anyColors = true;
				const Point2 *uv = mesh->hasVertexTexcoords() ? mesh->getVertexTexcoords() : NULL;
				shapeHasUv.push_back(uv ? 1u : 0u);
				if (uv) anyUv = true;
				const TangentSpace *tan = mesh->hasVertexTangents() ? mesh->getVertexTangents() : NULL;       /* trimesh.h:136-140 */
				shapeHasTangents.push_back(tan ? 1u : 0u);
				if (tan) anyTangents = true;
				for (size_t v = 0; v < mesh->getVertexCount(); ++v) {
					vtxDpdu.push_back(tan ? (float) tan[v].dpdu.x : 0.0f); vtxDpdu.push_back(tan ? (float) tan[v].dpdu.y : 0.0f);
					vtxDpdu.push_back(tan ? (float) tan[v].dpdu.z : 0.0f);
					float rgb[3] = { 0.0f, 0.0f, 0.0f };
					if (col) rgbOf(col[v], rgb);
					vtxCol.insert(vtxCol.end(), rgb, rgb + 3);
					vtxUv.push_back(uv ? (float) uv[v].x : 0.0f); vtxUv.push_back(uv ? (float) uv[v].y : 0.0f);
					vtxPos.push_back((float) pos[v].x); vtxPos.push_back((float) pos[v].y); vtxPos.push_back((float) pos[v].z);
					vtxNrm.push_back(nrm ? (float) nrm[v].x : 0.0f); vtxNrm.push_back(nrm ? (float) nrm[v].y : 0.0f); vtxNrm.push_back(nrm ? (float) nrm[v].z : 0.0f);
				}
				const Triangle *tris = mesh->getTriangles();                          /* trimesh.h:105; Triangle::idx[3], triangle.h */
				for (size_t t = 0; t < mesh->getTriangleCount(); ++t) {
					for (int k = 0; k < 3; ++k) triIdx.push_back(base + tris[t].idx[k]);
					/* TriAccel rebuilt exactly as ShapeKDTree::build does (skdtree.cpp:77-91) with the public load() */
					TriAccel ta;
					ta.load(pos[tris[t].idx[0]], pos[tris[t].idx[1]], pos[tris[t].idx[2]]);      /* triaccel.h:63 */
					ta.shapeIndex = (uint32_t) s; ta.primIndex = (uint32_t) t;
					const uint32_t *w = reinterpret_cast<const uint32_t *>(&ta);                  /* 12 dwords, triaccel.h:34-48 */
					triaccel.insert(triaccel.end(), w, w + 12);
				}
				shapeTriOffset.push_back(shapeTriOffset.back() + (uint32_t) mesh->getTriangleCount());
				shapeFlags.push_back(nrm ? MTSGPU_SHAPE_HAS_NORMALS : 0u);
				shapeType.push_back(MTSGPU_SHAPE_TRIMESH);
				if (shape->isLuminaire()) {
					/* triangle-area CDF of the emitter (trimesh.cpp:279-283) */
					const int l = lumIndex[shape->getLuminaire()];
					lumShape[l] = (int32_t) s;
					lumInvArea[l] = (float) (1 / mesh->getSurfaceArea());             /* shape.h; TriMesh::m_invSurfaceArea */
				}
			} else if (shape->getClass()->getName() == "Sphere") {
				/* one kd-tree primitive known by its AABB (skdtree.cpp:54-57,92-96).  src/shapes/sphere.cpp keeps centre,
				 * radius and transform private: read back from serialize() (:72-78) with the parent taken off.  The shape's
				 * BSDF and luminaire are nested in that stream (Shape::serialize, shape.cpp:130-138); they are skipped by
				 * seeking from the END, where the sphere's own fields have a fixed size. */
				ref<MemoryStream> st = serializedDetached(const_cast<Shape *>(shape));
				float *SP = &shapeParams[(size_t) MTSGPU_SHAPE_NPARAMS * s];
				std::string err;
				if (!mtsgpu_stream::parseSphere<Float>(st->getData(), st->getSize(), SP, &err)) SLog(EError, "gpupath: %s", err.c_str());
				/* its primitive: a TriAccel row with k = KNoTriangleFlag (skdtree.cpp:92-96), no vertices */
				TriAccel ta; memset(&ta, 0, sizeof(ta));
				ta.k = KNoTriangleFlag; ta.shapeIndex = (uint32_t) s; ta.primIndex = 0;       /* triaccel.h:34-48,28 */
				const uint32_t *w = reinterpret_cast<const uint32_t *>(&ta);
				triaccel.insert(triaccel.end(), w, w + 12);
				for (int k = 0; k < 3; ++k) triIdx.push_back(0xFFFFFFFFu);
				shapeTriOffset.push_back(shapeTriOffset.back() + 1);
				shapeFlags.push_back(0u);
				shapeType.push_back(MTSGPU_SHAPE_SPHERE);
				shapeHasColors.push_back(0u);
				shapeHasUv.push_back(0u);
				shapeHasTangents.push_back(0u);
				if (shape->isLuminaire()) {
					const int l = lumIndex[shape->getLuminaire()];
					lumShape[l] = (int32_t) s;
					lumInvArea[l] = SP[23];
				}
			} else if (shape->getClass()->getName() == "Cylinder") {
				/* one kd-tree primitive like the sphere; src/shapes/cylinder.cpp keeps its transform, radius and length private:
				 * read back from serialize() (:75-80), the constructor's derivation restated (:66-73).  The tree is Mitsuba's
				 * own, built with Cylinder::getClippedAABB */
				ref<MemoryStream> st = serializedDetached(const_cast<Shape *>(shape));
				std::string err;
				if (!mtsgpu_stream::parseCylinder<Float>(st->getData(), st->getSize(), shape->isLuminaire(),
				                                          &cylinders[(size_t) MTSGPU_CYLINDER_NDERIVED * s], &err)) SLog(EError, "gpupath: %s", err.c_str());
				anyCylinders = true;
				TriAccel ta; memset(&ta, 0, sizeof(ta));
				ta.k = KNoTriangleFlag; ta.shapeIndex = (uint32_t) s; ta.primIndex = 0;       /* triaccel.h:34-48,28 */
				const uint32_t *w = reinterpret_cast<const uint32_t *>(&ta);
				triaccel.insert(triaccel.end(), w, w + 12);
				for (int k = 0; k < 3; ++k) triIdx.push_back(0xFFFFFFFFu);
				shapeTriOffset.push_back(shapeTriOffset.back() + 1);
				shapeFlags.push_back(0u);
				shapeType.push_back(MTSGPU_SHAPE_CYLINDER);
				shapeHasColors.push_back(0u);
				shapeHasUv.push_back(0u);
				shapeHasTangents.push_back(0u);
			} else {
				SLog(EError, "gpupath: shape class %s is not on this path (triangle meshes of any loader, spheres and cylinders are)",
					shape->getClass()->getName().c_str());
			}
		}

		/* --- per-emitter triangle CDFs (DiscretePDF over triangle areas, trimesh.cpp:279-283) and the
		 *     luminaire selection CDF (weight = getSamplingWeight(), scene.cpp:320-330) --- */
		lumCdfOffset.push_back(0);
		for (size_t l = 0; l < lums.size(); ++l) {
			const int s = lumShape[l];
			if (s >= 0 && shapeType[s] == MTSGPU_SHAPE_TRIMESH) {
				const TriMesh *mesh = static_cast<const TriMesh *>(shapes[s]);
				/* DiscretePDF::build (pdf.h:82-95) restated: m_cdf is private */
				const Point *pos = mesh->getVertexPositions(); const Triangle *tris = mesh->getTriangles();
				const size_t n = mesh->getTriangleCount(), base = lumTriCdf.size();
				lumTriCdf.push_back(0.0f);
				for (size_t t = 0; t < n; ++t) lumTriCdf.push_back(lumTriCdf.back() + (float) tris[t].surfaceArea(pos));   /* triangle.h:65 */
				const float sum = lumTriCdf.back();
				for (size_t k = 0; k < n; ++k) lumTriCdf[base + k] /= sum;
				lumTriCdf[base + n] = 1.0f;
			}
			lumCdfOffset.push_back((uint32_t) lumTriCdf.size());
		}
		{
			/* Scene::m_luminairePDF (scene.cpp:320-330): weight = getSamplingWeight() (luminaire.h:180), DiscretePDF::build */
			lumSelCdf.push_back(0.0f);
			for (size_t l = 0; l < lums.size(); ++l) lumSelCdf.push_back(lumSelCdf.back() + (float) lums[l]->getSamplingWeight());
			sc.lum_sel_sum = lumSelCdf.back();
			for (size_t l = 0; l < lums.size(); ++l) {
				lumSelCdf[l] /= sc.lum_sel_sum;
				lumSelPdf.push_back((float) lums[l]->getSamplingWeight() / sc.lum_sel_sum);
			}
			lumSelCdf[lums.size()] = 1.0f;
		}

		/* --- the SAH kd-tree as Scene::initialize built it: m_nodes / m_indices are public through
		 *     sahkdtree3.h:106-108 (`using Parent::m_nodes; using Parent::m_indices;`).  The counts are protected
		 *     (gkdtree.h:2630-2631), so the node array is walked: children are adjacent and follow their parent
		 *     (gkdtree.h:1068-1138), the root is m_nodes[0]. --- */
		{
			typedef ShapeKDTree::KDNode KDNode;
			const KDNode *nodes = kd->m_nodes;
			uint32_t nNodes = 1, nIdx = 0;
			std::vector<uint32_t> stack(1, 0u);
			while (!stack.empty()) {
				const uint32_t i = stack.back(); stack.pop_back();
				const KDNode &n = nodes[i];
				if (n.isLeaf()) { nIdx = std::max(nIdx, (uint32_t) n.getPrimEnd()); continue; }          /* gkdtree.h:520-535 */
				const uint32_t left = (uint32_t) (n.getLeft() - nodes);                                    /* gkdtree.h:541-544 */
				nNodes = std::max(nNodes, left + 2);
				stack.push_back(left); stack.push_back(left + 1);
			}
			kdNodes.resize(2 * (size_t) nNodes);
			memcpy(&kdNodes[0], nodes, sizeof(KDNode) * nNodes);                     /* 8 bytes per node, relative offsets kept */
			kdIndices.assign(kd->m_indices, kd->m_indices + nIdx);
			sc.n_nodes = nNodes; sc.n_indices = nIdx;
			const AABB &box = kd->getAABB();                                         /* already enlarged, gkdtree.h:1170-1176 */
			for (int a = 0; a < 3; ++a) { sc.aabb_min[a] = (float) box.min[a]; sc.aabb_max[a] = (float) box.max[a]; }
		}

		sc.n_shapes = (uint32_t) shapes.size(); sc.n_tris = shapeTriOffset.back(); sc.n_verts = (uint32_t) (vtxPos.size() / 3);
		sc.vtx_pos = ptr(vtxPos); sc.vtx_nrm = ptr(vtxNrm); sc.tri_idx = ptr(triIdx);
		sc.shape_tri_offset = ptr(shapeTriOffset); sc.shape_bsdf = ptr(shapeBsdf); sc.shape_lum = ptr(shapeLum);
		sc.shape_flags = ptr(shapeFlags); sc.shape_type = ptr(shapeType); sc.shape_params = ptr(shapeParams);
		sc.kd_nodes = ptr(kdNodes); sc.kd_indices = ptr(kdIndices); sc.triaccel = ptr(triaccel);
		sc.n_bsdfs = (uint32_t) bsdfType.size(); sc.bsdf_type = ptr(bsdfType); sc.bsdf_params = ptr(bsdfParams);
		sc.n_lums = (uint32_t) lums.size(); sc.lum_type = ptr(lumType); sc.lum_params = ptr(lumParams); sc.lum_shape = ptr(lumShape);
		sc.lum_inv_area = ptr(lumInvArea); sc.lum_cdf_offset = ptr(lumCdfOffset); sc.lum_tri_cdf = ptr(lumTriCdf);
		sc.lum_sel_cdf = ptr(lumSelCdf); sc.lum_sel_pdf = ptr(lumSelPdf);
		sc.env_pixels = ptr(envPixels); sc.env_pdf = ptr(envPdf); sc.env_cdf = ptr(envCdf);
	}

private:
	template <typename T> static const T *ptr(const std::vector<T> &v) { return v.empty() ? NULL : &v[0]; }

	/* EnvMapLuminaire (src/luminaires/envmap.cpp): what its unserialization constructor does (:52-77) -- decode the EXR
	 * bytes serialize() carries with Mitsuba's own Bitmap, build the MIPMap with Mitsuba's own MIPMap::fromBitmap -- and
	 * what configure() does (:95-110): the luminance x sin(theta) density over level min(3, levels - 1) */
	void readEnvMap(Luminaire *lum, float *P) {
		ref<MemoryStream> st = serializedDetached(lum);
		size_t exrOffset = 0; uint32_t size = 0; std::string err;
		if (!mtsgpu_stream::parseEnvMapHeader<Float>(st->getData(), st->getSize(), P, &exrOffset, &size, &err)) SLog(EError, "gpupath: %s", err.c_str());
		ref<MemoryStream> exr = new MemoryStream(size);
		exr->write(st->getData() + exrOffset, size);                                  /* the EXR file's bytes (envmap.cpp:85-92) */
		exr->setPos(0);
		ref<Bitmap> bitmap = new Bitmap(Bitmap::EEXR, exr);                           /* bitmap.h */
		ref<MIPMap> mip = MIPMap::fromBitmap(bitmap);                                 /* mipmap.h:57 */
		sc.env_width = (uint32_t) mip->getWidth(); sc.env_height = (uint32_t) mip->getHeight();
		const Spectrum *px = mip->getImageData();                                     /* level 0, mipmap.h:78 */
		envPixels.resize((size_t) 3 * sc.env_width * sc.env_height);
		for (size_t i = 0; i < (size_t) sc.env_width * sc.env_height; ++i) rgbOf(px[i], &envPixels[3 * i]);
		const int level = std::min(3, mip->getLevels() - 1);
		const Vector2i res = mip->getLevelResolution(level);                          /* mipmap.h:84 */
		const Spectrum *coarse = mip->getImageData(level);
		sc.env_pdf_width = (uint32_t) res.x; sc.env_pdf_height = (uint32_t) res.y;
		const size_t n = (size_t) res.x * res.y;
		envPdf.resize(n); envCdf.assign(n + 1, 0.0f);
		for (int y = 0, index = 0; y < res.y; ++y) {
			const float sinFactor = std::sin(M_PI * (y + .5f) / res.y);
			for (int x = 0; x < res.x; ++x, ++index)
				envPdf[index] = (float) coarse[x + y * res.x].getLuminance() * sinFactor;
		}
		/* DiscretePDF::build (pdf.h:82-95): prefix sums, then pdf and cdf divided by the sum, last knot forced to 1 */
		for (size_t i = 0; i < n; ++i) envCdf[i + 1] = envCdf[i] + envPdf[i];
		const float sum = envCdf[n];
		for (size_t i = 0; i < n; ++i) { envPdf[i] /= sum; envCdf[i + 1] /= sum; }
		envCdf[n] = 1.0f;
	}

	/* An unfiltered `ldrtexture` the parser met in `st`: the encoded file goes through Mitsuba's own decoder, as
	 * LDRTexture(Stream *, InstanceManager *) does (ldrtexture.cpp:98-103), the decoded bytes through mtsgpu_ldr_texels, and
	 * the slots of the table entries from `firstEntry` on that show this texture receive its getAverage() = triangle(0, 0, 0)
	 * (ldrtexture.cpp:206): texel (0, 0) under repeat and clamp, and -- column 0 counts as out of range, mipmap.cpp:207 -- 0
	 * under black, 1 under white.  getMaximum() is not needed here: verifyEnergyConservation has run inside Mitsuba, and the
	 * kd / ks of the stream are its result. */
	void decodeLdrTexture(MemoryStream *st, const mtsgpu_stream::LdrTexture &t, size_t firstEntry) {
		ref<MemoryStream> file = new MemoryStream(t.size);
		file->write(st->getData() + t.offset, t.size);
		file->setPos(0);
		ref<Bitmap> bitmap = new Bitmap(static_cast<Bitmap::EFileFormat>(t.format), file);
		const uint32_t w = (uint32_t) bitmap->getWidth(), h = (uint32_t) bitmap->getHeight();
		std::vector<float> texels(3 * (size_t) w * h);
		if (w == 0 || h == 0 || mtsgpu_ldr_texels(bitmap->getBitsPerPixel(), w, h, bitmap->getData(), t.gamma, &texels[0]) != MTSGPU_OK)
			SLog(EError, "gpupath: texture \"%s\": %s", t.filename.c_str(), (w == 0 || h == 0) ? "empty bitmap" : mtsgpu_last_error(NULL));
		float average[3] = { texels[0], texels[1], texels[2] };
		if (t.wrapMode == MTSGPU_WRAP_BLACK || t.wrapMode == MTSGPU_WRAP_WHITE)
			average[0] = average[1] = average[2] = t.wrapMode == MTSGPU_WRAP_WHITE ? 1.0f : 0.0f;
		for (size_t b = firstEntry; b < bsdfType.size(); ++b)
			for (int slot = 0; slot < 2; ++slot) {
				const int o = mtsgpu_stream::bsdfSlotOffset(bsdfType[b], slot);
				if (bsdfSlotTexture[2 * b + slot] == t.texture && o >= 0)
					memcpy(&bsdfParams[MTSGPU_BSDF_NPARAMS * b + o], average, sizeof(average));
			}
		for (size_t b = firstEntry; b < bsdfMasks.size(); ++b)
			if (bsdfMasks[b].kind == MTSGPU_MASK_TEXTURE && bsdfMasks[b].texture == t.texture)
				memcpy(bsdfMasks[b].opacity, average, sizeof(average));
		ldrTexels.push_back(texels); ldrWidth.push_back(w); ldrHeight.push_back(h);
	}

	/* BSDF parameter block of one BSDF instance (shared instances are stored once) */
	int bsdfOf(const BSDF *bsdf) {
		if (!bsdf) return -1;
		std::map<const BSDF *, int>::const_iterator it = bsdfIndex.find(bsdf);
		if (it != bsdfIndex.end()) return it->second;
		/* one entry, or for a composite its children first and then the composite itself, whose block points at them */
		ref<MemoryStream> st = serializedBSDF(bsdf);
		std::string err;
		const size_t firstEntry = bsdfType.size(), firstLdr = ldrTextures.size();
		const int index = mtsgpu_stream::parseBSDFTable<Float>(st->getData(), st->getSize(), bsdfType, bsdfParams, &err, &bsdfColorSlots, &uvTextures, &bsdfSlotTexture,
			&ldrTextures, &bsdfMasks, &bsdfSnow, &mtsgpu_wiscombe_configure, &cloth);
		if (index < 0)
			SLog(EError, "gpupath: %s", err.c_str());
		for (size_t k = firstLdr; k < ldrTextures.size(); ++k)
			decodeLdrTexture(st.get(), ldrTextures[k], firstEntry);
		for (size_t b = 0; b < bsdfColorSlots.size(); ++b) if (bsdfColorSlots[b]) anyColorSlots = true;
		bsdfIndex[bsdf] = index;
		return index;
	}
};


/* What both plugins (gpupath, gpudirect) do in Integrator::render: flatten, upload, configure, render, feed the film. */
struct GPURenderDriver {
	mtsgpu_group *group;
	volatile int cancelFlag;
	std::string reduceNoteLogged;        /* the last fall-back reason that went to the log */
	std::string devices;
	uint64_t seed;

	GPURenderDriver() : group(NULL), cancelFlag(0), devices("0"), seed(0x5EED) { }
	~GPURenderDriver() { if (group) mtsgpu_group_destroy(group); }

	/* a call on the whole group reports through the group, a call on one member through that member */
	void check(int rc, mtsgpu_ctx *member = NULL) const {
		if (rc != MTSGPU_OK)
			SLog(EError, "libmtsgpu: %s", member ? mtsgpu_last_error(member) : mtsgpu_group_last_error(group));
	}

	void createGroup() {
		if (group) return;
		std::vector<int> devs;
		std::istringstream is(devices);
		for (std::string tok; std::getline(is, tok, ','); ) {
			char *end = NULL;
			const long d = strtol(tok.c_str(), &end, 10);
			if (tok.empty() || end == tok.c_str() || *end != '\0' || d < 0)
				SLog(EError, "libmtsgpu: the `devices` property must be a comma separated list of HIP device indices, got \"%s\"", devices.c_str());
			devs.push_back((int) d);
		}
		if (devs.empty()) SLog(EError, "libmtsgpu: the `devices` property names no device");
		if (mtsgpu_create_multi((int) devs.size(), &devs[0], &group) != MTSGPU_OK)
			SLog(EError, "libmtsgpu: %s", mtsgpu_last_error(NULL));              /* throws; RenderJob::run cancels the job, renderjob.cpp:126-130 */
	}

	/* direct: luminaireSamples / bsdfSamples of MIDirectIntegrator, or -1 / -1 for the path tracer */
	bool render(Scene *scene, RenderQueue *queue, const RenderJob *job, int cameraResID, int samplerResID,
			int maxDepth, int rrDepth, bool strictNormals, int luminaireSamples, int bsdfSamples) {
		ref<Scheduler> sched = Scheduler::getInstance();
		ref<Camera> camera = static_cast<Camera *>(sched->getResource(cameraResID));        /* integrator.cpp:91-96 */
		ref<Film> film = camera->getFilm();
		const Sampler *sampler = static_cast<const Sampler *>(sched->getResource(samplerResID, 0));

		createGroup();

		/* --- scene (re-uploaded per render call: the GUI edits scenes between renders) --- */
		{
			FlatScene flat(scene);
			check(flat.upload(group));
			check(flat.setVertexColors(group));
			check(flat.setUvTextures(group));
			check(flat.setSnowBsdfs(group));
			check(flat.setClothBsdfs(group));
			check(flat.setSpotTextures(group));
		}

		/* --- camera: raster space of the FULL film, crop window as offset + size (perspective.cpp:43-71, film.cpp:33-41) --- */
		mtsgpu_camera cam;
		memset(&cam, 0, sizeof(cam));
		const std::string camClass = camera->getClass()->getName();
		if (camClass != "PerspectiveCameraImpl" && camClass != "OrthographicCamera")
			SLog(EError, "libmtsgpu: camera class %s is not supported", camClass.c_str());
		const ProjectiveCamera *pc = static_cast<const ProjectiveCamera *>(camera.get());
		const Vector2i filmSize = film->getSize(), cropSize = film->getCropSize();              /* film.h:62-68 */
		const Point2i cropOffset = film->getCropOffset();
		{
			/* m_rasterToCamera is protected (perspective.cpp:69): rebuilt from the public projection transform the same
			 * way PerspectiveCameraImpl::configure builds it */
			const Float aspect = (Float) filmSize.x / (Float) filmSize.y;
			Transform screenToRaster;
			if (aspect >= 1.0f)                                                                  /* mapSmallerSide = true (camera.cpp:189) */
				screenToRaster = Transform::scale(Vector((Float) filmSize.x, (Float) filmSize.y, 1.0f))
					* Transform::scale(Vector(1 / (2 * aspect), -0.5f, 1.0f)) * Transform::translate(Vector(aspect, -1.0f, 0));
			else
				screenToRaster = Transform::scale(Vector((Float) filmSize.x, (Float) filmSize.y, 1.0f))
					* Transform::scale(Vector(0.5f, -0.5f * aspect, 1.0f)) * Transform::translate(Vector(1.0f, -1 / aspect, 0));
			const Transform rasterToCamera = pc->getProjectionTransform().inverse() * screenToRaster.inverse();   /* camera.h:204 */
			copyMatrix(cam.raster_to_camera, rasterToCamera.getMatrix());
			copyMatrix(cam.camera_to_world, camera->getInverseViewTransform().getMatrix());      /* camera.h:92 */
		}
		cam.near_clip = (float) pc->getNearClip(); cam.far_clip = (float) pc->getFarClip();      /* camera.h:220-223 */
		cam.kind = camClass == "OrthographicCamera" ? 1 : 0;
		if (cam.kind == 0) {
			const PerspectiveCamera *persp = static_cast<const PerspectiveCamera *>(camera.get());
			cam.aperture_radius = (float) persp->getApertureRadius(); cam.focus_depth = (float) persp->getFocusDepth();   /* camera.h:282-288 */
		}
		cam.width = cropSize.x; cam.height = cropSize.y;
		cam.crop_offset_x = cropOffset.x; cam.crop_offset_y = cropOffset.y;
		cam.film_width = filmSize.x; cam.film_height = filmSize.y;
		check(mtsgpu_group_set_camera(group, &cam));
		if (luminaireSamples >= 0) {
			for (int i = 0; i < mtsgpu_group_size(group); ++i)                                       /* direct.cpp:32-39 */
				check(mtsgpu_set_direct_integrator(mtsgpu_group_ctx(group, i), luminaireSamples, bsdfSamples), mtsgpu_group_ctx(group, i));
		} else {
			check(mtsgpu_group_set_integrator(group, maxDepth, rrDepth, strictNormals ? 1 : 0));     /* integrator.h:419-421 */
		}

		/* --- sampler: class, sampleCount, depth (ldsampler.cpp:45-57) --- */
		const std::string sname = sampler->getClass()->getName();
		const int skind = sname == "LowDiscrepancySampler" ? MTSGPU_SAMPLER_LD_KEYED
			: sname == "StratifiedSampler" ? MTSGPU_SAMPLER_STRATIFIED_KEYED
			: sname == "HaltonSequence" ? MTSGPU_SAMPLER_HALTON
			: sname == "HammersleySequence" ? MTSGPU_SAMPLER_HAMMERSLEY
			: MTSGPU_SAMPLER_INDEPENDENT_KEYED;
		const int depth = sampler->getProperties().getInteger("depth", 3);
		check(mtsgpu_group_set_sampler(group, skind, (uint32_t) sampler->getSampleCount(), depth, seed));

		/* --- the film's reconstruction filter: the 16x16 table Film::getTabulatedFilter() holds (rfilter.h:65-102) --- */
		const TabulatedFilter *tf = film->getTabulatedFilter();                                   /* film.h:78 */
		float table[256];
		for (int y = 0; y < 16; ++y) for (int x = 0; x < 16; ++x) table[16 * y + x] = (float) tf->lookup(x, y);
		const bool box = tf->getName() == "BoxFilter";                                            /* border-free fast path */
		check(mtsgpu_group_set_rfilter(group, (float) tf->getFilterSize().x, (float) tf->getFilterSize().y, box ? NULL : table));
		for (int i = 0; i < mtsgpu_group_size(group); ++i)
			check(mtsgpu_set_film_edges(mtsgpu_group_ctx(group, i), film->hasHighQualityEdges() ? 1 : 0), mtsgpu_group_ctx(group, i));   /* film.h:75 */

		/* --- test-case mode (`mitsuba -t`): a scene that asks for a t-test gets blocks with statistics
		 *     (renderproc.cpp:44-50); the device then runs the variance recurrence of SampleIntegrator::renderBlock
		 *     (integrator.cpp:171-202).  Like the reference, only with the box filter (renderjob.cpp:96-99): the library
		 *     refuses the render otherwise. --- */
		const bool statistics = scene->getTestType() == Scene::ETTest;                            /* scene.h:434 */
		check(mtsgpu_group_set_film_statistics(group, statistics ? 1 : 0));

		/* --- render: tiles sharded over the GPUs, films summed on GPU 0 (renderproc.cpp:123-130 in one collective) --- */
		cancelFlag = 0;
		const int bs = scene->getBlockSize();                                                     /* scene.h:543 */
		const int rc = mtsgpu_group_render(group, bs, /* ordered_reduce = */ box ? 0 : 1, &cancelFlag);
		if (rc == MTSGPU_ECANCEL) return false;
		if (rc != MTSGPU_OK) SLog(EError, "libmtsgpu: %s", mtsgpu_group_last_error(group));
		/* a collective that could not be used is not an error (the films were added up in member order instead), but
		 * the user should learn why the xGMI reduce did not run */
		const char *note = mtsgpu_group_reduce_note(group);
		if (note && note[0] && reduceNoteLogged != note) {          /* once per reason, not once per frame */
			SLog(EWarn, "libmtsgpu: film reduce fell back to the ordered sum: %s", note);
			reduceNoteLogged = note;
		}

		/* --- hand the film back as ImageBlocks: every Film plugin (exrfilm, pngfilm, mfilm) and the GUI keep working.
		 *     The sums of the crop window go out as border-less blocks: the filter has been applied already. --- */
		std::vector<float> rgbaw((size_t) cam.width * cam.height * 5);
		check(mtsgpu_read_film(mtsgpu_group_ctx(group, 0), &rgbaw[0]), mtsgpu_group_ctx(group, 0));
		std::vector<float> var3; std::vector<uint32_t> nsamp;
		if (statistics) {
			var3.resize((size_t) cam.width * cam.height * 3); nsamp.resize((size_t) cam.width * cam.height);
			check(mtsgpu_read_film_statistics(mtsgpu_group_ctx(group, 0), &var3[0], &nsamp[0]), mtsgpu_group_ctx(group, 0));
		}
		for (int y0 = 0; y0 < cam.height; y0 += bs) for (int x0 = 0; x0 < cam.width; x0 += bs) {
			ref<FilmBlock> block = new FilmBlock(Vector2i(bs, bs), statistics);
			block->setOffset(Point2i(x0 + cropOffset.x, y0 + cropOffset.y));                     /* imageblock.h:261 */
			block->setSize(Vector2i(std::min(bs, cam.width - x0), std::min(bs, cam.height - y0)));
			block->clear();
			size_t idx = 0;
			for (int y = 0; y < block->getSize().y; ++y) for (int x = 0; x < block->getSize().x; ++x, ++idx) {
				const float *p = &rgbaw[5 * ((size_t) (y0 + y) * cam.width + (x0 + x))];
				Spectrum s; s.fromLinearRGB(p[0], p[1], p[2]);
				block->setPixel(idx, s); block->setAlpha(idx, p[3]); block->setWeight(idx, p[4]);   /* spectrum, alpha, weight sums */
				if (statistics) {
					/* before putImageBlock, so that MFilm takes its statistics branch (mfilm.cpp:144-170); setVariance takes
					 * raster coordinates and subtracts the block's offset itself (imageblock.h:247-252) */
					const size_t fp = (size_t) (y0 + y) * cam.width + (x0 + x);
					Spectrum v; v.fromLinearRGB(var3[3 * fp], var3[3 * fp + 1], var3[3 * fp + 2]);
					block->setVariance(x0 + x + cropOffset.x, y0 + y + cropOffset.y, v, nsamp[fp]);
				}
			}
			film->putImageBlock(block);                                                           /* renderproc.cpp:126 */
			queue->signalWorkEnd(job, block);                                                     /* renderproc.cpp:128 */
		}
		return true;
	}
};

} /* namespace */

MTS_NAMESPACE_END
#endif /* MTSGPU_GPUCOMMON_H */
