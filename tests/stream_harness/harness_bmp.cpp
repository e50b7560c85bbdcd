// C entry points around mtsgpu_stream::parseBSDFTable with its bitmap output, for tests/test_stream_parsers_bmp.py (built with
// g++ by the test; no Mitsuba).  prec = 4: Float is float, 8: double.  with_bitmaps = 0: a caller that takes uv textures but
// has not asked for bitmaps.  Per bitmap: ints = texture, format, filterType, wrapMode, offset, size; floats = gamma, maxAnisotropy;
// 64 bytes of the file name.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table_bmp(const uint8_t *d, size_t n, int prec, int with_bitmaps, uint32_t *types, float *params, uint32_t *slots,
                                       int32_t *slot_tex, uint32_t cap_entries, uint32_t *n_entries, mtsgpu_uv_texture *textures, uint32_t cap_textures,
                                       uint32_t *n_textures, int64_t *bmp_ints, float *bmp_floats, char *bmp_names, uint32_t *n_bitmaps, int *own,
                                       char *msg, size_t cap) {
	std::vector<uint32_t> t, c;
	std::vector<float> p;
	std::vector<mtsgpu_uv_texture> tex;
	std::vector<int32_t> st;
	std::vector<mtsgpu_stream::LdrTexture> bmp;
	std::string err;
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err, &c, &tex, &st, with_bitmaps ? &bmp : NULL)
	                   : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err, &c, &tex, &st, with_bitmaps ? &bmp : NULL);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size(); *n_textures = (uint32_t) tex.size(); *n_bitmaps = (uint32_t) bmp.size();
	if (c.size() != t.size() || st.size() != 2 * t.size()) { if (msg && cap) snprintf(msg, cap, "%u masks and %u slot entries for %u entries", (unsigned) c.size(), (unsigned) st.size(), (unsigned) t.size()); return 3; }
	if (t.size() > cap_entries || tex.size() > cap_textures || bmp.size() > cap_textures) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) {
		memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float));
		memcpy(slots, c.data(), c.size() * sizeof(uint32_t)); memcpy(slot_tex, st.data(), st.size() * sizeof(int32_t));
	}
	if (!tex.empty()) memcpy(textures, tex.data(), tex.size() * sizeof(mtsgpu_uv_texture));
	for (size_t k = 0; k < bmp.size(); ++k) {
		const mtsgpu_stream::LdrTexture &b = bmp[k];
		int64_t *I = bmp_ints + 6 * k;
		I[0] = b.texture; I[1] = b.format; I[2] = b.filterType; I[3] = b.wrapMode; I[4] = (int64_t) b.offset; I[5] = b.size;
		bmp_floats[2 * k] = b.gamma; bmp_floats[2 * k + 1] = b.maxAnisotropy;
		snprintf(bmp_names + 64 * k, 64, "%s", b.filename.c_str());
	}
	return *own >= 0 ? 0 : 1;
}

extern "C" int sp_bsdf_slot_offset(uint32_t type, int slot) { return mtsgpu_stream::bsdfSlotOffset(type, slot); }
