// C entry point around mtsgpu_stream::parseBSDFTable with its mask output, for tests/test_stream_parsers_mask.py (built with g++
// by the test; no Mitsuba).  prec = 4: Float is float, 8: double.  with_masks = 0: a caller that has not asked for masks.
// Per entry: mask_ints = kind, texture, reserved; mask_opacity = the three floats.  bmp_texture: the texture index of each bitmap.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table_mask(const uint8_t *d, size_t n, int prec, int with_masks, uint32_t *types, float *params, uint32_t *slots,
                                        int32_t *slot_tex, int32_t *mask_ints, float *mask_opacity, uint32_t cap_entries, uint32_t *n_entries,
                                        mtsgpu_uv_texture *textures, uint32_t cap_textures, uint32_t *n_textures, int32_t *bmp_texture,
                                        uint32_t *n_bitmaps, int *own, char *msg, size_t cap) {
	std::vector<uint32_t> t, c;
	std::vector<float> p;
	std::vector<mtsgpu_uv_texture> tex;
	std::vector<int32_t> st;
	std::vector<mtsgpu_stream::LdrTexture> bmp;
	std::vector<mtsgpu_bsdf_mask> mk;
	std::string err;
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err, &c, &tex, &st, &bmp, with_masks ? &mk : NULL)
	                   : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err, &c, &tex, &st, &bmp, with_masks ? &mk : NULL);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size(); *n_textures = (uint32_t) tex.size(); *n_bitmaps = (uint32_t) bmp.size();
	if (c.size() != t.size() || st.size() != 2 * t.size() || (with_masks && mk.size() != t.size())) {
		if (msg && cap) snprintf(msg, cap, "%u colour masks, %u slot entries and %u masks for %u entries", (unsigned) c.size(), (unsigned) st.size(), (unsigned) mk.size(), (unsigned) t.size());
		return 3;
	}
	if (t.size() > cap_entries || tex.size() > cap_textures || bmp.size() > cap_textures) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) {
		memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float));
		memcpy(slots, c.data(), c.size() * sizeof(uint32_t)); memcpy(slot_tex, st.data(), st.size() * sizeof(int32_t));
	}
	for (size_t k = 0; k < mk.size(); ++k) {
		mask_ints[3 * k] = (int32_t) mk[k].kind; mask_ints[3 * k + 1] = mk[k].texture; mask_ints[3 * k + 2] = (int32_t) mk[k].reserved;
		memcpy(mask_opacity + 3 * k, mk[k].opacity, 3 * sizeof(float));
	}
	if (!tex.empty()) memcpy(textures, tex.data(), tex.size() * sizeof(mtsgpu_uv_texture));
	for (size_t k = 0; k < bmp.size(); ++k) bmp_texture[k] = bmp[k].texture;
	return *own >= 0 ? 0 : 1;
}
