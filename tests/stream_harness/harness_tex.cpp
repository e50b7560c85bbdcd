// C entry points around mtsgpu_stream::parseBSDFTable with its uv-texture outputs, for tests/test_stream_parsers_tex.py
// (built with g++ by the test; no Mitsuba).  prec = 4: Float is float, 8: double.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table_tex(const uint8_t *d, size_t n, int prec, uint32_t *types, float *params, uint32_t *slots, int32_t *slot_tex,
                                       uint32_t cap_entries, uint32_t *n_entries, mtsgpu_uv_texture *textures, uint32_t cap_textures,
                                       uint32_t *n_textures, int *own, char *msg, size_t cap) {
	std::vector<uint32_t> t, c;
	std::vector<float> p;
	std::vector<mtsgpu_uv_texture> tex;
	std::vector<int32_t> st;
	std::string err;
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err, &c, &tex, &st)
	                   : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err, &c, &tex, &st);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size(); *n_textures = (uint32_t) tex.size();
	if (c.size() != t.size() || st.size() != 2 * t.size()) { if (msg && cap) snprintf(msg, cap, "%u masks and %u slot entries for %u entries", (unsigned) c.size(), (unsigned) st.size(), (unsigned) t.size()); return 3; }
	if (t.size() > cap_entries || tex.size() > cap_textures) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) {
		memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float));
		memcpy(slots, c.data(), c.size() * sizeof(uint32_t)); memcpy(slot_tex, st.data(), st.size() * sizeof(int32_t));
	}
	if (!tex.empty()) memcpy(textures, tex.data(), tex.size() * sizeof(mtsgpu_uv_texture));
	return *own >= 0 ? 0 : 1;
}
