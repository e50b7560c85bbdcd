// C entry point around mtsgpu_stream::parseBSDFTable with its snow output, for tests/test_stream_parsers_snow.py (built with g++
// by the test; no Mitsuba, and not linked against the library: the test hands mtsgpu_wiscombe_configure over as a pointer).
// prec = 4: Float is float, 8: double.  with_snow = 0: a caller that has not asked for the list.  Per entry: snow = kind,
// reserved and the 14 derived words, 16 words in the layout of mtsgpu_bsdf_snow; mask_kind = the kind of its mask.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table_snow(const uint8_t *d, size_t n, int prec, int with_snow, void *configure, uint32_t *types, float *params,
                                        uint32_t *snow, int32_t *mask_kind, uint32_t cap_entries, uint32_t *n_entries, int *own, char *msg, size_t cap) {
	std::vector<uint32_t> t, c;
	std::vector<float> p;
	std::vector<mtsgpu_uv_texture> tex;
	std::vector<int32_t> st;
	std::vector<mtsgpu_stream::LdrTexture> bmp;
	std::vector<mtsgpu_bsdf_mask> mk;
	std::vector<mtsgpu_bsdf_snow> sn;
	std::string err;
	mtsgpu_stream::WiscombeConfigure f = reinterpret_cast<mtsgpu_stream::WiscombeConfigure>(configure);
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err, &c, &tex, &st, &bmp, &mk, with_snow ? &sn : NULL, f)
	                   : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err, &c, &tex, &st, &bmp, &mk, with_snow ? &sn : NULL, f);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size();
	if (c.size() != t.size() || st.size() != 2 * t.size() || mk.size() != t.size() || (with_snow && sn.size() != t.size())) {
		if (msg && cap) snprintf(msg, cap, "%u colour masks, %u slot entries, %u masks and %u snow records for %u entries", (unsigned) c.size(), (unsigned) st.size(),
		                         (unsigned) mk.size(), (unsigned) sn.size(), (unsigned) t.size());
		return 3;
	}
	if (t.size() > cap_entries) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) { memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float)); }
	static_assert(sizeof(mtsgpu_bsdf_snow) == 64, "16 words per record");
	if (!sn.empty()) memcpy(snow, sn.data(), sn.size() * sizeof(mtsgpu_bsdf_snow));
	for (size_t k = 0; k < mk.size(); ++k) mask_kind[k] = (int32_t) mk[k].kind;
	return *own >= 0 ? 0 : 1;
}
