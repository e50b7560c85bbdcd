// C entry point around mtsgpu_stream::parseBSDFTable with its cloth output, for tests/test_stream_parsers_cloth.py (built with g++
// by the test; no Mitsuba, and not linked against the library).  prec = 4: Float is float, 8: double.  with_cloth = 0: a caller
// that has not asked for the table.  Per entry: bsdf_weave.  Per weave, through ClothTable::fill: 24 words = the 18 scalars of
// mtsgpu_weave, n_pattern, n_yarns, then 0 / 1 for each of its two pointers, and two words of zero; the pattern words and the
// yarns (14 words each) of all weaves one behind the other.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table_cloth(const uint8_t *d, size_t n, int prec, int with_cloth, uint32_t *types, float *params, int32_t *bsdf_weave,
                                         uint32_t cap_entries, uint32_t *n_entries, uint32_t *weaves, uint32_t cap_weaves, uint32_t *n_weaves,
                                         uint32_t *pattern, uint32_t *yarns, uint32_t cap_words, int *own, char *msg, size_t cap) {
	std::vector<uint32_t> t, c;
	std::vector<float> p;
	std::vector<mtsgpu_uv_texture> tex;
	std::vector<int32_t> st;
	std::vector<mtsgpu_stream::LdrTexture> bmp;
	std::vector<mtsgpu_bsdf_mask> mk;
	std::vector<mtsgpu_bsdf_snow> sn;
	mtsgpu_stream::ClothTable cl;
	std::string err;
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err, &c, &tex, &st, &bmp, &mk, &sn, NULL, with_cloth ? &cl : NULL)
	                   : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err, &c, &tex, &st, &bmp, &mk, &sn, NULL, with_cloth ? &cl : NULL);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size();
	*n_weaves = (uint32_t) cl.weaves.size();
	if (c.size() != t.size() || st.size() != 2 * t.size() || mk.size() != t.size() || sn.size() != t.size() || (with_cloth && cl.bsdfWeave.size() != t.size())) {
		if (msg && cap) snprintf(msg, cap, "%u colour masks, %u slot entries, %u masks, %u snow records and %u weave indices for %u entries", (unsigned) c.size(),
		                         (unsigned) st.size(), (unsigned) mk.size(), (unsigned) sn.size(), (unsigned) cl.bsdfWeave.size(), (unsigned) t.size());
		return 3;
	}
	if (t.size() > cap_entries || cl.weaves.size() > cap_weaves) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) { memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float)); }
	for (size_t i = 0; i < cl.bsdfWeave.size(); ++i) bsdf_weave[i] = cl.bsdfWeave[i];
	std::vector<mtsgpu_weave> arr;
	cl.fill(arr);
	size_t np = 0, ny = 0;
	for (size_t k = 0; k < arr.size(); ++k) {
		uint32_t *o = weaves + 24 * k;
		memcpy(o, &arr[k], 20 * sizeof(uint32_t));
		o[20] = arr[k].pattern != NULL; o[21] = arr[k].yarns != NULL; o[22] = o[23] = 0;
		if (np + arr[k].n_pattern > cap_words || 14 * (ny + arr[k].n_yarns) > cap_words) { if (msg && cap) snprintf(msg, cap, "pool larger than the caller's arrays"); return 2; }
		if (arr[k].n_pattern) memcpy(pattern + np, arr[k].pattern, arr[k].n_pattern * sizeof(uint32_t));
		if (arr[k].n_yarns) memcpy(yarns + 14 * ny, arr[k].yarns, arr[k].n_yarns * sizeof(mtsgpu_yarn));
		np += arr[k].n_pattern; ny += arr[k].n_yarns;
	}
	return 0;
}
