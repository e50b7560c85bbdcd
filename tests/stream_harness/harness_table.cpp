// C entry point around mtsgpu_stream::parseBSDFTable for tests/test_stream_parsers_ward.py (built with g++ by the test; no
// Mitsuba).  prec = 4: Float is float, 8: double.  The table is returned in caller-owned arrays of `cap_entries` entries.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table(const uint8_t *d, size_t n, int prec, uint32_t *types, float *params, uint32_t cap_entries,
                                   uint32_t *n_entries, int *own, char *msg, size_t cap) {
	std::vector<uint32_t> t;
	std::vector<float> p;
	std::string err;
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err) : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size();
	if (t.size() > cap_entries) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) { memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float)); }
	return *own >= 0 ? 0 : 1;
}
