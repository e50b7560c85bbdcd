// C entry points around mtsgpu_stream::parseBSDFTable / parseBSDF with their colour-slot outputs, for
// tests/test_stream_parsers_vcol.py (built with g++ by the test; no Mitsuba).  prec = 4: Float is float, 8: double.
#include "streamparse.h"
#include <cstdio>
#include <cstring>

extern "C" int sp_parse_bsdf_table_vcol(const uint8_t *d, size_t n, int prec, uint32_t *types, float *params, uint32_t *slots, uint32_t cap_entries,
                                        uint32_t *n_entries, int *own, char *msg, size_t cap) {
	std::vector<uint32_t> t, c;
	std::vector<float> p;
	std::string err;
	*own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err, &c) : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err, &c);
	if (msg && cap) snprintf(msg, cap, "%s", *own >= 0 ? "" : err.c_str());
	*n_entries = (uint32_t) t.size();
	if (c.size() != t.size()) { if (msg && cap) snprintf(msg, cap, "%u masks for %u entries", (unsigned) c.size(), (unsigned) t.size()); return 3; }
	if (t.size() > cap_entries) { if (msg && cap) snprintf(msg, cap, "table larger than the caller's arrays"); return 2; }
	if (!t.empty()) {
		memcpy(types, t.data(), t.size() * sizeof(uint32_t)); memcpy(params, p.data(), p.size() * sizeof(float));
		memcpy(slots, c.data(), c.size() * sizeof(uint32_t));
	}
	return *own >= 0 ? 0 : 1;
}

// the same stream through a caller that takes no colour slots (parseBSDFTable without the last argument)
extern "C" int sp_parse_bsdf_table_plain(const uint8_t *d, size_t n, int prec, char *msg, size_t cap) {
	std::vector<uint32_t> t;
	std::vector<float> p;
	std::string err;
	const int own = (prec == 8) ? mtsgpu_stream::parseBSDFTable<double>(d, n, t, p, &err) : mtsgpu_stream::parseBSDFTable<float>(d, n, t, p, &err);
	if (msg && cap) snprintf(msg, cap, "%s", own >= 0 ? "" : err.c_str());
	return own >= 0 ? 0 : 1;
}
