// C entry point around mtsgpu_stream::parseSky for tests/test_stream_parsers_sky.py (built with g++ by the test; no Mitsuba).
// prec = 4: Float is float, 8: double.  P: MTSGPU_LUM_NPARAMS floats, zeroed by the caller.
#include "streamparse.h"
#include <cstdio>

extern "C" int sp_parse_sky(const uint8_t *d, size_t n, int prec, float *P, char *msg, size_t cap) {
	std::string err;
	const bool ok = (prec == 8) ? mtsgpu_stream::parseSky<double>(d, n, P, &err) : mtsgpu_stream::parseSky<float>(d, n, P, &err);
	if (msg && cap) snprintf(msg, cap, "%s", ok ? "" : err.c_str());
	return ok ? 0 : 1;
}
