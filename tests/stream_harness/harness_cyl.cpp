// C entry point around mtsgpu_stream::parseCylinder for tests/test_stream_parsers_cyl.py (built with g++ by the test; no Mitsuba).
// prec = 4: Float is float (SINGLE_PRECISION, the reference's default build), 8: double.  D: MTSGPU_CYLINDER_NDERIVED floats.
#include "streamparse.h"
#include <cstdio>

extern "C" int sp_parse_cylinder(const uint8_t *d, size_t n, int prec, int is_luminaire, float *D, char *msg, size_t cap) {
	std::string err;
	const bool ok = (prec == 8) ? mtsgpu_stream::parseCylinder<double>(d, n, is_luminaire != 0, D, &err)
	                            : mtsgpu_stream::parseCylinder<float>(d, n, is_luminaire != 0, D, &err);
	if (msg && cap) snprintf(msg, cap, "%s", ok ? "" : err.c_str());
	return ok ? 0 : 1;
}
