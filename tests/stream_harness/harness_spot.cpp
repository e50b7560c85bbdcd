// C entry points around mtsgpu_stream::parseSpotTextured and parseSpot for tests/test_stream_parsers_spot.py (built with g++ by the
// test; no Mitsuba).  prec = 4: Float is float (SINGLE_PRECISION, the reference's default build), 8: double.
// info [8] = present, isBitmap, bilinear, wrapMode, filterType, format, offset, size; tex [12] = the words of mtsgpu_uv_texture
#include "streamparse.h"
#include <cstdio>

extern "C" int sp_parse_spot_textured(const uint8_t *d, size_t n, int prec, float *P, uint32_t *tex, uint64_t *info, float *gamma, char *msg, size_t cap) {
	std::string err;
	mtsgpu_stream::SpotTexture t;
	const bool ok = (prec == 8) ? mtsgpu_stream::parseSpotTextured<double>(d, n, P, &t, &err) : mtsgpu_stream::parseSpotTextured<float>(d, n, P, &t, &err);
	if (ok) {
		memcpy(tex, &t.tex, sizeof(t.tex));
		info[0] = t.present; info[1] = t.isBitmap; info[2] = t.bilinear; info[3] = t.ldr.wrapMode; info[4] = (uint64_t) (int64_t) t.ldr.filterType;
		info[5] = (uint64_t) (int64_t) t.ldr.format; info[6] = t.ldr.offset; info[7] = t.ldr.size;
		*gamma = t.ldr.gamma;
	}
	if (msg && cap) snprintf(msg, cap, "%s", ok ? "" : err.c_str());
	return ok ? 0 : 1;
}
extern "C" int sp_parse_spot_plain(const uint8_t *d, size_t n, int prec, float *P, char *msg, size_t cap) {
	std::string err;
	const bool ok = (prec == 8) ? mtsgpu_stream::parseSpot<double>(d, n, P, &err) : mtsgpu_stream::parseSpot<float>(d, n, P, &err);
	if (msg && cap) snprintf(msg, cap, "%s", ok ? "" : err.c_str());
	return ok ? 0 : 1;
}
