// shade_snow.hip -- the k_shade_snw kernels: the Lambertian's queue of scenes with a snow BRDF (DSnows::bsdf_snow).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_snw(const ShadeBinLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk, const DSnows &snw) {
	launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_snw<0, decltype(r)::value, decltype(s)::value>; }, col, tex, tan, msk, snw);
}

} // namespace mg
