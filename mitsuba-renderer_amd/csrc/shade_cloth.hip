// shade_cloth.hip -- the k_shade_clo kernels: the Lambertian's queue of scenes with a woven-cloth BRDF (DCloths::bsdf_weave).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_clo(const ShadeBinLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk, const DSnows &snw,
                      const DCloths &clo) {
	launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_clo<0, decltype(r)::value, decltype(s)::value>; }, col, tex, tan, msk, snw, clo);
}

} // namespace mg
