// shade_mask.hip -- the k_shade_msk / k_shade_all_msk kernels: scenes with a mask adapter around a BSDF (DMasks::bsdf_mask).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_msk(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk) {
	shade_for_bin(bin, [&](auto bt) {
		constexpr int BT = decltype(bt)::value;
		if constexpr (BT < 9)
			launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_msk<BT, decltype(r)::value, decltype(s)::value>; }, col, tex, tan, msk);
	});
}

void launch_shade_all_msk(const ShadeAllLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk) {
	launch_shade_all_sky(a, [](auto s) { return &k_shade_all_msk<decltype(s)::value>; }, col, tex, tan, msk);
}

} // namespace mg
