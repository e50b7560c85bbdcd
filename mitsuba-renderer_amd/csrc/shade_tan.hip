// shade_tan.hip -- the k_shade_tan / k_shade_all_tan kernels: scenes with a tangent mesh (DTangents::tri_dpdu).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_tan(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex, const DTangents &tan) {
	shade_for_bin(bin, [&](auto bt) {
		constexpr int BT = decltype(bt)::value;
		if constexpr (BT <= 9)
			launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_tan<BT, decltype(r)::value, decltype(s)::value>; }, col, tex, tan);
	});
}

void launch_shade_all_tan(const ShadeAllLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan) {
	launch_shade_all_sky(a, [](auto s) { return &k_shade_all_tan<decltype(s)::value>; }, col, tex, tan);
}

} // namespace mg
