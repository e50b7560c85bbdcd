// shade_spot.hip -- the k_shade_spt kernels: scenes in which a spot luminaire has a projection texture (DSpots::lum_texture).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_spt(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex, const DTangents &tan, const DSpots &spt) {
	shade_for_bin(bin, [&](auto bt) {
		constexpr int BT = decltype(bt)::value;
		if constexpr (BT < kNumBsdfTypes)
			launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_spt<BT, decltype(r)::value, decltype(s)::value>; }, col, tex, tan, spt);
	});
}

} // namespace mg
