// shade_vcol.hip -- the k_shade_vcol / k_shade_all_vcol kernels: scenes with a coloured BSDF slot (DColors::bsdf_color_slots).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_vcol(const ShadeBinLaunch &a, int bin, const DColors &col) {
	shade_for_bin(bin, [&](auto bt) {
		constexpr int BT = decltype(bt)::value;
		if constexpr (BT < 9)
			launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_vcol<BT, decltype(r)::value, decltype(s)::value>; }, col);
	});
}

void launch_shade_all_vcol(const ShadeAllLaunch &a, const DColors &col) {
	launch_shade_all_sky(a, [](auto s) { return &k_shade_all_vcol<decltype(s)::value>; }, col);
}

} // namespace mg
