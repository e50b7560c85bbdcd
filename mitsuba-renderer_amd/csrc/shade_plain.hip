// shade_plain.hip -- the k_shade / k_shade_all kernels: scenes without a coloured or textured BSDF slot or a tangent mesh.
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_plain(const ShadeBinLaunch &a, int bin) {
	shade_for_bin(bin, [&](auto bt) {
		constexpr int BT = decltype(bt)::value;
		launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade<BT, decltype(r)::value, decltype(s)::value>; });
	});
}

void launch_shade_all_plain(const ShadeAllLaunch &a) {
	launch_shade_all_sky(a, [](auto s) { return &k_shade_all<decltype(s)::value>; });
}

} // namespace mg
