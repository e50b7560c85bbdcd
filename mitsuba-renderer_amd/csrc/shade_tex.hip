// shade_tex.hip -- the k_shade_tex / k_shade_all_tex kernels: scenes with a uv-textured BSDF slot (DTextures::bsdf_slot_texture).
#include "shade_path.h"
#include "shade_launch.h"

namespace mg {

void launch_shade_tex(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex) {
	shade_for_bin(bin, [&](auto bt) {
		constexpr int BT = decltype(bt)::value;
		if constexpr (BT < 9)
			launch_shade_rounds_sky(a, [](auto r, auto s) { return &k_shade_tex<BT, decltype(r)::value, decltype(s)::value>; }, col, tex);
	});
}

void launch_shade_all_tex(const ShadeAllLaunch &a, const DColors &col, const DTextures &tex) {
	launch_shade_all_sky(a, [](auto s) { return &k_shade_all_tex<decltype(s)::value>; }, col, tex);
}

} // namespace mg
