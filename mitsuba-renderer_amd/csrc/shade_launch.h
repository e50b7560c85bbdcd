// shade_launch.h -- private to the shading units: what launch_shade / launch_shade_all (shade.hip) call in the unit of each
// kernel family (shade_plain / _vcol / _tex / _tan / _mask / _snow / _cloth / _spot.hip), and the one ROUNDS x SKY ladder those units launch through.
#pragma once
#include <type_traits>
#include "kernels.h"

namespace mg {

// the arguments every k_shade* takes, with the launch they go to: a family appends its own (DColors, DTextures, DTangents, DMasks, DSnows, DCloths, DSpots)
struct ShadeBinLaunch {
	hipStream_t s; dim3 g, b;
	const DScene &sc; const DPaths &ps; const DConfig &cfg; const DQueues &q;
	const BinView &view; const BinView *views_dev; const uint32_t *bin_ids;
};
// the same for every k_shade_all*
struct ShadeAllLaunch {
	hipStream_t s; dim3 g, b;
	const DScene &sc; const DPaths &ps; const DConfig &cfg; const DQueues &q;
	const BinView *views_dev; uint32_t bin_mask;
};

// One material queue, per family.  plain: every bin.  vcol, tex: bins 0..8 (a composite's children and the terminal bin take no
// colours).  tan: bins 0..9 (the composite too, for the frame of its children).  msk: bins 0..8 (a composite takes no mask).  snw, clo: bin 0 (a snow record or a weave sits on a Lambertian entry).
// launch_shade asks for no other bin.
void launch_shade_plain(const ShadeBinLaunch &a, int bin);
void launch_shade_vcol(const ShadeBinLaunch &a, int bin, const DColors &col);
void launch_shade_tex(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex);
void launch_shade_tan(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex, const DTangents &tan);
void launch_shade_msk(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk);
void launch_shade_snw(const ShadeBinLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk, const DSnows &snw);
void launch_shade_clo(const ShadeBinLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk, const DSnows &snw,
                      const DCloths &clo);
// spt: bins 0..9, the superset family of a scene with a textured spot (colours, textures and tangents may each be absent)
void launch_shade_spt(const ShadeBinLaunch &a, int bin, const DColors &col, const DTextures &tex, const DTangents &tan, const DSpots &spt);
// All material queues of a bounce in one launch, per family
void launch_shade_all_plain(const ShadeAllLaunch &a);
void launch_shade_all_vcol(const ShadeAllLaunch &a, const DColors &col);
void launch_shade_all_tex(const ShadeAllLaunch &a, const DColors &col, const DTextures &tex);
void launch_shade_all_tan(const ShadeAllLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan);
void launch_shade_all_msk(const ShadeAllLaunch &a, const DColors &col, const DTextures &tex, const DTangents &tan, const DMasks &msk);

template <bool B> using ShadeFlag = std::integral_constant<bool, B>;
template <int BT> using ShadeBin = std::integral_constant<int, BT>;

// f(ShadeBin<BT>) for the bin's BT: 0..9, and kNumBsdfTypes for the terminal bin
template <class F>
inline void shade_for_bin(int bin, F f) {
	switch (bin) {
		case 0: f(ShadeBin<0>{}); break;
		case 1: f(ShadeBin<1>{}); break;
		case 2: f(ShadeBin<2>{}); break;
		case 3: f(ShadeBin<3>{}); break;
		case 4: f(ShadeBin<4>{}); break;
		case 5: f(ShadeBin<5>{}); break;
		case 6: f(ShadeBin<6>{}); break;
		case 7: f(ShadeBin<7>{}); break;
		case 8: f(ShadeBin<8>{}); break;
		case 9: f(ShadeBin<9>{}); break;
		default: f(ShadeBin<kNumBsdfTypes>{}); break;
	}
}

// The kernel its scene needs: the rounds of MIDirectIntegrator (DConfig::dr_mode) and / or a sky as background (DScene::sky).
// kernel(ShadeFlag<ROUNDS>, ShadeFlag<SKY>) names the instantiation; tail: what the family's kernels take after bin_ids
template <class K, class... Tail>
inline void launch_shade_rounds_sky(const ShadeBinLaunch &a, K kernel, const Tail &...tail) {
	auto go = [&](auto rounds, auto sky) {
		hipLaunchKernelGGL(kernel(rounds, sky), a.g, a.b, 0, a.s, a.sc, a.ps, a.cfg, a.q, a.view, a.views_dev, a.bin_ids, tail...);
	};
	const bool rounds = a.cfg.dr_mode != 0, sky = a.sc.sky != nullptr;
	if (rounds) { if (sky) go(ShadeFlag<true>{}, ShadeFlag<true>{}); else go(ShadeFlag<true>{}, ShadeFlag<false>{}); }
	else if (sky) go(ShadeFlag<false>{}, ShadeFlag<true>{});
	else go(ShadeFlag<false>{}, ShadeFlag<false>{});
}
// and of the fused launch: kernel(ShadeFlag<SKY>); tail: what the family's kernel takes after bin_mask
template <class K, class... Tail>
inline void launch_shade_all_sky(const ShadeAllLaunch &a, K kernel, const Tail &...tail) {
	auto go = [&](auto sky) {
		hipLaunchKernelGGL(kernel(sky), a.g, a.b, 0, a.s, a.sc, a.ps, a.cfg, a.q, a.views_dev, a.bin_mask, tail...);
	};
	if (a.sc.sky) go(ShadeFlag<true>{}); else go(ShadeFlag<false>{});
}

} // namespace mg
