// shade.hip -- K3+K5: launch_shade / launch_shade_all pick the kernel family of the scene.  The device code is shade_bsdf.h and
// shade_path.h; each family's kernels are instantiated in a unit of their own (shade_plain / _vcol / _tex / _tan / _mask / _snow / _cloth / _spot.hip).
#include "kdevice.h"
#include "shade_launch.h"

namespace mg {

// one material queue with the kernels its scene needs: a woven-cloth BRDF (DCloths::bsdf_weave; bin 0 alone, first: the cloth kernels
// serve snow and everything below it as well), a snow BRDF (DSnows::bsdf_snow; bin 0 alone, first: the snow kernels serve
// masks, tangents, textures and colours as well), a mask adapter (DMasks::bsdf_mask; bins 0..8, first: the mask kernels serve
// tangents, textures and colours as well), a tangent mesh (DTangents::tri_dpdu; bins 0..9 -- the composite too, for
// the frame of its children), a uv-textured or a coloured BSDF slot (DTextures::bsdf_slot_texture, DColors::bsdf_color_slots;
// bins 0..8 only -- a composite's children and the terminal bin take no colours)
void launch_shade(hipStream_t s, int bin, const DScene &sc, const DPaths &ps, const DConfig &cfg,
                  const DQueues &q, const BinView &view, const BinView *views_dev, uint32_t n_bound, const uint32_t *bin_ids, const DColors &col,
                  const DTextures &tex, const DTangents &tan, const DMasks &msk, const DSnows &snw, const DCloths &clo, const DSpots &spt) {
	const uint32_t n = views_dev ? n_bound : view.prefix[kBinShards];
	if (!n) return;
	if (!bin_ids) bin_ids = q.bin(bin);
	const ShadeBinLaunch a{ s, dim3(blocks_for(n, kShadeBlock)), dim3(kShadeBlock), sc, ps, cfg, q, view, views_dev, bin_ids };
	// a textured spot (DSpots::lum_texture; bins 0..9, first: the host refuses masks, snow and cloth beside one, and the spot kernels
	// serve tangents, textures and colours as well)
	if (bin >= 0 && bin <= 9 && spt.lum_texture != nullptr) launch_shade_spt(a, bin, col, tex, tan, spt);
	else if (bin == 0 && clo.bsdf_weave != nullptr) launch_shade_clo(a, col, tex, tan, msk, snw, clo);
	else if (bin == 0 && snw.bsdf_snow != nullptr) launch_shade_snw(a, col, tex, tan, msk, snw);
	else if (bin >= 0 && bin < 9 && msk.bsdf_mask != nullptr) launch_shade_msk(a, bin, col, tex, tan, msk);
	else if (bin >= 0 && bin <= 9 && tan.tri_dpdu != nullptr) launch_shade_tan(a, bin, col, tex, tan);
	else if (bin >= 0 && bin < 9 && tex.bsdf_slot_texture != nullptr) launch_shade_tex(a, bin, col, tex);
	else if (bin >= 0 && bin < 9 && col.bsdf_color_slots != nullptr) launch_shade_vcol(a, bin, col);
	else launch_shade_plain(a, bin);
}

void launch_shade_all(hipStream_t s, const DScene &sc, const DPaths &ps, const DConfig &cfg, const DQueues &q,
                      const BinView *views_dev, uint32_t bin_mask, uint32_t n_bound, const DColors &col, const DTextures &tex,
                      const DTangents &tan, const DMasks &msk) {
	bin_mask &= kShadeAllBins;
	if (!n_bound || !bin_mask) return;
	// every bin rounds its size up to whole workgroups
	const unsigned blocks = blocks_for(n_bound, kShadeBlock) + (unsigned) __builtin_popcount(bin_mask);
	const ShadeAllLaunch a{ s, dim3(blocks), dim3(kShadeBlock), sc, ps, cfg, q, views_dev, bin_mask };
	if (msk.bsdf_mask) launch_shade_all_msk(a, col, tex, tan, msk);
	else if (tan.tri_dpdu) launch_shade_all_tan(a, col, tex, tan);
	else if (tex.bsdf_slot_texture) launch_shade_all_tex(a, col, tex);
	else if (col.bsdf_color_slots) launch_shade_all_vcol(a, col);
	else launch_shade_all_plain(a);
}

} // namespace mg
