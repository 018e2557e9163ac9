// uwt_launch_warpimg.hip — dispatch of the image-warp kernels (k_warp_scatter, k_warp_resolve, k_warp_mosaic).
#include "uwt_warpimg_kernels.h"

namespace uwt {

void launch_warp_image(hipStream_t s, const LaunchSel& sel, const WarpImageArgs& a, int n_pairs) {
  const bool dense = a.poses != nullptr;
  if (a.n > 0) {
    const dim3 grid((a.n + kBlock - 1) / kBlock, n_pairs), blk(kBlock);
    UWT_WITH_AR(sel.arith,
      if (dense) hipLaunchKernelGGL((k_warp_scatter<AR, true>), grid, blk, 0, s, a);
      else hipLaunchKernelGGL((k_warp_scatter<AR, false>), grid, blk, 0, s, a));
  }
  const int groups = (a.L.pitch / 4) * a.L.ih;
  const dim3 grid((groups + kBlock - 1) / kBlock, n_pairs), blk(kBlock);
  if (dense) hipLaunchKernelGGL((k_warp_resolve<true>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((k_warp_resolve<false>), grid, blk, 0, s, a);
}

void launch_warp_mosaic(hipStream_t s, const LevelK& L, const uint8_t* image1, const uint8_t* image2, const uint8_t* warped, uint8_t* out) {
  const int n = 4 * L.iw * L.ih;
  hipLaunchKernelGGL(k_warp_mosaic, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, L, image1, image2, warped, out);
}

}  // namespace uwt
