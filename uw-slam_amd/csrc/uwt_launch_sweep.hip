// uwt_launch_sweep.hip — dispatch of the depth-sweep kernel (k_sweep).
#include "uwt_sweep_kernels.h"

namespace uwt {

void launch_sweep(hipStream_t s, const LaunchSel& sel, const SweepArgs& a, int n_jobs) {
  const int tiles = ((a.L.iw + kSweepTileW - 1) / kSweepTileW) * ((a.L.ih + kSweepTileH - 1) / kSweepTileH);
  const dim3 grid(tiles, n_jobs), blk(kBlock);
  UWT_WITH_AR(sel.arith, hipLaunchKernelGGL((k_sweep<AR>), grid, blk, 0, s, a));
}

}  // namespace uwt
