// uwt_launch_cloud.hip — dispatch of the point-cloud kernels (k_cloud_count, k_cloud_scan, k_cloud_write).
#include "uwt_cloud_kernels.h"

namespace uwt {

void launch_cloud(hipStream_t s, const LaunchSel& sel, const CloudArgs& a, int n_frames, bool compact) {
  const bool dense = a.tab == nullptr;
  const dim3 grid(a.bpf, n_frames), blk(kBlock);
  if (compact) {
    if (dense) hipLaunchKernelGGL((k_cloud_count<kCloudDense>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((k_cloud_count<kCloudTable>), grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), blk, 0, s, a.block_counts, a.block_base, a.bpf * n_frames);
  }
  UWT_WITH_AR(sel.arith,
    if (compact) {
      if (dense) hipLaunchKernelGGL((k_cloud_write<AR, kCloudDense, true>), grid, blk, 0, s, a);
      else hipLaunchKernelGGL((k_cloud_write<AR, kCloudTable, true>), grid, blk, 0, s, a);
    } else {
      if (dense) hipLaunchKernelGGL((k_cloud_write<AR, kCloudDense, false>), grid, blk, 0, s, a);
      else hipLaunchKernelGGL((k_cloud_write<AR, kCloudTable, false>), grid, blk, 0, s, a);
    });
}

}  // namespace uwt
