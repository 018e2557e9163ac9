// uwt_launch_points.hip — dispatch of the live call's device-resident tables: the batched patch producer
// (k_patch_points_batch) and the batched table evaluation (k_table_eval).
#include "uwt_launch.h"

namespace uwt {

void launch_patch_points_batch(hipStream_t s, int n_frames, const float2* kp, const int* n_kp, const int* slots,
                               const uint16_t* depth0, size_t slot_elems, int pitch, int w, int h, float4* out, int stride,
                               int* counts) {
  hipLaunchKernelGGL(k_patch_points_batch, dim3(n_frames), dim3(256), 0, s, kp, n_kp, slots, depth0, slot_elems, pitch, w, h, out,
                     stride, counts);
}

void launch_table_eval(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, int n_pairs) {
  const bool unit = (a.zf == 1.0f && a.af == 1.0f);
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  UWT_WITH_AR(sel.arith,
    if (unit && sel.acc64) hipLaunchKernelGGL((k_table_eval<AR, true, double>), grid, blk, 0, s, a, ta);
    else if (unit) hipLaunchKernelGGL((k_table_eval<AR, true, float>), grid, blk, 0, s, a, ta);
    else if (sel.acc64) hipLaunchKernelGGL((k_table_eval<AR, false, double>), grid, blk, 0, s, a, ta);
    else hipLaunchKernelGGL((k_table_eval<AR, false, float>), grid, blk, 0, s, a, ta));
}

}  // namespace uwt
