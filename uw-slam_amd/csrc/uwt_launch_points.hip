// uwt_launch_points.hip — dispatch of the sparse point producers over a slot list, for the batched calls and the per-stage entries:
// the patch producer (k_patch_points_batch), gradient_ (k_grad_mag_slots) and the candidate producer (k_candidates_slots,
// k_scan_counts); and of the batched table evaluation (k_table_eval; k_table_hist + k_table_general).
#include "uwt_launch.h"

namespace uwt {

void launch_patch_points_batch(hipStream_t s, int n_frames, const float2* kp, const int* n_kp, const int* slots,
                               const uint16_t* depth0, size_t slot_elems, int pitch, int w, int h, float4* out, int stride,
                               int* counts) {
  hipLaunchKernelGGL(k_patch_points_batch, dim3(n_frames), dim3(256), 0, s, kp, n_kp, slots, depth0, slot_elems, pitch, w, h, out,
                     stride, counts);
}

void launch_grad_mag(hipStream_t s, const LevelK& L, int n_frames, const int* slots, const int16_t* gx, const int16_t* gy, uint8_t* mag,
                     unsigned long long* sums) {
  const int blocks = (int)std::min<size_t>(256, ((size_t)L.n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_grad_mag_slots, dim3(blocks, n_frames), dim3(kBlock), 0, s, gx, gy, L.n, L.pitch, L.iw, slots, mag, sums);
}

void launch_candidates_slots(hipStream_t s, const LevelK& L, int n_frames, const int* slots, const int16_t* gx, const int16_t* gy,
                             const uint16_t* depth, double threshold, const CandidatesWork& w, float4* out, int* counts) {
  launch_grad_mag(s, L, n_frames, slots, gx, gy, w.mag, w.sums);
  const dim3 grid((L.gw + kBlock - 1) / kBlock, w.bands, n_frames);
  hipLaunchKernelGGL(k_candidates_slots<false>, grid, dim3(kBlock), 0, s, w.mag, depth, slots, L.pitch, L.iw, L.ih, L.gw, L.gh, w.bands,
                     w.sums, threshold, w.cells, (const int*)nullptr, (float4*)nullptr);
  hipLaunchKernelGGL(k_scan_counts, dim3(n_frames), dim3(1024), 0, s, w.cells, L.gw * w.bands, w.offsets, counts);
  hipLaunchKernelGGL(k_candidates_slots<true>, grid, dim3(kBlock), 0, s, w.mag, depth, slots, L.pitch, L.iw, L.ih, L.gw, L.gh, w.bands,
                     w.sums, threshold, (int*)nullptr, (const int*)w.offsets, out);
}

void launch_table_eval(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, int n_pairs) {
  if (sel.metric) return metric::launch_table_eval(s, sel, a, ta, n_pairs);
  const bool unit = (a.zf == 1.0f && a.af == 1.0f);
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  UWT_WITH_AR(sel.arith,
    if (unit && sel.acc64) hipLaunchKernelGGL((k_table_eval<AR, true, double>), grid, blk, 0, s, a, ta);
    else if (unit) hipLaunchKernelGGL((k_table_eval<AR, true, float>), grid, blk, 0, s, a, ta);
    else if (sel.acc64) hipLaunchKernelGGL((k_table_eval<AR, false, double>), grid, blk, 0, s, a, ta);
    else hipLaunchKernelGGL((k_table_eval<AR, false, float>), grid, blk, 0, s, a, ta));
}

void launch_table_general(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, const GeneralArgs& ga,
                          int n_pairs) {
  const bool unit = (a.zf == 1.0f && a.af == 1.0f);
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  if (ga.weights) UWT_WITH_AR(sel.arith, hipLaunchKernelGGL((k_table_hist<AR>), grid, blk, 0, s, a, ta, ga));
  if (sel.metric) return metric::launch_table_general(s, sel, a, ta, ga, n_pairs);   // (behind the scale pass, which forms no Jacobian)
  UWT_WITH_AR(sel.arith,
    if (unit) hipLaunchKernelGGL((k_table_general<AR, true>), grid, blk, 0, s, a, ta, ga);
    else hipLaunchKernelGGL((k_table_general<AR, false>), grid, blk, 0, s, a, ta, ga));
}

}  // namespace uwt
