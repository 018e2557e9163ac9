// uwt_launch_orb.hip — the launches of ORB detection and description: k_orb_layers, k_orb_fast, k_orb_rank, k_orb_select,
// k_orb_describe, k_orb_harris, k_orb_take_provided.
#include "uwt_orb_kernels.h"

namespace uwt {

void launch_orb_layers(hipStream_t s, const OrbArgs& a) {
  if (a.n_levels < 2) return;
  const int n = a.lw[1] * a.lh[1];   // the largest of the layers above 0
  if (n < 1) return;
  hipLaunchKernelGGL(k_orb_layers, dim3((unsigned)((n + kOrbBlock - 1) / kOrbBlock), (unsigned)(a.n_levels - 1), (unsigned)a.n_frames),
                     dim3(kOrbBlock), 0, s, a);
}

void launch_orb_fast(hipStream_t s, const OrbArgs& a, int level) {
  const int bw = a.lw[level] - 2 * a.edge, bh = a.lh[level] - 2 * a.edge;
  if (bw < 1 || bh < 1) return;   // the layer has no candidate band
  hipLaunchKernelGGL(k_orb_fast, dim3((unsigned)((bw + kOrbTile - 1) / kOrbTile), (unsigned)((bh + kOrbTile - 1) / kOrbTile),
                                      (unsigned)a.n_frames), dim3(kOrbBlock), 0, s, a, level);
}

void launch_orb_detect(hipStream_t s, const OrbArgs& a) {
  for (int l = 0; l < a.n_levels; l++) launch_orb_fast(s, a, l);
  hipLaunchKernelGGL(k_orb_rank, dim3((unsigned)a.n_levels, (unsigned)a.n_frames), dim3(kOrbRankBlock), 0, s, a);
  hipLaunchKernelGGL(k_orb_select, dim3((unsigned)a.n_frames), dim3(kOrbRankBlock), 0, s, a);
}

void launch_orb_describe(hipStream_t s, const OrbArgs& a, int rows) {
  if (rows < 1) return;
  hipLaunchKernelGGL(k_orb_describe, dim3((unsigned)((rows + kOrbDescWaves - 1) / kOrbDescWaves), (unsigned)a.n_frames),
                     dim3(64 * kOrbDescWaves), 0, s, a);
}

void launch_orb_take_provided(hipStream_t s, const OrbArgs& a, int j0, int n_pairs, const int* path, const OrbKeypoint* prev_kp,
                              const int* n_prev, int* mode) {
  hipLaunchKernelGGL(k_orb_take_provided, dim3((unsigned)((a.cap + 255) / 256), (unsigned)a.n_frames), dim3(256), 0, s, a, j0, n_pairs,
                     path, prev_kp, n_prev, mode);
}

void launch_orb_harris(hipStream_t s, const OrbArgs& a, int level, const int* xy, int n, long long* out) {
  if (n > 0) hipLaunchKernelGGL(k_orb_harris, dim3((unsigned)((n + kOrbBlock - 1) / kOrbBlock)), dim3(kOrbBlock), 0, s, a, level, xy, n, out);
}

}  // namespace uwt
