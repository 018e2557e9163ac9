// uwt_launch_surf.hip — the launches of SURF detection and description: k_surf_integral_rows / _cols, k_surf_response,
// k_surf_select, k_surf_describe, k_surf_response_layer, k_surf_take_provided.
#include "uwt_surf_kernels.h"

namespace uwt {

void launch_surf_integral(hipStream_t s, const SurfArgs& a) {
  hipLaunchKernelGGL(k_surf_integral_rows, dim3((unsigned)((a.h + 1 + 3) / 4), (unsigned)a.n_frames), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_surf_integral_cols, dim3((unsigned)((a.w + 255) / 256), (unsigned)a.n_frames), dim3(256), 0, s, a);
}

void launch_surf_detect(hipStream_t s, const SurfArgs& a) {
  const int small = a.w < a.h ? a.w : a.h;
  const size_t lds = (size_t)a.layers * (kSurfTile + 2) * (kSurfTile + 2) * sizeof(double);
  for (int o = 0; o < a.n_octaves; o++) {
    if (surf_filter_size(o, a.layers - 1) > small) continue;   // the largest filter does not fit: the octave is skipped
    const int gw = a.w >> o, gh = a.h >> o;
    hipLaunchKernelGGL(k_surf_response, dim3((unsigned)((gw + kSurfTile - 1) / kSurfTile), (unsigned)((gh + kSurfTile - 1) / kSurfTile),
                                             (unsigned)a.n_frames), dim3(kSurfBlock), lds, s, a, o);
  }
  hipLaunchKernelGGL(k_surf_select, dim3((unsigned)a.n_frames), dim3(kSurfSelectBlock), 0, s, a);
}

void launch_surf_response_layer(hipStream_t s, const SurfArgs& a, int octave, int layer, double* out) {
  const int n = (a.w >> octave) * (a.h >> octave);
  if (n > 0) hipLaunchKernelGGL(k_surf_response_layer, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, octave, layer, out);
}

void launch_surf_describe(hipStream_t s, const SurfArgs& a, int rows) {
  if (rows < 1) return;
  hipLaunchKernelGGL(k_surf_describe, dim3((unsigned)((rows + kSurfDescWaves - 1) / kSurfDescWaves), (unsigned)a.n_frames),
                     dim3(64 * kSurfDescWaves), 0, s, a);
}

void launch_surf_take_provided(hipStream_t s, const SurfArgs& a, int j0, int n_pairs, const int* path, const SurfKeypoint* prev_kp,
                               const int* n_prev, int* mode) {
  hipLaunchKernelGGL(k_surf_take_provided, dim3((unsigned)((a.cap + 255) / 256), (unsigned)a.n_frames), dim3(256), 0, s, a, j0, n_pairs,
                     path, prev_kp, n_prev, mode);
}

}  // namespace uwt
