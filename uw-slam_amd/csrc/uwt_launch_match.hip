// uwt_launch_match.hip — the launches of descriptor matching: k_knn2 (L2 / Hamming), k_knn2_merge, k_match_filter.
#include "uwt_match_kernels.h"

namespace uwt {

void launch_knn2(hipStream_t s, int norm, const MatchArgs& a, int dirs, int rows) {
  const int tiles = (rows + kMatchTile - 1) / kMatchTile;
  const dim3 grid((unsigned)((size_t)a.n_pairs * tiles), 1, dirs * a.splits);
  const size_t lds = sizeof(uint32_t) * 2 * kMatchTile * (size_t)a.words;
  if (norm == kMatchHamming) hipLaunchKernelGGL(k_knn2<kMatchHamming>, grid, dim3(256), lds, s, a, tiles);
  else hipLaunchKernelGGL(k_knn2<kMatchL2>, grid, dim3(256), lds, s, a, tiles);
}

void launch_knn2_merge(hipStream_t s, const MatchArgs& a, int rows, Knn2* out) {
  const int chunks = (rows + 255) / 256;
  hipLaunchKernelGGL(k_knn2_merge, dim3((unsigned)((size_t)a.n_pairs * chunks)), dim3(256), 0, s, a, chunks, out);
}

void launch_match_filter(hipStream_t s, const MatchArgs& a, float ratio, MatchOut* out, int* counts) {
  hipLaunchKernelGGL(k_match_filter, dim3(a.n_pairs), dim3(1024), 0, s, a, ratio, out, counts);
}

}  // namespace uwt
