// uwt_launch_ransac.hip — the launches of the RANSAC inlier selection: k_ransac_gather, k_ransac.
#include "uwt_ransac_kernels.h"

namespace uwt {

void launch_ransac(hipStream_t s, const RansacArgs& a, int rows) {
  const int chunks = (rows + 255) / 256;
  if (chunks > 0) hipLaunchKernelGGL(k_ransac_gather, dim3((unsigned)((size_t)a.n_pairs * chunks)), dim3(256), 0, s, a, chunks);
  hipLaunchKernelGGL(k_ransac, dim3(a.n_pairs), dim3(kRansacBlock), 0, s, a);
}

}  // namespace uwt
