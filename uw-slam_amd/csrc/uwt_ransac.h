// uwt_ransac.h — internal: the records, limits and the launcher of the RANSAC inlier selection (uwt_ransac_inliers_batch* and the
// chained tracking call; include/uwt.h states the contract).  The kernels are in uwt_ransac_kernels.h, their only launches in
// uwt_launch_ransac.hip; uwt_capi_match.hip sees this header alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "uwt_match.h"

namespace uwt {

constexpr int kRansacBlock = 256;            // hypotheses of a round: one per lane
constexpr int kRansacMaxHypotheses = 65536;  // UWT_RANSAC_MAX_HYPOTHESES
constexpr int kRansacMinSample = 8;          // matches of a sample; fewer matches: no inliers

struct RansacInfo { int status, n_inliers, best_hypothesis, hypotheses_run; double F[9]; };

// need(k) for every N in 8..kMatchMaxRows and k in 8..N, row N from ransac_need_row(N) on (entry k at + k - 8)
constexpr size_t ransac_need_row(int n) { return (size_t)(n - 8) * (size_t)(n - 7) / 2; }
constexpr size_t kRansacNeedEntries = ransac_need_row(kMatchMaxRows + 1);
// every N a call can meet when its match counts are known to the device alone: the rows of need(k) it asks for
inline std::vector<int> ransac_all_rows(int cap) {
  std::vector<int> ns;
  for (int n = kRansacMinSample; n <= cap; n++) ns.push_back(n);
  return ns;
}

struct RansacArgs {
  const MatchOut* matches;   // n_pairs x cap
  const int* n_matches;      // n_pairs
  const float* kp_prev;      // n_pairs x kp_cap records of rec_floats floats that begin with (x, y)
  const float* kp_cur;
  const int* n_kp_prev;
  const int* n_kp_cur;
  float4* quads;             // n_pairs x cap: (x, y, x', y') of every match, written by k_ransac_gather
  const int* need;           // the need(k) triangle
  int cap, kp_cap, n_pairs;
  int rec_floats;            // floats of a key-point record: 2 for the staged (x, y) tables, 8 for uwt_keypoint
  int max_hypotheses;
  uint32_t seed;
  double t2;                 // distance * distance
  int invalid_status;        // what a pair with a bad index reports (UWT_ERR_INVALID_ARG)
  unsigned char* mask;       // n_pairs x cap
  MatchOut* good;            // n_pairs x cap
  int* counts;               // n_pairs
  RansacInfo* info;          // n_pairs
};

// k_ransac_gather over `rows` matches per pair at most (0: no gather launch), then k_ransac: one block per pair
void launch_ransac(hipStream_t s, const RansacArgs& a, int rows);

}  // namespace uwt
