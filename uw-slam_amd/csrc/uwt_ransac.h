// uwt_ransac.h — internal: the records, limits and launchers of the RANSAC inlier selection (uwt_ransac_inliers_batch*;
// include/uwt.h states the contract).  The kernels are in uwt_ransac_kernels.h, their only launches in uwt_launch_ransac.hip;
// uwt_capi_match.hip sees this header alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uwt_match.h"

namespace uwt {

constexpr int kRansacBlock = 256;            // hypotheses of a round: one per lane
constexpr int kRansacMaxHypotheses = 65536;  // UWT_RANSAC_MAX_HYPOTHESES
constexpr int kRansacMinSample = 8;          // matches of a sample; fewer matches: no inliers

struct RansacInfo { int status, n_inliers, best_hypothesis, hypotheses_run; double F[9]; };

// need(k) for every N in 8..kMatchMaxRows and k in 8..N, row N from ransac_need_row(N) on (entry k at + k - 8)
constexpr size_t ransac_need_row(int n) { return (size_t)(n - 8) * (size_t)(n - 7) / 2; }
constexpr size_t kRansacNeedEntries = ransac_need_row(kMatchMaxRows + 1);

struct RansacArgs {
  const MatchOut* matches;   // n_pairs x cap
  const int* n_matches;      // n_pairs
  const float2* kp_prev;     // n_pairs x kp_cap
  const float2* kp_cur;
  const int* n_kp_prev;
  const int* n_kp_cur;
  float4* quads;             // n_pairs x cap: (x, y, x', y') of every match, written by k_ransac_gather
  const int* need;           // the need(k) triangle
  int cap, kp_cap, n_pairs;
  int max_hypotheses;
  uint32_t seed;
  double t2;                 // distance * distance
  int invalid_status;        // what a pair with a bad index reports (UWT_ERR_INVALID_ARG)
  unsigned char* mask;       // n_pairs x cap
  MatchOut* good;            // n_pairs x cap
  int* counts;               // n_pairs
  RansacInfo* info;          // n_pairs
};

// k_ransac_gather over `rows` matches per pair at most, then k_ransac: one block per pair
void launch_ransac(hipStream_t s, const RansacArgs& a, int rows);
// the same with the key points read from records of rec_floats floats that begin with (x, y): rec_prev / rec_cur, n_pairs x a.kp_cap
// records in device memory (a.kp_prev / a.kp_cur are not read); rows: the bound on a pair's matches (cap)
void launch_ransac_records(hipStream_t s, const RansacArgs& a, const float* rec_prev, const float* rec_cur, int rec_floats, int rows);

}  // namespace uwt
