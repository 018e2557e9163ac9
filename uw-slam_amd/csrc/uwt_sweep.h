// uwt_sweep.h — internal: the records and the launcher of the depth sweep (uwt_sweep_depth_batch*; include/uwt.h states what the call
// computes).  The kernel is in uwt_sweep_kernels.h, its only launch in uwt_launch_sweep.hip.
#pragma once

#include "uwt_launch.h"

namespace uwt {

constexpr int kSweepMaxViews = 4;
constexpr int kSweepMaxHyp = 64;
constexpr int kSweepTileW = 32, kSweepTileH = 8;   // a block's tile of the reference image: one pixel per thread of the selection pass

// uwt_sweep_info as the kernel writes it
struct SweepInfo {
  int status, n_selected, n_outcome[8];
  long long sum_cost, sum_code, reserved;
};

// One sweep over a batch of jobs.  Every plane of job j lies j * L.n elements behind job 0's.
struct SweepArgs {
  LevelK L;
  const uint8_t* img;                  // slot 0 of the level's image plane
  const int* ref_slots;                // n_jobs (device)
  const int* view_slots;               // n_jobs x n_views (device)
  const float* poses;                  // n_jobs x n_views x 7 (device)
  const uint16_t* codes;               // n_hyp (device)
  const uint8_t* mag;                  // source 1: gradient_ of job j's reference slot at mag + j * L.n; else null
  const unsigned long long* mag_sums;  // source 1: n_jobs sums of gradient_ over the image
  double threshold;
  int n_views, n_hyp, radius;
  long long poor_limit;                // max_mean_abs * (2 r + 1)^2 * n_views
  long long uniq_num, uniq_den;
  int min_parallax, refine;
  uint16_t* depth;                     // n_jobs x L.n
  uint16_t* cost;                      // n_jobs x L.n, or null
  uint8_t* outcome;                    // n_jobs x L.n, or null
  SweepInfo* info;                     // n_jobs, all-zero ahead of the launch
  int invalid_status;                  // what a job with a non-finite pose reports
};
// k_sweep on s.  Grid (tiles of the level's image, n_jobs).
void launch_sweep(hipStream_t s, const LaunchSel& sel, const SweepArgs& a, int n_jobs);

}  // namespace uwt
