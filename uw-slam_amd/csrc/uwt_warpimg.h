// uwt_warpimg.h — internal: the records and launchers of Tracker::ObtainImageTransformed and DebugShowWarpedPerspective on the device
// (uwt_obtain_image_transformed, uwt_warp_image_batch*, uwt_warp_mosaic; include/uwt.h states what the calls compute).  The kernels
// are in uwt_warpimg_kernels.h, their only launches in uwt_launch_warpimg.hip.
#pragma once

#include "uwt_launch.h"

namespace uwt {

// uwt_warp_quality as the kernels write it
struct WarpQuality {
  int status, n_points, n_landed, n_covered;
  long long sum_abs, sum_sq, sum_abs_unaligned, reserved;
};

// One scatter + resolve over a batch of pairs.  Every plane of pair p lies p * L.n elements behind pair 0's (winner: int32 words).
struct WarpImageArgs {
  LevelK L;
  const uint8_t* img;        // slot 0 of the level's image plane
  const uint16_t* depth;     // slot 0 of the level's depth plane, or null (dense form)
  const int* ref_slots;      // n_pairs (device): the frame `original` is read from
  const int* tgt_slots;      // n_pairs (device), or null: no image2 (no absdiff, no sums)
  const float* poses;        // n_pairs x 7 (device): the dense form; null: the explicit form
  const float4* pts;         // explicit form: the table (n rows) and its warped rows
  const float4* warped_pts;
  int n;                     // rows per pair: explicit n, dense gw * gh
  int* winner;               // n_pairs x L.n, all -1 ahead of the scatter
  uint8_t* warped;           // n_pairs x L.n, or null
  uint8_t* valid;            // n_pairs x L.n, or null
  uint8_t* absdiff;          // n_pairs x L.n, or null
  WarpQuality* quality;      // n_pairs, all-zero ahead of the scatter; or null
  int keep;                  // 1: pixels no row lands on keep what `warped` held (uwt_obtain_image_transformed); 0: they become 0
  int invalid_status;        // what a pair with a non-finite pose reports
};
// k_warp_scatter then k_warp_resolve on s (a.n == 0: the resolve alone).  Grid (blocks, n_pairs).
void launch_warp_image(hipStream_t s, const LaunchSel& sel, const WarpImageArgs& a, int n_pairs);
// k_warp_mosaic: image1, image2, warped are pitched planes of the level, out 2 iw x 2 ih tight
void launch_warp_mosaic(hipStream_t s, const LevelK& L, const uint8_t* image1, const uint8_t* image2, const uint8_t* warped, uint8_t* out);

}  // namespace uwt
