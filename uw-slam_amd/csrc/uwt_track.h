// uwt_track.h — internal: the records and launchers of the joints of the chained tracking call (uwt_tracking_batch*; include/uwt.h
// states what the call computes).  The kernels are in uwt_track_kernels.h, their only launches in uwt_launch_track.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uwt_match.h"
#include "uwt_orb.h"
#include "uwt_ransac.h"
#include "uwt_surf.h"

namespace uwt {

// a key point (x, y) lies inside level 0 (w x h): what the live call asks of its key points (host lists: check_keypoints; the chain:
// k_good_keypoints).  Comparisons only, so a NaN fails.
__host__ __device__ inline bool inside_level0(float x, float y, float w, float h) { return x >= 0.f && x < w && y >= 0.f && y < h; }

struct TrackInfo { int status, used_provided, n_kp_prev, n_kp_cur, n_symmetric, n_matches, best_hypothesis, hypotheses_run; };

// what a detector asks of a provided record: uwt_surf_describe_batch's host check, uwt_orb_describe_batch's (on a w x h frame under the
// call's n_levels and edge_threshold)
struct SurfRecordRule {
  __host__ __device__ bool operator()(const Keypoint& k) const { return surf_keypoint_ok(k.x, k.y, k.size); }
};
struct OrbRecordRule {
  int n_levels, edge, w, h;
  __host__ __device__ bool operator()(const Keypoint& k) const { return orb_keypoint_ok(k.x, k.y, k.octave, n_levels, edge, w, h); }
};

// `usekeypoints` per pair, on the device: path[p] = kPathProvided when the previous frame is described at its provided key points
// (prev_kp != null, n_prev[p] >= 1 and >= min_matches), kPathDetect when it is detected, kPathNone — and refused[p] = 1 — when the
// provided list is unusable: a count outside 0..cap, or a record of a used list that fails the detector's rule.  One block per pair.
void launch_track_predicate(hipStream_t s, int n_pairs, const Keypoint* prev_kp, const int* n_prev, int cap, int min_matches,
                            const SurfRecordRule& rule, int* path, int* refused);
void launch_track_predicate(hipStream_t s, int n_pairs, const Keypoint* prev_kp, const int* n_prev, int cap, int min_matches,
                            const OrbRecordRule& rule, int* path, int* refused);
// the counts of a device-input matching call as the kernels may use them: a count outside 0..cap is 0
void launch_match_counts(hipStream_t s, int n_pairs, int cap, const int* n_query, const int* n_train, int* out_query, int* out_train);
struct GoodKeypointsArgs {
  const MatchOut* good;         // n_pairs x cap: goodMatches
  int* n_matches;               // n_pairs: their number; set to 0 for a pair that fails the check below
  const SurfKeypoint* kp_prev;  // n_pairs x cap: the query set's records
  const SurfKeypoint* kp_cur;   // the train set's
  SurfKeypoint* kept_prev;      // n_pairs x cap, out
  SurfKeypoint* kept_cur;
  float2* feat_kp;              // n_pairs x feat_stride: the live call's key points
  int* feat_nkp;                // n_pairs: min(count, feat_stride)
  int* outside;                 // n_pairs: 1 when one of the first feat_stride kept (x, y) lies outside level 0 (w x h)
  int cap, feat_stride, n_pairs;
  float w, h;
};
// getGoodKeypoints on whole records, the live call's key points and the inside-level-0 check.  One block per pair.
void launch_good_keypoints(hipStream_t s, const GoodKeypointsArgs& a);

struct TrackInfoArgs {
  const int* refused;           // n_pairs (k_track_predicate)
  const int* outside;           // n_pairs (k_good_keypoints)
  const int* path;
  const int* n_kp_prev;
  const int* n_kp_cur;
  const int* n_symmetric;
  const int* n_matches;
  const RansacInfo* ransac;
  TrackInfo* info;              // out
  int* stats_status;            // the status word of pair 0's uwt_stats (null: none), stats_stride ints apart: a pair whose front end
  int stats_stride;             // failed gets its status there too
  int invalid_status, n_pairs;
};
void launch_tracking_info(hipStream_t s, const TrackInfoArgs& a);

}  // namespace uwt
