// uwt_launch_track.hip — the launches of the chained tracking call's joints: k_track_predicate, k_match_counts,
// k_good_keypoints, k_tracking_info.
#include "uwt_track_kernels.h"

namespace uwt {

namespace {
template <typename Rule>
void track_predicate(hipStream_t s, int n_pairs, const Keypoint* prev_kp, const int* n_prev, int cap, int min_matches, const Rule& rule,
                     int* path, int* refused) {
  hipLaunchKernelGGL(k_track_predicate<Rule>, dim3((unsigned)n_pairs), dim3(256), 0, s, n_pairs, prev_kp, n_prev, cap, min_matches, rule,
                     path, refused);
}
}  // namespace

void launch_track_predicate(hipStream_t s, int n_pairs, const Keypoint* prev_kp, const int* n_prev, int cap, int min_matches,
                            const SurfRecordRule& rule, int* path, int* refused) {
  track_predicate(s, n_pairs, prev_kp, n_prev, cap, min_matches, rule, path, refused);
}
void launch_track_predicate(hipStream_t s, int n_pairs, const Keypoint* prev_kp, const int* n_prev, int cap, int min_matches,
                            const OrbRecordRule& rule, int* path, int* refused) {
  track_predicate(s, n_pairs, prev_kp, n_prev, cap, min_matches, rule, path, refused);
}

void launch_match_counts(hipStream_t s, int n_pairs, int cap, const int* n_query, const int* n_train, int* out_query, int* out_train) {
  hipLaunchKernelGGL(k_match_counts, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, n_pairs, cap, n_query, n_train, out_query,
                     out_train);
}

void launch_good_keypoints(hipStream_t s, const GoodKeypointsArgs& a) {
  hipLaunchKernelGGL(k_good_keypoints, dim3((unsigned)a.n_pairs), dim3(256), 0, s, a);
}

void launch_tracking_info(hipStream_t s, const TrackInfoArgs& a) {
  hipLaunchKernelGGL(k_tracking_info, dim3((unsigned)((a.n_pairs + 255) / 256)), dim3(256), 0, s, a);
}

}  // namespace uwt
