// uwt_track_kernels.h — the joints of the chained tracking call: small kernels that keep the data of System::Tracking's stages on the
// device between them.  None of them does floating-point arithmetic: they compare, copy and count.
//   k_track_predicate      usekeypoints per pair, with the checks of a provided list the host cannot make (the record rule: SURF's or ORB's)
//   k_match_counts         device counts of a matching call clamped to what the kernels may use
//   k_good_keypoints       getGoodKeypoints on whole records, the live call's key points, the inside-level-0 check
//   k_tracking_info        the per-pair record
#pragma once

#include "uwt_track.h"

namespace uwt {

// Rule: the detector's range check of a provided record (SurfRecordRule, OrbRecordRule), taken by value.
template <typename Rule>
static __global__ __launch_bounds__(256) void k_track_predicate(int n_pairs, const Keypoint* __restrict__ prev_kp,
                                                                const int* __restrict__ n_prev, int cap, int min_matches, Rule ok,
                                                                int* __restrict__ path, int* __restrict__ refused) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = prev_kp ? n_prev[p] : 0;
  int bad = (n < 0 || n > cap) ? 1 : 0;
  const bool use = !bad && prev_kp && n >= 1 && n >= min_matches;
  if (use) {
    const Keypoint* k = prev_kp + (size_t)p * cap;
    for (int i = tid; i < n; i += 256) bad |= ok(k[i]) ? 0 : 1;
  }
  bad = __syncthreads_or(bad);
  if (tid == 0) {
    path[p] = bad ? kPathNone : (use ? kPathProvided : kPathDetect);
    refused[p] = bad ? 1 : 0;
  }
}

static __global__ __launch_bounds__(256) void k_match_counts(int n_pairs, int cap, const int* __restrict__ n_query,
                                                             const int* __restrict__ n_train, int* __restrict__ out_query,
                                                             int* __restrict__ out_train) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pairs) return;
  const int q = n_query[p], t = n_train[p];
  out_query[p] = (q < 0 || q > cap) ? 0 : q;
  out_train[p] = (t < 0 || t > cap) ? 0 : t;
}

// One block per pair.  The indices of goodMatches lie inside both sets (k_ransac refuses a pair otherwise and leaves count 0).
static __global__ __launch_bounds__(256) void k_good_keypoints(GoodKeypointsArgs a) {
  const int p = blockIdx.x, tid = threadIdx.x;
  int n = a.n_matches[p];
  n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
  const MatchOut* good = a.good + (size_t)p * a.cap;
  const SurfKeypoint* Q = a.kp_prev + (size_t)p * a.cap;
  const SurfKeypoint* T = a.kp_cur + (size_t)p * a.cap;
  const int nf = n < a.feat_stride ? n : a.feat_stride;
  int out = 0;
  for (int i = tid; i < nf; i += 256) {   // the check the host makes on the live call's key points (check_keypoints)
    const SurfKeypoint* k = Q + good[i].query_idx;
    out |= inside_level0(k->x, k->y, a.w, a.h) ? 0 : 1;
  }
  out = __syncthreads_or(out);
  if (out) {
    if (tid == 0) { a.n_matches[p] = 0; a.feat_nkp[p] = 0; a.outside[p] = 1; }
    return;
  }
  for (int i = tid; i < n; i += 256) {
    const MatchOut m = good[i];
    const SurfKeypoint kq = Q[m.query_idx], kt = T[m.train_idx];
    a.kept_prev[(size_t)p * a.cap + i] = kq;
    a.kept_cur[(size_t)p * a.cap + i] = kt;
    if (i < nf) a.feat_kp[(size_t)p * a.feat_stride + i] = make_float2(kq.x, kq.y);
  }
  if (tid == 0) { a.n_matches[p] = n; a.feat_nkp[p] = nf; a.outside[p] = 0; }
}

static __global__ __launch_bounds__(256) void k_tracking_info(TrackInfoArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.n_pairs) return;
  const RansacInfo* r = a.ransac + p;
  TrackInfo o;
  o.status = (a.refused[p] || a.outside[p]) ? a.invalid_status : r->status;
  o.used_provided = a.path[p] == kPathProvided ? 1 : 0;
  o.n_kp_prev = a.n_kp_prev[p];
  o.n_kp_cur = a.n_kp_cur[p];
  o.n_symmetric = a.n_symmetric[p];
  o.n_matches = a.n_matches[p];
  o.best_hypothesis = r->best_hypothesis;
  o.hypotheses_run = r->hypotheses_run;
  a.info[p] = o;
  if (o.status && a.stats_status) a.stats_status[(size_t)p * a.stats_stride] = o.status;
}

}  // namespace uwt
