// uwt_capi_tracking.hip — host side of libuwt_hip.so: System::Tracking for a batch of pairs as one chain on the device.  Every stage
// is the existing one (SURF, the matcher, the RANSAC selection, the live call), entered through its device-input form; the joints
// between them are the kernels of uwt_track_kernels.h.  Nothing here reads a result back: the asynchronous call only enqueues.
#include "uwt_ctx.h"
#include "uwt_track.h"

namespace {

static_assert(sizeof(uwt_tracking_params) == 56, "uwt_tracking_params layout");
static_assert(sizeof(uwt_tracking_info) == 32 && sizeof(TrackInfo) == sizeof(uwt_tracking_info), "uwt_tracking_info layout");
static_assert(sizeof(uwt_stats) % sizeof(int) == 0 && offsetof(uwt_stats, status) == 0, "uwt_stats: the status word first");

constexpr int kTrackFeatKeypoints = 200;   // key points the live call takes (kPatchMaxKeypoints: the stride of the context's feat_kp)

// the call's scratch: [paths | refused | outside | counts (query sides, then train sides) | symMatch counts | RANSAC records |
// key points (query sides, then train sides) | symMatches | descriptors]
struct TrackLayout { size_t path, refused, outside, counts, n_sym, rinfo, kp, sym, desc; };
TrackLayout track_carve(Carve& cv, int n_pairs, int cap) {
  TrackLayout l;
  const size_t n = (size_t)n_pairs;
  l.path = cv.take<int>(n);
  l.refused = cv.take<int>(n);
  l.outside = cv.take<int>(n);
  l.counts = cv.take<int>(2 * n);
  l.n_sym = cv.take<int>(n);
  l.rinfo = cv.take<uwt_ransac_info>(n);
  l.kp = cv.take<uwt_keypoint>(2 * n * cap);
  l.sym = cv.take<uwt_match>(n * cap);
  l.desc = cv.take<float>(2 * n * cap * 64);
  return l;
}

// the synchronous form's inputs and results, carved behind the call's own
struct TrackIoLayout { size_t prev_kp, n_prev, poses, stats, info, good, kept_prev, kept_cur, n_matches; };
TrackIoLayout track_io_carve(Carve& cv, int n_pairs, int cap) {
  TrackIoLayout l;
  const size_t n = (size_t)n_pairs;
  l.prev_kp = cv.take<uwt_keypoint>(n * cap);
  l.n_prev = cv.take<int>(n);
  l.poses = cv.take<float>(7 * n);
  l.stats = cv.take<uwt_stats>(n);
  l.info = cv.take<uwt_tracking_info>(n);
  l.good = cv.take<uwt_match>(n * cap);
  l.kept_prev = cv.take<uwt_keypoint>(n * cap);
  l.kept_cur = cv.take<uwt_keypoint>(n * cap);
  l.n_matches = cv.take<int>(n);
  return l;
}

// Every check the host can make; nothing is enqueued and no buffer grows when one fails.  *tp: the parameters in force.
int tracking_check(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                   const uwt_tracking_params* params, int cap, bool has_prev_kp, bool has_n_prev, uwt_tracking_params* tp) {
  if (!ref_slots || !tgt_slots) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list");
  if (n_pairs < 1 || n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_pairs outside 1..max_pairs");
  if (params) *tp = *params;
  else uwt_default_tracking_params(tp);
  uwt_surf_params sp;
  int st = surf_check(c, what, n_pairs, ref_slots, cap, &tp->surf, &sp);
  if (!st) st = surf_check(c, what, n_pairs, tgt_slots, cap, &tp->surf, &sp);
  if (st) return st;
  if (!ransac_params_ok(tp->ransac)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": distance, confidence or max_hypotheses outside its range");
  if (!std::isfinite(tp->ratio)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": ratio is not finite");
  if (tp->min_matches < 0) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": min_matches < 0");
  if (has_prev_kp != has_n_prev) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": exactly one of the provided key points and their counts is null");
  return UWT_OK;
}

// The chain, enqueued on the context stream (the arguments have passed tracking_check; the scratch holds `l` at its base).
int tracking_enqueue(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                     const uwt_tracking_params& tp, int cap, const TrackLayout& l, const uwt_tracking_io& io) {
  void* b = c->track_buf.p;
  int* d_path = Carve::at<int>(b, l.path);
  int* d_refused = Carve::at<int>(b, l.refused);
  int* d_outside = Carve::at<int>(b, l.outside);
  int* d_counts = Carve::at<int>(b, l.counts);
  int* d_n_sym = Carve::at<int>(b, l.n_sym);
  uwt_ransac_info* d_rinfo = Carve::at<uwt_ransac_info>(b, l.rinfo);
  uwt_keypoint* d_kp = Carve::at<uwt_keypoint>(b, l.kp);
  uwt_match* d_sym = Carve::at<uwt_match>(b, l.sym);
  float* d_desc = Carve::at<float>(b, l.desc);
  const size_t side = (size_t)n_pairs * cap;   // records of one side of the batch

  int st = features_device_begin(c, what, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  // 1. usekeypoints, per pair
  launch_track_predicate(c->stream, n_pairs, reinterpret_cast<const SurfKeypoint*>(io.d_prev_kp), io.d_n_prev, cap, tp.min_matches, d_path,
                         d_refused);
  HIPCHK(c, hipGetLastError());
  // 2. the query and train sets
  std::vector<int32_t> slots((size_t)2 * n_pairs);
  std::copy(ref_slots, ref_slots + n_pairs, slots.begin());
  std::copy(tgt_slots, tgt_slots + n_pairs, slots.begin() + n_pairs);
  st = surf_track_enqueue(c, tp.surf, n_pairs, slots.data(), cap, d_path, io.d_prev_kp, io.d_n_prev, d_kp, d_desc, d_counts);
  if (st) return st;
  // 3. symMatches
  st = match_descriptors_enqueue(c, what, MatchIn::device, n_pairs, UWT_NORM_L2, 64, d_desc, d_counts, d_desc + side * 64, d_counts + n_pairs, cap,
                                 tp.ratio, d_sym, d_n_sym);
  if (st) return st;
  // 4. goodMatches
  st = ransac_device_enqueue(c, n_pairs, cap, tp.ransac, d_sym, d_n_sym, d_kp, d_counts, d_kp + side, d_counts + n_pairs, io.d_good,
                             io.d_n_matches, d_rinfo);
  if (st) return st;
  // 5. getGoodKeypoints, and the live call's key points
  GoodKeypointsArgs ga;
  ga.good = reinterpret_cast<const MatchOut*>(io.d_good);
  ga.n_matches = io.d_n_matches;
  ga.kp_prev = reinterpret_cast<const SurfKeypoint*>(d_kp);
  ga.kp_cur = reinterpret_cast<const SurfKeypoint*>(d_kp + side);
  ga.kept_prev = reinterpret_cast<SurfKeypoint*>(io.d_kept_prev);
  ga.kept_cur = reinterpret_cast<SurfKeypoint*>(io.d_kept_cur);
  ga.feat_kp = c->feat_kp;
  ga.feat_nkp = c->feat_nkp;
  ga.outside = d_outside;
  ga.cap = cap; ga.feat_stride = kTrackFeatKeypoints; ga.n_pairs = n_pairs;
  ga.w = (float)c->lv[0].gw; ga.h = (float)c->lv[0].gh;
  launch_good_keypoints(c->stream, ga);
  HIPCHK(c, hipGetLastError());
  // 6. ObtainPatchesPoints + EstimatePoseFeatures
  st = features_device_enqueue(c, n_pairs, io.d_poses, io.d_stats);
  if (st) return st;
  TrackInfoArgs ia;
  ia.refused = d_refused; ia.outside = d_outside; ia.path = d_path;
  ia.n_kp_prev = d_counts; ia.n_kp_cur = d_counts + n_pairs;
  ia.n_symmetric = d_n_sym; ia.n_matches = io.d_n_matches;
  ia.ransac = reinterpret_cast<const RansacInfo*>(d_rinfo);
  ia.info = reinterpret_cast<TrackInfo*>(io.d_info);
  ia.stats_status = reinterpret_cast<int*>(io.d_stats);
  ia.stats_stride = (int)(sizeof(uwt_stats) / sizeof(int));
  ia.invalid_status = UWT_ERR_INVALID_ARG; ia.n_pairs = n_pairs;
  launch_tracking_info(c->stream, ia);
  HIPCHK(c, hipGetLastError());
  return compute_end(c, c->dep_first, c->dep_n);
}

}  // namespace

extern "C" {

int uwt_default_tracking_params(uwt_tracking_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  uwt_default_surf_params(&p->surf);
  uwt_default_ransac_params(&p->ransac);
  p->ratio = 0.65f;      // ratio_, include/Tracker.h:80
  p->min_matches = 110;  // src/System.cpp:208
  return UWT_OK;
}

int uwt_tracking_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                             const uwt_tracking_params* params, int32_t cap, const uwt_tracking_io* io) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_tracking_batch_async";
  if (!c || !io || !io->d_poses || !io->d_info || !io->d_good || !io->d_kept_prev || !io->d_kept_cur || !io->d_n_matches)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_tracking_params tp;
  int st = tracking_check(c, what, n_pairs, ref_slots, tgt_slots, params, cap, io->d_prev_kp != nullptr, io->d_n_prev != nullptr, &tp);
  if (st) return st;
  if (io->d_prev_kp && (io->d_prev_kp == io->d_kept_prev || io->d_prev_kp == io->d_kept_cur || io->d_n_prev == io->d_n_matches))
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": the provided key points or counts are also an output of this call");
  Carve cv(256);
  const TrackLayout l = track_carve(cv, n_pairs, cap);
  st = c->track_buf.reserve(c, c->stream, cv.total());
  if (st) return st;
  return tracking_enqueue(c, what, n_pairs, ref_slots, tgt_slots, tp, cap, l, *io);
}

int uwt_tracking_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, const uwt_tracking_params* params,
                       int32_t cap, const uwt_keypoint* prev_kp, const int32_t* n_prev, float* poses_out, uwt_stats* stats_out,
                       uwt_tracking_info* info_out, uwt_match* good_out, uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_tracking_batch";
  if (!c || !poses_out || !info_out || !good_out || !kept_prev_out || !kept_cur_out)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_tracking_params tp;
  int st = tracking_check(c, what, n_pairs, ref_slots, tgt_slots, params, cap, prev_kp != nullptr, n_prev != nullptr, &tp);
  if (st) return st;
  Carve cv(256);
  const TrackLayout l = track_carve(cv, n_pairs, cap);
  const TrackIoLayout o = track_io_carve(cv, n_pairs, cap);
  st = c->track_buf.reserve(c, c->stream, cv.total());
  if (st) return st;
  void* b = c->track_buf.p;
  const size_t recs = (size_t)n_pairs * cap;
  uwt_tracking_io io;
  io.d_prev_kp = prev_kp ? Carve::at<uwt_keypoint>(b, o.prev_kp) : nullptr;
  io.d_n_prev = prev_kp ? Carve::at<int32_t>(b, o.n_prev) : nullptr;
  io.d_poses = Carve::at<float>(b, o.poses);
  io.d_stats = Carve::at<uwt_stats>(b, o.stats);
  io.d_info = Carve::at<uwt_tracking_info>(b, o.info);
  io.d_good = Carve::at<uwt_match>(b, o.good);
  io.d_kept_prev = Carve::at<uwt_keypoint>(b, o.kept_prev);
  io.d_kept_cur = Carve::at<uwt_keypoint>(b, o.kept_cur);
  io.d_n_matches = Carve::at<int32_t>(b, o.n_matches);
  if (prev_kp) {
    HIPCHK(c, hipMemcpyAsync((void*)io.d_prev_kp, prev_kp, sizeof(uwt_keypoint) * recs, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((void*)io.d_n_prev, n_prev, sizeof(int32_t) * n_pairs, hipMemcpyHostToDevice, c->stream));
  }
  st = tracking_enqueue(c, what, n_pairs, ref_slots, tgt_slots, tp, cap, l, io);
  if (st) return st;
  std::vector<uwt_stats> stats((size_t)n_pairs);
  std::vector<int32_t> counts((size_t)n_pairs);
  HIPCHK(c, hipMemcpyAsync(poses_out, io.d_poses, sizeof(float) * 7 * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(stats.data(), io.d_stats, sizeof(uwt_stats) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info_out, io.d_info, sizeof(uwt_tracking_info) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(counts.data(), io.d_n_matches, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  st = rows_to_host(c, cap, n_pairs, {{io.d_good, sizeof(uwt_match), counts.data(), good_out},
                                      {io.d_kept_prev, sizeof(uwt_keypoint), counts.data(), kept_prev_out},
                                      {io.d_kept_cur, sizeof(uwt_keypoint), counts.data(), kept_cur_out}});
  if (st) return st;
  if (stats_out) std::copy(stats.begin(), stats.end(), stats_out);
  return first_failure(c, what, stats.data(), n_pairs);
}

}  // extern "C"
