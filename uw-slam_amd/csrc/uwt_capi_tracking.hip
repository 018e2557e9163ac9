// uwt_capi_tracking.hip — host side of libuwt_hip.so: System::Tracking for a batch of pairs as one chain on the device.  Every stage
// is the existing one (SURF or ORB, the matcher, the RANSAC selection, the live call), entered through its device-input form; the joints
// between them are the kernels of uwt_track_kernels.h.  Nothing here reads a result back: the asynchronous call only enqueues.  The
// chain is written once: a TrackDetector holds what differs between RobustMatcher(0) and RobustMatcher(1).
#include "uwt_ctx.h"
#include "uwt_track.h"

namespace {

static_assert(sizeof(uwt_tracking_params) == 56, "uwt_tracking_params layout");
static_assert(sizeof(uwt_tracking_orb_params) == 56, "uwt_tracking_orb_params layout");
static_assert(sizeof(uwt_tracking_info) == 32 && sizeof(TrackInfo) == sizeof(uwt_tracking_info), "uwt_tracking_info layout");
static_assert(sizeof(uwt_stats) % sizeof(int) == 0 && offsetof(uwt_stats, status) == 0, "uwt_stats: the status word first");

constexpr int kTrackFeatKeypoints = 200;   // key points the live call takes (kPatchMaxKeypoints: the stride of the context's feat_kp)

// the call's scratch: [paths | refused | outside | counts (query sides, then train sides) | symMatch counts | RANSAC records |
// key points (query sides, then train sides) | symMatches | descriptors]
struct TrackLayout { size_t path, refused, outside, counts, n_sym, rinfo, kp, sym, desc; };
TrackLayout track_carve(Carve& cv, int n_pairs, int cap, size_t desc_row) {
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
  l.desc = cv.take<uint8_t>(2 * n * cap * desc_row);
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

// What the chain asks of a detector, bound to one call's parameters: the matcher's norm and the elements and bytes of a descriptor
// row, the host checks of a call over n frames, the record rule's predicate launch, and the detector's device-path form
// (surf_track_enqueue / orb_track_enqueue over the 2 n_pairs slots).  The other parameters of the call are the same for both.
struct TrackDetector {
  int norm, dim;
  size_t desc_row;
  std::function<int(const char* what, int n_frames, const int32_t* slots)> check;
  std::function<void(int n_pairs, const Keypoint* prev_kp, const int* n_prev, int* path, int* refused)> predicate;
  std::function<int(int n_pairs, const int32_t* slots, const int* d_path, const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev,
                    uwt_keypoint* d_kp, unsigned char* d_desc, int* d_counts)> enqueue;
  uwt_ransac_params ransac;
  float ratio;
  int min_matches;
};

TrackDetector surf_detector(uwt_ctx* c, const uwt_tracking_params* params, int cap) {
  uwt_tracking_params tp;
  if (params) tp = *params;
  else uwt_default_tracking_params(&tp);
  const uwt_surf_params sp = tp.surf;
  TrackDetector d;
  d.norm = UWT_NORM_L2; d.dim = 64; d.desc_row = sizeof(float) * 64;
  d.ransac = tp.ransac; d.ratio = tp.ratio; d.min_matches = tp.min_matches;
  d.check = [=](const char* what, int n, const int32_t* slots) {
    uwt_surf_params in_force;
    return surf_check(c, what, n, slots, cap, &sp, &in_force);
  };
  const int min_matches = tp.min_matches;
  d.predicate = [=](int n_pairs, const Keypoint* prev_kp, const int* n_prev, int* path, int* refused) {
    launch_track_predicate(c->stream, n_pairs, prev_kp, n_prev, cap, min_matches, SurfRecordRule{}, path, refused);
  };
  d.enqueue = [=](int n_pairs, const int32_t* slots, const int* d_path, const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev,
                  uwt_keypoint* d_kp, unsigned char* d_desc, int* d_counts) {
    return surf_track_enqueue(c, sp, n_pairs, slots, cap, d_path, d_prev_kp, d_n_prev, d_kp, reinterpret_cast<float*>(d_desc), d_counts);
  };
  return d;
}

TrackDetector orb_detector(uwt_ctx* c, const uwt_tracking_orb_params* params, int cap) {
  uwt_tracking_orb_params tp;
  if (params) tp = *params;
  else uwt_default_tracking_orb_params(&tp);
  const uwt_orb_params op = tp.orb;
  TrackDetector d;
  d.norm = UWT_NORM_HAMMING; d.dim = 32; d.desc_row = 32;
  d.ransac = tp.ransac; d.ratio = tp.ratio; d.min_matches = tp.min_matches;
  d.check = [=](const char* what, int n, const int32_t* slots) {
    uwt_orb_params in_force;
    return orb_check(c, what, n, slots, cap, &op, &in_force);
  };
  const int min_matches = tp.min_matches;
  d.predicate = [=](int n_pairs, const Keypoint* prev_kp, const int* n_prev, int* path, int* refused) {   // (op has passed d.check)
    launch_track_predicate(c->stream, n_pairs, prev_kp, n_prev, cap, min_matches,
                           OrbRecordRule{op.n_levels, op.edge_threshold, c->p.width, c->p.height}, path, refused);
  };
  d.enqueue = [=](int n_pairs, const int32_t* slots, const int* d_path, const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev,
                  uwt_keypoint* d_kp, unsigned char* d_desc, int* d_counts) {
    return orb_track_enqueue(c, op, n_pairs, slots, cap, d_path, d_prev_kp, d_n_prev, d_kp, d_desc, d_counts);
  };
  return d;
}

// Every check the host can make; nothing is enqueued and no buffer grows when one fails.
int tracking_check(uwt_ctx* c, const char* what, const TrackDetector& d, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                   bool has_prev_kp, bool has_n_prev) {
  if (!ref_slots || !tgt_slots) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list");
  if (n_pairs < 1 || n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_pairs outside 1..max_pairs");
  int st = d.check(what, n_pairs, ref_slots);
  if (!st) st = d.check(what, n_pairs, tgt_slots);
  if (st) return st;
  if (!ransac_params_ok(d.ransac)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": distance, confidence or max_hypotheses outside its range");
  if (!std::isfinite(d.ratio)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": ratio is not finite");
  if (d.min_matches < 0) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": min_matches < 0");
  if (has_prev_kp != has_n_prev) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": exactly one of the provided key points and their counts is null");
  return UWT_OK;
}

// The chain, enqueued on the context stream (the arguments have passed tracking_check; the scratch holds `l` at its base).
int tracking_enqueue(uwt_ctx* c, const char* what, const TrackDetector& d, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                     int cap, const TrackLayout& l, const uwt_tracking_io& io, const Start& start = Start()) {
  void* b = c->track_buf.p;
  int* d_path = Carve::at<int>(b, l.path);
  int* d_refused = Carve::at<int>(b, l.refused);
  int* d_outside = Carve::at<int>(b, l.outside);
  int* d_counts = Carve::at<int>(b, l.counts);
  int* d_n_sym = Carve::at<int>(b, l.n_sym);
  uwt_ransac_info* d_rinfo = Carve::at<uwt_ransac_info>(b, l.rinfo);
  uwt_keypoint* d_kp = Carve::at<uwt_keypoint>(b, l.kp);
  uwt_match* d_sym = Carve::at<uwt_match>(b, l.sym);
  unsigned char* d_desc = Carve::at<unsigned char>(b, l.desc);
  const size_t side = (size_t)n_pairs * cap;   // records of one side of the batch

  int st = features_device_begin(c, what, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  // 1. usekeypoints, per pair
  d.predicate(n_pairs, reinterpret_cast<const Keypoint*>(io.d_prev_kp), io.d_n_prev, d_path, d_refused);
  HIPCHK(c, hipGetLastError());
  // 2. the query and train sets
  std::vector<int32_t> slots((size_t)2 * n_pairs);
  std::copy(ref_slots, ref_slots + n_pairs, slots.begin());
  std::copy(tgt_slots, tgt_slots + n_pairs, slots.begin() + n_pairs);
  st = d.enqueue(n_pairs, slots.data(), d_path, io.d_prev_kp, io.d_n_prev, d_kp, d_desc, d_counts);
  if (st) return st;
  // 3. symMatches
  st = match_descriptors_enqueue(c, what, MatchIn::device, n_pairs, d.norm, d.dim, d_desc, d_counts, d_desc + side * d.desc_row,
                                 d_counts + n_pairs, cap, d.ratio, d_sym, d_n_sym);
  if (st) return st;
  // 4. goodMatches
  st = ransac_device_enqueue(c, n_pairs, cap, d.ransac, d_sym, d_n_sym, d_kp, d_counts, d_kp + side, d_counts + n_pairs, io.d_good,
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
  st = features_device_enqueue(c, n_pairs, io.d_poses, io.d_stats, start);
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


// The asynchronous form of either detector (`what`: the entry's name).
int tracking_async(uwt_ctx* c, const char* what, const TrackDetector& d, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                   int cap, const uwt_tracking_io* io, const float* d_seeds = nullptr, const uwt_seed_options* sopt = nullptr) {
  if (!c || !io || !io->d_poses || !io->d_info || !io->d_good || !io->d_kept_prev || !io->d_kept_cur || !io->d_n_matches)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  start.d_seeds = d_seeds;
  st = seeds_clear_of(c, what, d_seeds, n_pairs, io->d_poses, io->d_stats);
  if (st) return st;
  if (d_seeds && n_pairs >= 1 && cap >= 1) {   // every output of the chain: the front end writes its own before the seeds are read
    const size_t P = (size_t)n_pairs, rows = P * (size_t)cap;
    const struct { const void* p; size_t bytes; } outs[] = {{io->d_info, sizeof(uwt_tracking_info) * P}, {io->d_good, sizeof(uwt_match) * rows},
                                                            {io->d_kept_prev, sizeof(uwt_keypoint) * rows},
                                                            {io->d_kept_cur, sizeof(uwt_keypoint) * rows}, {io->d_n_matches, sizeof(int32_t) * P}};
    for (const auto& o : outs) {
      st = seeds_clear_of_range(c, what, d_seeds, n_pairs, o.p, o.bytes);
      if (st) return st;
    }
  }
  st = tracking_check(c, what, d, n_pairs, ref_slots, tgt_slots, io->d_prev_kp != nullptr, io->d_n_prev != nullptr);
  if (st) return st;
  if (io->d_prev_kp && (io->d_prev_kp == io->d_kept_prev || io->d_prev_kp == io->d_kept_cur || io->d_n_prev == io->d_n_matches))
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": the provided key points or counts are also an output of this call");
  Carve cv(256, c->guard_bytes);
  const TrackLayout l = track_carve(cv, n_pairs, cap, d.desc_row);
  st = c->track_buf.reserve(c, c->stream, cv);
  if (st) return st;
  return tracking_enqueue(c, what, d, n_pairs, ref_slots, tgt_slots, cap, l, *io, start);
}

// The synchronous form of either detector, host in and out.
int tracking_sync(uwt_ctx* c, const char* what, const TrackDetector& d, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int cap,
                  const uwt_keypoint* prev_kp, const int32_t* n_prev, float* poses_out, uwt_stats* stats_out, uwt_tracking_info* info_out,
                  uwt_match* good_out, uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out, const float* seeds = nullptr,
                  const uwt_seed_options* sopt = nullptr) {
  if (!c || !poses_out || !info_out || !good_out || !kept_prev_out || !kept_cur_out)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  st = tracking_check(c, what, d, n_pairs, ref_slots, tgt_slots, prev_kp != nullptr, n_prev != nullptr);
  if (st) return st;
  st = stage_host_seeds(c, seeds, n_pairs, &start);
  if (st) return st;
  Carve cv(256, c->guard_bytes);
  const TrackLayout l = track_carve(cv, n_pairs, cap, d.desc_row);
  const TrackIoLayout o = track_io_carve(cv, n_pairs, cap);
  st = c->track_buf.reserve(c, c->stream, cv);
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
  st = tracking_enqueue(c, what, d, n_pairs, ref_slots, tgt_slots, cap, l, io, start);
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

int uwt_default_tracking_orb_params(uwt_tracking_orb_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  uwt_default_orb_params(&p->orb);
  uwt_default_ransac_params(&p->ransac);
  p->ratio = 0.65f;
  p->min_matches = 110;
  return UWT_OK;
}

int uwt_tracking_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                             const uwt_tracking_params* params, int32_t cap, const uwt_tracking_io* io) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_async(c, "uwt_tracking_batch_async", surf_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, io);
}

int uwt_tracking_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, const uwt_tracking_params* params,
                       int32_t cap, const uwt_keypoint* prev_kp, const int32_t* n_prev, float* poses_out, uwt_stats* stats_out,
                       uwt_tracking_info* info_out, uwt_match* good_out, uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_sync(c, "uwt_tracking_batch", surf_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, prev_kp, n_prev, poses_out,
                       stats_out, info_out, good_out, kept_prev_out, kept_cur_out);
}

int uwt_tracking_orb_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                 const uwt_tracking_orb_params* params, int32_t cap, const uwt_tracking_io* io) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_async(c, "uwt_tracking_orb_batch_async", orb_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, io);
}

int uwt_tracking_batch_seeded(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                              const uwt_tracking_params* params, int32_t cap, const uwt_keypoint* prev_kp, const int32_t* n_prev,
                              float* poses_out, uwt_stats* stats_out, uwt_tracking_info* info_out, uwt_match* good_out,
                              uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out, const float* seeds, const uwt_seed_options* sopt) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_sync(c, "uwt_tracking_batch_seeded", surf_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, prev_kp, n_prev,
                       poses_out, stats_out, info_out, good_out, kept_prev_out, kept_cur_out, seeds, sopt);
}

int uwt_tracking_orb_batch_seeded(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                  const uwt_tracking_orb_params* params, int32_t cap, const uwt_keypoint* prev_kp, const int32_t* n_prev,
                                  float* poses_out, uwt_stats* stats_out, uwt_tracking_info* info_out, uwt_match* good_out,
                                  uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out, const float* seeds,
                                  const uwt_seed_options* sopt) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_sync(c, "uwt_tracking_orb_batch_seeded", orb_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, prev_kp,
                       n_prev, poses_out, stats_out, info_out, good_out, kept_prev_out, kept_cur_out, seeds, sopt);
}

int uwt_tracking_batch_seeded_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                    const uwt_tracking_params* params, int32_t cap, const uwt_tracking_io* io, const float* d_seeds,
                                    const uwt_seed_options* sopt) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_async(c, "uwt_tracking_batch_seeded_async", surf_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, io,
                        d_seeds, sopt);
}

int uwt_tracking_orb_batch_seeded_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                        const uwt_tracking_orb_params* params, int32_t cap, const uwt_tracking_io* io,
                                        const float* d_seeds, const uwt_seed_options* sopt) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_async(c, "uwt_tracking_orb_batch_seeded_async", orb_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, io,
                        d_seeds, sopt);
}

int uwt_tracking_orb_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                           const uwt_tracking_orb_params* params, int32_t cap, const uwt_keypoint* prev_kp, const int32_t* n_prev,
                           float* poses_out, uwt_stats* stats_out, uwt_tracking_info* info_out, uwt_match* good_out,
                           uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  return tracking_sync(c, "uwt_tracking_orb_batch", orb_detector(c, params, cap), n_pairs, ref_slots, tgt_slots, cap, prev_kp, n_prev,
                       poses_out, stats_out, info_out, good_out, kept_prev_out, kept_cur_out);
}

}  // extern "C"
