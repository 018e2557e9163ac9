// uwt_capi_tables.hip — host side of libuwt_hip.so: alignment over point tables — the candidate and patch producers, the batch
// calls that build the tables on the device and evaluate them there, and the caller's own tables as a batch of one pair.
#include "uwt_ctx.h"
#include "uwt_track.h"

extern "C" {

// ---- the sparse point producers: per-stage entries over a slot list in the scratch ------------------------------------
namespace {

// the first min(n, 200) key points (x, y) inside level 0 (its grid is its image)
int check_keypoints(uwt_ctx* c, const char* what, const float* kp, int n) {
  const float w = (float)c->lv[0].gw, h = (float)c->lv[0].gh;
  for (int i = 0; i < std::min(n, kPatchMaxKeypoints); i++)
    if (!inside_level0(kp[2 * i], kp[2 * i + 1], w, h))
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key point outside the image");
  return UWT_OK;
}

// The candidate producer's work area for n frames on one level: row bands enough for a lone frame to spread over the chip, a few
// rows per thread at least.  [sums | gradient_ planes | (x, band) counts | their offsets]
struct CandidatesLayout {
  int bands;
  size_t o_sums, o_mag, o_cells, o_off;
};
CandidatesLayout candidates_work_layout(Carve& cv, const LevelK& L, int n) {
  CandidatesLayout o;
  const int col_blocks = (L.gw + kBlock - 1) / kBlock;
  o.bands = std::max(1, std::min(L.gh / 8, 512 / std::max(1, col_blocks * n)));
  const size_t m = (size_t)L.gw * o.bands * n;
  o.o_sums = cv.take<unsigned long long>((size_t)n);
  o.o_mag = cv.take<uint8_t>((size_t)L.n * n);
  o.o_cells = cv.take<int>(m);
  o.o_off = cv.take<int>(m);
  return o;
}
constexpr size_t kCandidatesAlign = 256;

// the device slot list first .. first + n - 1 at d (a fill per slot: no host buffer, no staging copy)
int stage_slots(uwt_ctx* c, int* d, int first, int n) {
  for (int f = 0; f < n; f++) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(d + f), first + f, 1, c->stream));
  return UWT_OK;
}

// Tracker::ObtainCandidatePoints on level lvl for the frames of the device slot list d_slots (n), enqueued on the context stream:
// the work area at `work` (candidates_work_layout), frame f's table at out + f * gw * gh, its full count at counts[f]
int enqueue_candidates(uwt_ctx* c, int lvl, int n, const int* d_slots, double threshold, void* work, float4* out, int* counts) {
  const LevelK& L = c->lv[lvl];
  Carve cv(kCandidatesAlign, c->guard_bytes);
  const CandidatesLayout o = candidates_work_layout(cv, L, n);
  uwt::CandidatesWork w;
  w.sums = Carve::at<unsigned long long>(work, o.o_sums);
  w.mag = Carve::at<uint8_t>(work, o.o_mag);
  w.cells = Carve::at<int>(work, o.o_cells);
  w.offsets = Carve::at<int>(work, o.o_off);
  w.bands = o.bands;
  HIPCHK(c, hipMemsetAsync(w.sums, 0, 8 * (size_t)n, c->stream));
  uwt::launch_candidates_slots(c->stream, L, n, d_slots, c->gx[lvl], c->gy[lvl], c->p.has_depth ? c->depth[lvl] : nullptr, threshold, w,
                               out, counts);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

}  // namespace

int uwt_gradient_magnitude(uwt_ctx* c, int32_t slot, int32_t lvl, uint8_t* mag_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !mag_out || !slot_range_ok(c, slot, 1) || lvl < 0 || lvl >= c->p.n_levels)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_gradient_magnitude");
  const LevelK& L = c->lv[lvl];   // gradient_[lvl]: the level's image, img_w x img_h
  // scratch: [sum (not read) | slot list at 64 | the plane at 256]
  Carve cv(64, c->guard_bytes);
  const size_t o_sum = cv.take<unsigned long long>(1), o_slot = cv.take<int>(1);
  cv.align = 256;
  const size_t o_mag = cv.take<uint8_t>((size_t)L.n);
  int st = c->scratch.reserve(c, c->stream, cv, cv.tight());
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  unsigned long long* d_sum = Carve::at<unsigned long long>(c->scratch.p, o_sum);
  int* d_slot = Carve::at<int>(c->scratch.p, o_slot);
  uint8_t* d_mag = Carve::at<uint8_t>(c->scratch.p, o_mag);
  st = stage_slots(c, d_slot, slot, 1);
  if (st) return st;
  uwt::launch_grad_mag(c->stream, L, 1, d_slot, c->gx[lvl], c->gy[lvl], d_mag, d_sum);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpy2DAsync(mag_out, L.iw, d_mag, L.pitch, L.iw, L.ih, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_obtain_candidate_points_batch(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t lvl, double threshold,
                                      float* pts_out, int32_t cap, int32_t* counts_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !counts_out || cap < 0 || (cap > 0 && !pts_out) || n_frames < 1 || !slot_range_ok(c, first_slot, n_frames) || lvl < 0 ||
      lvl >= c->p.n_levels)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_obtain_candidate_points_batch");
  if (!std::isfinite(threshold))   // as the batched tracking calls (candidates_enqueue), the cloud and the sweep refuse it
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_obtain_candidate_points_batch: threshold is not finite");
  const LevelK& L = c->lv[lvl];
  const size_t rows = (size_t)L.gw * L.gh;   // a frame's table: a row for every cell of the point grid (the bound is never reached)
  // scratch: [the producer's work area | slot list | counts | tables]
  Carve cv(kCandidatesAlign, c->guard_bytes);
  candidates_work_layout(cv, L, n_frames);   // (at the base, where enqueue_candidates carves it again)
  const size_t o_slots = cv.take<int>((size_t)n_frames), o_cnt = cv.take<int>((size_t)n_frames),
               o_tab = cv.take<float4>((size_t)n_frames * rows);
  int st = c->scratch.reserve(c, c->stream, cv, cv.tight());
  if (st) return st;
  st = compute_begin(c, first_slot, n_frames);
  if (st) return st;
  int* d_slots = Carve::at<int>(c->scratch.p, o_slots);
  int* d_cnt = Carve::at<int>(c->scratch.p, o_cnt);
  float4* d_tab = Carve::at<float4>(c->scratch.p, o_tab);
  st = stage_slots(c, d_slots, first_slot, n_frames);
  if (!st) st = enqueue_candidates(c, lvl, n_frames, d_slots, threshold, c->scratch.p, d_tab, d_cnt);
  if (st) return st;
  return counted_rows_to_host(c, d_tab, rows, d_cnt, n_frames, cap, pts_out, counts_out);
}

int uwt_obtain_candidate_points(uwt_ctx* c, int32_t slot, int32_t lvl, double threshold, float* pts_out, int32_t cap,
                                int32_t* count_out) {
  if (!count_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_obtain_candidate_points");
  return uwt_obtain_candidate_points_batch(c, slot, 1, lvl, threshold, pts_out, cap, count_out);
}

int uwt_obtain_patch_points(uwt_ctx* c, int32_t slot, const float* kp, int32_t n_kp, float* pts_out, int32_t cap,
                            int32_t* count_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !count_out || n_kp < 0 || (n_kp > 0 && !kp) || cap < 0 || (cap > 0 && !pts_out) || !slot_range_ok(c, slot, 1))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_obtain_patch_points");
  int st = check_keypoints(c, "uwt_obtain_patch_points", kp, n_kp);
  if (st) return st;
  const int stride = std::min(cap, kPatchMaxKeypoints * kPatchMaxRows);   // rows written at most
  // scratch: [key point count | slot list | row count | key points at 64 | table at 4096]; the count, the slot and the key points
  // go down in one copy, so they are ONE array of the carve (nothing may come between them)
  Carve cv(64, c->guard_bytes);
  const size_t o_hdr = cv.take<uint8_t>(64 + sizeof(float2) * kPatchMaxKeypoints), o_kp = o_hdr + 64;
  cv.align = 4096;
  const size_t o_tab = cv.take<float4>((size_t)stride);
  st = c->scratch.reserve(c, c->stream, cv, cv.tight());
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  int* d_hdr = Carve::at<int>(c->scratch.p, o_hdr);
  float2* d_kp = Carve::at<float2>(c->scratch.p, o_kp);
  float4* d_tab = Carve::at<float4>(c->scratch.p, o_tab);
  const int hdr[2] = {std::min(n_kp, kPatchMaxKeypoints), slot};
  std::vector<uint8_t> in(64 + sizeof(float2) * hdr[0]);
  std::memcpy(in.data(), hdr, sizeof(hdr));
  if (hdr[0]) std::memcpy(in.data() + 64, kp, sizeof(float2) * hdr[0]);
  HIPCHK(c, hipMemcpyAsync(d_hdr, in.data(), in.size(), hipMemcpyHostToDevice, c->stream));
  uwt::launch_patch_points_batch(c->stream, 1, d_kp, d_hdr, d_hdr + 1, c->p.has_depth ? c->depth[0] : nullptr, (size_t)c->lv[0].n,
                                 c->lv[0].pitch, c->lv[0].gw, c->lv[0].gh, d_tab, stride, d_hdr + 2);
  HIPCHK(c, hipGetLastError());
  return counted_rows_to_host(c, d_tab, 0, d_hdr + 2, 1, stride, pts_out, count_out);
}

// ---- the live call for a batch of pairs: tables built and evaluated on the device --------------------------------
namespace {

constexpr int kFeatTableRows = kPatchMaxKeypoints * kPatchMaxRows;   // rows of one pair's table at most (its stride)
constexpr int kFeatKpFloats = 2 * kPatchMaxKeypoints;                 // one frame's key points as the caller passes them

// the context's params with Tracker::EstimatePoseFeatures' locals (src/Tracker.cpp:633-640, 661, 834, 856): level 0 only, 10
// iterations, epsilon 1e-3, last_error 50000, z_factor 0.002, no angle factor, gain 1 (Residuals.mul(1)), the early exit of :782,
// the hand-off of :856; identity weights (:769), round() (:746).  Metric Jacobian mode: z_factor 1 — the 0.002 compensates the pixel
// coordinate in the reference's column 2 (uwt.h "the metric Jacobian")
uwt_params feature_params(const uwt_ctx* c) {
  uwt_params q = c->p;
  q.first_level = q.last_level = 0;
  q.max_iters = 10;
  q.epsilon = 0.001f;
  q.initial_error = 50000.0f;
  q.z_factor = c->jacobian == UWT_JACOBIAN_METRIC ? 1.0f : 0.002f;
  q.angle_factor = 1.0f;
  q.gain = 1.0f;
  q.early_exit = 1;
  q.handoff_scale_t = 1;
  return q;
}

// the live call's device buffers and staging ring, allocated on the first call (uwt_destroy frees them); each piece is retried
// on its own after a failed allocation
int ensure_features(uwt_ctx* c) {
  const size_t mp = (size_t)c->p.max_pairs;
  if (!c->feat_tab) HIPCHK(c, hipMalloc((void**)&c->feat_tab, sizeof(float4) * kFeatTableRows * mp));
  if (!c->feat_cnt) HIPCHK(c, hipMalloc((void**)&c->feat_cnt, sizeof(int) * mp));
  if (!c->feat_kp) HIPCHK(c, hipMalloc((void**)&c->feat_kp, sizeof(float) * kFeatKpFloats * mp));
  if (!c->feat_nkp) HIPCHK(c, hipMalloc((void**)&c->feat_nkp, sizeof(int) * mp));
  if (!c->feat_recs) HIPCHK(c, hipMalloc((void**)&c->feat_recs, sizeof(uint32_t) * kRecWords * kFeatMaxSlices * mp));
  for (int i = 0; i < uwt_ctx::kPairStages; i++)
    if (!c->ev_feat[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_feat[i], hipEventDisableTiming));
  if (!c->h_feat) HIPCHK(c, hipHostMalloc((void**)&c->h_feat, sizeof(float) * (1 + kFeatKpFloats) * mp * uwt_ctx::kPairStages));
  return UWT_OK;
}

// the pair lists of a batch call: not null, n in 1..max_pairs, every slot in range
int check_pair_lists(uwt_ctx* c, const char* what, int n, const int32_t* slots_a, const int32_t* slots_b) {
  if (!slots_a || !slots_b) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  if (n < 1 || n > c->p.max_pairs) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": count outside 1..max_pairs");
  for (int f = 0; f < n; f++)
    if (slots_a[f] < 0 || slots_a[f] >= c->p.max_frames || slots_b[f] < 0 || slots_b[f] >= c->p.max_frames)
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": slot out of range");
  return UWT_OK;
}

int check_features_args(uwt_ctx* c, const char* what, int n, const int32_t* slots_a, const int32_t* slots_b, const float* kp,
                        const int32_t* n_kp) {
  if (!kp || !n_kp) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  int st = check_pair_lists(c, what, n, slots_a, slots_b);
  if (st) return st;
  for (int f = 0; f < n; f++) {
    if (n_kp[f] < 0) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": negative key point count");
    st = check_keypoints(c, what, kp + (size_t)f * kFeatKpFloats, n_kp[f]);
    if (st) return st;
  }
  return UWT_OK;
}


// the batched producer over feat_kp / feat_nkp as they are on the device: frame f's table at feat_tab + f * kFeatTableRows from its
// key points and the depth of slot d_slots[f]
int enqueue_patch_producer(uwt_ctx* c, int n, const int* d_slots) {
  uwt::launch_patch_points_batch(c->stream, n, c->feat_kp, c->feat_nkp, d_slots, c->p.has_depth ? c->depth[0] : nullptr,
                                 (size_t)c->lv[0].n, c->lv[0].pitch, c->lv[0].gw, c->lv[0].gh, c->feat_tab, kFeatTableRows,
                                 c->feat_cnt);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// The caller's key points and counts are copied before the call returns (into the next block of a pinned ring, as
// upload_pairs does with the pair lists), then asynchronously to the device, and the batched producer builds the tables.
int enqueue_patch_tables(uwt_ctx* c, int n, const int* d_slots, const float* kp, const int32_t* n_kp) {
  const size_t mp = (size_t)c->p.max_pairs;
  const int stage = (c->feat_stage + 1) % uwt_ctx::kPairStages;
  HIPCHK(c, hipEventSynchronize(c->ev_feat[stage]));   // the copy that last read this block (kPairStages calls ago)
  float* block = c->h_feat + (size_t)stage * (1 + kFeatKpFloats) * mp;
  int* h_n = reinterpret_cast<int*>(block);
  float* h_kp = block + mp;
  std::memcpy(h_n, n_kp, sizeof(int) * n);
  std::memcpy(h_kp, kp, sizeof(float) * kFeatKpFloats * n);
  c->feat_stage = stage;
  HIPCHK(c, hipMemcpyAsync(c->feat_nkp, h_n, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->feat_kp, h_kp, sizeof(float) * kFeatKpFloats * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_feat[stage], c->stream));
  return enqueue_patch_producer(c, n, d_slots);
}

// the options of a batched table call: null = {0, 0}; weights in 0..2, sampler in 0..1, reserved words zero
int table_options(uwt_ctx* c, const char* what, const uwt_table_options* opt, uwt_table_options* out) {
  std::memset(out, 0, sizeof(*out));
  if (!opt) return UWT_OK;
  if (opt->weights < 0 || opt->weights > 2 || opt->sampler < 0 || opt->sampler > 1)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": uwt_table_options: weights outside 0..2 or sampler outside 0..1");
  for (int32_t r : opt->reserved)
    if (r) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": uwt_table_options: reserved word not zero");
  *out = *opt;
  return UWT_OK;
}
constexpr uwt_table_options kIdentityTables = {};

// One level of device-resident tables: pair i's rows at ta.tables + i * ta.stride, its count at ta.counts[i]; slices: the grid's
// bound on a table's slices, which every pair's count obeys (the counts stay on the device), and the record stride
struct TableLevel {
  TableArgs ta;
  int slices;
};

// EstimatePose over device-resident tables for n_pairs pairs (their lists on the device), enqueued on the context stream under
// the solver constants q, levels q.first_level .. q.last_level (lv[lvl] each): k_init_state, then per level up to q.max_iters
// k_table_eval launches (each evaluates every pair still iterating and updates it in its tail; a pair that has left the level
// makes the later launches return at once) and k_level_end; k_write_out.  The blocks beyond a pair's own slice count return at
// once.  polls: the host reads the early exits back on the dense batch's schedule (enqueue_estimate) — the count
// of pairs still on the level after evaluation first_poll - 1, then after twice as many, ..., each read one evaluation late; no
// launch once none is left.  Without, nothing here waits for the device.
// opt (checked by table_options): robust weights and / or the bilinear sampler — an evaluation is then k_table_hist (weights only)
// + k_table_general, records of the general kind; the pairs' histogram rows are cleared here once, every scale pass leaves them so.
// q.weights and q.sampler are not looked at.
// start: where the alignments start and how they cross the levels (the seeded entries; the default: identity, q's hand-off).
int enqueue_table_estimate(uwt_ctx* c, int n_pairs, const uwt_params& q, const TableLevel* lv, uint32_t* recs, bool polls,
                           const uwt_table_options& opt, float* d_poses, StatsOut* d_stats, const Start& start = Start()) {
  const int tb = 128, blocks = (n_pairs + tb - 1) / tb;
  const bool general = opt.weights || opt.sampler;
  if (opt.weights) {
    int st = ensure_general_buffers(c);
    if (st) return st;
    HIPCHK(c, hipMemsetAsync(c->hist, 0, sizeof(unsigned int) * kHistBins * (size_t)n_pairs, c->stream));
  }
  const GeneralArgs ga = {opt.sampler, opt.weights, q.gain, c->hist, c->scale};
  hipLaunchKernelGGL(k_init_state, dim3(blocks), dim3(tb), 0, c->stream, c->state, n_pairs, start.rec(q), start.d_gate);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(c->d_tickets, 0, sizeof(unsigned int) * (size_t)n_pairs, c->stream));
  for (int lvl = q.first_level; lvl >= q.last_level; lvl--) {
    ResidualArgs ra = residual_args(c, lvl, q);
    ra.slices = lv[lvl].slices;
    ra.partials = recs;
    UpdateArgs ua = update_args(c, lvl, q, general);
    ua.partials = recs;
    ua.slices = ra.slices;
    LatePoll late(c->tn.first_poll);
    for (int k = 0; k < q.max_iters; k++) {
      ua.k = k;
      int st = late.arm(c, c->stream, polls, k, q.max_iters, &ua.active);
      if (st) return st;
      arm_tail(c, ra, ua);
      if (general) uwt::launch_table_general(c->stream, launch_sel(c), ra, lv[lvl].ta, ga, n_pairs);
      else uwt::launch_table_eval(c->stream, launch_sel(c), ra, lv[lvl].ta, n_pairs);
      HIPCHK(c, hipGetLastError());
      bool none_left = false;
      st = late.look(c, c->stream, &none_left);
      if (st) return st;
      if (none_left) break;
    }
    hipLaunchKernelGGL(k_level_end, dim3(blocks), dim3(tb), 0, c->stream, c->state, n_pairs, lvl, start.rec(q));
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_write_out, dim3(blocks), dim3(tb), 0, c->stream, c->state, n_pairs, d_poses, d_stats);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// System::Tracking's live call for n_pairs pairs, enqueued on the context stream: the producer over the reference frames, then
// enqueue_table_estimate under feature_params and the call's options (null: identity weights, round()), which the host never
// polls.  No read-back, no wait for the device.
int features_enqueue(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, const float* kp,
                     const int32_t* n_kp, const uwt_table_options* opt_or_null, float* d_poses, StatsOut* d_stats,
                     const Start& start = Start()) {
  uwt_table_options opt;
  int st = table_options(c, what, opt_or_null, &opt);
  if (st) return st;
  st = check_features_args(c, what, n_pairs, ref_slots, tgt_slots, kp, n_kp);
  if (st) return st;
  st = ensure_features(c);
  if (st) return st;
  st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  st = compute_begin_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  st = enqueue_patch_tables(c, n_pairs, c->d_ref, kp, n_kp);
  if (st) return st;
  // the grid's slices: the batch's bound on a table's rows
  int rows = 0;
  for (int i = 0; i < n_pairs; i++) rows = std::max(rows, std::min(n_kp[i], kPatchMaxKeypoints) * kPatchMaxRows);
  const TableLevel lv0 = {{c->feat_tab, c->feat_cnt, kFeatTableRows}, table_slices(rows)};
  return enqueue_table_estimate(c, n_pairs, feature_params(c), &lv0, c->feat_recs, false, opt, d_poses, d_stats, start);
}

}  // namespace

int uwt_obtain_patch_points_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const float* kp, const int32_t* n_kp,
                                  float* pts_out, int32_t cap, int32_t* counts_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !counts_out || cap < 0 || (cap > 0 && !pts_out)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_obtain_patch_points_batch");
  int st = check_features_args(c, "uwt_obtain_patch_points_batch", n_frames, slots, slots, kp, n_kp);
  if (st) return st;
  st = ensure_features(c);
  if (st) return st;
  st = upload_pairs(c, n_frames, slots, slots);   // the slot list travels as the pair lists do
  if (st) return st;
  st = compute_begin_pairs(c, n_frames, slots, slots);
  if (st) return st;
  st = enqueue_patch_tables(c, n_frames, c->d_ref, kp, n_kp);
  if (st) return st;
  return counted_rows_to_host(c, c->feat_tab, kFeatTableRows, c->feat_cnt, n_frames, cap, pts_out, counts_out);
}

namespace {

int features_async(uwt_ctx* c, const char* what, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, const float* kp,
                   const int32_t* n_kp, const uwt_table_options* opt, float* d_poses_out, uwt_stats* d_stats_out,
                   const float* d_seeds = nullptr, const uwt_seed_options* sopt = nullptr) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_poses_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  start.d_seeds = d_seeds;
  st = seeds_clear_of(c, what, d_seeds, n_pairs, d_poses_out, d_stats_out);
  if (st) return st;
  st = features_enqueue(c, what, n_pairs, ref_slots, tgt_slots, kp, n_kp, opt, d_poses_out, reinterpret_cast<StatsOut*>(d_stats_out), start);
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int features_sync(uwt_ctx* c, const char* what, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, const float* kp,
                  const int32_t* n_kp, const uwt_table_options* opt, float* poses_out, uwt_stats* stats_out,
                  const float* seeds = nullptr, const uwt_seed_options* sopt = nullptr) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !poses_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  if (seeds && (n_pairs < 1 || n_pairs > c->p.max_pairs)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": count outside 1..max_pairs");
  st = stage_host_seeds(c, seeds, n_pairs, &start);
  if (st) return st;
  st = features_enqueue(c, what, n_pairs, ref_slots, tgt_slots, kp, n_kp, opt, c->d_poses, c->d_stats, start);
  if (st) return st;
  return read_back_pairs(c, what, n_pairs, poses_out, stats_out);
}

}  // namespace

int uwt_default_table_options(uwt_table_options* o) {
  if (!o) return UWT_ERR_INVALID_ARG;
  std::memset(o, 0, sizeof(*o));
  return UWT_OK;
}

int uwt_track_features_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                   const float* kp, const int32_t* n_kp, float* d_poses_out, uwt_stats* d_stats_out) {
  return features_async(c, "uwt_track_features_batch_async", n_pairs, ref_slots, tgt_slots, kp, n_kp, nullptr, d_poses_out, d_stats_out);
}

int uwt_estimate_pose_features_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                     const float* kp, const int32_t* n_kp, float* poses_out, uwt_stats* stats_out) {
  return features_sync(c, "uwt_estimate_pose_features_batch", n_pairs, ref_slots, tgt_slots, kp, n_kp, nullptr, poses_out, stats_out);
}

int uwt_track_features_batch_opt_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                       const float* kp, const int32_t* n_kp, const uwt_table_options* opt, float* d_poses_out,
                                       uwt_stats* d_stats_out) {
  return features_async(c, "uwt_track_features_batch_opt_async", n_pairs, ref_slots, tgt_slots, kp, n_kp, opt, d_poses_out, d_stats_out);
}

int uwt_estimate_pose_features_batch_opt(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                         const float* kp, const int32_t* n_kp, const uwt_table_options* opt, float* poses_out,
                                         uwt_stats* stats_out) {
  return features_sync(c, "uwt_estimate_pose_features_batch_opt", n_pairs, ref_slots, tgt_slots, kp, n_kp, opt, poses_out, stats_out);
}

int uwt_track_features_batch_seeded_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                          const float* kp, const int32_t* n_kp, const uwt_table_options* opt, float* d_poses_out,
                                          uwt_stats* d_stats_out, const float* d_seeds, const uwt_seed_options* sopt) {
  return features_async(c, "uwt_track_features_batch_seeded_async", n_pairs, ref_slots, tgt_slots, kp, n_kp, opt, d_poses_out, d_stats_out,
                        d_seeds, sopt);
}

int uwt_estimate_pose_features_batch_seeded(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                            const float* kp, const int32_t* n_kp, const uwt_table_options* opt, float* poses_out,
                                            uwt_stats* stats_out, const float* seeds, const uwt_seed_options* sopt) {
  return features_sync(c, "uwt_estimate_pose_features_batch_seeded", n_pairs, ref_slots, tgt_slots, kp, n_kp, opt, poses_out, stats_out,
                       seeds, sopt);
}

// ---- semi-dense tracking for a batch of pairs: candidate tables built and evaluated on the device ------------------------
namespace {


// Tracker::ObtainCandidatePoints(previous) on levels last_level..first_level, then Tracker::EstimatePose(previous, current) over
// those tables, for n_pairs pairs, enqueued on the context stream: per level the slot-list producer (pair i's table at cand_tab +
// level offset + i * gw * gh, its count at cand_cnt[lvl * n_pairs + i]), then enqueue_table_estimate under the context's params,
// polled under early_exit.  The only waits are the early-exit polls.  with_options: an _opt entry — weights and sampler are the
// call's (opt_or_null, null: identity and round()), the context's are not looked at; else the context's must be identity and round().
int candidates_enqueue(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                       bool with_options, const uwt_table_options* opt_or_null, float* d_poses, StatsOut* d_stats,
                       const Start& start = Start()) {
  const uwt_params& p = c->p;
  uwt_table_options opt;
  int st = table_options(c, what, opt_or_null, &opt);
  if (st) return st;
  st = check_pair_lists(c, what, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  if (!std::isfinite(threshold)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": threshold is not finite");
  if (!with_options && (p.weights || p.sampler))
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": identity weights and the nearest sampler only; robust weights or the "
                                                            "bilinear sampler over candidate tables: uwt_estimate_pose_points, or "
                                                            "uwt_track_candidates_batch_opt_async / uwt_estimate_pose_candidates_batch_opt");
  size_t rows = 0, work = 0, tab_off[UWT_MAX_LEVELS] = {};
  int smax = 1;
  for (int l = p.last_level; l <= p.first_level; l++) {
    const LevelK& L = c->lv[l];
    tab_off[l] = rows;
    rows += (size_t)L.gw * L.gh * n_pairs;
    Carve cv(kCandidatesAlign, c->guard_bytes);
    candidates_work_layout(cv, L, n_pairs);
    work = std::max(work, cv.total());
    smax = std::max(smax, table_slices(L.gw * L.gh));
  }
  st = c->cand_tab.reserve(c, c->stream, rows * sizeof(float4));
  if (!st) st = c->cand_cnt.reserve(c, c->stream, sizeof(int) * UWT_MAX_LEVELS * (size_t)n_pairs);
  if (!st) st = c->cand_work.reserve(c, c->stream, work);
  if (!st) st = c->cand_recs.reserve(c, c->stream, sizeof(uint32_t) * kRecWords * (size_t)smax * n_pairs);
  if (st) return st;
  st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  st = compute_begin_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  TableLevel lv[UWT_MAX_LEVELS];
  for (int l = p.last_level; l <= p.first_level; l++) {
    float4* tab = (float4*)c->cand_tab.p + tab_off[l];
    int* cnt = (int*)c->cand_cnt.p + (size_t)l * n_pairs;
    st = enqueue_candidates(c, l, n_pairs, c->d_ref, threshold, c->cand_work.p, tab, cnt);
    if (st) return st;
    const int cells = c->lv[l].gw * c->lv[l].gh;   // the bound every pair's count obeys
    lv[l] = {{tab, cnt, cells}, table_slices(cells)};
  }
  return enqueue_table_estimate(c, n_pairs, p, lv, (uint32_t*)c->cand_recs.p, p.early_exit != 0, opt, d_poses, d_stats, start);
}

}  // namespace

namespace {

int candidates_async(uwt_ctx* c, const char* what, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                     bool with_options, const uwt_table_options* opt, float* d_poses_out, uwt_stats* d_stats_out,
                     const float* d_seeds = nullptr, const uwt_seed_options* sopt = nullptr) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_poses_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  start.d_seeds = d_seeds;
  st = seeds_clear_of(c, what, d_seeds, n_pairs, d_poses_out, d_stats_out);
  if (st) return st;
  st = candidates_enqueue(c, what, n_pairs, ref_slots, tgt_slots, threshold, with_options, opt, d_poses_out,
                          reinterpret_cast<StatsOut*>(d_stats_out), start);
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int candidates_sync(uwt_ctx* c, const char* what, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                    bool with_options, const uwt_table_options* opt, float* poses_out, uwt_stats* stats_out,
                    const float* seeds = nullptr, const uwt_seed_options* sopt = nullptr) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !poses_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  if (seeds && (n_pairs < 1 || n_pairs > c->p.max_pairs)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": count outside 1..max_pairs");
  st = stage_host_seeds(c, seeds, n_pairs, &start);
  if (st) return st;
  st = candidates_enqueue(c, what, n_pairs, ref_slots, tgt_slots, threshold, with_options, opt, c->d_poses, c->d_stats, start);
  if (st) return st;
  return read_back_pairs(c, what, n_pairs, poses_out, stats_out);
}

}  // namespace

int uwt_track_candidates_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                                     float* d_poses_out, uwt_stats* d_stats_out) {
  return candidates_async(c, "uwt_track_candidates_batch_async", n_pairs, ref_slots, tgt_slots, threshold, false, nullptr, d_poses_out,
                          d_stats_out);
}

int uwt_estimate_pose_candidates_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                                       float* poses_out, uwt_stats* stats_out) {
  return candidates_sync(c, "uwt_estimate_pose_candidates_batch", n_pairs, ref_slots, tgt_slots, threshold, false, nullptr, poses_out,
                         stats_out);
}

int uwt_track_candidates_batch_opt_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                                         const uwt_table_options* opt, float* d_poses_out, uwt_stats* d_stats_out) {
  return candidates_async(c, "uwt_track_candidates_batch_opt_async", n_pairs, ref_slots, tgt_slots, threshold, true, opt, d_poses_out,
                          d_stats_out);
}

int uwt_estimate_pose_candidates_batch_opt(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                           double threshold, const uwt_table_options* opt, float* poses_out, uwt_stats* stats_out) {
  return candidates_sync(c, "uwt_estimate_pose_candidates_batch_opt", n_pairs, ref_slots, tgt_slots, threshold, true, opt, poses_out,
                         stats_out);
}

int uwt_track_candidates_batch_seeded_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                            double threshold, const uwt_table_options* opt, float* d_poses_out, uwt_stats* d_stats_out,
                                            const float* d_seeds, const uwt_seed_options* sopt) {
  return candidates_async(c, "uwt_track_candidates_batch_seeded_async", n_pairs, ref_slots, tgt_slots, threshold, true, opt, d_poses_out,
                          d_stats_out, d_seeds, sopt);
}

int uwt_estimate_pose_candidates_batch_seeded(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                              double threshold, const uwt_table_options* opt, float* poses_out, uwt_stats* stats_out,
                                              const float* seeds, const uwt_seed_options* sopt) {
  return candidates_sync(c, "uwt_estimate_pose_candidates_batch_seeded", n_pairs, ref_slots, tgt_slots, threshold, true, opt, poses_out,
                         stats_out, seeds, sopt);
}

// ---- the caller's own tables: a batch of one pair whose tables arrive from the host -----------------------------------------
int uwt_estimate_pose_points(uwt_ctx* c, int32_t ref_slot, int32_t tgt_slot, const float* const* tables,
                             const int32_t* n_points, float pose_out[7], uwt_stats* stats_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !tables || !n_points || !pose_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_points: null argument");
  const uwt_params& p = c->p;
  size_t total = 0;
  int rows = 0;
  for (int l = p.last_level; l <= p.first_level; l++) {
    // the bound this entry has always refused beyond, kept so that what it accepts does not move; it limits nothing here (the
    // records come from the scratch)
    if (n_points[l] < 0 || (size_t)n_points[l] > c->partial_records * (size_t)(kBlock * 32) || (n_points[l] > 0 && !tables[l]))
      return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_points: bad table (null, negative or too many points)");
    total += (size_t)n_points[l];
    rows = std::max(rows, n_points[l]);
  }
  int st = upload_pairs(c, 1, &ref_slot, &tgt_slot);
  if (st) return st;
  // scratch: [a count per level | the evaluations' records | the tables]
  Carve cv(256, c->guard_bytes);
  const size_t o_cnt = cv.take<int>(UWT_MAX_LEVELS), o_recs = cv.take<uint32_t>((size_t)table_slices(rows) * kRecWords),
               o_tab = cv.take<float4>(total);
  st = c->scratch.reserve(c, c->stream, cv, cv.tight());
  if (st) return st;
  st = compute_begin_pairs(c, 1, &ref_slot, &tgt_slot);
  if (st) return st;
  int* d_cnt = Carve::at<int>(c->scratch.p, o_cnt);
  float4* d_tab = Carve::at<float4>(c->scratch.p, o_tab);
  TableLevel lv[UWT_MAX_LEVELS];
  for (int l = p.last_level; l <= p.first_level; l++) {
    if (n_points[l]) HIPCHK(c, hipMemcpyAsync(d_tab, tables[l], (size_t)n_points[l] * 16, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(d_cnt + l), n_points[l], 1, c->stream));
    lv[l] = {{d_tab, d_cnt + l, n_points[l]}, table_slices(n_points[l])};
    d_tab += n_points[l];
  }
  st = enqueue_table_estimate(c, 1, p, lv, Carve::at<uint32_t>(c->scratch.p, o_recs), p.early_exit != 0, {p.weights, p.sampler},
                              c->d_poses, c->d_stats);
  if (!st) st = compute_end(c, c->dep_first, c->dep_n);
  if (st) return st;
  uwt_stats tmp;
  HIPCHK(c, hipMemcpyAsync(pose_out, c->d_poses, sizeof(float) * 7, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&tmp, c->d_stats, sizeof(tmp), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (stats_out) *stats_out = tmp;
  if (tmp.status != UWT_OK)
    return fail(c, UWT_ERR_PAIR_FAILED, std::string("uwt_estimate_pose_points: ") + uwt_status_string(tmp.status));
  return UWT_OK;
}

}  // extern "C"

// ---- what the chained tracking call uses of this unit (declared in uwt_ctx.h) -------------------------------------------------------
int uwt::features_device_begin(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots) {
  int st = check_pair_lists(c, what, n_pairs, ref_slots, tgt_slots);
  if (!st) st = ensure_features(c);
  if (!st) st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
  return st;
}

// features_enqueue behind its staging: the key points and their counts are on the device already, so the grid's slices are the
// bound of any table (a pair's own slice count comes from its producer's count: the bound shows in no bit)
int uwt::features_device_enqueue(uwt_ctx* c, int n_pairs, float* d_poses, uwt_stats* d_stats, const Start& start) {
  int st = enqueue_patch_producer(c, n_pairs, c->d_ref);
  if (st) return st;
  Start gated = start;
  gated.d_gate = c->feat_nkp;
  const TableLevel lv0 = {{c->feat_tab, c->feat_cnt, kFeatTableRows}, table_slices(kFeatTableRows)};
  return enqueue_table_estimate(c, n_pairs, feature_params(c), &lv0, c->feat_recs, false, kIdentityTables, d_poses,
                                reinterpret_cast<StatsOut*>(d_stats), gated);
}

int uwt::candidates_level0_enqueue(uwt_ctx* c, int n, const int* d_slots, double threshold, const float4** tab, size_t* stride,
                                   const int** counts) {
  const LevelK& L = c->lv[0];
  const size_t rows = (size_t)L.gw * L.gh;
  Carve cv(kCandidatesAlign, c->guard_bytes);
  candidates_work_layout(cv, L, n);
  int st = c->cand_tab.reserve(c, c->stream, rows * n * sizeof(float4));
  if (!st) st = c->cand_cnt.reserve(c, c->stream, sizeof(int) * UWT_MAX_LEVELS * (size_t)n);
  if (!st) st = c->cand_work.reserve(c, c->stream, cv);
  if (st) return st;
  *tab = (const float4*)c->cand_tab.p;
  *stride = rows;
  *counts = (const int*)c->cand_cnt.p;
  return enqueue_candidates(c, 0, n, d_slots, threshold, c->cand_work.p, (float4*)c->cand_tab.p, (int*)c->cand_cnt.p);
}
