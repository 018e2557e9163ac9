// uwt_capi.hip — host side of libuwt_hip.so: the C ABI declared in include/uwt.h over the gfx950 kernels.
// HIP only; there is no CPU path in this library.
#include "uwt_ctx.h"

namespace {

// x VEC pixels per thread at the finest slicing, the one a single pair runs with: short blocks, at most kMaxSlices of them per
// level (the records the next launch's fold pulls in).  A lone pair's evaluation is a chain of latencies, and every further group a
// thread walks adds a dependent gather round trip to it: ONE group per thread (round 6; 2 until then) wherever that stays under
// kMaxSlices — 640 x 480: level 1 in 75 blocks, level 2 in 19; level 0 would need 300 and keeps two groups (150 blocks: 300 records
// to fold cost more than the second round trip, measured) — takes the 4 x 10 alignment of one pair from 0.411 to 0.392 ms and the
// reference schedule from 0.126 to 0.120 ms (profiles/r06/EXPERIMENTS.md 10).  Batches coarsen the slicing in enqueue_estimate.
// The f64 partial sums group differently with the slicing — 1e-16 relative, far below the f32 rounding of A and b.
constexpr int kGroupsPerThread = 1;

// the defaults of uwt_tuning (include/uwt.h); measured choices, see the comments at their uses
uwt_tuning default_tuning() {
  uwt_tuning t;
  std::memset(&t, 0, sizeof(t));
  t.split = 2;
  t.split_min = 8;
  t.split_min_px = 32LL * 640 * 480;
  t.stream_bytes = 200LL << 20;
  t.tail_update = 1;
  t.target_blocks = 0;
  t.coarse = 1;
  t.coarse_batch_px = kCoarseMaxPixels;   // e.g. level 3 of 640x480: +0.8 % on the default batch; larger levels lose (2 waves / SIMD)
  t.coarse_weighted = 1;
  t.overlap_gradients = 1;
  t.first_poll = 3;
  t.chained = -1;
  t.speculation = 1;
  t.fused_stages = 1;
  t.pyramid_batch = 1;
  t.typed_loads = 1;
  return t;
}

// Tracker::InitializePyramid (src/Tracker.cpp:297-340): fx halves in double then narrows (:317);
// cx_l = (cx0 + 0.5) / 2^l - 0.5 evaluated in double (:319); invfx = 1 / fx in float (:328).
void init_levels(uwt_ctx* c) {
  const uwt_params& p = c->p;
  float fx = p.fx, fy = p.fy;
  for (int l = 0; l < p.n_levels; l++) {
    if (l > 0) {
      fx = (float)((double)fx * 0.5);
      fy = (float)((double)fy * 0.5);
    }
    uwt_level& I = c->info[l];
    I.w = p.width >> l;    // the point grid: w_[lvl], h_[lvl] (src/Tracker.cpp:312-313)
    I.h = p.height >> l;
    // the level's image: the cv::resize(.., Size(), 0.5, 0.5) chain of src/System.cpp:246-251, dsize = cvRound(ssize * 0.5)
    I.img_w = l == 0 ? p.width : (int32_t)std::lrint((double)c->info[l - 1].img_w * 0.5);   // (lrint: half to even, as cvRound)
    I.img_h = l == 0 ? p.height : (int32_t)std::lrint((double)c->info[l - 1].img_h * 0.5);
    I.pitch = (I.img_w + 3) & ~3;
    I.fx = fx;
    I.fy = fy;
    I.cx = l == 0 ? p.cx : (float)(((double)p.cx + 0.5) / (double)(1 << l) - 0.5);
    I.cy = l == 0 ? p.cy : (float)(((double)p.cy + 0.5) / (double)(1 << l) - 0.5);
    I.invfx = 1.0f / fx;
    I.invfy = 1.0f / fy;
    LevelK& L = c->lv[l];
    L.pitch = I.pitch; L.iw = I.img_w; L.ih = I.img_h; L.gw = I.w; L.gh = I.h;
    L.n = I.pitch * I.img_h;
    L.ng = I.pitch * I.h;
    L.fx = I.fx; L.fy = I.fy; L.cx = I.cx; L.cy = I.cy; L.invfx = I.invfx; L.invfy = I.invfy;
    // "(col - cx) * invfx" (src/Tracker.cpp:1439): MatOp_AddEx::multiply scales s = -cx by invfx in double, convertTo narrows
    L.bx = (float)(-(double)I.cx * (double)I.invfx);
    L.by = (float)(-(double)I.cy * (double)I.invfy);
    L.zscale = (float)((double)p.depth_scale / std::pow(2.0, (double)l));  // src/Tracker.cpp:1266
    L.magic = (uint32_t)((0x100000000ull + (uint64_t)I.pitch - 1) / (uint64_t)I.pitch);
  }
  const int div = 1 << (p.n_levels - 1);
  c->whole = p.width % div == 0 && p.height % div == 0;
}

// rows of w elements, src_pitch elements apart, into rows dst_pitch elements apart (pad columns are never read): four elements per thread
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spread_rows(const T* __restrict__ src, T* __restrict__ dst, int w, size_t src_pitch, size_t dst_pitch,
                                                        size_t rows) {
  const int per_row = (w + 3) >> 2;
  const size_t total = rows * (size_t)per_row;
  for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
    const size_t r = i / (size_t)per_row;
    const int x = (int)(i - r * (size_t)per_row) * 4;
    const T* s = src + r * src_pitch + x;
    T* d = dst + r * dst_pitch + x;
    if (x + 3 < w) {   // a whole group: the device rows start on multiples of four elements (dst_pitch % 4 == 0), so one store
      const T v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
      if constexpr (sizeof(T) == 1) {
        *reinterpret_cast<uint32_t*>(d) = (uint32_t)v0 | ((uint32_t)v1 << 8) | ((uint32_t)v2 << 16) | ((uint32_t)v3 << 24);
      } else {
        *reinterpret_cast<uint2*>(d) = make_uint2((uint32_t)v0 | ((uint32_t)v1 << 16), (uint32_t)v2 | ((uint32_t)v3 << 16));
      }
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (x + j < w) d[j] = s[j];
    }
  }
}

// `rows` host rows of w elements, src_stride BYTES apart, into device rows dst_pitch elements apart: ONE linear copy of the host span
// (first byte of the first row to last byte of the last; what lies between the rows of a strided view belongs to its parent image)
// into the stream's staging area, then k_spread_rows.  A 2-D copy costs about 5 us PER ROW on this runtime (measured: 138
// alignments/s streamed at 725 x 465 against 50 k through this path).  reserve: bytes the staging area should hold at least.
// (the stream's staging area only ever grows; growing waits for the stream that may still read the old one)
static int rows_in(uwt_ctx* c, void* dst, size_t dst_pitch, const void* host, size_t elem, size_t w, size_t src_stride, size_t rows,
                   hipStream_t s, int which, size_t reserve) {
  const size_t span = (rows - 1) * src_stride + w * elem;
  int st = c->stage[which].reserve(c, s, std::max(span, reserve));
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(c->stage[which].p, host, span, hipMemcpyHostToDevice, s));
  const size_t work = rows * ((w + 3) / 4);
  const unsigned blocks = (unsigned)std::min<size_t>((work + kBlock - 1) / kBlock, 1u << 16);
  if (elem == 1)
    hipLaunchKernelGGL(k_spread_rows<uint8_t>, dim3(blocks), dim3(kBlock), 0, s, (const uint8_t*)c->stage[which].p, (uint8_t*)dst, (int)w, src_stride,
                       dst_pitch, rows);
  else
    hipLaunchKernelGGL(k_spread_rows<uint16_t>, dim3(blocks), dim3(kBlock), 0, s, (const uint16_t*)c->stage[which].p, (uint16_t*)dst, (int)w,
                       src_stride / 2, dst_pitch, rows);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// n tightly packed level-0 frames (width x height) into slots first_slot.. of a level-0 plane: one linear copy where the device
// rows are tight too (width a multiple of 4), through the staging area otherwise (a slot is pitch * height)
static int copy_frames_in(uwt_ctx* c, void* plane0, const void* host, size_t elem, int first_slot, int n, hipStream_t s, int which) {
  const size_t w = c->p.width, h = c->p.height, pitch = c->lv[0].pitch;
  unsigned char* dst = (unsigned char*)plane0 + (size_t)first_slot * c->lv[0].n * elem;
  if (pitch == w) {
    HIPCHK(c, hipMemcpyAsync(dst, host, w * h * elem * n, hipMemcpyHostToDevice, s));
    return UWT_OK;
  }
  return rows_in(c, dst, pitch, host, elem, w, w * elem, h * (size_t)n, s, which, w * h * n * (c->p.has_depth ? 2 : 1));   // (the depth frames of the call follow)
}

// one level-0 frame whose host rows are row_stride BYTES apart (a cv::Mat view: Frame::images_[0] = distortion(ROI), src/System.cpp:235)
static int copy_strided_frame_in(uwt_ctx* c, void* plane0, const void* host, size_t elem, size_t row_stride, int slot, hipStream_t s) {
  const size_t w = c->p.width, h = c->p.height, pitch = c->lv[0].pitch;
  unsigned char* dst = (unsigned char*)plane0 + (size_t)slot * c->lv[0].n * elem;
  if (row_stride == w * elem) return copy_frames_in(c, plane0, host, elem, slot, 1, s, 0);
  if (row_stride % elem == 0 && row_stride <= 4 * w * elem)   // the span crosses whole: at most four times the frame's bytes
    return rows_in(c, dst, pitch, host, elem, w, row_stride, h, s, 0, 0);
  HIPCHK(c, hipMemcpy2DAsync(dst, pitch * elem, host, row_stride, w * elem, h, hipMemcpyHostToDevice, s));   // a column out of a very wide parent
  return UWT_OK;
}

constexpr int kFewFrames = 8;   // up to here a frame set takes the one-launch forms (k_pyramid_all, k_scharr3_levels)

template <typename T>
void launch_pyramid_all(uwt_ctx* c, T* const* planes_in, T* const* planes, int n, const int* d_slots, int first_slot, hipStream_t on) {
  PyramidArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  a.src = planes_in[0];
  for (int l = 0; l < c->p.n_levels; l++) {
    a.dst[l] = planes[l];
    a.stride[l] = c->lv[l].n;
    a.pitch[l] = c->lv[l].pitch;
  }
  a.w = c->lv[0].iw;
  a.h = c->lv[0].ih;
  a.n_levels = c->p.n_levels;
  a.slots = d_slots;
  a.first_slot = first_slot;
  const int tiles = ((a.w + 63) / 64) * ((a.h + 63) / 64);
  hipLaunchKernelGGL(k_pyramid_all<T>, dim3(tiles, n), dim3(kBlock), 0, on, a);
}

int prof_begin(uwt_ctx* c, size_t* idx, int lvl = 0, int evaluations = 1) {
  if (c->prof_ev_level.size() < c->ev_used / 2 + 1) { c->prof_ev_level.resize(c->ev_used / 2 + 1); c->prof_ev_evals.resize(c->ev_used / 2 + 1); }
  c->prof_ev_level[c->ev_used / 2] = lvl;
  c->prof_ev_evals[c->ev_used / 2] = evaluations;   // evaluations the bracketed launch stands for (k_coarse: a whole level)
  if (c->ev_used + 2 > c->ev_pool.size()) {
    for (int i = 0; i < 64; i++) {
      hipEvent_t e;
      HIPCHK(c, hipEventCreate(&e));
      c->ev_pool.push_back(e);
    }
  }
  *idx = c->ev_used;
  c->ev_used += 2;
  HIPCHK(c, hipEventRecord(c->ev_pool[*idx], c->stream));
  return UWT_OK;
}

// closes prof_begin's bracket behind the launch on stream s, which evaluated `pixels` pixels `evaluations` times
hipError_t prof_end(uwt_ctx* c, size_t idx, hipStream_t s, long long pixels, int evaluations = 1) {
  c->prof_launches += evaluations;
  c->prof_pixels += pixels * evaluations;
  return hipEventRecord(c->ev_pool[idx + 1], s);
}

// stream s waits for level lvl's gradients, unless it is the first level
hipError_t wait_level(const uwt_ctx* c, hipStream_t s, const hipEvent_t* level_ready, int lvl) {
  return level_ready && lvl != c->p.first_level ? hipStreamWaitEvent(s, level_ready[lvl], 0) : hipSuccess;
}

int prof_collect(uwt_ctx* c) {  // after a stream sync
  for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_pool[i], c->ev_pool[i + 1]));
    c->prof_ms += ms;
    const int lvl = c->prof_ev_level[i / 2];
    if (lvl >= 0 && lvl < UWT_MAX_LEVELS) { c->prof_level_ms[lvl] += ms; c->prof_level_launches[lvl] += c->prof_ev_evals[i / 2]; }
  }
  c->ev_used = 0;
  return UWT_OK;
}

// Slicing follows the batch: the create-time slicing (kGroupsPerThread) gives a single pair enough blocks to spread over the
// chip; a batch that fills it alone runs fewer, longer blocks (less reduction overhead per pixel, fewer records to fold),
// still at least target_blocks per launch.
// fixed (fixed schedules of the batch path, every pair stays to the level's end): a block should also be long enough to carry
// its fixed costs — the matrix set-up, the two-pass LDS fold, the record, the ticket — i.e. 16 groups per thread, as long as
// the launch still fills the chip once (1024 resident blocks).  Level 2 of a 1024-pair batch: 1 slice of 19 groups per thread
// instead of 4 of 5, +4.6 % on that level's launches.  Early-exit schedules keep the finer slicing: pairs leave a level at
// different evaluations and the blocks of those that stay have to fill the chip (coarser: 437 k -> 314 k alignments/s, measured).
void level_slicing(const uwt_ctx* c, int lvl, int n_pairs, int target_blocks, bool fixed, int& groups_per_block, int& slices) {
  const int n_groups = c->lv[lvl].ng / c->vecl[lvl];
  int want = (target_blocks + n_pairs - 1) / n_pairs;
  want = std::max(1, std::min(want, c->slices[lvl]));
  if (fixed) {
    const int by_work = std::max(1, n_groups / (kBlock * 16));
    want = std::min(want, std::max(by_work, (1024 + n_pairs - 1) / n_pairs));
  }
  const int gpt = (n_groups + want * kBlock - 1) / (want * kBlock);
  groups_per_block = gpt * kBlock;
  slices = (n_groups + groups_per_block - 1) / groups_per_block;
}

// Which chained form a call takes, if any.
// Identity weights: the chained flow pays where an alignment is bound by kernel boundaries and dependent round trips, not by
// arithmetic: a few pairs on their own (the drop-in call).  In a batch every block would repeat its pair's update.  Measured at
// 640x480 (round 2, profiles/r03/DESIGN_lab_notes_r01-r03.md): ahead up to 6 pairs in fixed schedules, up to 16 in early-exit
// schedules (half the launches between two read-backs), level from there on (uwt_tuning::chained = 1 / 0 force it on / off).
// Robust weights (round 6): a few pairs per call — the drop-in use with the Tukey / Huber weighting on.
enum class Chained { none, identity, robust };

Chained chained_form(const uwt_ctx* c, int n_pairs) {
  const uwt_params& p = c->p;
  const int chained = c->tn.chained;
  if (p.accumulate_f64 == 0) return Chained::none;
  if (p.sampler == 0 && p.weights == 0 && (chained > 0 || (chained < 0 && n_pairs <= (p.early_exit ? 16 : 6))))
    return Chained::identity;
  if (p.weights != 0 && !c->profiling && !c->compute_only && (chained > 0 || (chained < 0 && n_pairs <= 4)))
    return Chained::robust;
  return Chained::none;
}

// What the synchronous small call (uwt_estimate_pose_batch) asks of the identity-weight chained flow for one call
struct CallOpts {
  bool speculate = false;              // launch a level's usual number of evaluations without reading back, check once at the
                                       // end, redo conservatively if cut short
  InlinePairs pairs = {};              // on: the (at most two) pairs' slots travel in the kernel arguments: no pair list upload
  bool window = false;                 // uwt_track_batch_async: record the window events of the early preparation (uwt_ctx::ev_window)
                                       // where the schedule has a window
};

// The arguments of a k_coarse / k_coarse_w4 / k_coarse_weighted launch but for what differs from site to site: the levels
// (coarse_level, n_levels), resume, u.pair_base and where the pairs' states are kept (state_out).
CoarseArgs coarse_args(const UpdateRule& rule, const StartRec& start, const InlinePairs& pairs) {
  CoarseArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.u.rule = rule;
  ca.start = start;
  ca.pairs = pairs;
  return ca;
}

// Robust weights over the nearest sampler: a coarse level runs in one k_coarse_weighted launch (uwt_tuning::coarse_weighted).  Not in
// the metric Jacobian mode: that kernel keeps 20 bytes of scratch per lane in every form and a metric kernel may have none, so the
// level stays on the per-evaluation launches — the same device functions, the same bits.
bool coarse_weighted_on(const uwt_ctx* c) { return c->tn.coarse_weighted != 0 && c->jacobian != UWT_JACOBIAN_METRIC; }

// level lvl as the i-th of the launch
void coarse_level(uwt_ctx* c, CoarseArgs& ca, int i, int lvl) {
  ca.lv[i] = residual_args(c, lvl);
  ca.lv[i].state = nullptr;
  ca.level_id[i] = lvl;
}

// The chained form of Tracker::EstimatePose for a few pairs (dense points, any level size): one launch step per evaluation —
// each block first applies the update of the previous evaluation (and the level hand-off when a level begins), then
// evaluates — and one k_finish at the end.
// Identity weights (nearest sampler): one k_iterate launch per evaluation; levels x iterations + 1 launches instead of
// 2 x levels x iterations + levels + 2.
// Robust weights: an evaluation is two launches instead of three (scale pass, weighted sums, update): the update of
// evaluation k — and the level hand-off where a level ends — runs at the head of evaluation k + 1's scale pass
// (k_hist_iterate), the weighted sums behind it.  640 x 480, one pair, 4 x 10: 91 launches -> 61.  Same device functions as
// the launches it replaces: the same poses bit for bit.
int enqueue_estimate_chained(uwt_ctx* c, bool robust, int n_pairs, float* d_poses, StatsOut* d_stats,
                             const hipEvent_t* level_ready, const CallOpts& opt, const Start& start) {
  const uwt_params& p = c->p;
  uint32_t* recs[2] = {c->partials, c->partials2};
  PairState* states[2] = {c->state, c->state2};
  int rp = 0, sp = 0;            // parity of the records / states the NEXT evaluation writes
  IterArgs ia;
  std::memset(&ia, 0, sizeof(ia));
  ia.u.rule = update_rule(p, robust);
  ia.start = start.rec(p);        // seeds: read by the first launch alone (mode 0, or k_coarse / k_coarse_weighted without resume)
  // Speculative launching (identity weights, early-exit schedules, the synchronous one- or two-pair call): every read-back of
  // "who is still iterating" costs a host round trip of about two evaluations; instead each level gets the evaluations levels
  // usually take plus one, nothing is read back, and the level switch notes on the device whether a pair was cut short — the
  // caller looks once, behind the results, and redoes the alignment the careful way in that (rare) case.
  const bool speculate = opt.speculate && p.early_exit;
  const int evals = speculate ? std::min(p.max_iters, std::max(c->spec_budget, c->tn.first_poll + 1)) : p.max_iters;
  ia.cut_short = speculate ? &c->d_small->cut : nullptr;
  if (speculate) c->h_small->cut = 0;   // host store into page-locked memory, ahead of the launches that may set it
  ia.pairs = opt.pairs;
  // robust weights: the per-pair residual histograms (and the ticket word of each) start an alignment all-zero; every scale
  // pass leaves them so
  if (robust) HIPCHK(c, hipMemsetAsync(c->hist, 0, sizeof(unsigned int) * kHistBins * n_pairs, c->stream));
  // The coarsest levels — those a single block evaluates — run to their end in one launch, at least one finer level left for
  // the chained launches.
  int start_lvl = p.first_level;
  bool after_coarse = false;
  CoarseArgs ca = coarse_args(ia.u.rule, ia.start, ia.pairs);
  ca.state_out = states[sp ^ 1];     // where the first chained launch looks for its state
  if (!robust) {   // identity weights: up to kCoarseMaxLevels levels in one k_coarse launch
    int nc = 0;
    while (nc < kCoarseMaxLevels && start_lvl - nc > p.last_level && c->lv[start_lvl - nc].ng <= kCoarseMaxPixels) nc++;
    if (nc > 0 && c->tn.coarse && !c->profiling && !c->compute_only) {
      for (int i = 0; i < nc; i++) {
        HIPCHK(c, wait_level(c, c->stream, level_ready, p.first_level - i));
        coarse_level(c, ca, i, p.first_level - i);
      }
      ca.n_levels = nc;
      uwt::launch_coarse_chain(c->stream, launch_sel(c), ca, n_pairs);
      HIPCHK(c, hipGetLastError());
      start_lvl -= nc;
      after_coarse = true;
    }
  } else {   // robust weights over the nearest sampler: one k_coarse_weighted launch per level
    while (coarse_weighted_on(c) && p.sampler == 0 && start_lvl > p.last_level && c->lv[start_lvl].ng <= kCoarseMaxPixels) {
      HIPCHK(c, wait_level(c, c->stream, level_ready, start_lvl));
      coarse_level(c, ca, 0, start_lvl);
      ca.n_levels = 1;
      ca.resume = after_coarse ? 1 : 0;
      uwt::launch_coarse_level(c->stream, launch_sel(c), ca, n_pairs, p.weights);
      HIPCHK(c, hipGetLastError());
      start_lvl--;
      after_coarse = true;
    }
  }
  bool first = true;
  int prev_slices = 0, prev_k = 0, prev_lvl = p.first_level;
  for (int lvl = start_lvl; lvl >= p.last_level; lvl--) {
    HIPCHK(c, wait_level(c, c->stream, level_ready, lvl));
    ResidualArgs ra = residual_args(c, lvl);
    ra.state = nullptr;
    level_slicing(c, lvl, n_pairs, c->tn.target_blocks ? c->tn.target_blocks : 4096, false, ra.groups_per_block, ra.slices);
    int next_poll = c->tn.first_poll;   // see enqueue_estimate
    for (int k = 0; k < evals; k++) {
      ia.mode = first ? (after_coarse ? 3 : 0) : (k == 0 ? 2 : 1);
      ia.u.partials = recs[rp ^ 1];
      ia.u.slices = prev_slices;
      ia.u.k = prev_k;
      ia.prev_lvl = prev_lvl;
      ia.state_in = states[sp ^ 1];
      ia.state_out = states[sp];
      ra.partials = recs[rp];
      if (robust) ra.state = states[sp];   // the weighted launch reads the state the scale pass has just published
      // the update inside launch k belongs to evaluation k - 1: a poll at launch k sees what the separate-kernel flow saw
      // after its update k - 1
      const bool poll = p.early_exit && !speculate && k == next_poll && k < p.max_iters;
      ia.u.active = poll ? c->d_active : nullptr;
      int st = poll ? poll_arm(c) : UWT_OK;
      if (st) return st;
      size_t ev = 0;
      if (c->profiling) {   // (identity weights: the robust form is not taken in a profiled call)
        st = prof_begin(c, &ev, lvl);
        if (st) return st;
        ra.probe = 1;
        c->prof_slices = ra.slices;
        c->prof_pairs = n_pairs;
        c->prof_records = recs[rp];
      }
      if (robust) {
        uwt::launch_hist_iterate(c->stream, launch_sel(c), ra, ia, n_pairs, p.sampler, p.weights, c->hist, c->scale);
        uwt::launch_weighted(c->stream, launch_sel(c), ra, n_pairs, p.sampler, p.weights);
      } else {
        uwt::launch_iterate(c->stream, launch_sel(c), ra, ia, n_pairs);
      }
      HIPCHK(c, hipGetLastError());
      if (c->profiling) HIPCHK(c, prof_end(c, ev, c->stream, (long long)n_pairs * c->lv[lvl].gw * c->lv[lvl].gh));
      first = false;
      prev_slices = ra.slices;
      prev_k = k;
      prev_lvl = lvl;
      rp ^= 1;
      sp ^= 1;
      if (poll) {  // stop launching once every pair has left this level
        bool left = true;
        st = poll_any_left(c, &left);
        if (st) return st;
        if (!left) break;
        next_poll *= 2;
      }
    }
  }
  // the last evaluation's update, the last level's hand-off, results
  ia.mode = 2;
  ia.u.partials = recs[rp ^ 1];
  ia.u.slices = prev_slices;
  ia.u.k = prev_k;
  ia.u.active = nullptr;
  ia.prev_lvl = prev_lvl;
  ia.state_in = states[sp ^ 1];
  // The final state lands in whichever of the two buffers the last evaluation did not read (that depends on the parity of
  // the launch count); nothing reads either buffer after a chained call — results leave through d_poses / d_stats.
  ia.state_out = ia.state_in == c->state ? c->state2 : c->state;
  uwt::launch_finish(c->stream, ia, n_pairs, d_poses, d_stats);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// Tracker::EstimatePose for a batch, enqueued on the context's stream (src/Tracker.cpp:362-597)
int enqueue_estimate(uwt_ctx* c, int n_pairs, float* d_poses, StatsOut* d_stats, const hipEvent_t* level_ready = nullptr,
                     const CallOpts& opt = CallOpts(), const Start& start = Start()) {
  const uwt_params& p = c->p;
  const Chained form = chained_form(c, n_pairs);
  if (form != Chained::none)
    return enqueue_estimate_chained(c, form == Chained::robust, n_pairs, d_poses, d_stats, level_ready, opt, start);
  const int tb = 128;
  const bool general = p.sampler != 0 || p.weights != 0;
  // A batch is cut into parts that run the same schedule on streams of their own (fixed schedules; 16 pairs and the pixels of
  // 32 640x480 pairs or more): the launches of one part run in the gaps of the other's — the tail of a residual launch, the
  // update launch, the kernel boundaries: +2..4 % at 256..1024 pairs, +7..9 % at 32..64 in a pipeline of calls; three parts gain
  // nothing more, four lose (measured).  Results do not depend on it (a pair's blocks, records and state are its own; the
  // slicing is the whole batch's).  Part 0 runs on the context's stream.
  // (early-exit schedules stay on one stream: interleaving the two halves' read-backs was built and gave +1.7 %; so do profiled
  // calls: the read-backs and the events around launches exist with one part only)
  const int parts = (p.early_exit || c->profiling || (long long)n_pairs * c->lv[0].ng < c->tn.split_min_px)
                        ? 1 : std::max(1, std::min(c->tn.split, n_pairs / std::max(1, c->tn.split_min)));
  const int target_blocks = c->tn.target_blocks ? c->tn.target_blocks : (parts >= 2 ? 1024 : 4096);
  // the accumulation kernels stream a level's reference planes past the caches (ResidualArgs::stream_planes) when the batch's
  // planes of that level — u8 + 2 x i16 [+ u16] per reference pixel, the target's u8 — exceed what the 256 MB memory-side cache
  // holds across an evaluation; a smaller batch finds them there again at the next evaluation (uwt_tuning::stream_bytes)
  auto streams = [&](int lvl) -> int {
    return (long long)n_pairs * c->lv[lvl].n * (p.has_depth ? 8 : 6) > c->tn.stream_bytes ? 1 : 0;
  };
  int smax = 1;
  for (int lvl = p.first_level; lvl >= p.last_level; lvl--) {
    int gpb, sl;
    level_slicing(c, lvl, n_pairs, target_blocks, !p.early_exit, gpb, sl);
    smax = std::max(smax, sl);
  }
  // robust weights: the per-pair residual histograms (and the ticket word of each) start an alignment all-zero; every scale
  // pass leaves them so (k_resid_hist_v)
  if (general && p.weights)
    HIPCHK(c, hipMemsetAsync(c->hist, 0, sizeof(unsigned int) * kHistBins * n_pairs, c->stream));
  // The coarsest levels of a batch in ONE launch each (round 3): one block per pair runs the level to its end — evaluation,
  // update, exit test and hand-off on the device, the record in LDS (four blocks per CU) — instead of a residual and an update
  // launch per evaluation whose blocks, a few pixel groups long, run 25-50 % below the level-0 rate.  f64 sums, levels of up to
  // coarse_batch_px pixels (rows of whole groups of four or not: the kernels' VEC switch); identity weights: k_coarse_w4;
  // robust weights over the nearest sampler: k_coarse_weighted (histogram, scale, weighted sums and update of a whole level in
  // one block); the bilinear sampler stays on the launches.  Square pixels with unit factors or not: the kernels' PLAIN switch.
  bool coarse_lvl[UWT_MAX_LEVELS] = {};
  if (p.accumulate_f64 != 0 && (!general || (p.sampler == 0 && p.weights != 0 && coarse_weighted_on(c))) && c->tn.coarse_batch_px > 0 &&
      !c->compute_only && !(c->profiling && p.early_exit))
    for (int lvl = p.first_level; lvl >= p.last_level; lvl--)
      coarse_lvl[lvl] = c->lv[lvl].ng <= c->tn.coarse_batch_px;
  // one coarse level of pairs [base, base + cnt) on stream s; resume: the pairs' states exist (a level ran before this one)
  auto run_coarse = [&](int base, int cnt, hipStream_t s, int lvl, bool resume) -> int {
    // (the seeds are read without resume only; the kernel indexes them by the pair's place in the call)
    CoarseArgs ca = coarse_args(update_rule(p, general), start.rec(p), InlinePairs{});
    coarse_level(c, ca, 0, lvl);
    ca.n_levels = 1;
    ca.u.pair_base = base;
    ca.state_out = c->state;
    ca.resume = resume ? 1 : 0;
    size_t ev = 0;
    if (c->profiling) {
      int st = prof_begin(c, &ev, lvl, p.max_iters);
      if (st) return st;
    }
    uwt::launch_coarse_level(s, launch_sel(c), ca, cnt, general ? p.weights : 0);
    HIPCHK(c, hipGetLastError());
    // (fixed schedules only: the level runs max_iters evaluations; the launch stands for that many)
    if (c->profiling) HIPCHK(c, prof_end(c, ev, s, (long long)cnt * c->lv[lvl].gw * c->lv[lvl].gh, p.max_iters));
    return UWT_OK;
  };
  // tn.tail_update: the update in the tail of the evaluation's launch where the batch runs as parts, on one stream only when
  // forced (see tail_update).  The pairs' ticket counters are zero between launches by construction; a call that an error
  // cut short may have left some.
  const bool tickets = c->tn.tail_update >= (parts > 1 ? 1 : 2);
  const bool tail = tickets && !c->compute_only;
  if (tickets) HIPCHK(c, hipMemsetAsync(c->d_tickets, 0, sizeof(unsigned int) * (size_t)n_pairs, c->stream));
  struct Part { int base, cnt; hipStream_t s; ResidualArgs ra; UpdateArgs ua; };
  Part pt[uwt_ctx::kMaxParts];
  // The window of the early preparation (uwt_ctx::ev_window): once a part has finished level 1 of a schedule that ends on level 0,
  // what is left of it reads the level-0 planes alone.  Identity weights, fixed schedules, any number of parts; no window for a
  // schedule that ends above level 0 or has level 0 alone, nor in a profiled call (its kernels are timed with nothing beside them).
  const bool window = opt.window && !general && !p.early_exit && p.last_level == 0 && p.first_level >= 1 && !c->profiling &&
                      !c->compute_only;
  // every early return below (a failed launch or event call) leaves part streams forked and not joined: drain them before
  // the error reaches the caller, so that uwt_sync / uwt_destroy on the context stream really mean "nothing is running"
  struct JoinGuard {
    uwt_ctx* c; int parts; bool joined = false;
    ~JoinGuard() {
      if (joined) return;
      for (int i = 1; i < parts; i++) (void)hipStreamSynchronize(c->part_stream[i]);
    }
  } guard{c, parts};
  if (parts > 1) HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
  for (int i = 0; i < parts; i++) {
    Part& q = pt[i];
    q.base = (int)((long long)n_pairs * i / parts);
    q.cnt = (int)((long long)n_pairs * (i + 1) / parts) - q.base;
    q.s = i ? c->part_stream[i] : c->stream;
    if (i) HIPCHK(c, hipStreamWaitEvent(q.s, c->ev_fork, 0));
    if (!coarse_lvl[p.first_level]) {
      hipLaunchKernelGGL(k_init_state, dim3((q.cnt + tb - 1) / tb), dim3(tb), 0, q.s, c->state + q.base, q.cnt, start.rec(p, q.base),
                         nullptr);
      HIPCHK(c, hipGetLastError());
    }
  }
  for (int lvl = p.first_level; lvl >= p.last_level; lvl--) {
    for (int i = 0; i < parts; i++) {
      Part& q = pt[i];
      HIPCHK(c, wait_level(c, q.s, level_ready, lvl));
      if (coarse_lvl[lvl]) {
        int st = run_coarse(q.base, q.cnt, q.s, lvl, lvl != p.first_level);
        if (st) return st;
        if (window && lvl == 1) HIPCHK(c, hipEventRecord(c->ev_window[i], q.s));
        continue;
      }
      q.ra = residual_args(c, lvl);
      q.ua = update_args(c, lvl, general);
      q.ra.pair_base = q.ua.pair_base = q.base;
      q.ra.stream_planes = streams(lvl);
      level_slicing(c, lvl, n_pairs, target_blocks, !p.early_exit, q.ra.groups_per_block, q.ra.slices);
      q.ua.slices = q.ra.slices;
      // A pair's records sit at (pair * slices + slice): the place depends on the level's slice count, and the parts are at
      // different levels at times.  A part's records are shifted so that they start at base * smax whatever the level —
      // behind everything the parts before it can touch, inside the buffer (slices <= smax).
      const size_t shift = (size_t)q.base * (size_t)(smax - q.ra.slices) * kRecWords;
      q.ra.partials = c->partials + shift;
      q.ua.partials = c->partials + shift;
    }
    if (coarse_lvl[lvl]) continue;
    // Early exit (one part): the host reads back how many pairs are still iterating after the update of evaluation
    // first_poll - 1, then after twice as many, ...  With the reference's constants a level ends at its third evaluation as a
    // rule (error rises or stalls, src/Tracker.cpp:508), so the first look comes after three (uwt_tuning::first_poll).
    // The read-back is taken one evaluation late (round 3): the count of evaluation k is copied to page-locked memory
    // behind its update, evaluation k + 1 is enqueued, and only then does the host wait for the copy — the GPU works on
    // k + 1 meanwhile instead of idling for the host's round trip (~25 us per look).  When the count says "nobody left",
    // evaluation k + 1 has been enqueued for nothing: its blocks see level_done and return at once (a few us).
    // Several parts: their launches are enqueued in turns, evaluation by evaluation, so that every stream has work from the start.
    LatePoll late(c->tn.first_poll);   // (one part)
    bool level_done = false;
    for (int k = 0; k < p.max_iters && !level_done; k++)
      for (int i = 0; i < parts; i++) {
        Part& q = pt[i];
        size_t ev = 0;
        if (c->profiling) {   // (one part)
          int st = prof_begin(c, &ev, lvl);
          if (st) return st;
          q.ra.probe = 1;
          c->prof_slices = q.ra.slices;
          c->prof_pairs = q.cnt;
          c->prof_records = c->partials;
        }
        q.ua.k = k;
        int st = late.arm(c, q.s, p.early_exit != 0, k, p.max_iters, &q.ua.active);
        if (st) return st;
        if (tail) arm_tail(c, q.ra, q.ua);
        st = general ? launch_general(c, q.s, q.ra, q.cnt, false) : launch_residual(c, q.s, q.ra, q.cnt, false);
        if (st) return st;
        if (c->profiling) HIPCHK(c, prof_end(c, ev, q.s, (long long)q.cnt * c->lv[lvl].gw * c->lv[lvl].gh));
        if (!tail) {
          hipLaunchKernelGGL(k_gn_update, dim3(q.cnt), dim3(kUpdateBlock), 0, q.s, q.ua);
          HIPCHK(c, hipGetLastError());
        }
        st = late.look(c, q.s, &level_done);   // reference-mode early exit: every pair has left this level
        if (st) return st;
        if (level_done) break;
      }
    for (int i = 0; i < parts; i++) {
      hipLaunchKernelGGL(k_level_end, dim3((pt[i].cnt + tb - 1) / tb), dim3(tb), 0, pt[i].s, c->state + pt[i].base, pt[i].cnt, lvl,
                         start.rec(p));
      HIPCHK(c, hipGetLastError());
      if (window && lvl == 1) HIPCHK(c, hipEventRecord(c->ev_window[i], pt[i].s));
    }
  }
  for (int i = 0; i < parts; i++) {
    hipLaunchKernelGGL(k_write_out, dim3((pt[i].cnt + tb - 1) / tb), dim3(tb), 0, pt[i].s, c->state + pt[i].base, pt[i].cnt,
                       d_poses + 7 * (size_t)pt[i].base, d_stats ? d_stats + pt[i].base : nullptr);
    HIPCHK(c, hipGetLastError());
    if (window && parts > 1 && i == 0) HIPCHK(c, hipEventRecord(c->ev_first_end, pt[0].s));   // (where the next call's preparation starts)
    if (i) {
      HIPCHK(c, hipEventRecord(c->ev_join[i], pt[i].s));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[i], 0));
    }
  }
  guard.joined = true;
  if (window) c->win_parts = parts;
  return UWT_OK;
}

// slot-range dependencies between the context stream and the copy stream (uwt_ctx::SlotDep; dep_wait is below)
int dep_note(uwt_ctx* c, uwt_ctx::SlotDep* ring, int& next, bool& dropped, hipStream_t on, int first, int n) {
  uwt_ctx::SlotDep& d = ring[next];
  if (d.used) dropped = true;
  d.first = first; d.n = n; d.used = true;
  HIPCHK(c, hipEventRecord(d.ev, on));
  next = (next + 1) % uwt_ctx::kDeps;
  return UWT_OK;
}

}  // namespace

// ---- what the other host units call too (declared in uwt_ctx.h) -----------------------------------------------------------
namespace uwt {

// UWT_ERR_PAIR_FAILED, naming the first failing pair's status, when any of a batch call's n pairs failed
int first_failure(uwt_ctx* c, const char* what, const uwt_stats* stats, int n) {
  for (int i = 0; i < n; i++)
    if (stats[i].status != UWT_OK)
      return fail(c, UWT_ERR_PAIR_FAILED, std::string(what) + ": at least one pair failed, first status: " +
                                              uwt_status_string(stats[i].status));
  return UWT_OK;
}

// ---- the seeded calls (uwt.h "seeded calls") --------------------------------------------------------------------------------
// the options of a seeded call: null = {0}; handoff in 0..1, reserved words zero
int seed_options(uwt_ctx* c, const char* what, const uwt_seed_options* sopt, Start* out) {
  *out = Start();
  if (!sopt) return UWT_OK;
  if (sopt->handoff < 0 || sopt->handoff > 1)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": uwt_seed_options: handoff outside 0..1");
  for (int32_t r : sopt->reserved)
    if (r) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": uwt_seed_options: reserved word not zero");
  out->keep = sopt->handoff;
  return UWT_OK;
}

// Device seeds may share no byte with an output of the same call: an alignment may be evaluated again by launches that run after
// results were written (the speculative rerun; any later launch form that revisits a pair), and each must find the seed.
int seeds_clear_of_range(uwt_ctx* c, const char* what, const float* d_seeds, int n_pairs, const void* out, size_t bytes) {
  if (!d_seeds || n_pairs < 1 || !out || !bytes) return UWT_OK;
  const uintptr_t s0 = (uintptr_t)d_seeds, s1 = s0 + sizeof(float) * 7 * (size_t)n_pairs, o0 = (uintptr_t)out, o1 = o0 + bytes;
  if (s0 < o1 && o0 < s1) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": the seeds overlap an output of the call");
  return UWT_OK;
}

int seeds_clear_of(uwt_ctx* c, const char* what, const float* d_seeds, int n_pairs, const void* d_poses_out, const void* d_stats_out) {
  if (n_pairs < 1) return UWT_OK;
  int st = seeds_clear_of_range(c, what, d_seeds, n_pairs, d_poses_out, sizeof(float) * 7 * (size_t)n_pairs);
  if (!st) st = seeds_clear_of_range(c, what, d_seeds, n_pairs, d_stats_out, sizeof(uwt_stats) * (size_t)n_pairs);
  return st;
}

// The synchronous forms: the caller's seeds into the context's page-locked block, which the kernels read in place (the calls are
// synchronous: the block is free again when they return).  Null seeds: the identity, nothing staged.  n_pairs in 1..max_pairs.
int stage_host_seeds(uwt_ctx* c, const float* seeds, int n_pairs, Start* start) {
  start->d_seeds = nullptr;
  if (!seeds) return UWT_OK;
  if (!c->h_seeds) {
    HIPCHK(c, hipHostMalloc((void**)&c->h_seeds, sizeof(float) * 7 * (size_t)c->p.max_pairs));
    HIPCHK(c, hipHostGetDevicePointer((void**)&c->d_seeds, c->h_seeds, 0));
  }
  std::memcpy(c->h_seeds, seeds, sizeof(float) * 7 * (size_t)n_pairs);
  start->d_seeds = c->d_seeds;
  return UWT_OK;
}


hipError_t DevBuf::release() {
  const hipError_t e = block ? hipFree(block) : hipSuccess;
  p = block = nullptr, bytes = 0;
  gaps.clear();
  return e;
}

// With guards (uwt_ctx::guard_bytes): [lead | want bytes, the carve's gaps inside | tail], p behind the lead — a multiple of 256, so p
// is aligned as hipMalloc's blocks are; a carve's last gap is its tail.  The gaps are those of THIS use, filled on every use.  A block
// serves carved and plain uses in turn (the shared scratch), so EVERY block is allocated with room for a tail behind `bytes`: a later
// plain use of up to `bytes` finds its tail gap inside the allocation whatever made the block.
int DevBuf::reserve(uwt_ctx* c, hipStream_t stream, size_t want, const Carve* cv) {
  const size_t g = c->guard_bytes, lead = (g + 255) & ~(size_t)255, tail = g && !(cv && cv->guard) ? g : 0;
  if (stream != c->copy) close_window(c);   // an entry's work area (an asynchronous upload's staging is ordered by the slot rings)
  if (want > bytes || (g && !block)) {
    if (block) HIPCHK(c, hipStreamSynchronize(stream));
    HIPCHK(c, release());
    HIPCHK(c, hipMalloc(&block, lead + want + g));
    p = static_cast<unsigned char*>(block) + lead;
    bytes = want;
  }
  if (!g) return UWT_OK;
  gaps.clear();
  gaps.push_back({-(long long)lead, lead, -1});
  if (cv && cv->guard) gaps.insert(gaps.end(), cv->gaps.begin(), cv->gaps.end());
  else gaps.push_back({(long long)want, tail, 0});
  for (const GuardGap& gap : gaps) {
    if (gap.at + (long long)gap.bytes > (long long)(bytes + g)) return fail(c, UWT_ERR_INVALID_ARG, "DevBuf::reserve: a guard gap outside its block");
    if (gap.bytes) HIPCHK(c, hipMemsetAsync(static_cast<unsigned char*>(p) + gap.at, kGuardPattern, gap.bytes, stream));
  }
  return UWT_OK;
}

int DevBuf::reserve(uwt_ctx* c, hipStream_t stream, const Carve& cv) { return reserve(c, stream, cv.total(), &cv); }
int DevBuf::reserve(uwt_ctx* c, hipStream_t stream, const Carve& cv, size_t want) { return reserve(c, stream, want, &cv); }

int DevBuf::adopt(uwt_ctx* c, hipStream_t stream, const Carve& inner, const void* base) {
  const long long shift = static_cast<const unsigned char*>(base) - static_cast<const unsigned char*>(p);
  if (stream != c->copy) close_window(c);
  for (GuardGap gap : inner.gaps) {
    gap.at += shift;
    gap.array += 1000;   // (told apart from the block's own arrays in a report)
    if (gap.at < 0 || gap.at + (long long)gap.bytes > (long long)(bytes + c->guard_bytes))
      return fail(c, UWT_ERR_INVALID_ARG, "DevBuf::adopt: a guard gap outside its block");
    gaps.push_back(gap);
    if (gap.bytes) HIPCHK(c, hipMemsetAsync(static_cast<unsigned char*>(p) + gap.at, kGuardPattern, gap.bytes, stream));
  }
  return UWT_OK;
}

// One step of the resize chain: level plane `src` (sw x sh, rows of src_pitch) -> `dst` (dw x dh = cvRound halves, rows of
// dst_pitch).  src/dst point at slot 0 of the level planes; the frames processed are slots[0..n) if given, else first_slot..+n.
// Whole cells in tight rows of whole groups of four: k_halve; every other size: k_resize_half.
template <typename T>
int launch_resize(uwt_ctx* c, const T* src, T* dst, int sw, int sh, int src_pitch, int dw, int dh, int dst_pitch, size_t sfs,
                  size_t dfs, int n_frames, const int* d_slots, int first_slot, hipStream_t on) {
  if (n_frames == 0) return UWT_OK;
  hipStream_t stream = on ? on : c->stream;
  if (sw == 2 * dw && sh == 2 * dh && dw % 4 == 0) {
    const int groups = (dw / 4) * dh;
    hipLaunchKernelGGL((k_halve<T, 4>), dim3((groups + kBlock - 1) / kBlock, n_frames), dim3(kBlock), 0, stream, src,
                       dst, dw, dh, src_pitch, dst_pitch, sfs, dfs, d_slots, first_slot);
  } else {
    const int groups = (dst_pitch / 4) * dh;
    hipLaunchKernelGGL((k_resize_half<T>), dim3((groups + kBlock - 1) / kBlock, n_frames), dim3(kBlock), 0, stream, src,
                       dst, sw, sh, src_pitch, dw, dh, dst_pitch, sfs, dfs, d_slots, first_slot);
  }
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}
template int launch_resize<uint8_t>(uwt_ctx*, const uint8_t*, uint8_t*, int, int, int, int, int, int, size_t, size_t, int, const int*, int, hipStream_t);
template int launch_resize<uint16_t>(uwt_ctx*, const uint16_t*, uint16_t*, int, int, int, int, int, int, size_t, size_t, int, const int*, int, hipStream_t);

// src/gx/gy point at slot 0 of the level planes; the frames processed are slots[0..n) if given, else first_slot..+n
int launch_scharr(uwt_ctx* c, const uint8_t* src, int16_t* gx, int16_t* gy, int w, int h, int pitch, size_t fs, int n_frames,
                  const int* d_slots, int first_slot, hipStream_t on) {
  if (n_frames == 0) return UWT_OK;
  hipStream_t stream = on ? on : c->stream;
  if (h >= 8 * kGradVRows) {  // four rows per thread on the tall levels
    const int tiles = ((w + kGradVW - 1) / kGradVW) * ((h + 4 * kGradVRows - 1) / (4 * kGradVRows));
    hipLaunchKernelGGL(k_scharr3_v4<4>, dim3(tiles, n_frames), dim3(kBlock), 0, stream, src, gx, gy, w, h, pitch, fs, d_slots,
                       first_slot);
  } else {
    const int tiles = ((w + kGradVW - 1) / kGradVW) * ((h + kGradVRows - 1) / kGradVRows);
    hipLaunchKernelGGL(k_scharr3_v4<1>, dim3(tiles, n_frames), dim3(kBlock), 0, stream, src, gx, gy, w, h, pitch, fs, d_slots,
                       first_slot);
  }
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

LaunchSel launch_sel(const uwt_ctx* c) {
  LaunchSel sel;
  sel.arith = c->p.arith == UWT_ARITH_LEGACY ? kArithLegacy : kArithOpenCV;
  sel.depth = c->p.has_depth != 0;
  sel.acc64 = c->p.accumulate_f64 != 0;
  sel.compute_only = c->compute_only;
  sel.metric = c->jacobian == UWT_JACOBIAN_METRIC;
  return sel;
}

int launch_residual(uwt_ctx* c, hipStream_t s, const ResidualArgs& a, int n_pairs, bool dump) {
  uwt::launch_residual(s, launch_sel(c), a, n_pairs, dump);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

ResidualArgs residual_args(uwt_ctx* c, int lvl, const uwt_params& q) {
  ResidualArgs a;
  std::memset(&a, 0, sizeof(a));
  a.img = c->img[lvl];
  a.gx = c->gx[lvl];
  a.gy = c->gy[lvl];
  a.depth = c->depth[lvl];
  a.ref_slots = c->d_ref;
  a.tgt_slots = c->d_tgt;
  a.state = c->state;
  a.L = c->lv[lvl];
  a.zf = q.z_factor;
  a.af = q.angle_factor;
  a.groups_per_block = c->groups_per_block[lvl];
  a.slices = c->slices[lvl];
  a.partials = c->partials;
  a.scale = c->scale;
  a.gain = q.gain;
  a.typed_loads = c->tn.typed_loads;
  return a;
}

// One residual evaluation on the general path (robust weights and/or bilinear sampler): with weights on, one histogram pass
// estimates the scale first (MedianMat / MedianAbsoluteDeviation, src/Tracker.cpp:1571-1619), then the weighted accumulation runs.
int launch_general(uwt_ctx* c, hipStream_t s, const ResidualArgs& ra, int n_pairs, bool dump) {
  uwt::launch_general(s, launch_sel(c), ra, n_pairs, c->p.sampler, c->p.weights, c->hist, c->scale, dump);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// the update's rule under the constants q; general: the records are the general path's
UpdateRule update_rule(const uwt_params& q, bool general) {
  return {q.max_iters, q.early_exit, q.epsilon, q.gain, general ? 1 : 0, q.arith == UWT_ARITH_LEGACY ? 1 : 0};
}

UpdateArgs update_args(uwt_ctx* c, int lvl, const uwt_params& q, bool general) {
  UpdateArgs ua;
  std::memset(&ua, 0, sizeof(ua));
  ua.partials = c->partials;
  ua.state = c->state;
  ua.slices = c->slices[lvl];
  ua.rule = update_rule(q, general);
  return ua;
}

// the general path's per-pair histograms and scales, for a context created without robust weights (uwt_update_params, the table
// batch's options); each piece is retried on its own after a failed allocation
int ensure_general_buffers(uwt_ctx* c) {
  if (c->hist && c->scale) return UWT_OK;
  const size_t mp = (size_t)c->p.max_pairs;
  if (!c->hist) HIPCHK(c, hipMalloc((void**)&c->hist, sizeof(unsigned int) * kHistBins * mp));
  if (!c->scale) {
    HIPCHK(c, hipMalloc((void**)&c->scale, sizeof(PairScale) * mp));
    HIPCHK(c, hipMemset(c->scale, 0, sizeof(PairScale) * mp));
    HIPCHK(c, hipStreamSynchronize(nullptr));   // (the NULL stream's memset against the context's non-blocking streams: see uwt_create)
  }
  return UWT_OK;
}

// the update of the evaluation `ra` launches, in that launch's tail (tail_update_wave) instead of k_gn_update(ua)
void arm_tail(uwt_ctx* c, ResidualArgs& ra, const UpdateArgs& ua) {
  ra.tail.on = 1;
  ra.tail.tickets = c->d_tickets;
  ra.tail.state = ua.state;
  ra.tail.active = ua.active;
  ra.tail.k = ua.k;
  ra.tail.rule = ua.rule;
}

// Reference-mode early exit, read back synchronously: the launch handed c->d_active counts the pairs still iterating on its
// level.  poll_arm clears the counter ahead of that launch; poll_any_left copies the count back behind it, waits for the
// stream and tells whether any pair is left.
int poll_arm(uwt_ctx* c) {
  HIPCHK(c, hipMemsetAsync(c->d_active, 0, sizeof(int), c->stream));
  return UWT_OK;
}

int poll_any_left(uwt_ctx* c, bool* left) {
  HIPCHK(c, hipMemcpyAsync(c->h_active, c->d_active, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *left = *c->h_active != 0;
  return UWT_OK;
}

// the late form of the batch paths (LatePoll, uwt_ctx.h)
int LatePoll::arm(uwt_ctx* c, hipStream_t s, bool polls, int k, int max_iters, int** active) {
  due = polls && (k + 1 == next) && (k + 1 < max_iters);
  int* counter = c->d_active + (c->poll_seq & 1);
  *active = due ? counter : nullptr;
  if (due) HIPCHK(c, hipMemsetAsync(counter, 0, sizeof(int), s));
  return UWT_OK;
}

int LatePoll::look(uwt_ctx* c, hipStream_t s, bool* none_left) {
  *none_left = false;
  if (pending >= 0) {   // the look at the evaluation before this one, taken while this one runs
    HIPCHK(c, hipEventSynchronize(c->ev_poll[pending]));
    *none_left = c->h_active[pending] == 0;
    pending = -1;
    if (*none_left) return UWT_OK;
  }
  if (due) {
    const int slot = c->poll_seq & 1;
    HIPCHK(c, hipMemcpyAsync(c->h_active + slot, c->d_active + slot, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipEventRecord(c->ev_poll[slot], s));
    pending = slot;
    c->poll_seq++;
    next *= 2;
  }
  return UWT_OK;
}

int dep_wait(uwt_ctx* c, const uwt_ctx::SlotDep* ring, int next, bool dropped, hipStream_t waiter, int first, int n) {
  for (int i = 0; i < uwt_ctx::kDeps; i++) {
    const uwt_ctx::SlotDep& d = ring[i];
    const bool oldest = dropped && i == next;   // ring[next] is the oldest survivor once the ring has wrapped
    if (d.used && (oldest || (d.first < first + n && first < d.first + d.n))) HIPCHK(c, hipStreamWaitEvent(waiter, d.ev, 0));
  }
  return UWT_OK;
}
// a compute call on slots [first, first + n): ordered behind the uploads into them ...
// (and behind the whole of a batch call before it: the window that call left for the next one's early preparation closes)
int compute_begin(uwt_ctx* c, int first, int n) {
  close_window(c);
  return dep_wait(c, c->fresh, c->fresh_next, c->fresh_dropped, c->stream, first, n);
}
// ... and remembered, so that a later upload into them waits for it
int compute_end(uwt_ctx* c, int first, int n) {
  c->busy_seq[c->busy_next] = ++c->ticket_seq;
  return dep_note(c, c->busy, c->busy_next, c->busy_dropped, c->stream, first, n);
}

// the slot range the pair lists of a call name, ordered behind the asynchronous uploads into it (compute_begin) and kept as the
// range the call depends on (compute_end)
int compute_begin_pairs(uwt_ctx* c, int n, const int32_t* slots_a, const int32_t* slots_b) {
  int lo = c->p.max_frames, hi = 0;
  for (int i = 0; i < n; i++) {
    lo = std::min(lo, std::min(slots_a[i], slots_b[i]));
    hi = std::max(hi, std::max(slots_a[i], slots_b[i]) + 1);
  }
  c->dep_first = lo;
  c->dep_n = hi - lo;
  return compute_begin(c, c->dep_first, c->dep_n);
}

// the range checks of a call's pair lists
static int check_pair_lists_range(uwt_ctx* c, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots) {
  if (!ref_slots || !tgt_slots || n_pairs < 1) return fail(c, UWT_ERR_INVALID_ARG, "null pair lists or n_pairs < 1");
  if (n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_CAPACITY, "n_pairs exceeds max_pairs");
  for (int i = 0; i < n_pairs; i++)
    if (ref_slots[i] < 0 || ref_slots[i] >= c->p.max_frames || tgt_slots[i] < 0 || tgt_slots[i] >= c->p.max_frames)
      return fail(c, UWT_ERR_INVALID_ARG, "pair slot out of range");
  return UWT_OK;
}

// The caller's lists are copied before this returns (they may be temporaries): into a pinned staging buffer, then
// asynchronously to the device.  Unchanged lists (the steady state of a resident batch) are not re-sent.
// early false: every entry's form — the lists go to the current device set on the context stream, behind whatever read it.
// early (an open window, track_batch_enqueue): the previous call's launches still read the current set, so new lists go to the
// idle one on the side stream — the caller has made that stream wait for the window events, which lie behind the entry of the
// previous call and so behind the end of every call that read the idle set — and the idle set becomes the current one; lists the
// idle set holds already (a caller that alternates two lists) make it current without a copy.
static int send_pairs(uwt_ctx* c, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, bool early) {
  const size_t block = 2 * (size_t)c->p.max_pairs;
  auto holds = [&](int set) {
    const int* h_ref = c->h_pairs + c->pair_stage[set] * block;
    const int* h_tgt = h_ref + c->p.max_pairs;
    return n_pairs == c->n_pairs_cached[set] && !std::memcmp(h_ref, ref_slots, sizeof(int) * n_pairs) &&
           !std::memcmp(h_tgt, tgt_slots, sizeof(int) * n_pairs);
  };
  auto make_current = [&](int set) {
    c->pair_set = set;
    c->d_ref = c->d_pair_set[set];
    c->d_tgt = c->d_ref + c->p.max_pairs;
  };
  if (holds(c->pair_set)) return UWT_OK;
  const int set = early ? c->pair_set ^ 1 : c->pair_set;
  if (early && holds(set)) {
    make_current(set);
    return UWT_OK;
  }
  int stage = (c->pair_stage_last + 1) % uwt_ctx::kPairStages;
  while (stage == c->pair_stage[0] || stage == c->pair_stage[1]) stage = (stage + 1) % uwt_ctx::kPairStages;
  HIPCHK(c, hipEventSynchronize(c->ev_pairs[stage]));  // the copy that last read this block (at least two lists ago)
  int* h_ref = c->h_pairs + stage * block;
  int* h_tgt = h_ref + c->p.max_pairs;
  std::memcpy(h_ref, ref_slots, sizeof(int) * n_pairs);
  std::memcpy(h_tgt, tgt_slots, sizeof(int) * n_pairs);
  c->pair_stage[set] = c->pair_stage_last = stage;
  c->n_pairs_cached[set] = n_pairs;
  make_current(set);
  hipStream_t s = early ? c->side : c->stream;
  HIPCHK(c, hipMemcpyAsync(c->d_ref, h_ref, sizeof(int) * n_pairs, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->d_tgt, h_tgt, sizeof(int) * n_pairs, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(c->ev_pairs[stage], s));
  return UWT_OK;
}

int upload_pairs(uwt_ctx* c, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots) {
  close_window(c);
  int st = check_pair_lists_range(c, n_pairs, ref_slots, tgt_slots);
  return st ? st : send_pairs(c, n_pairs, ref_slots, tgt_slots, false);
}

// the synchronous form of a batch call enqueued with the context's d_poses / d_stats: both copied back, the stream drained
int read_back_pairs(uwt_ctx* c, const char* what, int n, float* poses_out, uwt_stats* stats_out) {
  close_window(c);
  std::vector<uwt_stats> tmp((size_t)n);
  HIPCHK(c, hipMemcpyAsync(poses_out, c->d_poses, sizeof(float) * 7 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_stats, sizeof(uwt_stats) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (stats_out) std::copy(tmp.begin(), tmp.end(), stats_out);
  return first_failure(c, what, tmp.data(), n);
}

// Every set's n_items arrays of `cap` rows to the same layout in host memory, item i's rows below the set's counts[i] only (the
// rows past an item's count stay as the caller left them): one copy of each set's whole block behind what the context stream
// holds, ONE wait for all of them, the rows picked out on the host.  counts may be the target of a copy enqueued before: it is
// read after the wait.
int rows_to_host(uwt_ctx* c, int cap, int n_items, std::initializer_list<RowSet> sets) {
  close_window(c);
  std::vector<std::vector<unsigned char>> tmp;
  for (const RowSet& s : sets) {
    tmp.emplace_back(s.d_rows ? s.elem_bytes * (size_t)cap * n_items : 0);
    if (s.d_rows) HIPCHK(c, hipMemcpyAsync(tmp.back().data(), s.d_rows, tmp.back().size(), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  size_t k = 0;
  for (const RowSet& s : sets) {
    const unsigned char* rows = tmp[k++].data();
    const size_t item = s.elem_bytes * (size_t)cap;
    for (int i = 0; s.d_rows && i < n_items; i++)
      std::memcpy((unsigned char*)s.host_out + item * i, rows + item * i, s.elem_bytes * (size_t)std::min(std::max(s.counts[i], 0), cap));
  }
  return UWT_OK;
}

// the point tables of n_items frames (frame f's rows at d_rows + f * stride, its full count at d_counts[f]) to the caller: the
// counts are read first, then one copy per frame of its min(count, cap) rows, packed at f * cap in pts_out
int counted_rows_to_host(uwt_ctx* c, const float4* d_rows, size_t stride, const int* d_counts, int n_items, int cap, float* pts_out,
                         int32_t* counts_out) {
  close_window(c);
  HIPCHK(c, hipMemcpyAsync(counts_out, d_counts, sizeof(int) * n_items, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int f = 0; f < n_items; f++) {
    const int k = std::min(counts_out[f], cap);
    if (k > 0)
      HIPCHK(c, hipMemcpyAsync(pts_out + (size_t)f * cap * 4, d_rows + (size_t)f * stride, (size_t)k * 16, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}
}  // namespace uwt

extern "C" {

int uwt_abi_version(void) { return UWT_ABI_VERSION; }

#ifndef UWT_SOURCE_SHA256
#define UWT_SOURCE_SHA256 "unknown (built outside csrc/Makefile)"
#endif
const char* uwt_source_id(void) { return UWT_SOURCE_SHA256; }

const char* uwt_status_string(int status) {
  switch (status) {
    case UWT_OK: return "ok";
    case UWT_ERR_INVALID_ARG: return "invalid argument";
    case UWT_ERR_NO_VALID_POINTS: return "no valid points";
    case UWT_ERR_HIP: return "HIP error";
    case UWT_ERR_NO_DEVICE: return "no gfx950 device";
    case UWT_ERR_CAPACITY: return "capacity exceeded";
    case UWT_ERR_PAIR_FAILED: return "at least one pair failed";
    default: return "unknown status";
  }
}

const char* uwt_last_error(const uwt_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

int uwt_default_params(uwt_params* p, int32_t width, int32_t height, float fx, float fy, float cx, float cy) {
  if (!p) return UWT_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  p->width = width; p->height = height;
  p->fx = fx; p->fy = fy; p->cx = cx; p->cy = cy;
  p->n_levels = 5;          // src/Options.cpp:26
  p->first_level = 4;       // src/Tracker.cpp:368
  p->last_level = 1;        // :369
  p->max_iters = 50;        // :366
  p->epsilon = 0.001f;      // :364
  p->gain = 50.0f;          // :559
  p->z_factor = 1.0f;       // :371
  p->angle_factor = 1.0f;   // :372
  p->depth_scale = 0.0002f; // :1261
  p->initial_error = 50000.0f;  // :393
  p->early_exit = 1;
  p->has_depth = 0;
  p->handoff_scale_t = 0;
  p->accumulate_f64 = 1;
  p->sampler = 0;           // nearest neighbour, round() (src/Tracker.cpp:472)
  p->weights = 0;           // IdentityWeights (src/Tracker.cpp:495)
  p->max_frames = 2;
  p->max_pairs = 1;
  p->device = 0;
  p->arith = UWT_ARITH_OPENCV;
  return UWT_OK;
}

int uwt_create(const uwt_params* p, uwt_ctx** out) {
  if (!p || !out) return UWT_ERR_INVALID_ARG;
  *out = nullptr;
  if (p->n_levels < 1 || p->n_levels > UWT_MAX_LEVELS || p->width < 1 || p->height < 1) return UWT_ERR_INVALID_ARG;
  // any size whose coarsest level still has a point grid (w_[lvl] = width >> lvl >= 1, src/Tracker.cpp:312-313)
  if ((p->width >> (p->n_levels - 1)) < 1 || (p->height >> (p->n_levels - 1)) < 1) return UWT_ERR_INVALID_ARG;
  if (p->first_level >= p->n_levels || p->last_level < 0 || p->last_level > p->first_level) return UWT_ERR_INVALID_ARG;
  if (p->max_iters < 1 || p->max_frames < 1 || p->max_pairs < 1) return UWT_ERR_INVALID_ARG;
  {   // the kernels divide a level's linear index by its row pitch with one multiply (LevelK::magic): index * pitch < 2^32
    const uint64_t pitch0 = ((uint64_t)p->width + 3) & ~3ull;
    if (pitch0 * p->height * pitch0 >= 0x100000000ull) return UWT_ERR_INVALID_ARG;
  }
  if (p->sampler < 0 || p->sampler > 1 || p->weights < 0 || p->weights > 2) return UWT_ERR_INVALID_ARG;
  if (p->sampler == 1 && p->weights == 1) return UWT_ERR_INVALID_ARG;  // the reference's Tukey medians are defined on integer residuals
  if (p->arith != UWT_ARITH_OPENCV && p->arith != UWT_ARITH_LEGACY) return UWT_ERR_INVALID_ARG;
  if (p->has_depth) {   // every depth of every level inside the dense warp's domain (uwt.h "the dense warp's division")
    const double ds = std::fabs((double)p->depth_scale);
    if (!std::isfinite(ds)) return UWT_ERR_INVALID_ARG;
    if (ds != 0.0 && (ds * 32767.0 > UWT_DEPTH_MAX || ds / (double)(1 << (p->n_levels - 1)) < UWT_DEPTH_MIN)) return UWT_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || p->device < 0 || p->device >= ndev) return UWT_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, p->device) != hipSuccess) return UWT_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return UWT_ERR_NO_DEVICE;  // code objects are gfx950 only

  uwt_ctx* c = new (std::nothrow) uwt_ctx();
  if (!c) return UWT_ERR_CAPACITY;
  c->p = *p;
  init_levels(c);
  c->tn = default_tuning();
  size_t max_slices = 1;
  for (int l = 0; l < p->n_levels; l++) {
    c->vecl[l] = 4;
    const int n_groups = c->lv[l].ng / c->vecl[l];
    const int gpt = std::max(kGroupsPerThread, (n_groups + kMaxSlices * kBlock - 1) / (kMaxSlices * kBlock));
    c->groups_per_block[l] = kBlock * gpt;
    c->slices[l] = (n_groups + c->groups_per_block[l] - 1) / c->groups_per_block[l];
    if ((size_t)c->slices[l] > max_slices) max_slices = c->slices[l];
  }
  c->partial_records = max_slices * (size_t)p->max_pairs;

#define CREATE_CHK(expr)                                                             \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) {                                                          \
      std::fprintf(stderr, "uwt_create: %s: %s\n", #expr, hipGetErrorString(e_));    \
      uwt_destroy(c);                                                                \
      return UWT_ERR_HIP;                                                            \
    }                                                                                \
  } while (0)
  CREATE_CHK(hipSetDevice(p->device));
  CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  CREATE_CHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  for (int i = 1; i < uwt_ctx::kMaxParts; i++) {
    CREATE_CHK(hipStreamCreateWithFlags(&c->part_stream[i], hipStreamNonBlocking));
    CREATE_CHK(hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming));
  }
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  CREATE_CHK(hipStreamCreateWithFlags(&c->copy, hipStreamNonBlocking));
  for (int i = 0; i < uwt_ctx::kDeps; i++) {
    CREATE_CHK(hipEventCreateWithFlags(&c->busy[i].ev, hipEventDisableTiming));
    CREATE_CHK(hipEventCreateWithFlags(&c->fresh[i].ev, hipEventDisableTiming));
  }
  for (int i = 0; i < uwt_ctx::kPairStages; i++) CREATE_CHK(hipEventCreateWithFlags(&c->ev_pairs[i], hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_pyramids, hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_side_done, hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_entry, hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_first_end, hipEventDisableTiming));
  for (int i = 0; i < uwt_ctx::kMaxParts; i++) CREATE_CHK(hipEventCreateWithFlags(&c->ev_window[i], hipEventDisableTiming));
  for (int l = 0; l < UWT_MAX_LEVELS; l++) CREATE_CHK(hipEventCreateWithFlags(&c->ev_level[l], hipEventDisableTiming));
  for (int l = 0; l < p->n_levels; l++) {
    const size_t n = (size_t)c->lv[l].n * p->max_frames;
    CREATE_CHK(hipMalloc((void**)&c->img[l], n + 4096));
    CREATE_CHK(hipMalloc((void**)&c->gx[l], n * 2));
    CREATE_CHK(hipMalloc((void**)&c->gy[l], n * 2));
    if (p->has_depth) CREATE_CHK(hipMalloc((void**)&c->depth[l], n * 2));
    if (c->lv[l].pitch != c->lv[l].iw) {   // the pad columns of pitched rows: never part of a result, defined all the same
      CREATE_CHK(hipMemset(c->img[l], 0, n + 4096));
      CREATE_CHK(hipMemset(c->gx[l], 0, n * 2));
      CREATE_CHK(hipMemset(c->gy[l], 0, n * 2));
      if (p->has_depth) CREATE_CHK(hipMemset(c->depth[l], 0, n * 2));
    }
  }
  CREATE_CHK(hipMalloc((void**)&c->state, sizeof(PairState) * p->max_pairs));
  for (int i = 0; i < 2; i++) CREATE_CHK(hipMalloc((void**)&c->d_pair_set[i], sizeof(int) * 2 * (size_t)p->max_pairs));
  c->d_ref = c->d_pair_set[0];
  c->d_tgt = c->d_ref + p->max_pairs;
  CREATE_CHK(hipMalloc((void**)&c->partials, c->partial_records * kRecWords * sizeof(uint32_t)));
  CREATE_CHK(hipMalloc((void**)&c->partials2, c->partial_records * kRecWords * sizeof(uint32_t)));
  CREATE_CHK(hipMalloc((void**)&c->state2, sizeof(PairState) * p->max_pairs));
  CREATE_CHK(hipMalloc((void**)&c->d_poses, sizeof(float) * 7 * p->max_pairs));
  CREATE_CHK(hipMalloc((void**)&c->d_stats, sizeof(StatsOut) * p->max_pairs));
  CREATE_CHK(hipMalloc((void**)&c->d_active, 2 * sizeof(int)));
  CREATE_CHK(hipMalloc((void**)&c->d_tickets, sizeof(unsigned int) * (size_t)c->p.max_pairs));
  CREATE_CHK(hipMemset(c->d_tickets, 0, sizeof(unsigned int) * (size_t)c->p.max_pairs));
  for (int i = 0; i < 2; i++) CREATE_CHK(hipEventCreateWithFlags(&c->ev_poll[i], hipEventDisableTiming));
  CREATE_CHK(hipHostMalloc((void**)&c->h_small, sizeof(uwt_ctx::SmallResults)));
  CREATE_CHK(hipHostGetDevicePointer((void**)&c->d_small, c->h_small, 0));
  if (p->sampler || p->weights) {
    CREATE_CHK(hipMalloc((void**)&c->hist, sizeof(unsigned int) * kHistBins * p->max_pairs));
    CREATE_CHK(hipMalloc((void**)&c->scale, sizeof(PairScale) * p->max_pairs));
    CREATE_CHK(hipMemset(c->scale, 0, sizeof(PairScale) * p->max_pairs));
  }
  CREATE_CHK(hipHostMalloc((void**)&c->h_active, 2 * sizeof(int)));
  CREATE_CHK(hipHostMalloc((void**)&c->h_pairs, sizeof(int) * 2 * p->max_pairs * uwt_ctx::kPairStages));
  std::memset(c->h_pairs, 0xff, sizeof(int) * 2 * p->max_pairs * uwt_ctx::kPairStages);
  // hipMemset returns before the device has run it, and it runs on the NULL stream, which the context's streams (non-blocking) do not
  // wait for: without this the zeros of the pitched planes could land on top of the first upload's rows (seen as rare parity events
  // once uploads into pitched rows became a kernel: profiles/r06/EXPERIMENTS.md 14)
  CREATE_CHK(hipStreamSynchronize(nullptr));
#undef CREATE_CHK
  *out = c;
  return UWT_OK;
}

extern "C++" {
// every buffer of the context that grows on use, by the name uwt_debug_check_guards reports
struct NamedBuf { const char* name; DevBuf* b; };
static std::vector<NamedBuf> growable(uwt_ctx* c) {
  return {{"scratch", &c->scratch}, {"stage[0]", &c->stage[0]}, {"stage[1]", &c->stage[1]}, {"cand_tab", &c->cand_tab},
          {"cand_cnt", &c->cand_cnt}, {"cand_work", &c->cand_work}, {"cand_recs", &c->cand_recs}, {"match_desc", &c->match_desc},
          {"match_cnt", &c->match_cnt}, {"match_part", &c->match_part}, {"match_out", &c->match_out}, {"ransac_buf", &c->ransac_buf},
          {"surf_buf", &c->surf_buf}, {"orb_buf", &c->orb_buf}, {"orb_pat", &c->orb_pat}, {"track_buf", &c->track_buf},
          {"warp_buf", &c->warp_buf}, {"cloud_buf", &c->cloud_buf}, {"sweep_buf", &c->sweep_buf}};
}

static void drain_streams(uwt_ctx* c) {
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->side) (void)hipStreamSynchronize(c->side);  // an aborted uwt_track_batch_async may have left work there
  if (c->copy) (void)hipStreamSynchronize(c->copy);
  for (int i = 1; i < uwt_ctx::kMaxParts; i++)
    if (c->part_stream[i]) (void)hipStreamSynchronize(c->part_stream[i]);
}

}  // extern "C++"

int uwt_debug_guards(uwt_ctx* c, int64_t guard_bytes) {
  if (!c) return UWT_ERR_INVALID_ARG;
  if (guard_bytes < 0 || guard_bytes > (1ll << 24)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_debug_guards: guard_bytes outside 0..2^24");
  (void)hipSetDevice(c->p.device);
  close_window(c);
  drain_streams(c);
  for (const NamedBuf& nb : growable(c)) HIPCHK(c, nb.b->release());
  if (c->orb_pattern_state == 2) c->orb_pattern_state = 1;   // the device copy of the pattern went with orb_pat: the next ORB call sends it
  c->guard_bytes = (size_t)guard_bytes;
  return UWT_OK;
}

int uwt_debug_check_guards(uwt_ctx* c, int64_t* damaged_bytes_out) {
  if (!c || !damaged_bytes_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_debug_check_guards: null argument");
  (void)hipSetDevice(c->p.device);
  drain_streams(c);
  long long damaged = 0;
  std::string first;
  std::vector<unsigned char> host;
  for (const NamedBuf& nb : growable(c))
    for (const GuardGap& gap : nb.b->gaps) {
      if (!gap.bytes) continue;
      host.resize(gap.bytes);
      HIPCHK(c, hipMemcpy(host.data(), static_cast<unsigned char*>(nb.b->p) + gap.at, gap.bytes, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < gap.bytes; i++)
        if (host[i] != kGuardPattern) {
          if (!damaged)
            first = std::string("uwt_debug_check_guards: ") + nb.name + ": the gap behind array " + std::to_string(gap.array) +
                    " is damaged from its byte " + std::to_string(i) + " on (the gap: " + std::to_string(gap.bytes) + " bytes at offset " +
                    std::to_string(gap.at) + ")";
          damaged++;
        }
    }
  *damaged_bytes_out = damaged;
  if (damaged) c->last_error = first;
  return UWT_OK;
}

int uwt_debug_window_open(const uwt_ctx* c, int32_t* out) {
  if (!c || !out) return UWT_ERR_INVALID_ARG;   // (a const context: no last_error to set)
  *out = c->win_open ? 1 : 0;
  return UWT_OK;
}

int uwt_destroy(uwt_ctx* c) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  drain_streams(c);
  for (const NamedBuf& nb : growable(c)) (void)nb.b->release();
  // the fixed-size allocations of uwt_create, uwt_update_params, ensure_features and ransac_need_rows (null: nothing to free)
  for (int l = 0; l < UWT_MAX_LEVELS; l++)
    for (void* p : {(void*)c->img[l], (void*)c->depth[l], (void*)c->gx[l], (void*)c->gy[l]}) (void)hipFree(p);
  for (void* p : {(void*)c->state, (void*)c->d_pair_set[0], (void*)c->d_pair_set[1], (void*)c->partials, (void*)c->partials2, (void*)c->state2,
                  (void*)c->d_poses, (void*)c->d_stats, (void*)c->d_active, (void*)c->d_tickets, (void*)c->hist, (void*)c->scale,
                  (void*)c->feat_tab, (void*)c->feat_cnt, (void*)c->feat_kp, (void*)c->feat_nkp, (void*)c->feat_recs,
                  (void*)c->ransac_need})
    (void)hipFree(p);
  for (void* p : {(void*)c->h_small, (void*)c->h_active, (void*)c->h_pairs, (void*)c->h_feat, (void*)c->h_cloud, (void*)c->h_sweep, (void*)c->h_seeds}) (void)hipHostFree(p);
  auto drop = [](hipEvent_t e) { if (e) (void)hipEventDestroy(e); };
  for (hipEvent_t e : c->ev_poll) drop(e);
  for (hipEvent_t e : c->ev_feat) drop(e);
  for (hipEvent_t e : c->ev_pool) drop(e);
  for (hipEvent_t e : c->ev_join) drop(e);
  for (hipEvent_t e : c->ev_pairs) drop(e);
  for (hipEvent_t e : c->ev_cloud) drop(e);
  for (hipEvent_t e : c->ev_sweep) drop(e);
  for (hipEvent_t e : c->ev_level) drop(e);
  for (hipEvent_t e : c->ev_window) drop(e);
  for (hipEvent_t e : {c->ev_fork, c->ev_pyramids, c->ev_side_done, c->ev_entry, c->ev_first_end}) drop(e);
  for (int i = 0; i < uwt_ctx::kDeps; i++) { drop(c->busy[i].ev); drop(c->fresh[i].ev); }
  for (hipStream_t s : c->part_stream)
    if (s) (void)hipStreamDestroy(s);
  for (hipStream_t s : {c->side, c->copy, c->stream})
    if (s) (void)hipStreamDestroy(s);
  delete c;
  return UWT_OK;
}

int uwt_get_params(const uwt_ctx* c, uwt_params* out) {
  if (!c || !out) return UWT_ERR_INVALID_ARG;
  *out = c->p;
  return UWT_OK;
}

int uwt_get_tuning(const uwt_ctx* c, uwt_tuning* out) {
  if (!c || !out) return UWT_ERR_INVALID_ARG;
  *out = c->tn;
  return UWT_OK;
}

int uwt_set_tuning(uwt_ctx* c, const uwt_tuning* t) {
  if (!c || !t) return UWT_ERR_INVALID_ARG;
  if (t->split < 1 || t->split > uwt_ctx::kMaxParts || t->split_min < 1 || t->split_min_px < 1 || t->stream_bytes < 0 ||
      t->tail_update < 0 || t->tail_update > 2 || t->target_blocks < 0 || t->target_blocks > (1 << 20) || t->coarse_batch_px < 0 ||
      t->coarse_batch_px > (1 << 24) || t->first_poll < 1 || t->first_poll > (1 << 20) || t->chained < -1 || t->chained > 1)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_set_tuning: value out of range");   // (first_poll is doubled and incremented by the schedulers: bounded well inside int)
  (void)hipSetDevice(c->p.device);
  close_window(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->side));   // (joined into the context stream by every call that ended well; an early preparation runs there)
  c->tn = *t;
  c->spec_budget = c->spec_calm = 0;
  for (int32_t* b : {&c->tn.coarse, &c->tn.coarse_weighted, &c->tn.speculation, &c->tn.fused_stages, &c->tn.pyramid_batch, &c->tn.typed_loads})
    *b = *b != 0;
  if (c->tn.overlap_gradients < 0 || c->tn.overlap_gradients > 3) c->tn.overlap_gradients = 1;   // (an on / off switch until the early preparation)
  std::memset(c->tn.reserved, 0, sizeof(c->tn.reserved));
  return UWT_OK;
}

int uwt_get_jacobian(const uwt_ctx* c, int32_t* out) {
  if (!c || !out) return UWT_ERR_INVALID_ARG;
  *out = c->jacobian;
  return UWT_OK;
}

int uwt_set_jacobian(uwt_ctx* c, int32_t mode) {
  if (!c) return UWT_ERR_INVALID_ARG;
  if (mode != UWT_JACOBIAN_REFERENCE && mode != UWT_JACOBIAN_METRIC)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_set_jacobian: mode is neither UWT_JACOBIAN_REFERENCE nor UWT_JACOBIAN_METRIC");
  (void)hipSetDevice(c->p.device);
  close_window(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->side));   // (as uwt_set_tuning)
  c->jacobian = mode;
  c->spec_budget = c->spec_calm = 0;   // another solver: the speculative budget starts over
  return UWT_OK;
}

int uwt_update_params(uwt_ctx* c, const uwt_params* p) {
  if (!c || !p) return UWT_ERR_INVALID_ARG;
  const uwt_params& o = c->p;
  if (p->width != o.width || p->height != o.height || p->fx != o.fx || p->fy != o.fy || p->cx != o.cx || p->cy != o.cy ||
      p->n_levels != o.n_levels || p->has_depth != o.has_depth || p->max_frames != o.max_frames ||
      p->max_pairs != o.max_pairs || p->device != o.device || p->depth_scale != o.depth_scale)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_update_params: geometry / capacity fields differ from the context's");
  if (p->first_level >= p->n_levels || p->last_level < 0 || p->last_level > p->first_level || p->max_iters < 1 ||
      p->sampler < 0 || p->sampler > 1 || p->weights < 0 || p->weights > 2 || (p->sampler == 1 && p->weights == 1) ||
      (p->arith != UWT_ARITH_OPENCV && p->arith != UWT_ARITH_LEGACY))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_update_params: bad solver constants");
  (void)hipSetDevice(o.device);
  close_window(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (p->sampler || p->weights) {
    const int st = ensure_general_buffers(c);
    if (st) return st;
  }
  c->p = *p;
  c->spec_budget = c->spec_calm = 0;   // a new schedule: the speculative budget starts over
  return UWT_OK;
}

int uwt_level_info(const uwt_ctx* c, int32_t lvl, uwt_level* out) {
  if (!c || !out || lvl < 0 || lvl >= c->p.n_levels) return UWT_ERR_INVALID_ARG;
  *out = c->info[lvl];
  return UWT_OK;
}

int uwt_set_frame(uwt_ctx* c, int32_t slot, const uint8_t* gray, size_t row_stride, const uint16_t* depth,
                  size_t depth_row_stride) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !gray || !slot_range_ok(c, slot, 1)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_set_frame: bad slot/pointer");
  const int w = c->p.width;
  if (row_stride < (size_t)w) return fail(c, UWT_ERR_INVALID_ARG, "uwt_set_frame: row stride < width");
  int st0 = compute_begin(c, slot, 1);
  if (st0) return st0;
  if (c->p.has_depth && (!depth || depth_row_stride < (size_t)w * 2)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_set_frame: depth required");
  // tight or strided host rows alike: one linear copy of the span the rows cover, and a kernel that spreads them where either side
  // is pitched (a 2-D copy is issued row by row: 2.3 ms for a 725 x 465 view)
  if ((st0 = copy_strided_frame_in(c, c->img[0], gray, 1, row_stride, slot, c->stream))) return st0;
  if (c->p.has_depth && (st0 = copy_strided_frame_in(c, c->depth[0], depth, 2, depth_row_stride, slot, c->stream))) return st0;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_host_alloc(size_t bytes, void** out) {
  if (!out || !bytes) return UWT_ERR_INVALID_ARG;
  *out = nullptr;
  return hipHostMalloc(out, bytes) == hipSuccess ? UWT_OK : UWT_ERR_HIP;
}

int uwt_host_free(void* p) { return (!p || hipHostFree(p) == hipSuccess) ? UWT_OK : UWT_ERR_HIP; }

int uwt_upload_frames_async(uwt_ctx* c, int32_t first_slot, int32_t n, const uint8_t* gray, const uint16_t* depth) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !gray || !slot_range_ok(c, first_slot, n)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_upload_frames_async: bad range");
  if (n == 0) return UWT_OK;
  // behind the compute work that still reads or writes these slots, beside everything else on the context stream
  int st = dep_wait(c, c->busy, c->busy_next, c->busy_dropped, c->copy, first_slot, n);
  if (st) return st;
  st = copy_frames_in(c, c->img[0], gray, 1, first_slot, n, c->copy, 1);
  if (st) return st;
  if (c->p.has_depth && depth && (st = copy_frames_in(c, c->depth[0], depth, 2, first_slot, n, c->copy, 1))) return st;
  return dep_note(c, c->fresh, c->fresh_next, c->fresh_dropped, c->copy, first_slot, n);
}

int uwt_upload_frames(uwt_ctx* c, int32_t first_slot, int32_t n, const uint8_t* gray, const uint16_t* depth) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !gray || !slot_range_ok(c, first_slot, n)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_upload_frames: bad range");
  int st0 = compute_begin(c, first_slot, n);   // on the context stream: behind asynchronous uploads into the same slots
  if (st0) return st0;
  if (n && (st0 = copy_frames_in(c, c->img[0], gray, 1, first_slot, n, c->stream, 0))) return st0;
  if (c->p.has_depth) {
    if (!depth) return fail(c, UWT_ERR_INVALID_ARG, "uwt_upload_frames: depth required");
    if (n && (st0 = copy_frames_in(c, c->depth[0], depth, 2, first_slot, n, c->stream, 0))) return st0;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

static int plane_ptr(uwt_ctx* c, int slot, int lvl, int plane, void** out, size_t* elem) {
  if (!c || !out || !slot_range_ok(c, slot, 1) || lvl < 0 || lvl >= c->p.n_levels) return UWT_ERR_INVALID_ARG;
  const size_t n = c->lv[lvl].n;
  switch (plane) {
    case UWT_PLANE_IMAGE: *out = c->img[lvl] + slot * n; *elem = 1; break;
    case UWT_PLANE_DEPTH:
      if (!c->p.has_depth) return UWT_ERR_INVALID_ARG;
      *out = c->depth[lvl] + slot * n; *elem = 2; break;
    case UWT_PLANE_GRADX: *out = c->gx[lvl] + slot * n; *elem = 2; break;
    case UWT_PLANE_GRADY: *out = c->gy[lvl] + slot * n; *elem = 2; break;
    default: return UWT_ERR_INVALID_ARG;
  }
  return UWT_OK;
}

int uwt_plane_device_ptr(uwt_ctx* c, int32_t slot, int32_t lvl, int32_t plane, void** out) {
  size_t elem;
  int st = plane_ptr(c, slot, lvl, plane, out, &elem);
  if (c) close_window(c);   // (a caller about to read or write planes itself)
  return st ? fail(c, st, "uwt_plane_device_ptr: bad slot/level/plane") : UWT_OK;
}

int uwt_get_plane(uwt_ctx* c, int32_t slot, int32_t lvl, int32_t plane, void* host_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  void* d;
  size_t elem;
  int st = plane_ptr(c, slot, lvl, plane, &d, &elem);
  if (st || !host_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_get_plane: bad slot/level/plane");
  close_window(c);   // the plane is read behind the call before: the next call's preparation may not overtake the copy
  const LevelK& L = c->lv[lvl];   // the level's image, img_w x img_h, without the pad columns of its rows
  HIPCHK(c, hipMemcpy2DAsync(host_out, (size_t)L.iw * elem, d, (size_t)L.pitch * elem, (size_t)L.iw * elem, L.ih, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

// System::AddFrame's pyramid loop for slots first_slot..+n.  depth_slots (device list of n_depth slots), when given,
// restricts the depth pyramids to those slots: only a pair's reference frame is ever read through its depth
// (src/Tracker.cpp:1266-1272).  on: the stream (null: the context's).
static int enqueue_pyramids(uwt_ctx* c, int first_slot, int n, const int* depth_slots = nullptr, int n_depth = 0, hipStream_t on = nullptr) {
  hipStream_t stream = on ? on : c->stream;
  const bool fused = n <= kFewFrames && c->p.n_levels >= 3 && c->p.n_levels <= kPyrMaxLevels && c->whole && c->lv[0].iw % 4 == 0 &&
                     c->lv[0].ih % 4 == 0 && c->tn.fused_stages;
  if (fused) {   // the whole pyramid of each plane in one launch
    if (n) launch_pyramid_all<uint8_t>(c, c->img, c->img, n, nullptr, first_slot, stream);
    if (c->p.has_depth) {
      if (depth_slots) { if (n_depth) launch_pyramid_all<uint16_t>(c, c->depth, c->depth, n_depth, depth_slots, 0, stream); }
      else if (n) launch_pyramid_all<uint16_t>(c, c->depth, c->depth, n, nullptr, first_slot, stream);
    }
    HIPCHK(c, hipGetLastError());
    return UWT_OK;
  }
  // batches: levels 1..3 in one pass over level 0 (k_pyramid_batch), the levels beyond by the per-level chain
  int l0 = 1;
  if (c->p.n_levels >= 4 && c->lv[0].iw % 16 == 0 && c->lv[0].ih % 8 == 0 && c->tn.pyramid_batch) {
    const int tiles = ((c->lv[0].iw + 127) / 128) * ((c->lv[0].ih + 63) / 64);
    if (n) {
      PyramidBatchArgs<uint8_t> a;
      a.src = c->img[0];
      for (int l = 0; l < 4; l++) { a.stride[l] = c->lv[l].n; a.pitch[l] = c->lv[l].pitch; if (l) a.dst[l - 1] = c->img[l]; }
      a.w = c->lv[0].iw; a.h = c->lv[0].ih; a.slots = nullptr; a.first_slot = first_slot;
      hipLaunchKernelGGL(k_pyramid_batch<uint8_t>, dim3(tiles, n), dim3(kBlock), 0, stream, a);
    }
    const int nd16 = !c->p.has_depth ? 0 : (depth_slots ? n_depth : n);
    if (nd16) {
      PyramidBatchArgs<uint16_t> a;
      a.src = c->depth[0];
      for (int l = 0; l < 4; l++) { a.stride[l] = c->lv[l].n; a.pitch[l] = c->lv[l].pitch; if (l) a.dst[l - 1] = c->depth[l]; }
      a.w = c->lv[0].iw; a.h = c->lv[0].ih; a.slots = depth_slots; a.first_slot = depth_slots ? 0 : first_slot;
      hipLaunchKernelGGL(k_pyramid_batch<uint16_t>, dim3(tiles, nd16), dim3(kBlock), 0, stream, a);
    }
    HIPCHK(c, hipGetLastError());
    l0 = 4;
  }
  for (int l = l0; l < c->p.n_levels; l++) {
    const LevelK& S = c->lv[l - 1];
    const LevelK& D = c->lv[l];
    int st = launch_resize<uint8_t>(c, c->img[l - 1], c->img[l], S.iw, S.ih, S.pitch, D.iw, D.ih, D.pitch, S.n, D.n, n, nullptr, first_slot, stream);
    if (st) return st;
    if (c->p.has_depth) {
      st = depth_slots ? launch_resize<uint16_t>(c, c->depth[l - 1], c->depth[l], S.iw, S.ih, S.pitch, D.iw, D.ih, D.pitch, S.n, D.n, n_depth, depth_slots, 0, stream)
                       : launch_resize<uint16_t>(c, c->depth[l - 1], c->depth[l], S.iw, S.ih, S.pitch, D.iw, D.ih, D.pitch, S.n, D.n, n, nullptr, first_slot, stream);
      if (st) return st;
    }
  }
  return UWT_OK;
}

static int enqueue_gradient_level(uwt_ctx* c, int l, int first_slot, int n, const int* d_slots, hipStream_t on = nullptr) {
  return launch_scharr(c, c->img[l], c->gx[l], c->gy[l], c->lv[l].iw, c->lv[l].ih, c->lv[l].pitch, c->lv[l].n, n, d_slots, first_slot, on);
}

static int enqueue_gradients(uwt_ctx* c, int first_slot, int n, const int* d_slots = nullptr) {
  if (n && n <= kFewFrames && c->p.n_levels <= kGradMaxLevels && c->tn.fused_stages) {   // every level in one launch
    GradLevelsArgs a;
    std::memset(&a, 0, sizeof(a));
    int tiles = 0;
    for (int l = 0; l < c->p.n_levels; l++) {
      a.src[l] = c->img[l]; a.gx[l] = c->gx[l]; a.gy[l] = c->gy[l];
      a.w[l] = c->lv[l].iw; a.h[l] = c->lv[l].ih; a.pitch[l] = c->lv[l].pitch; a.stride[l] = c->lv[l].n;
      tiles += ((a.w[l] + kGradVW - 1) / kGradVW) * ((a.h[l] + kGradVRows - 1) / kGradVRows);
      a.tile_end[l] = tiles;
    }
    a.n_levels = c->p.n_levels;
    a.slots = d_slots;
    a.first_slot = first_slot;
    hipLaunchKernelGGL(k_scharr3_levels, dim3(tiles, n), dim3(kBlock), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return UWT_OK;
  }
  for (int l = 0; l < c->p.n_levels; l++) {
    int st = enqueue_gradient_level(c, l, first_slot, n, d_slots);
    if (st) return st;
  }
  return UWT_OK;
}

int uwt_set_deferred(uwt_ctx* c, int32_t on) {
  if (!c) return UWT_ERR_INVALID_ARG;
  c->deferred = on != 0;
  return UWT_OK;
}

// uwt_build_pyramids / uwt_apply_gradient: `gradients` or the pyramids of slots first_slot..+n, waited for unless deferred
static int prepare_frames(uwt_ctx* c, const char* bad_range, bool gradients, int32_t first_slot, int32_t n) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !slot_range_ok(c, first_slot, n)) return fail(c, UWT_ERR_INVALID_ARG, bad_range);
  int st = compute_begin(c, first_slot, n);
  if (st) return st;
  st = gradients ? enqueue_gradients(c, first_slot, n) : enqueue_pyramids(c, first_slot, n);
  if (st) return st;
  if (!c->deferred) HIPCHK(c, hipStreamSynchronize(c->stream));
  else return compute_end(c, first_slot, n);   // still in flight: a later asynchronous upload into these slots waits for it
  return UWT_OK;
}

int uwt_build_pyramids(uwt_ctx* c, int32_t first_slot, int32_t n) { return prepare_frames(c, "uwt_build_pyramids: bad range", false, first_slot, n); }
int uwt_apply_gradient(uwt_ctx* c, int32_t first_slot, int32_t n) { return prepare_frames(c, "uwt_apply_gradient: bad range", true, first_slot, n); }

// uwt_estimate_pose_batch and its seeded form (seeds null, sopt null: the unseeded call)
static int estimate_pose_batch(uwt_ctx* c, const char* what, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                               float* poses_out, uwt_stats* stats_out, const float* seeds, const uwt_seed_options* sopt) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !poses_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  if (!ref_slots || !tgt_slots || n_pairs < 1) return fail(c, UWT_ERR_INVALID_ARG, "null pair lists or n_pairs < 1");
  if (n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_CAPACITY, "n_pairs exceeds max_pairs");
  Start start;
  int st = seed_options(c, what, sopt, &start);
  if (st) return st;
  st = stage_host_seeds(c, seeds, n_pairs, &start);
  if (st) return st;
  const bool chained = chained_form(c, n_pairs) == Chained::identity;
  CallOpts opt;
  opt.pairs.on = n_pairs <= 2 && chained;
  if (opt.pairs.on) {   // the slots travel in the kernel arguments
    for (int i = 0; i < n_pairs; i++) {
      if (ref_slots[i] < 0 || ref_slots[i] >= c->p.max_frames || tgt_slots[i] < 0 || tgt_slots[i] >= c->p.max_frames)
        return fail(c, UWT_ERR_INVALID_ARG, "pair slot out of range");
      opt.pairs.slots[2 * i] = ref_slots[i];
      opt.pairs.slots[2 * i + 1] = tgt_slots[i];
    }
  } else {
    st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
    if (st) return st;
  }
  st = compute_begin(c, 0, c->p.max_frames);
  if (st) return st;
  std::vector<uwt_stats> tmp(n_pairs);
  // A small batch has its results written by the last kernel straight into page-locked host memory: nothing to copy back.
  const bool small = n_pairs <= uwt_ctx::kSmallBatch;
  static_assert(sizeof(StatsOut) == sizeof(uwt_stats), "stats are copied as they are");
  // One or two pairs under an early-exit schedule are launched speculatively (see enqueue_estimate_chained): no read-back
  // inside the alignment, one look at the "cut short" flag behind the results.  If it is set the alignment is run again with
  // twice the evaluations per level (the budget stays: the next frames of a sequence tend to need what this one needed; it
  // comes down again after kSpecCalm calls that were not cut), and the careful way — read-backs — if that is cut short too.
  opt.speculate = n_pairs <= 2 && c->p.early_exit && !c->profiling && chained && c->tn.speculation;
  for (int attempt = 0; attempt < 3; attempt++) {
    st = enqueue_estimate(c, n_pairs, small ? c->d_small->poses : c->d_poses, small ? c->d_small->stats : c->d_stats, nullptr, opt,
                          start);   // (a rerun starts from the staged seeds again)
    if (st) return st;
    if (!small) {
      HIPCHK(c, hipMemcpyAsync(poses_out, c->d_poses, sizeof(float) * 7 * n_pairs, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_stats, sizeof(uwt_stats) * n_pairs, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (small) {
      std::memcpy(poses_out, c->h_small->poses, sizeof(float) * 7 * n_pairs);
      std::memcpy(tmp.data(), c->h_small->stats, sizeof(uwt_stats) * n_pairs);
    }
    if (!opt.speculate) break;
    const int base = c->tn.first_poll + 1;
    if (c->h_small->cut == 0) {
      if (c->spec_budget > base && ++c->spec_calm >= uwt_ctx::kSpecCalm) { c->spec_budget = std::max(base, c->spec_budget / 2); c->spec_calm = 0; }
      break;
    }
    c->spec_calm = 0;
    c->spec_budget = std::min(c->p.max_iters, 2 * std::max(c->spec_budget, base));
    if (attempt == 1) opt.speculate = false;   // cut short twice: the third run reads back
  }
  if (c->profiling) {
    st = prof_collect(c);
    if (st) return st;
  }
  if (stats_out) std::copy(tmp.begin(), tmp.end(), stats_out);
  return first_failure(c, what, tmp.data(), n_pairs);
}

int uwt_estimate_pose_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                            float* poses_out, uwt_stats* stats_out) {
  return estimate_pose_batch(c, "uwt_estimate_pose_batch", n_pairs, ref_slots, tgt_slots, poses_out, stats_out, nullptr, nullptr);
}

int uwt_default_seed_options(uwt_seed_options* o) {
  if (!o) return UWT_ERR_INVALID_ARG;
  std::memset(o, 0, sizeof(*o));
  return UWT_OK;
}

int uwt_estimate_pose_batch_seeded(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                   float* poses_out, uwt_stats* stats_out, const float* seeds, const uwt_seed_options* sopt) {
  return estimate_pose_batch(c, "uwt_estimate_pose_batch_seeded", n_pairs, ref_slots, tgt_slots, poses_out, stats_out, seeds, sopt);
}

static int track_batch_enqueue(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                               const int32_t* ref_slots, const int32_t* tgt_slots, float* d_poses_out, uwt_stats* d_stats_out,
                               const Start& start = Start()) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c) return fail(c, UWT_ERR_INVALID_ARG, "uwt_track_batch_async: bad argument");
  // the window the previous call left (uwt_ctx::win_open) is taken here whatever becomes of this call: one that fails leaves none
  const bool had_window = c->win_open;
  const int win_parts = c->win_parts;
  close_window(c);
  c->win_parts = 0;
  if (!d_poses_out || !slot_range_ok(c, first_slot, n_frames))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_track_batch_async: bad argument");
  int st = seeds_clear_of(c, "uwt_track_batch_seeded_async", start.d_seeds, n_pairs, d_poses_out, d_stats_out);
  if (st) return st;
  // The side stream pays from ~768 pairs on (+1.7 % at 1024); below, its events cost more than the overlap returns
  // (one pair: +14 % latency).  A profiled call times its kernels alone: nothing runs beside them.  overlap_gradients 3 forces
  // it at any batch size; 2 keeps the side stream and turns the early preparation off.
  const int og = c->tn.overlap_gradients;
  const bool overlap = og != 0 && !c->profiling && (n_pairs >= 768 || og == 3);
  // Early preparation: the previous entry on this context was a batch call that left a window (uwt_ctx::win_open) — this call's
  // pyramids and its gradients of the levels >= 1 go on the side stream behind that call's level 1, under its level 0.
  const bool early = had_window && overlap && og != 2;
  st = check_pair_lists_range(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  // once anything is on the side stream, an error may not leave it running (uwt_sync, uwt_destroy and the next entry look at
  // the context stream, which a call that ends well makes wait for it)
  struct SideGuard {
    uwt_ctx* c; bool armed = false;
    ~SideGuard() { if (armed) (void)hipStreamSynchronize(c->side); }
  } side_guard{c};
  if (early) {
    HIPCHK(c, hipEventRecord(c->ev_entry, c->stream));   // the previous call's end
    side_guard.armed = true;
    for (int i = 0; i < win_parts; i++) HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_window[i], 0));
    // Where in the window: a batch that runs as parts ends staggered — the first part is through about half a millisecond
    // before the last (1024 pairs of 640 x 480), and while the last runs alone half of the chip's block slots stand empty.  The
    // preparation goes there, behind the first part's end: measured +2.5 % on the default batch, against +0.7 % right behind
    // level 1, where its 2 GB of traffic slow both parts' level-0 launches by nearly what it takes alone (profiles/r24).
    if (win_parts > 1) HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_first_end, 0));
  }
  st = send_pairs(c, n_pairs, ref_slots, tgt_slots, early);
  if (st) return st;
  // The alignment reads every slot the pair lists name, and with grad_refs_only the reference slots lie "wherever they
  // lie" (uwt.h): the dependency range of the call is the union of the prepared range and the pairs' slots, so that an
  // asynchronous upload into ANY slot this call reads waits for it, and this call for any upload into them.
  int lo = first_slot, hi = first_slot + n_frames;
  for (int i = 0; i < n_pairs; i++) {
    lo = std::min(lo, std::min(ref_slots[i], tgt_slots[i]));
    hi = std::max(hi, std::max(ref_slots[i], tgt_slots[i]) + 1);
  }
  c->dep_first = lo;
  c->dep_n = hi - lo;
  // behind the asynchronous uploads into these slots (an early preparation reads them on the side stream)
  st = dep_wait(c, c->fresh, c->fresh_next, c->fresh_dropped, c->stream, c->dep_first, c->dep_n);
  if (!st && early) st = dep_wait(c, c->fresh, c->fresh_next, c->fresh_dropped, c->side, c->dep_first, c->dep_n);
  if (st) return st;
  // The tracker reads gradients and depth of the previous (reference) frame only (src/Tracker.cpp:407-408, 1266-1272).
  // grad_refs_only computes those planes — gradients of every level, depth levels 1.. — for the pairs' reference slots
  // alone; otherwise every prepared frame gets them, as System::AddFrame / System::Tracking do for each new frame
  // (src/System.cpp:246-251, 197-213).
  const int* g_slots = grad_refs_only ? c->d_ref : nullptr;   // gradient frames: a slot list or the range
  const int g_first = g_slots ? 0 : first_slot, g_n = g_slots ? n_pairs : n_frames;
  hipStream_t prep = early ? c->side : c->stream;
  st = grad_refs_only ? enqueue_pyramids(c, first_slot, n_frames, c->d_ref, n_pairs, prep) : enqueue_pyramids(c, first_slot, n_frames, nullptr, 0, prep);
  if (st) return st;
  CallOpts opt;
  opt.window = overlap && og != 2;   // (the next call decides for itself; without the switch nothing is recorded)
  if (!overlap) {
    st = enqueue_gradients(c, g_first, g_n, g_slots);
    if (st) return st;
    return enqueue_estimate(c, n_pairs, d_poses_out, reinterpret_cast<StatsOut*>(d_stats_out), nullptr, opt, start);
  }
  HIPCHK(c, hipEventRecord(c->ev_pyramids, prep));
  if (early) {
    // every level >= 1 now, each level's event gating the iterations that read it; level 0 behind the previous call's end (its
    // launches read gx[0] / gy[0] to their last), under this call's coarse levels as without the window.  The context stream
    // waits for the pyramids and the first level's gradients; the part streams fork from it.
    for (int l = c->p.n_levels - 1; l >= 1; l--) {
      st = enqueue_gradient_level(c, l, g_first, g_n, g_slots, c->side);
      if (st) return st;
      HIPCHK(c, hipEventRecord(c->ev_level[l], c->side));
    }
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_entry, 0));
    st = enqueue_gradient_level(c, 0, g_first, g_n, g_slots, c->side);
    if (st) return st;
    HIPCHK(c, hipEventRecord(c->ev_level[0], c->side));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pyramids, 0));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_level[c->p.first_level], 0));
  } else {
    // The alignment starts at the coarsest iterated level and only then needs the finer gradients: the first level's are
    // computed here, the others on the side stream, each level's event gating the iterations that read it.
    st = enqueue_gradient_level(c, c->p.first_level, g_first, g_n, g_slots);
    if (st) return st;
    side_guard.armed = true;
    HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_pyramids, 0));
    for (int l = c->p.first_level - 1; l >= 0; l--) {
      st = enqueue_gradient_level(c, l, g_first, g_n, g_slots, c->side);
      if (st) return st;
      HIPCHK(c, hipEventRecord(c->ev_level[l], c->side));
    }
    for (int l = c->p.first_level + 1; l < c->p.n_levels; l++) {  // levels the solver never iterates: ApplyGradient still fills them
      st = enqueue_gradient_level(c, l, g_first, g_n, g_slots, c->side);
      if (st) return st;
    }
  }
  HIPCHK(c, hipEventRecord(c->ev_side_done, c->side));
  st = enqueue_estimate(c, n_pairs, d_poses_out, reinterpret_cast<StatsOut*>(d_stats_out), c->ev_level, opt, start);
  // whatever follows on the context stream (the next call's pyramids, a plane read-back) is ordered after the side work
  const hipError_t e = hipStreamWaitEvent(c->stream, c->ev_side_done, 0);
  if (st) return st;
  if (e != hipSuccess) return fail(c, UWT_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
  side_guard.armed = false;
  c->win_open = c->win_parts > 0;
  return UWT_OK;
}

int uwt_track_batch_async(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                          const int32_t* ref_slots, const int32_t* tgt_slots, float* d_poses_out, uwt_stats* d_stats_out) {
  int st = track_batch_enqueue(c, first_slot, n_frames, grad_refs_only, n_pairs, ref_slots, tgt_slots, d_poses_out, d_stats_out);
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int uwt_track_batch_seeded_async(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                                 const int32_t* ref_slots, const int32_t* tgt_slots, float* d_poses_out, uwt_stats* d_stats_out,
                                 const float* d_seeds, const uwt_seed_options* sopt) {
  Start start;
  int st = seed_options(c, "uwt_track_batch_seeded_async", sopt, &start);
  if (st) return st;
  start.d_seeds = d_seeds;
  st = track_batch_enqueue(c, first_slot, n_frames, grad_refs_only, n_pairs, ref_slots, tgt_slots, d_poses_out, d_stats_out, start);
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int uwt_track_batch_host_async(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                               const int32_t* ref_slots, const int32_t* tgt_slots, float* h_poses_out, uwt_stats* h_stats_out,
                               int64_t* ticket_out) {
  if (!c || !h_poses_out || !ticket_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_track_batch_host_async: null argument");
  int st = track_batch_enqueue(c, first_slot, n_frames, grad_refs_only, n_pairs, ref_slots, tgt_slots, c->d_poses,
                               reinterpret_cast<uwt_stats*>(c->d_stats));
  if (st) return st;
  // results follow the alignment on the context stream into the caller's (page-locked) buffers; the context's own device
  // buffers are free again before the next call's write-out because the stream is in order
  HIPCHK(c, hipMemcpyAsync(h_poses_out, c->d_poses, sizeof(float) * 7 * n_pairs, hipMemcpyDeviceToHost, c->stream));
  if (h_stats_out)
    HIPCHK(c, hipMemcpyAsync(h_stats_out, c->d_stats, sizeof(uwt_stats) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  st = compute_end(c, c->dep_first, c->dep_n);
  if (st) return st;
  *ticket_out = c->ticket_seq;
  return UWT_OK;
}

int uwt_wait_ticket(uwt_ctx* c, int64_t ticket) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (ticket < 1 || ticket > c->ticket_seq) return fail(c, UWT_ERR_INVALID_ARG, "uwt_wait_ticket: unknown ticket");
  for (int i = 0; i < uwt_ctx::kDeps; i++)
    if (c->busy[i].used && c->busy_seq[i] == ticket) {
      HIPCHK(c, hipEventSynchronize(c->busy[i].ev));
      return UWT_OK;
    }
  // older than the ring: everything recorded before the oldest surviving entry is complete when that entry is
  HIPCHK(c, hipEventSynchronize(c->busy[c->busy_next].ev));
  return UWT_OK;
}

int uwt_sync(uwt_ctx* c) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  HIPCHK(c, hipStreamSynchronize(c->copy));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->side));   // (every call that ended well has joined it into the context stream: nothing left as a rule)
  if (c->profiling) {
    int st = prof_collect(c);
    if (st) return st;
  }
  return UWT_OK;
}

int uwt_stream(uwt_ctx* c, void** out) {
  if (!c || !out) return UWT_ERR_INVALID_ARG;
  close_window(c);
  *out = (void*)c->stream;
  return UWT_OK;
}

int uwt_profile_enable(uwt_ctx* c, int32_t on) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c) return UWT_ERR_INVALID_ARG;
  close_window(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ev_used = 0;
  c->profiling = (on & 1) != 0;
  c->compute_only = (on & 2) != 0;
  c->prof_ms = 0.0;
  c->prof_launches = 0;
  c->prof_pixels = 0;
  for (int l = 0; l < UWT_MAX_LEVELS; l++) { c->prof_level_ms[l] = 0.0; c->prof_level_launches[l] = 0; }
  return UWT_OK;
}

int uwt_profile_read_levels(uwt_ctx* c, double* ms_by_level, int64_t* launches_by_level, int32_t n_levels) {
  if (!c || !ms_by_level || !launches_by_level || n_levels < 1 || n_levels > UWT_MAX_LEVELS) return UWT_ERR_INVALID_ARG;
  for (int l = 0; l < n_levels; l++) { ms_by_level[l] = c->prof_level_ms[l]; launches_by_level[l] = c->prof_level_launches[l]; }
  return UWT_OK;
}

int uwt_profile_read(uwt_ctx* c, double* ms_total, int64_t* launches, int64_t* pixels) {
  if (!c) return UWT_ERR_INVALID_ARG;
  if (ms_total) *ms_total = c->prof_ms;
  if (launches) *launches = c->prof_launches;
  if (pixels) *pixels = c->prof_pixels;
  return UWT_OK;
}

int uwt_profile_clock(uwt_ctx* c, double* shader_ghz) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !shader_ghz) return UWT_ERR_INVALID_ARG;
  *shader_ghz = 0.0;
  if (!c->prof_slices || !c->prof_pairs) return fail(c, UWT_ERR_INVALID_ARG, "no profiled residual launch yet");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int n = std::min(c->prof_pairs, 64);
  double cyc = 0.0, sec = 0.0;
  for (int p = 0; p < n; p++) {  // slice 0 of the first pairs of the last profiled launch
    uint32_t w[2];
    HIPCHK(c, hipMemcpy(w, (c->prof_records ? c->prof_records : c->partials) + ((size_t)p * c->prof_slices) * kRecWords + 60, sizeof(w), hipMemcpyDeviceToHost));
    cyc += (double)w[0];
    sec += (double)w[1] * 1e-8;  // s_memrealtime: 100 MHz
  }
  if (sec > 0.0) *shader_ghz = cyc / sec * 1e-9;
  return UWT_OK;
}

}  // extern "C"
