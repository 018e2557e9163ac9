// uwt_capi.hip — host side of libuwt_hip.so: the C ABI declared in include/uwt.h over the gfx950 kernels.
// HIP only; there is no CPU path in this library.
#include "../../include/uwt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "uwt_launch.h"
#include "uwt_match.h"
#include "uwt_ransac.h"
#include "uwt_surf.h"

using namespace uwt;

static_assert(sizeof(StatsOut) == sizeof(uwt_stats), "uwt_stats layout");

struct uwt_ctx {
  uwt_params p;
  uwt_level info[UWT_MAX_LEVELS];
  LevelK lv[UWT_MAX_LEVELS];
  int vecl[UWT_MAX_LEVELS];             // pixels per vector group at each level: 4 (rows are pitched to whole groups of four)
  bool whole = true;                    // the level-0 size is divisible by 2^(n_levels-1): every level's image is its grid, every cell of
                                        // the resize chain whole (the one-launch pyramid forms apply)
  int slices[UWT_MAX_LEVELS];
  int groups_per_block[UWT_MAX_LEVELS];
  hipStream_t stream = nullptr;
  // Side stream of uwt_track_batch_async: the gradients of the finer levels (HBM-bound) run beside the first, coarse
  // iterations of the alignment (VALU-bound), which only read the coarsest iterated level (uwt_tuning::overlap_gradients).
  hipStream_t side = nullptr;
  static constexpr int kMaxParts = 4;
  int dep_first = 0, dep_n = 0;         // slot range the running tracker call depends on (track_batch_enqueue)
  hipStream_t part_stream[kMaxParts] = {};   // compute streams of parts 1.. of a split batch (part 0: `stream`)
  hipEvent_t ev_fork = nullptr, ev_join[kMaxParts] = {};
  // launch-shape switches (uwt_tuning; defaults: default_tuning()).  split: parts a fixed-schedule batch is cut into (1 = one
  // stream); split_min: pairs per part at least; stream_bytes: a level whose planes of the whole batch exceed this is read
  // non-temporally; split_min_px: level-0 pixels of the batch at least — below, a launch is too short for a second stream to pay
  // (the host enqueues twice as many)
  uwt_tuning tn;
  hipEvent_t ev_pyramids = nullptr, ev_side_done = nullptr, ev_level[UWT_MAX_LEVELS] = {};
  uint8_t* img[UWT_MAX_LEVELS] = {};
  uint16_t* depth[UWT_MAX_LEVELS] = {};
  int16_t* gx[UWT_MAX_LEVELS] = {};
  int16_t* gy[UWT_MAX_LEVELS] = {};
  PairState* state = nullptr;
  int* d_ref = nullptr;
  int* d_tgt = nullptr;
  // pinned staging of the pair lists, a ring of kPairStages [ref(max_pairs) | tgt(max_pairs)] blocks: a new list is
  // written to the next block while the asynchronous copy of the previous one may still be reading its own
  static constexpr int kPairStages = 4;
  int* h_pairs = nullptr;
  hipEvent_t ev_pairs[kPairStages] = {};
  int pair_stage = 0;                   // block holding the lists that are on the device
  int n_pairs_cached = 0;
  // Copy stream + slot-range dependencies (uwt_upload_frames_async): `busy` = compute work enqueued on `stream` that
  // reads or writes a slot range, `fresh` = uploads enqueued on `copy` into a slot range.  An upload waits for the busy
  // entries it overlaps, a compute call for the fresh ones; both rings are in stream order, so once an entry has been
  // dropped the oldest survivor stands for everything before it.
  struct SlotDep { int first = 0, n = 0; hipEvent_t ev = nullptr; bool used = false; };
  static constexpr int kDeps = 8;
  hipStream_t copy = nullptr;
  SlotDep busy[kDeps], fresh[kDeps];
  int busy_next = 0, fresh_next = 0;
  long long ticket_seq = 0;              // compute calls noted so far; busy_seq[i] = the call ring entry i stands for
  long long busy_seq[kDeps] = {};
  bool busy_dropped = false, fresh_dropped = false;
  uint32_t* partials = nullptr;
  uint32_t* partials2 = nullptr;        // the other parity of the chained (k_iterate) flow
  PairState* state2 = nullptr;
  size_t partial_records = 0;
  float* d_poses = nullptr;
  StatsOut* d_stats = nullptr;
  unsigned int* hist = nullptr;         // general path: [pair][2][kHistBins]
  PairScale* scale = nullptr;           // general path: [pair]
  int* d_active = nullptr;              // early-exit polling counters
  unsigned int* d_tickets = nullptr;    // tail update: one counter per pair, zero between launches
  // tn.tail_update: the update in the tail of the residual launch instead of a k_gn_update launch: 1 = where a batch runs as
  // parts on streams of their own (the tail's ~10 us of dependent round trips and the solve run under the other part's
  // launches: +1.2 % at 1024 pairs, +3 % with Huber weights at 256; on one stream the tail is exposed at the end of every
  // launch and loses ~3 us per evaluation to the update launch), 0 = never, 2 = always.  tn.target_blocks: blocks per residual
  // launch the batch-dependent slicing aims at; 0: 1024 for a batch that runs as two halves (one block per slot of the chip),
  // else 4096
  int* h_active = nullptr;              // pinned
  void* scratch = nullptr;              // per-stage entry points
  size_t scratch_bytes = 0;
  // the live call for a batch of pairs (uwt_track_features_batch_async, uwt_obtain_patch_points_batch), allocated on first use:
  // max_pairs tables of kPatchMaxKeypoints x kPatchMaxRows rows and their counts, the key points as the device reads them, the
  // evaluation's records (kFeatMaxSlices per pair), and a pinned staging ring for the caller's key points (as h_pairs)
  float4* feat_tab = nullptr;
  int* feat_cnt = nullptr;
  float2* feat_kp = nullptr;
  int* feat_nkp = nullptr;
  uint32_t* feat_recs = nullptr;
  float* h_feat = nullptr;              // kPairStages blocks of [n (max_pairs ints) | key points (max_pairs x 400 floats)]
  hipEvent_t ev_feat[kPairStages] = {};
  int feat_stage = 0;
  // semi-dense tracking for a batch of pairs (uwt_track_candidates_batch_async), each buffer grown on use to what a call needs:
  // every iterated level's tables (gw x gh rows per pair and level) and counts (UWT_MAX_LEVELS x pairs), the producer's work
  // area for its finest level, and the evaluations' records (the largest level's slice bound per pair)
  float4* cand_tab = nullptr;
  size_t cand_tab_bytes = 0;
  int* cand_cnt = nullptr;
  size_t cand_cnt_bytes = 0;
  void* cand_work = nullptr;
  size_t cand_work_bytes = 0;
  uint32_t* cand_recs = nullptr;
  size_t cand_recs_bytes = 0;
  // descriptor matching (uwt_knn_match_batch, uwt_match_descriptors_batch*), each buffer grown on use to what a call needs: both
  // descriptor sets of every pair, their counts (query | train), the 2-NN parts of both directions, and the synchronous calls' results
  void* match_desc = nullptr;
  size_t match_desc_bytes = 0;
  int* match_cnt = nullptr;
  size_t match_cnt_bytes = 0;
  Knn2* match_part = nullptr;
  size_t match_part_bytes = 0;
  void* match_out = nullptr;
  size_t match_out_bytes = 0;
  // RANSAC inlier selection (uwt_ransac_inliers_batch*): the staged key points of both frames, their counts, the (x, y, x', y')
  // table of every match and, for the synchronous call, its inputs and results — grown on use; and need(k) of the contract for
  // every N in 8..UWT_MATCH_MAX_ROWS, k in 8..N (allocated whole on first use, 33 MB; a row is filled the first time a call can
  // meet its N under the parameters the rows were computed for)
  void* ransac_buf = nullptr;
  size_t ransac_buf_bytes = 0;
  int* ransac_need = nullptr;
  std::vector<int> ransac_need_host;
  std::vector<unsigned char> ransac_row_done;
  double ransac_need_confidence = 0.0;
  int ransac_need_hypotheses = 0;
  // SURF detection and description (uwt_surf_*): per chunk of frames the slot list, the counts, the integral images, the raw
  // candidates with their order keys, and the key points and descriptors before they go to the caller — grown on use
  void* surf_buf = nullptr;
  size_t surf_buf_bytes = 0;
  void* stage[2] = {nullptr, nullptr};  // uploads of frames whose rows are pitched on the device: [0] context stream, [1] copy stream
  size_t stage_bytes[2] = {0, 0};
  bool profiling = false;
  int spec_budget = 0;                  // speculative launching: evaluations a level gets (0: first_poll + 1); doubled when an alignment
                                        // was cut short, halved again after kSpecCalm calls in a row that were not
  int spec_calm = 0;
  static constexpr int kSpecCalm = 64;
  // the synchronous small-batch call: results and the cut-short flag are written by the last kernel straight into this
  // page-locked block (no device-to-host copies)
  static constexpr int kSmallBatch = 8;
  struct SmallResults { float poses[kSmallBatch * 7]; StatsOut stats[kSmallBatch]; int cut; };
  SmallResults* h_small = nullptr;      // pinned, device-visible
  SmallResults* d_small = nullptr;      // its device address
  bool deferred = false;                // uwt_set_deferred: stage calls return once enqueued
  unsigned poll_seq = 0;                // batch path: read-backs alternate between two counters / events (taken one evaluation late)
  hipEvent_t ev_poll[2] = {};
  const uint32_t* prof_records = nullptr;
  bool compute_only = false;            // uwt_profile_enable(ctx, 2): residual launches run their no-memory diagnostic twin
  std::vector<hipEvent_t> ev_pool;      // start/stop pairs
  size_t ev_used = 0;
  double prof_ms = 0.0;
  long long prof_launches = 0, prof_pixels = 0;
  double prof_level_ms[UWT_MAX_LEVELS] = {};        // the same durations by pyramid level (uwt_profile_read_levels)
  long long prof_level_launches[UWT_MAX_LEVELS] = {};
  std::vector<int> prof_ev_level, prof_ev_evals;                      // level of the launch each event pair brackets
  int prof_slices = 0, prof_pairs = 0;   // slicing of the last profiled residual launch (uwt_profile_clock)
  std::string last_error;
};

namespace {

// x VEC pixels per thread at the finest slicing, the one a single pair runs with: short blocks, at most kMaxSlices of them per
// level (the records the next launch's fold pulls in).  A lone pair's evaluation is a chain of latencies, and every further group a
// thread walks adds a dependent gather round trip to it: ONE group per thread (round 6; 2 until then) wherever that stays under
// kMaxSlices — 640 x 480: level 1 in 75 blocks, level 2 in 19; level 0 would need 300 and keeps two groups (150 blocks: 300 records
// to fold cost more than the second round trip, measured) — takes the 4 x 10 alignment of one pair from 0.411 to 0.392 ms and the
// reference schedule from 0.126 to 0.120 ms (profiles/r06/EXPERIMENTS.md 10).  Batches coarsen the slicing in enqueue_estimate.
// The f64 partial sums group differently with the slicing — 1e-16 relative, far below the f32 rounding of A and b.
constexpr int kGroupsPerThread = 1;

int fail(uwt_ctx* c, int code, const std::string& msg) {
  if (c) c->last_error = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                                                   \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess)                                                                                   \
      return fail(ctx, UWT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                     \
  } while (0)

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

int ensure_scratch(uwt_ctx* c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return UWT_OK;
  if (c->scratch) HIPCHK(c, hipFree(c->scratch));
  c->scratch = nullptr;
  c->scratch_bytes = 0;
  HIPCHK(c, hipMalloc(&c->scratch, bytes));
  c->scratch_bytes = bytes;
  return UWT_OK;
}

bool slot_range_ok(const uwt_ctx* c, int first, int n) { return first >= 0 && n >= 0 && (long long)first + n <= c->p.max_frames; }

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

// One step of the resize chain: level plane `src` (sw x sh, rows of src_pitch) -> `dst` (dw x dh = cvRound halves, rows of
// dst_pitch).  src/dst point at slot 0 of the level planes; the frames processed are slots[0..n) if given, else first_slot..+n.
// Whole cells in tight rows of whole groups of four: k_halve; every other size: k_resize_half.
template <typename T>
int launch_resize(uwt_ctx* c, const T* src, T* dst, int sw, int sh, int src_pitch, int dw, int dh, int dst_pitch, size_t sfs,
                  size_t dfs, int n_frames, const int* d_slots = nullptr, int first_slot = 0) {
  if (n_frames == 0) return UWT_OK;
  if (sw == 2 * dw && sh == 2 * dh && dw % 4 == 0) {
    const int groups = (dw / 4) * dh;
    hipLaunchKernelGGL((k_halve<T, 4>), dim3((groups + kBlock - 1) / kBlock, n_frames), dim3(kBlock), 0, c->stream, src,
                       dst, dw, dh, src_pitch, dst_pitch, sfs, dfs, d_slots, first_slot);
  } else {
    const int groups = (dst_pitch / 4) * dh;
    hipLaunchKernelGGL((k_resize_half<T>), dim3((groups + kBlock - 1) / kBlock, n_frames), dim3(kBlock), 0, c->stream, src,
                       dst, sw, sh, src_pitch, dw, dh, dst_pitch, sfs, dfs, d_slots, first_slot);
  }
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
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

// the staging area of a stream's uploads (which: 0 the context stream, 1 the copy stream); it only ever grows, and growing waits for
// the stream that may still read the old one
static int ensure_stage(uwt_ctx* c, int which, size_t bytes, hipStream_t s) {
  if (bytes <= c->stage_bytes[which]) return UWT_OK;
  if (c->stage[which]) {
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipFree(c->stage[which]));
  }
  c->stage[which] = nullptr;
  c->stage_bytes[which] = 0;
  HIPCHK(c, hipMalloc(&c->stage[which], bytes));
  c->stage_bytes[which] = bytes;
  return UWT_OK;
}

// `rows` host rows of w elements, src_stride BYTES apart, into device rows dst_pitch elements apart: ONE linear copy of the host span
// (first byte of the first row to last byte of the last; what lies between the rows of a strided view belongs to its parent image)
// into the stream's staging area, then k_spread_rows.  A 2-D copy costs about 5 us PER ROW on this runtime (measured: 138
// alignments/s streamed at 725 x 465 against 50 k through this path).  reserve: bytes the staging area should hold at least.
static int rows_in(uwt_ctx* c, void* dst, size_t dst_pitch, const void* host, size_t elem, size_t w, size_t src_stride, size_t rows,
                   hipStream_t s, int which, size_t reserve) {
  const size_t span = (rows - 1) * src_stride + w * elem;
  int st = ensure_stage(c, which, std::max(span, reserve), s);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(c->stage[which], host, span, hipMemcpyHostToDevice, s));
  const size_t work = rows * ((w + 3) / 4);
  const unsigned blocks = (unsigned)std::min<size_t>((work + kBlock - 1) / kBlock, 1u << 16);
  if (elem == 1)
    hipLaunchKernelGGL(k_spread_rows<uint8_t>, dim3(blocks), dim3(kBlock), 0, s, (const uint8_t*)c->stage[which], (uint8_t*)dst, (int)w, src_stride,
                       dst_pitch, rows);
  else
    hipLaunchKernelGGL(k_spread_rows<uint16_t>, dim3(blocks), dim3(kBlock), 0, s, (const uint16_t*)c->stage[which], (uint16_t*)dst, (int)w,
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

// cv::resize(src, dst, Size(), 0.5, 0.5) of one host image of any size through pitched scratch planes (rows padded to whole
// groups of four, as the context's level planes are); dst is dw x dh
template <typename T>
int resize_half_host(uwt_ctx* c, const T* src, int sw, int sh, T* dst, int dw, int dh) {
  const size_t sp = ((size_t)sw + 3) & ~(size_t)3, dp = ((size_t)dw + 3) & ~(size_t)3, es = sizeof(T);
  const size_t off = (sp * sh * es + 255) & ~(size_t)255;
  int st = ensure_scratch(c, off + dp * dh * es + 64);
  if (st) return st;
  unsigned char* d = (unsigned char*)c->scratch;
  HIPCHK(c, hipMemcpy2DAsync(d, sp * es, src, (size_t)sw * es, (size_t)sw * es, sh, hipMemcpyHostToDevice, c->stream));
  st = launch_resize<T>(c, (const T*)d, (T*)(d + off), sw, sh, (int)sp, dw, dh, (int)dp, sp * sh, dp * dh, 1);
  if (st) return st;
  HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dw * es, d + off, dp * es, (size_t)dw * es, dh, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

constexpr int kFewFrames = 8;   // up to here a frame set takes the one-launch forms (k_pyramid_all, k_scharr3_levels)

template <typename T>
void launch_pyramid_all(uwt_ctx* c, T* const* planes_in, T* const* planes, int n, const int* d_slots, int first_slot) {
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
  hipLaunchKernelGGL(k_pyramid_all<T>, dim3(tiles, n), dim3(kBlock), 0, c->stream, a);
}

// src/gx/gy point at slot 0 of the level planes; the frames processed are slots[0..n) if given, else first_slot..+n
int launch_scharr(uwt_ctx* c, const uint8_t* src, int16_t* gx, int16_t* gy, int w, int h, int pitch, size_t fs, int n_frames,
                  const int* d_slots = nullptr, int first_slot = 0, hipStream_t on = nullptr) {
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
  return sel;
}

int launch_residual(uwt_ctx* c, hipStream_t s, const ResidualArgs& a, int n_pairs, bool dump) {
  uwt::launch_residual(s, launch_sel(c), a, n_pairs, dump);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

ResidualArgs residual_args(uwt_ctx* c, int lvl) {
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
  a.zf = c->p.z_factor;
  a.af = c->p.angle_factor;
  a.groups_per_block = c->groups_per_block[lvl];
  a.slices = c->slices[lvl];
  a.partials = c->partials;
  a.scale = c->scale;
  a.gain = c->p.gain;
  a.typed_loads = c->tn.typed_loads;
  return a;
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

GeneralArgs general_args(uwt_ctx* c) {
  GeneralArgs ga;
  ga.sampler = c->p.sampler;
  ga.weights = c->p.weights;
  ga.gain = c->p.gain;
  ga.hist = c->hist;
  ga.scale = c->scale;
  return ga;
}

// One residual evaluation on the general path (robust weights and/or bilinear sampler): with weights on, one histogram pass
// estimates the scale first (MedianMat / MedianAbsoluteDeviation, src/Tracker.cpp:1571-1619), then the weighted accumulation runs.
int launch_general(uwt_ctx* c, hipStream_t s, const ResidualArgs& ra, int n_pairs, bool dump) {
  uwt::launch_general(s, launch_sel(c), ra, n_pairs, c->p.sampler, c->p.weights, c->hist, c->scale, dump);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

UpdateArgs update_args(uwt_ctx* c, int lvl) {
  UpdateArgs ua;
  std::memset(&ua, 0, sizeof(ua));
  ua.partials = c->partials;
  ua.state = c->state;
  ua.slices = c->slices[lvl];
  ua.max_iters = c->p.max_iters;
  ua.early_exit = c->p.early_exit;
  ua.epsilon = c->p.epsilon;
  ua.gain = c->p.gain;
  ua.legacy_solve = c->p.arith == UWT_ARITH_LEGACY ? 1 : 0;
  return ua;
}

// the update of the evaluation `ra` launches, in that launch's tail (tail_update_wave) instead of k_gn_update(ua)
void arm_tail(uwt_ctx* c, ResidualArgs& ra, const UpdateArgs& ua) {
  ra.tail.on = 1;
  ra.tail.tickets = c->d_tickets;
  ra.tail.state = ua.state;
  ra.tail.active = ua.active;
  ra.tail.k = ua.k;
  ra.tail.max_iters = ua.max_iters;
  ra.tail.early_exit = ua.early_exit;
  ra.tail.general = ua.general;
  ra.tail.legacy_solve = ua.legacy_solve;
  ra.tail.epsilon = ua.epsilon;
  ra.tail.gain = ua.gain;
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
  bool inline_pairs = false;           // the (at most two) pairs' slots travel in the kernel arguments: no pair list upload
  int pair_slots[4] = {0, 0, 0, 0};    // ref 0, tgt 0, ref 1, tgt 1
};

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
                             const hipEvent_t* level_ready, const CallOpts& opt) {
  const uwt_params& p = c->p;
  uint32_t* recs[2] = {c->partials, c->partials2};
  PairState* states[2] = {c->state, c->state2};
  int rp = 0, sp = 0;            // parity of the records / states the NEXT evaluation writes
  IterArgs ia;
  std::memset(&ia, 0, sizeof(ia));
  ia.u.max_iters = p.max_iters;
  ia.u.early_exit = p.early_exit;
  ia.u.epsilon = p.epsilon;
  ia.u.gain = p.gain;
  ia.u.general = robust ? 1 : 0;
  ia.u.legacy_solve = p.arith == UWT_ARITH_LEGACY ? 1 : 0;
  ia.scale_t = p.handoff_scale_t;
  ia.initial_error = p.initial_error;
  // Speculative launching (identity weights, early-exit schedules, the synchronous one- or two-pair call): every read-back of
  // "who is still iterating" costs a host round trip of about two evaluations; instead each level gets the evaluations levels
  // usually take plus one, nothing is read back, and the level switch notes on the device whether a pair was cut short — the
  // caller looks once, behind the results, and redoes the alignment the careful way in that (rare) case.
  const bool speculate = opt.speculate && p.early_exit;
  const int evals = speculate ? std::min(p.max_iters, std::max(c->spec_budget, c->tn.first_poll + 1)) : p.max_iters;
  ia.cut_short = speculate ? &c->d_small->cut : nullptr;
  if (speculate) c->h_small->cut = 0;   // host store into page-locked memory, ahead of the launches that may set it
  ia.inline_pairs = opt.inline_pairs ? 1 : 0;
  for (int i = 0; i < 4; i++) ia.pair_slots[i] = opt.pair_slots[i];
  // robust weights: the per-pair residual histograms (and the ticket word of each) start an alignment all-zero; every scale
  // pass leaves them so
  if (robust) HIPCHK(c, hipMemsetAsync(c->hist, 0, sizeof(unsigned int) * kHistBins * n_pairs, c->stream));
  // The coarsest levels — those a single block evaluates — run to their end in one launch, at least one finer level left for
  // the chained launches.
  int start_lvl = p.first_level;
  bool after_coarse = false;
  CoarseArgs ca;
  std::memset(&ca, 0, sizeof(ca));
  ca.u = ia.u;
  ca.state_out = states[sp ^ 1];     // where the first chained launch looks for its state
  ca.scale_t = ia.scale_t;
  ca.initial_error = ia.initial_error;
  ca.inline_pairs = ia.inline_pairs;
  for (int i = 0; i < 4; i++) ca.pair_slots[i] = ia.pair_slots[i];
  if (!robust) {   // identity weights: up to kCoarseMaxLevels levels in one k_coarse launch
    int nc = 0;
    while (nc < kCoarseMaxLevels && start_lvl - nc > p.last_level && c->lv[start_lvl - nc].ng <= kCoarseMaxPixels) nc++;
    if (nc > 0 && c->tn.coarse && !c->profiling && !c->compute_only) {
      for (int i = 0; i < nc; i++) {
        const int lvl = p.first_level - i;
        if (level_ready && lvl != p.first_level) HIPCHK(c, hipStreamWaitEvent(c->stream, level_ready[lvl], 0));  // its gradients
        ca.lv[i] = residual_args(c, lvl);
        ca.lv[i].state = nullptr;
        ca.level_id[i] = lvl;
      }
      ca.n_levels = nc;
      uwt::launch_coarse_chain(c->stream, launch_sel(c), ca, n_pairs);
      HIPCHK(c, hipGetLastError());
      start_lvl -= nc;
      after_coarse = true;
    }
  } else {   // robust weights over the nearest sampler: one k_coarse_weighted launch per level
    while (c->tn.coarse_weighted && p.sampler == 0 && start_lvl > p.last_level && c->lv[start_lvl].ng <= kCoarseMaxPixels) {
      if (level_ready && start_lvl != p.first_level) HIPCHK(c, hipStreamWaitEvent(c->stream, level_ready[start_lvl], 0));  // its gradients
      ca.lv[0] = residual_args(c, start_lvl);
      ca.lv[0].state = nullptr;
      ca.level_id[0] = start_lvl;
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
    if (level_ready && lvl != p.first_level) HIPCHK(c, hipStreamWaitEvent(c->stream, level_ready[lvl], 0));  // its gradients
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
      if (c->profiling) {
        HIPCHK(c, hipEventRecord(c->ev_pool[ev + 1], c->stream));
        c->prof_launches += 1;
        c->prof_pixels += (long long)n_pairs * c->lv[lvl].gw * c->lv[lvl].gh;
      }
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
                     const CallOpts& opt = CallOpts()) {
  const uwt_params& p = c->p;
  const Chained form = chained_form(c, n_pairs);
  if (form != Chained::none)
    return enqueue_estimate_chained(c, form == Chained::robust, n_pairs, d_poses, d_stats, level_ready, opt);
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
  if (p.accumulate_f64 != 0 && (!general || (p.sampler == 0 && p.weights != 0 && c->tn.coarse_weighted)) && c->tn.coarse_batch_px > 0 &&
      !c->compute_only && !(c->profiling && p.early_exit))
    for (int lvl = p.first_level; lvl >= p.last_level; lvl--)
      coarse_lvl[lvl] = c->lv[lvl].ng <= c->tn.coarse_batch_px;
  // one coarse level of pairs [base, base + cnt) on stream s; resume: the pairs' states exist (a level ran before this one)
  auto run_coarse = [&](int base, int cnt, hipStream_t s, int lvl, bool resume) -> int {
    CoarseArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    ca.lv[0] = residual_args(c, lvl);
    ca.lv[0].state = nullptr;
    ca.level_id[0] = lvl;
    ca.n_levels = 1;
    UpdateArgs u = update_args(c, lvl);
    u.pair_base = base;
    ca.u = u;
    ca.state_out = c->state;
    ca.scale_t = p.handoff_scale_t;
    ca.initial_error = p.initial_error;
    ca.resume = resume ? 1 : 0;
    size_t ev = 0;
    if (c->profiling) {
      int st = prof_begin(c, &ev, lvl, p.max_iters);
      if (st) return st;
    }
    uwt::launch_coarse_level(s, launch_sel(c), ca, cnt, general ? p.weights : 0);
    HIPCHK(c, hipGetLastError());
    if (c->profiling) {   // (fixed schedules only: the level runs max_iters evaluations; the launch stands for that many)
      HIPCHK(c, hipEventRecord(c->ev_pool[ev + 1], s));
      c->prof_launches += p.max_iters;
      c->prof_pixels += (long long)cnt * c->lv[lvl].gw * c->lv[lvl].gh * p.max_iters;
    }
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
      hipLaunchKernelGGL(k_init_state, dim3((q.cnt + tb - 1) / tb), dim3(tb), 0, q.s, c->state + q.base, q.cnt, p.initial_error);
      HIPCHK(c, hipGetLastError());
    }
  }
  for (int lvl = p.first_level; lvl >= p.last_level; lvl--) {
    for (int i = 0; i < parts; i++) {
      Part& q = pt[i];
      if (level_ready && lvl != p.first_level) HIPCHK(c, hipStreamWaitEvent(q.s, level_ready[lvl], 0));  // its gradients
      if (coarse_lvl[lvl]) {
        int st = run_coarse(q.base, q.cnt, q.s, lvl, lvl != p.first_level);
        if (st) return st;
        continue;
      }
      q.ra = residual_args(c, lvl);
      q.ua = update_args(c, lvl);
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
      if (general) q.ua.general = 1;
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
    int next_poll = c->tn.first_poll;
    int pending = -1;   // slot of the look not yet taken
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
        const bool poll = p.early_exit && (k + 1 == next_poll) && (k + 1 < p.max_iters);   // (one part)
        const int slot = c->poll_seq & 1;
        q.ua.active = poll ? c->d_active + slot : nullptr;
        if (poll) HIPCHK(c, hipMemsetAsync(c->d_active + slot, 0, sizeof(int), q.s));
        if (tail) arm_tail(c, q.ra, q.ua);
        int st = general ? launch_general(c, q.s, q.ra, q.cnt, false) : launch_residual(c, q.s, q.ra, q.cnt, false);
        if (st) return st;
        if (c->profiling) {
          HIPCHK(c, hipEventRecord(c->ev_pool[ev + 1], q.s));
          c->prof_launches += 1;
          c->prof_pixels += (long long)q.cnt * c->lv[lvl].gw * c->lv[lvl].gh;
        }
        if (!tail) {
          hipLaunchKernelGGL(k_gn_update, dim3(q.cnt), dim3(kUpdateBlock), 0, q.s, q.ua);
          HIPCHK(c, hipGetLastError());
        }
        if (pending >= 0) {   // the look at the evaluation before this one, taken while this one runs
          HIPCHK(c, hipEventSynchronize(c->ev_poll[pending]));
          level_done = c->h_active[pending] == 0;   // reference-mode early exit: every pair has left this level
          pending = -1;
          if (level_done) break;
        }
        if (poll) {
          HIPCHK(c, hipMemcpyAsync(c->h_active + slot, c->d_active + slot, sizeof(int), hipMemcpyDeviceToHost, q.s));
          HIPCHK(c, hipEventRecord(c->ev_poll[slot], q.s));
          pending = slot;
          c->poll_seq++;
          next_poll *= 2;
        }
      }
    for (int i = 0; i < parts; i++) {
      hipLaunchKernelGGL(k_level_end, dim3((pt[i].cnt + tb - 1) / tb), dim3(tb), 0, pt[i].s, c->state + pt[i].base, pt[i].cnt, lvl,
                         p.handoff_scale_t, p.initial_error);
      HIPCHK(c, hipGetLastError());
    }
  }
  for (int i = 0; i < parts; i++) {
    hipLaunchKernelGGL(k_write_out, dim3((pt[i].cnt + tb - 1) / tb), dim3(tb), 0, pt[i].s, c->state + pt[i].base, pt[i].cnt,
                       d_poses + 7 * (size_t)pt[i].base, d_stats ? d_stats + pt[i].base : nullptr);
    HIPCHK(c, hipGetLastError());
    if (i) {
      HIPCHK(c, hipEventRecord(c->ev_join[i], pt[i].s));
      HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[i], 0));
    }
  }
  guard.joined = true;
  return UWT_OK;
}

// ---- slot-range dependencies between the context stream and the copy stream --------------------------------------
int dep_note(uwt_ctx* c, uwt_ctx::SlotDep* ring, int& next, bool& dropped, hipStream_t on, int first, int n) {
  uwt_ctx::SlotDep& d = ring[next];
  if (d.used) dropped = true;
  d.first = first; d.n = n; d.used = true;
  HIPCHK(c, hipEventRecord(d.ev, on));
  next = (next + 1) % uwt_ctx::kDeps;
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
int compute_begin(uwt_ctx* c, int first, int n) { return dep_wait(c, c->fresh, c->fresh_next, c->fresh_dropped, c->stream, first, n); }
// ... and remembered, so that a later upload into them waits for it
int compute_end(uwt_ctx* c, int first, int n) {
  c->busy_seq[c->busy_next] = ++c->ticket_seq;
  return dep_note(c, c->busy, c->busy_next, c->busy_dropped, c->stream, first, n);
}

// The caller's lists are copied before this returns (they may be temporaries): into a pinned staging buffer, then
// asynchronously to the device.  Unchanged lists (the steady state of a resident batch) are not re-sent.
int upload_pairs(uwt_ctx* c, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots) {
  if (!ref_slots || !tgt_slots || n_pairs < 1) return fail(c, UWT_ERR_INVALID_ARG, "null pair lists or n_pairs < 1");
  if (n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_CAPACITY, "n_pairs exceeds max_pairs");
  for (int i = 0; i < n_pairs; i++)
    if (ref_slots[i] < 0 || ref_slots[i] >= c->p.max_frames || tgt_slots[i] < 0 || tgt_slots[i] >= c->p.max_frames)
      return fail(c, UWT_ERR_INVALID_ARG, "pair slot out of range");
  const size_t block = 2 * (size_t)c->p.max_pairs;
  {
    const int* h_ref = c->h_pairs + c->pair_stage * block;
    const int* h_tgt = h_ref + c->p.max_pairs;
    if (n_pairs == c->n_pairs_cached && !std::memcmp(h_ref, ref_slots, sizeof(int) * n_pairs) &&
        !std::memcmp(h_tgt, tgt_slots, sizeof(int) * n_pairs))
      return UWT_OK;
  }
  const int stage = (c->pair_stage + 1) % uwt_ctx::kPairStages;
  HIPCHK(c, hipEventSynchronize(c->ev_pairs[stage]));  // the copy that last read this block (kPairStages lists ago)
  int* h_ref = c->h_pairs + stage * block;
  int* h_tgt = h_ref + c->p.max_pairs;
  std::memcpy(h_ref, ref_slots, sizeof(int) * n_pairs);
  std::memcpy(h_tgt, tgt_slots, sizeof(int) * n_pairs);
  c->pair_stage = stage;
  c->n_pairs_cached = n_pairs;
  HIPCHK(c, hipMemcpyAsync(c->d_ref, h_ref, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_tgt, h_tgt, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_pairs[stage], c->stream));
  return UWT_OK;
}

// UWT_ERR_PAIR_FAILED, naming the first failing pair's status, when any of a batch call's n pairs failed
int first_failure(uwt_ctx* c, const char* what, const uwt_stats* stats, int n) {
  for (int i = 0; i < n; i++)
    if (stats[i].status != UWT_OK)
      return fail(c, UWT_ERR_PAIR_FAILED, std::string(what) + ": at least one pair failed, first status: " +
                                              uwt_status_string(stats[i].status));
  return UWT_OK;
}

// the synchronous form of a batch call enqueued with the context's d_poses / d_stats: both copied back, the stream drained
int read_back_pairs(uwt_ctx* c, const char* what, int n, float* poses_out, uwt_stats* stats_out) {
  std::vector<uwt_stats> tmp((size_t)n);
  HIPCHK(c, hipMemcpyAsync(poses_out, c->d_poses, sizeof(float) * 7 * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_stats, sizeof(uwt_stats) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (stats_out) std::copy(tmp.begin(), tmp.end(), stats_out);
  return first_failure(c, what, tmp.data(), n);
}

int run_se3_op(uwt_ctx* c, int op, const float* a, int na, const float* b, int nb, float* out, int nout, int* flag) {
  if (!c) return UWT_ERR_INVALID_ARG;
  int st = ensure_scratch(c, 4096);
  if (st) return st;
  float* d = (float*)c->scratch;  // [0,64) a, [64,128) b, [128,256) out, [256] flag
  HIPCHK(c, hipMemcpyAsync(d, a, sizeof(float) * na, hipMemcpyHostToDevice, c->stream));
  if (b) HIPCHK(c, hipMemcpyAsync(d + 64, b, sizeof(float) * nb, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_se3_ops, dim3(1), dim3(1), 0, c->stream, op, d, d + 64, d + 128, (int*)(d + 256));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, d + 128, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
  int f = 1;
  HIPCHK(c, hipMemcpyAsync(&f, d + 256, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (flag) *flag = f;
  return UWT_OK;
}

}  // namespace

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
  CREATE_CHK(hipMalloc((void**)&c->d_ref, sizeof(int) * p->max_pairs));
  CREATE_CHK(hipMalloc((void**)&c->d_tgt, sizeof(int) * p->max_pairs));
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

int uwt_destroy(uwt_ctx* c) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->side) (void)hipStreamSynchronize(c->side);  // an aborted uwt_track_batch_async may have left work there
  if (c->copy) (void)hipStreamSynchronize(c->copy);
  for (int i = 1; i < uwt_ctx::kMaxParts; i++)
    if (c->part_stream[i]) (void)hipStreamSynchronize(c->part_stream[i]);
  for (int l = 0; l < UWT_MAX_LEVELS; l++) {
    if (c->img[l]) (void)hipFree(c->img[l]);
    if (c->depth[l]) (void)hipFree(c->depth[l]);
    if (c->gx[l]) (void)hipFree(c->gx[l]);
    if (c->gy[l]) (void)hipFree(c->gy[l]);
  }
  if (c->state) (void)hipFree(c->state);
  if (c->d_ref) (void)hipFree(c->d_ref);
  if (c->d_tgt) (void)hipFree(c->d_tgt);
  if (c->partials) (void)hipFree(c->partials);
  if (c->partials2) (void)hipFree(c->partials2);
  if (c->state2) (void)hipFree(c->state2);
  if (c->d_poses) (void)hipFree(c->d_poses);
  if (c->d_stats) (void)hipFree(c->d_stats);
  if (c->d_active) (void)hipFree(c->d_active);
  if (c->d_tickets) (void)hipFree(c->d_tickets);
  for (int i = 0; i < 2; i++)
    if (c->ev_poll[i]) (void)hipEventDestroy(c->ev_poll[i]);
  if (c->h_small) (void)hipHostFree(c->h_small);
  if (c->hist) (void)hipFree(c->hist);
  if (c->scale) (void)hipFree(c->scale);
  if (c->h_active) (void)hipHostFree(c->h_active);
  if (c->h_pairs) (void)hipHostFree(c->h_pairs);
  if (c->scratch) (void)hipFree(c->scratch);
  if (c->feat_tab) (void)hipFree(c->feat_tab);
  if (c->feat_cnt) (void)hipFree(c->feat_cnt);
  if (c->feat_kp) (void)hipFree(c->feat_kp);
  if (c->feat_nkp) (void)hipFree(c->feat_nkp);
  if (c->feat_recs) (void)hipFree(c->feat_recs);
  if (c->cand_tab) (void)hipFree(c->cand_tab);
  if (c->cand_cnt) (void)hipFree(c->cand_cnt);
  if (c->cand_work) (void)hipFree(c->cand_work);
  if (c->cand_recs) (void)hipFree(c->cand_recs);
  if (c->match_desc) (void)hipFree(c->match_desc);
  if (c->match_cnt) (void)hipFree(c->match_cnt);
  if (c->match_part) (void)hipFree(c->match_part);
  if (c->match_out) (void)hipFree(c->match_out);
  if (c->ransac_buf) (void)hipFree(c->ransac_buf);
  if (c->ransac_need) (void)hipFree(c->ransac_need);
  if (c->surf_buf) (void)hipFree(c->surf_buf);
  if (c->h_feat) (void)hipHostFree(c->h_feat);
  for (hipEvent_t e : c->ev_feat)
    if (e) (void)hipEventDestroy(e);
  for (void* p : c->stage)
    if (p) (void)hipFree(p);
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->side) (void)hipStreamDestroy(c->side);
  for (int i = 1; i < uwt_ctx::kMaxParts; i++) {
    if (c->part_stream[i]) (void)hipStreamDestroy(c->part_stream[i]);
    if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->copy) (void)hipStreamDestroy(c->copy);
  for (int i = 0; i < uwt_ctx::kDeps; i++) {
    if (c->busy[i].ev) (void)hipEventDestroy(c->busy[i].ev);
    if (c->fresh[i].ev) (void)hipEventDestroy(c->fresh[i].ev);
  }
  for (int i = 0; i < uwt_ctx::kPairStages; i++)
    if (c->ev_pairs[i]) (void)hipEventDestroy(c->ev_pairs[i]);
  if (c->ev_pyramids) (void)hipEventDestroy(c->ev_pyramids);
  if (c->ev_side_done) (void)hipEventDestroy(c->ev_side_done);
  for (int l = 0; l < UWT_MAX_LEVELS; l++)
    if (c->ev_level[l]) (void)hipEventDestroy(c->ev_level[l]);
  if (c->stream) (void)hipStreamDestroy(c->stream);
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
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tn = *t;
  c->spec_budget = c->spec_calm = 0;
  for (int32_t* b : {&c->tn.coarse, &c->tn.coarse_weighted, &c->tn.overlap_gradients, &c->tn.speculation, &c->tn.fused_stages,
                     &c->tn.pyramid_batch, &c->tn.typed_loads})
    *b = *b != 0;
  std::memset(c->tn.reserved, 0, sizeof(c->tn.reserved));
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
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((p->sampler || p->weights) && !c->hist) {
    HIPCHK(c, hipMalloc((void**)&c->hist, sizeof(unsigned int) * kHistBins * o.max_pairs));
    HIPCHK(c, hipMalloc((void**)&c->scale, sizeof(PairScale) * o.max_pairs));
    HIPCHK(c, hipMemset(c->scale, 0, sizeof(PairScale) * o.max_pairs));
    HIPCHK(c, hipStreamSynchronize(nullptr));   // (the NULL stream's memset against the context's non-blocking streams: see uwt_create)
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
  return st ? fail(c, st, "uwt_plane_device_ptr: bad slot/level/plane") : UWT_OK;
}

int uwt_get_plane(uwt_ctx* c, int32_t slot, int32_t lvl, int32_t plane, void* host_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  void* d;
  size_t elem;
  int st = plane_ptr(c, slot, lvl, plane, &d, &elem);
  if (st || !host_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_get_plane: bad slot/level/plane");
  const LevelK& L = c->lv[lvl];   // the level's image, img_w x img_h, without the pad columns of its rows
  HIPCHK(c, hipMemcpy2DAsync(host_out, (size_t)L.iw * elem, d, (size_t)L.pitch * elem, (size_t)L.iw * elem, L.ih, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

// System::AddFrame's pyramid loop for slots first_slot..+n.  depth_slots (device list of n_depth slots), when given,
// restricts the depth pyramids to those slots: only a pair's reference frame is ever read through its depth
// (src/Tracker.cpp:1266-1272).
static int enqueue_pyramids(uwt_ctx* c, int first_slot, int n, const int* depth_slots = nullptr, int n_depth = 0) {
  const bool fused = n <= kFewFrames && c->p.n_levels >= 3 && c->p.n_levels <= kPyrMaxLevels && c->whole && c->lv[0].iw % 4 == 0 &&
                     c->lv[0].ih % 4 == 0 && c->tn.fused_stages;
  if (fused) {   // the whole pyramid of each plane in one launch
    if (n) launch_pyramid_all<uint8_t>(c, c->img, c->img, n, nullptr, first_slot);
    if (c->p.has_depth) {
      if (depth_slots) { if (n_depth) launch_pyramid_all<uint16_t>(c, c->depth, c->depth, n_depth, depth_slots, 0); }
      else if (n) launch_pyramid_all<uint16_t>(c, c->depth, c->depth, n, nullptr, first_slot);
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
      hipLaunchKernelGGL(k_pyramid_batch<uint8_t>, dim3(tiles, n), dim3(kBlock), 0, c->stream, a);
    }
    const int nd16 = !c->p.has_depth ? 0 : (depth_slots ? n_depth : n);
    if (nd16) {
      PyramidBatchArgs<uint16_t> a;
      a.src = c->depth[0];
      for (int l = 0; l < 4; l++) { a.stride[l] = c->lv[l].n; a.pitch[l] = c->lv[l].pitch; if (l) a.dst[l - 1] = c->depth[l]; }
      a.w = c->lv[0].iw; a.h = c->lv[0].ih; a.slots = depth_slots; a.first_slot = depth_slots ? 0 : first_slot;
      hipLaunchKernelGGL(k_pyramid_batch<uint16_t>, dim3(tiles, nd16), dim3(kBlock), 0, c->stream, a);
    }
    HIPCHK(c, hipGetLastError());
    l0 = 4;
  }
  for (int l = l0; l < c->p.n_levels; l++) {
    const LevelK& S = c->lv[l - 1];
    const LevelK& D = c->lv[l];
    int st = launch_resize<uint8_t>(c, c->img[l - 1], c->img[l], S.iw, S.ih, S.pitch, D.iw, D.ih, D.pitch, S.n, D.n, n, nullptr, first_slot);
    if (st) return st;
    if (c->p.has_depth) {
      st = depth_slots ? launch_resize<uint16_t>(c, c->depth[l - 1], c->depth[l], S.iw, S.ih, S.pitch, D.iw, D.ih, D.pitch, S.n, D.n, n_depth, depth_slots)
                       : launch_resize<uint16_t>(c, c->depth[l - 1], c->depth[l], S.iw, S.ih, S.pitch, D.iw, D.ih, D.pitch, S.n, D.n, n, nullptr, first_slot);
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

int uwt_build_pyramids(uwt_ctx* c, int32_t first_slot, int32_t n) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !slot_range_ok(c, first_slot, n)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_build_pyramids: bad range");
  int st = compute_begin(c, first_slot, n);
  if (st) return st;
  st = enqueue_pyramids(c, first_slot, n);
  if (st) return st;
  if (!c->deferred) HIPCHK(c, hipStreamSynchronize(c->stream));
  else return compute_end(c, first_slot, n);   // still in flight: a later asynchronous upload into these slots waits for it
  return UWT_OK;
}

int uwt_apply_gradient(uwt_ctx* c, int32_t first_slot, int32_t n) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !slot_range_ok(c, first_slot, n)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_apply_gradient: bad range");
  int st = compute_begin(c, first_slot, n);
  if (st) return st;
  st = enqueue_gradients(c, first_slot, n);
  if (st) return st;
  if (!c->deferred) HIPCHK(c, hipStreamSynchronize(c->stream));
  else return compute_end(c, first_slot, n);   // still in flight: a later asynchronous upload into these slots waits for it
  return UWT_OK;
}

int uwt_estimate_pose_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                            float* poses_out, uwt_stats* stats_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !poses_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_batch: null argument");
  if (!ref_slots || !tgt_slots || n_pairs < 1) return fail(c, UWT_ERR_INVALID_ARG, "null pair lists or n_pairs < 1");
  if (n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_CAPACITY, "n_pairs exceeds max_pairs");
  int st;
  const bool chained = chained_form(c, n_pairs) == Chained::identity;
  CallOpts opt;
  opt.inline_pairs = n_pairs <= 2 && chained;
  if (opt.inline_pairs) {   // the slots travel in the kernel arguments
    for (int i = 0; i < n_pairs; i++) {
      if (ref_slots[i] < 0 || ref_slots[i] >= c->p.max_frames || tgt_slots[i] < 0 || tgt_slots[i] >= c->p.max_frames)
        return fail(c, UWT_ERR_INVALID_ARG, "pair slot out of range");
      opt.pair_slots[2 * i] = ref_slots[i];
      opt.pair_slots[2 * i + 1] = tgt_slots[i];
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
    st = enqueue_estimate(c, n_pairs, small ? c->d_small->poses : c->d_poses, small ? c->d_small->stats : c->d_stats, nullptr, opt);
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
  return first_failure(c, "uwt_estimate_pose_batch", tmp.data(), n_pairs);
}

static int track_batch_enqueue(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                               const int32_t* ref_slots, const int32_t* tgt_slots, float* d_poses_out, uwt_stats* d_stats_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !d_poses_out || !slot_range_ok(c, first_slot, n_frames))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_track_batch_async: bad argument");
  int st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
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
  st = compute_begin(c, c->dep_first, c->dep_n);   // behind the asynchronous uploads into these slots
  if (st) return st;
  // The tracker reads gradients and depth of the previous (reference) frame only (src/Tracker.cpp:407-408, 1266-1272).
  // grad_refs_only computes those planes — gradients of every level, depth levels 1.. — for the pairs' reference slots
  // alone; otherwise every prepared frame gets them, as System::AddFrame / System::Tracking do for each new frame
  // (src/System.cpp:246-251, 197-213).
  const int* g_slots = grad_refs_only ? c->d_ref : nullptr;   // gradient frames: a slot list or the range
  const int g_first = g_slots ? 0 : first_slot, g_n = g_slots ? n_pairs : n_frames;
  st = grad_refs_only ? enqueue_pyramids(c, first_slot, n_frames, c->d_ref, n_pairs) : enqueue_pyramids(c, first_slot, n_frames);
  if (st) return st;
  // The side stream pays from ~768 pairs on (+1.7 % at 1024); below, its events cost more than the overlap returns
  // (one pair: +14 % latency).  A profiled call times its kernels alone: nothing runs beside them.
  if (!c->tn.overlap_gradients || c->profiling || n_pairs < 768) {
    st = enqueue_gradients(c, g_first, g_n, g_slots);
    if (st) return st;
    return enqueue_estimate(c, n_pairs, d_poses_out, reinterpret_cast<StatsOut*>(d_stats_out));
  }
  // The alignment starts at the coarsest iterated level and only then needs the finer gradients: the first level's are
  // computed here, the others on the side stream, each level's event gating the iterations that read it.
  HIPCHK(c, hipEventRecord(c->ev_pyramids, c->stream));
  st = enqueue_gradient_level(c, c->p.first_level, g_first, g_n, g_slots);
  if (st) return st;
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
  HIPCHK(c, hipEventRecord(c->ev_side_done, c->side));
  st = enqueue_estimate(c, n_pairs, d_poses_out, reinterpret_cast<StatsOut*>(d_stats_out), c->ev_level);
  // whatever follows on the context stream (the next call's pyramids, a plane read-back) is ordered after the side work
  const hipError_t e = hipStreamWaitEvent(c->stream, c->ev_side_done, 0);
  if (st) return st;
  if (e != hipSuccess) return fail(c, UWT_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
  return UWT_OK;
}

int uwt_track_batch_async(uwt_ctx* c, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                          const int32_t* ref_slots, const int32_t* tgt_slots, float* d_poses_out, uwt_stats* d_stats_out) {
  int st = track_batch_enqueue(c, first_slot, n_frames, grad_refs_only, n_pairs, ref_slots, tgt_slots, d_poses_out, d_stats_out);
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
  if (c->profiling) {
    int st = prof_collect(c);
    if (st) return st;
  }
  return UWT_OK;
}

int uwt_stream(uwt_ctx* c, void** out) {
  if (!c || !out) return UWT_ERR_INVALID_ARG;
  *out = (void*)c->stream;
  return UWT_OK;
}

int uwt_profile_enable(uwt_ctx* c, int32_t on) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c) return UWT_ERR_INVALID_ARG;
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

/* ---- per-stage entry points ---------------------------------------------------------------------------------- */

int uwt_halve_u8(uwt_ctx* c, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !src || !dst || w < 2 || h < 2 || (w & 1) || (h & 1)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_halve_u8");
  return resize_half_host<uint8_t>(c, src, w, h, dst, w / 2, h / 2);
}

int uwt_halve_u16(uwt_ctx* c, const uint16_t* src, int32_t w, int32_t h, uint16_t* dst) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !src || !dst || w < 2 || h < 2 || (w & 1) || (h & 1)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_halve_u16");
  return resize_half_host<uint16_t>(c, src, w, h, dst, w / 2, h / 2);
}

int uwt_half_size(int32_t n) { return (int)std::lrint((double)n * 0.5); }   // cvRound(n * 0.5): half to even

int uwt_resize_half_u8(uwt_ctx* c, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !src || !dst || w < 1 || h < 1 || uwt_half_size(w) < 1 || uwt_half_size(h) < 1) return fail(c, UWT_ERR_INVALID_ARG, "uwt_resize_half_u8");
  return resize_half_host<uint8_t>(c, src, w, h, dst, uwt_half_size(w), uwt_half_size(h));
}

int uwt_resize_half_u16(uwt_ctx* c, const uint16_t* src, int32_t w, int32_t h, uint16_t* dst) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !src || !dst || w < 1 || h < 1 || uwt_half_size(w) < 1 || uwt_half_size(h) < 1) return fail(c, UWT_ERR_INVALID_ARG, "uwt_resize_half_u16");
  return resize_half_host<uint16_t>(c, src, w, h, dst, uwt_half_size(w), uwt_half_size(h));
}

int uwt_scharr3(uwt_ctx* c, const uint8_t* src, int32_t w, int32_t h, int16_t* gx, int16_t* gy) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !src || !gx || !gy || w < 1 || h < 1) return fail(c, UWT_ERR_INVALID_ARG, "uwt_scharr3");
  const size_t pitch = ((size_t)w + 3) & ~(size_t)3;   // rows padded to whole groups of four, as the context's level planes are
  const size_t n = pitch * h, off = (n + 255) & ~(size_t)255;
  int st = ensure_scratch(c, off + n * 4);
  if (st) return st;
  uint8_t* d = (uint8_t*)c->scratch;
  int16_t* dgx = (int16_t*)(d + off);
  int16_t* dgy = dgx + n;
  HIPCHK(c, hipMemcpy2DAsync(d, pitch, src, w, w, h, hipMemcpyHostToDevice, c->stream));
  st = launch_scharr(c, d, dgx, dgy, w, h, (int)pitch, n, 1);
  if (st) return st;
  HIPCHK(c, hipMemcpy2DAsync(gx, (size_t)w * 2, dgx, pitch * 2, (size_t)w * 2, h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(gy, (size_t)w * 2, dgy, pitch * 2, (size_t)w * 2, h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_warp(uwt_ctx* c, int32_t lvl, const float* pts, int32_t n, const float pose[7], float* warped_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !pts || !pose || !warped_out || n < 1 || lvl < 0 || lvl >= c->p.n_levels)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_warp");
  const size_t bytes = sizeof(float) * 4 * (size_t)n;
  int st = ensure_scratch(c, bytes * 2);
  if (st) return st;
  float4* din = (float4*)c->scratch;
  float4* dout = din + n;
  HIPCHK(c, hipMemcpyAsync(din, pts, bytes, hipMemcpyHostToDevice, c->stream));
  Pose P;
  for (int k = 0; k < 4; k++) P.q[k] = pose[k];
  for (int k = 0; k < 3; k++) P.t[k] = pose[4 + k];
  UWT_WITH_AR(c->p.arith == UWT_ARITH_LEGACY ? kArithLegacy : kArithOpenCV, hipLaunchKernelGGL(k_warp_table<AR>, dim3((n + 255) / 256), dim3(256), 0, c->stream, din, dout, n, P, c->lv[lvl]));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(warped_out, dout, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

// The two per-stage residual entries: one evaluation of the production kernel for pair (ref_slot, tgt_slot) at `pose`, with the
// level's own slicing, its records folded like k_gn_update's.  general: the context's sampler / weights (the scale pass, then the
// weighted sums' dump form, always taken: its sums do not depend on which dumps are asked for), else the identity path (its
// dump form when a dump is asked for, the production kernel otherwise).
static int residual_jacobian_entry(uwt_ctx* c, const char* name, bool general, int32_t ref_slot, int32_t tgt_slot, int32_t lvl,
                                   const float pose[7], uwt_accum* acc_out, double* err_num_out, float* inv_mad_out, float* J_out,
                                   float* r_out, uint8_t* valid_out, float* w_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !pose || !acc_out || lvl < 0 || lvl >= c->p.n_levels || !slot_range_ok(c, ref_slot, 1) || !slot_range_ok(c, tgt_slot, 1))
    return fail(c, UWT_ERR_INVALID_ARG, name);
  if (general && !c->p.sampler && !c->p.weights)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(name) + ": context uses the nearest/identity fast path");
  int st = upload_pairs(c, 1, &ref_slot, &tgt_slot);
  if (st) return st;
  const LevelK& L = c->lv[lvl];
  const size_t n = L.ng;   // device dumps are indexed like the planes (pitch x gh positions); the host receives the gw x gh grid
  const bool dump = general || J_out || r_out || valid_out;
  if (dump) {
    st = ensure_scratch(c, n * (6 * 4 + 4 + 4 + 1) + 512);
    if (st) return st;
  }
  ResidualArgs a = residual_args(c, lvl);
  for (int k = 0; k < 4; k++) a.pose.q[k] = pose[k];
  for (int k = 0; k < 3; k++) a.pose.t[k] = pose[4 + k];
  if (general) {   // the scale pass reads the pose from the pair's state
    hipLaunchKernelGGL(k_set_pose, dim3(1), dim3(64), 0, c->stream, c->state, a.pose, c->p.initial_error);
    HIPCHK(c, hipGetLastError());
  } else {
    a.state = nullptr;
  }
  if (dump) {
    a.dumpJ = (float*)c->scratch;
    a.dumpR = a.dumpJ + 6 * n;
    a.dumpW = a.dumpR + n;
    a.dumpV = (uint8_t*)(a.dumpW + n);
  }
  if (general && c->p.weights)   // the pair's bins and ticket word: all-zero ahead of the scale pass
    HIPCHK(c, hipMemsetAsync(c->hist, 0, sizeof(unsigned int) * kHistBins, c->stream));
  st = general ? launch_general(c, c->stream, a, 1, true) : launch_residual(c, c->stream, a, 1, dump);
  if (st) return st;
  std::vector<uint32_t> recs((size_t)a.slices * kRecWords);
  HIPCHK(c, hipMemcpyAsync(recs.data(), c->partials, recs.size() * 4, hipMemcpyDeviceToHost, c->stream));
  PairScale sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.inv_mad = 1.f;
  if (general && c->p.weights) HIPCHK(c, hipMemcpyAsync(&sc, c->scale, sizeof(sc), hipMemcpyDeviceToHost, c->stream));
  if (J_out) HIPCHK(c, hipMemcpy2DAsync(J_out, (size_t)L.gw * 24, a.dumpJ, (size_t)L.pitch * 24, (size_t)L.gw * 24, L.gh, hipMemcpyDeviceToHost, c->stream));
  if (r_out) HIPCHK(c, hipMemcpy2DAsync(r_out, (size_t)L.gw * 4, a.dumpR, (size_t)L.pitch * 4, (size_t)L.gw * 4, L.gh, hipMemcpyDeviceToHost, c->stream));
  if (w_out) HIPCHK(c, hipMemcpy2DAsync(w_out, (size_t)L.gw * 4, a.dumpW, (size_t)L.pitch * 4, (size_t)L.gw * 4, L.gh, hipMemcpyDeviceToHost, c->stream));
  if (valid_out) HIPCHK(c, hipMemcpy2DAsync(valid_out, (size_t)L.gw, a.dumpV, (size_t)L.pitch, (size_t)L.gw, L.gh, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::memset(acc_out, 0, sizeof(*acc_out));
  double err = 0.0;
  for (int s = 0; s < a.slices; s++) {  // same slice-ordered f64 fold as k_gn_update
    const uint32_t* r = recs.data() + (size_t)s * kRecWords;
    double d[30];
    std::memcpy(d, r, sizeof(d));
    for (int k = 0; k < 21; k++) acc_out->A[k] += d[k];
    for (int k = 0; k < 6; k++) acc_out->jtr[k] += d[21 + k];
    if (general) err += d[29];   // the error numerator of the general kind's records
    acc_out->n_valid += (int32_t)r[54];
    int64_t sr2;
    std::memcpy(&sr2, r + 56, 8);
    acc_out->sum_r2 += sr2;
  }
  if (err_num_out) *err_num_out = err;
  if (inv_mad_out) *inv_mad_out = sc.inv_mad;
  return UWT_OK;
}

int uwt_residual_jacobian(uwt_ctx* c, int32_t ref_slot, int32_t tgt_slot, int32_t lvl, const float pose[7],
                          uwt_accum* acc_out, float* J_out, float* r_out, uint8_t* valid_out) {
  return residual_jacobian_entry(c, "uwt_residual_jacobian", false, ref_slot, tgt_slot, lvl, pose, acc_out, nullptr, nullptr, J_out,
                                 r_out, valid_out, nullptr);
}

int uwt_residual_jacobian_weighted(uwt_ctx* c, int32_t ref_slot, int32_t tgt_slot, int32_t lvl, const float pose[7],
                                   uwt_accum* acc_out, double* err_num_out, float* inv_mad_out, float* J_out, float* r_out,
                                   uint8_t* valid_out, float* w_out) {
  return residual_jacobian_entry(c, "uwt_residual_jacobian_weighted", true, ref_slot, tgt_slot, lvl, pose, acc_out, err_num_out,
                                 inv_mad_out, J_out, r_out, valid_out, w_out);
}

static int ls_accumulate_impl(uwt_ctx* c, const float* J, const float* r, const float* w, int32_t n, int32_t divide, bool sse,
                              int32_t count, float A[36], float b[6], float* error, int32_t* num_constraints) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !J || !r || !A || !b || !error || !num_constraints || n < 0) return fail(c, UWT_ERR_INVALID_ARG, "uwt_ls_accumulate");
  const size_t fl = (size_t)n * 8 + 128 + 64;
  int st = ensure_scratch(c, fl * 4);
  if (st) return st;
  float* dJ = (float*)c->scratch;
  float* dr = dJ + (size_t)n * 6;
  float* dw = dr + n;
  float* dp = dw + n;
  if (n) {
    HIPCHK(c, hipMemcpyAsync(dJ, J, sizeof(float) * 6 * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dr, r, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    if (w) HIPCHK(c, hipMemcpyAsync(dw, w, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
  }
  // one thread per accumulator chain (per lane chain in the SSE form), each in the reference's order: k_ls_sequential
  if (sse) hipLaunchKernelGGL(k_ls_sequential<true>, dim3(1), dim3(128), 0, c->stream, dJ, dr, w ? dw : nullptr, n, dp);
  else hipLaunchKernelGGL(k_ls_sequential<false>, dim3(1), dim3(128), 0, c->stream, dJ, dr, w ? dw : nullptr, n, dp);
  HIPCHK(c, hipGetLastError());
  float parts[112];
  HIPCHK(c, hipMemcpyAsync(parts, dp, sizeof(float) * (sse ? 112 : 28), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float s[28];
  for (int k = 0; k < 28; k++)   // LS::finishNoDivide (:39-139): the four lanes folded left to right
    s[k] = sse ? ((parts[4 * k] + parts[4 * k + 1]) + parts[4 * k + 2]) + parts[4 * k + 3] : parts[k];
  int q = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++, q++) { A[6 * i + j] = s[q]; A[6 * j + i] = s[q]; }
  for (int i = 0; i < 6; i++) b[i] = -s[21 + i];  // LS stores b = -Σ w r J (src/LeastSquares.cpp:206; 0 - x - y = -(x + y) in IEEE)
  *error = s[27];
  *num_constraints = count;
  if (divide) {          // LS::finish (:141-146)
    const float nf = (float)count;
    for (int i = 0; i < 36; i++) A[i] = A[i] / nf;
    for (int i = 0; i < 6; i++) b[i] = b[i] / nf;
    *error = *error / nf;
  }
  return UWT_OK;
}

int uwt_ls_accumulate(uwt_ctx* c, const float* J, const float* r, const float* w, int32_t n, int32_t divide, float A[36],
                      float b[6], float* error, int32_t* num_constraints) {
  return ls_accumulate_impl(c, J, r, w, n, divide, false, n /* one per LS::update call (:208) */, A, b, error, num_constraints);
}

int uwt_ls_accumulate_sse(uwt_ctx* c, const float* J, const float* r, const float* w, int32_t n, int32_t divide,
                          int32_t count_quirk, float A[36], float b[6], float* error, int32_t* num_constraints) {
  if (n < 0 || (n & 3)) return fail(c, UWT_ERR_INVALID_ARG, "uwt_ls_accumulate_sse: n must be a multiple of 4");
  return ls_accumulate_impl(c, J, r, w, n, divide, true, count_quirk ? (n / 4) * 6 : n, A, b, error, num_constraints);
}

int uwt_se3_exp(uwt_ctx* c, const float xi[6], float pose_out[7]) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!xi || !pose_out) return UWT_ERR_INVALID_ARG;
  return run_se3_op(c, 0, xi, 6, nullptr, 0, pose_out, 7, nullptr);
}

int uwt_se3_mul(uwt_ctx* c, const float a[7], const float b[7], float out[7]) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!a || !b || !out) return UWT_ERR_INVALID_ARG;
  return run_se3_op(c, 1, a, 7, b, 7, out, 7, nullptr);
}

int uwt_se3_matrix(uwt_ctx* c, const float pose[7], float T_out[16]) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!pose || !T_out) return UWT_ERR_INVALID_ARG;
  return run_se3_op(c, 2, pose, 7, nullptr, 0, T_out, 16, nullptr);
}

int uwt_se3_handoff(uwt_ctx* c, float pose[7], int32_t scale_t) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!pose) return UWT_ERR_INVALID_ARG;
  float out[7];
  int flag = 1;
  int st = run_se3_op(c, scale_t ? 4 : 3, pose, 7, nullptr, 0, out, 7, &flag);
  if (st) return st;
  if (!flag) return fail(c, UWT_ERR_INVALID_ARG, "uwt_se3_handoff: quaternion close to zero (SOPHUS_ENSURE)");
  std::memcpy(pose, out, sizeof(out));
  return UWT_OK;
}

int uwt_solve_delta(uwt_ctx* c, const float A[36], const float b[6], float delta_out[6], float* Ainv_out, int32_t* nonsingular) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!A || !b || !delta_out) return UWT_ERR_INVALID_ARG;
  float out[42];
  int flag = 0;
  int st = run_se3_op(c, (c && c->p.arith == UWT_ARITH_LEGACY) ? 6 : 5, A, 36, b, 6, out, 42, &flag);
  if (st) return st;
  std::memcpy(delta_out, out, 6 * sizeof(float));
  if (Ainv_out) std::memcpy(Ainv_out, out + 6, 36 * sizeof(float));
  if (nonsingular) *nonsingular = flag;
  return UWT_OK;
}

int uwt_estimate_pose_points(uwt_ctx* c, int32_t ref_slot, int32_t tgt_slot, const float* const* tables,
                             const int32_t* n_points, float pose_out[7], uwt_stats* stats_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !tables || !n_points || !pose_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_points: null argument");
  const uwt_params& p = c->p;
  size_t total = 0;
  for (int l = p.last_level; l <= p.first_level; l++) {
    // one partial record per 8192 points; the context owns max_slices x max_pairs records
    if (n_points[l] < 0 || (size_t)n_points[l] > c->partial_records * (size_t)(kBlock * 32) || (n_points[l] > 0 && !tables[l]))
      return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_points: bad table (null, negative or too many points)");
    total += (size_t)n_points[l];
  }
  int st = upload_pairs(c, 1, &ref_slot, &tgt_slot);
  if (st) return st;
  st = ensure_scratch(c, std::max<size_t>(16, total * 16));
  if (st) return st;
  float4* d_tab[UWT_MAX_LEVELS] = {};
  size_t off = 0;
  for (int l = p.last_level; l <= p.first_level; l++) {
    d_tab[l] = (float4*)c->scratch + off;
    if (n_points[l]) HIPCHK(c, hipMemcpyAsync(d_tab[l], tables[l], (size_t)n_points[l] * 16, hipMemcpyHostToDevice, c->stream));
    off += (size_t)n_points[l];
  }
  const int tb = 64;
  hipLaunchKernelGGL(k_init_state, dim3(1), dim3(tb), 0, c->stream, c->state, 1, p.initial_error);
  HIPCHK(c, hipGetLastError());
  const int per_block = kBlock * 32;
  for (int lvl = p.first_level; lvl >= p.last_level; lvl--) {
    ResidualArgs ra = residual_args(c, lvl);
    PointsArgs pa;
    pa.pts = d_tab[lvl];
    pa.n_pts = n_points[lvl];
    pa.pts_per_block = per_block;
    ra.slices = std::max(1, (pa.n_pts + per_block - 1) / per_block);
    UpdateArgs ua = update_args(c, lvl);
    ua.slices = ra.slices;
    const bool general = p.sampler || p.weights;   // robust weights / bilinear sampler: the per-stage form over the table
    if (general) ua.general = 1;
    int next_poll = 2;
    for (int k = 0; k < p.max_iters; k++) {
      if (general) {
        if (p.weights) HIPCHK(c, hipMemsetAsync(c->hist + (size_t)ra.pair_base * kHistBins, 0, sizeof(unsigned int) * kHistBins, c->stream));
        uwt::launch_points_general(c->stream, launch_sel(c), ra, pa, general_args(c));
      } else {
        uwt::launch_points(c->stream, launch_sel(c), ra, pa);
      }
      HIPCHK(c, hipGetLastError());
      ua.k = k;
      const bool poll = p.early_exit && (k + 1 == next_poll) && (k + 1 < p.max_iters);
      ua.active = poll ? c->d_active : nullptr;
      st = poll ? poll_arm(c) : UWT_OK;
      if (st) return st;
      hipLaunchKernelGGL(k_gn_update, dim3(1), dim3(kUpdateBlock), 0, c->stream, ua);
      HIPCHK(c, hipGetLastError());
      if (poll) {
        bool left = true;
        st = poll_any_left(c, &left);
        if (st) return st;
        if (!left) break;
        next_poll *= 2;
      }
    }
    hipLaunchKernelGGL(k_level_end, dim3(1), dim3(tb), 0, c->stream, c->state, 1, lvl, p.handoff_scale_t, p.initial_error);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_write_out, dim3(1), dim3(tb), 0, c->stream, c->state, 1, c->d_poses, c->d_stats);
  HIPCHK(c, hipGetLastError());
  uwt_stats tmp;
  HIPCHK(c, hipMemcpyAsync(pose_out, c->d_poses, sizeof(float) * 7, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&tmp, c->d_stats, sizeof(tmp), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (stats_out) *stats_out = tmp;
  if (tmp.status != UWT_OK)
    return fail(c, UWT_ERR_PAIR_FAILED, std::string("uwt_estimate_pose_points: ") + uwt_status_string(tmp.status));
  return UWT_OK;
}

int uwt_robust_weights(uwt_ctx* c, const float* residuals, int32_t n, int32_t kind, float* weights_out, float* median_out,
                       float* mad_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !residuals || n < 1 || (kind != kWeightsIdentity && kind != kWeightsTukeyRef))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_robust_weights: null residuals, n < 1, or a kind other than identity / Tukey");
  const size_t bytes = sizeof(float) * (size_t)n;
  int st = ensure_scratch(c, 2 * bytes + 64);
  if (st) return st;
  float* d_r = (float*)c->scratch;
  float* d_w = d_r + n;
  float* d_stats = d_w + n;
  HIPCHK(c, hipMemcpyAsync(d_r, residuals, bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_robust_weights, dim3(1), dim3(1024), 0, c->stream, d_r, n, kind, weights_out ? d_w : nullptr, d_stats);
  HIPCHK(c, hipGetLastError());
  float stats[2] = {0.f, 0.f};
  if (weights_out) HIPCHK(c, hipMemcpyAsync(weights_out, d_w, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (median_out) *median_out = stats[0];
  if (mad_out) *mad_out = stats[1];
  return UWT_OK;
}

// ---- the sparse point producers: per-stage entries over a slot list in the scratch ------------------------------------
namespace {

// the first min(n, 200) key points (x, y) inside level 0 (its grid is its image)
int check_keypoints(uwt_ctx* c, const char* what, const float* kp, int n) {
  const float w = (float)c->lv[0].gw, h = (float)c->lv[0].gh;
  for (int i = 0; i < std::min(n, kPatchMaxKeypoints); i++)
    if (!(kp[2 * i] >= 0.f && kp[2 * i] < w && kp[2 * i + 1] >= 0.f && kp[2 * i + 1] < h))
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key point outside the image");
  return UWT_OK;
}

// The candidate producer's work area for n frames on one level: row bands enough for a lone frame to spread over the chip, a few
// rows per thread at least.  [sums | gradient_ planes | (x, band) counts | their offsets]
struct CandidatesLayout {
  int bands;
  size_t o_mag, o_cells, o_off, total;
};
CandidatesLayout candidates_work_layout(const LevelK& L, int n) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  CandidatesLayout o;
  const int col_blocks = (L.gw + kBlock - 1) / kBlock;
  o.bands = std::max(1, std::min(L.gh / 8, 512 / std::max(1, col_blocks * n)));
  const size_t m = (size_t)L.gw * o.bands * n;
  o.o_mag = up(8 * (size_t)n);
  o.o_cells = o.o_mag + up((size_t)L.n * n);
  o.o_off = o.o_cells + up(4 * m);
  o.total = o.o_off + up(4 * m);
  return o;
}

// the device slot list first .. first + n - 1 at d (a fill per slot: no host buffer, no staging copy)
int stage_slots(uwt_ctx* c, int* d, int first, int n) {
  for (int f = 0; f < n; f++) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(d + f), first + f, 1, c->stream));
  return UWT_OK;
}

// Tracker::ObtainCandidatePoints on level lvl for the frames of the device slot list d_slots (n), enqueued on the context stream:
// the work area at `work` (candidates_work_layout), frame f's table at out + f * gw * gh, its full count at counts[f]
int enqueue_candidates(uwt_ctx* c, int lvl, int n, const int* d_slots, double threshold, void* work, float4* out, int* counts) {
  const LevelK& L = c->lv[lvl];
  const CandidatesLayout o = candidates_work_layout(L, n);
  uint8_t* base = (uint8_t*)work;
  uwt::CandidatesWork w;
  w.sums = (unsigned long long*)base;
  w.mag = base + o.o_mag;
  w.cells = (int*)(base + o.o_cells);
  w.offsets = (int*)(base + o.o_off);
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
  int st = ensure_scratch(c, 256 + (size_t)L.n);
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  // scratch: [sum (not read) | slot list | the plane]
  unsigned long long* d_sum = (unsigned long long*)c->scratch;
  int* d_slot = (int*)((uint8_t*)c->scratch + 64);
  uint8_t* d_mag = (uint8_t*)c->scratch + 256;
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
  const LevelK& L = c->lv[lvl];
  const size_t rows = (size_t)L.gw * L.gh;   // a frame's table: a row for every cell of the point grid (the bound is never reached)
  // scratch: [the producer's work area | slot list | counts | tables]
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_slots = candidates_work_layout(L, n_frames).total, o_cnt = o_slots + up(4 * (size_t)n_frames),
               o_tab = o_cnt + up(4 * (size_t)n_frames);
  int st = ensure_scratch(c, o_tab + (size_t)n_frames * rows * sizeof(float4));
  if (st) return st;
  st = compute_begin(c, first_slot, n_frames);
  if (st) return st;
  uint8_t* base = (uint8_t*)c->scratch;
  int* d_slots = (int*)(base + o_slots);
  int* d_cnt = (int*)(base + o_cnt);
  float4* d_tab = (float4*)(base + o_tab);
  st = stage_slots(c, d_slots, first_slot, n_frames);
  if (!st) st = enqueue_candidates(c, lvl, n_frames, d_slots, threshold, base, d_tab, d_cnt);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(counts_out, d_cnt, sizeof(int) * n_frames, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int f = 0; f < n_frames; f++) {   // each frame's points are packed at f * cap in the caller's buffer
    const int k = std::min(counts_out[f], cap);
    if (k > 0)
      HIPCHK(c, hipMemcpyAsync(pts_out + (size_t)f * cap * 4, d_tab + (size_t)f * rows, (size_t)k * 16, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
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
  st = ensure_scratch(c, 4096 + (size_t)stride * sizeof(float4));
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  // scratch: [key point count | slot list | row count | key points at 64 | table at 4096]; the count, the slot and the key points
  // go down in one copy
  int* d_hdr = (int*)c->scratch;
  float2* d_kp = (float2*)((uint8_t*)c->scratch + 64);
  float4* d_tab = (float4*)((uint8_t*)c->scratch + 4096);
  const int hdr[2] = {std::min(n_kp, kPatchMaxKeypoints), slot};
  std::vector<uint8_t> in(64 + sizeof(float2) * hdr[0]);
  std::memcpy(in.data(), hdr, sizeof(hdr));
  if (hdr[0]) std::memcpy(in.data() + 64, kp, sizeof(float2) * hdr[0]);
  HIPCHK(c, hipMemcpyAsync(d_hdr, in.data(), in.size(), hipMemcpyHostToDevice, c->stream));
  uwt::launch_patch_points_batch(c->stream, 1, d_kp, d_hdr, d_hdr + 1, c->p.has_depth ? c->depth[0] : nullptr, (size_t)c->lv[0].n,
                                 c->lv[0].pitch, c->lv[0].gw, c->lv[0].gh, d_tab, stride, d_hdr + 2);
  HIPCHK(c, hipGetLastError());
  int cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, d_hdr + 2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *count_out = cnt;
  const int m = std::min(cnt, stride);
  if (m > 0) {
    HIPCHK(c, hipMemcpyAsync(pts_out, d_tab, (size_t)m * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return UWT_OK;
}

// ---- the live call for a batch of pairs: tables built and evaluated on the device --------------------------------
namespace {

constexpr int kFeatTableRows = kPatchMaxKeypoints * kPatchMaxRows;   // rows of one pair's table at most (its stride)
constexpr int kFeatKpFloats = 2 * kPatchMaxKeypoints;                 // one frame's key points as the caller passes them

// the context's params with Tracker::EstimatePoseFeatures' locals (src/Tracker.cpp:633-640, 661, 834, 856): level 0 only, 10
// iterations, epsilon 1e-3, last_error 50000, z_factor 0.002, no angle factor, gain 1 (Residuals.mul(1)), the early exit of :782,
// the hand-off of :856; identity weights (:769), round() (:746)
uwt_params feature_params(const uwt_ctx* c) {
  uwt_params q = c->p;
  q.first_level = q.last_level = 0;
  q.max_iters = 10;
  q.epsilon = 0.001f;
  q.initial_error = 50000.0f;
  q.z_factor = 0.002f;
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

// The caller's key points and counts are copied before the call returns (into the next block of a pinned ring, as
// upload_pairs does with the pair lists), then asynchronously to the device, and the batched producer builds frame f's table
// at feat_tab + f * kFeatTableRows from the key points and the depth of slot d_slots[f].
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
  uwt::launch_patch_points_batch(c->stream, n, c->feat_kp, c->feat_nkp, d_slots, c->p.has_depth ? c->depth[0] : nullptr,
                                 (size_t)c->lv[0].n, c->lv[0].pitch, c->lv[0].gw, c->lv[0].gh, c->feat_tab, kFeatTableRows,
                                 c->feat_cnt);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

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
int enqueue_table_estimate(uwt_ctx* c, int n_pairs, const uwt_params& q, const TableLevel* lv, uint32_t* recs, bool polls,
                           float* d_poses, StatsOut* d_stats) {
  const int tb = 128, blocks = (n_pairs + tb - 1) / tb;
  hipLaunchKernelGGL(k_init_state, dim3(blocks), dim3(tb), 0, c->stream, c->state, n_pairs, q.initial_error);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemsetAsync(c->d_tickets, 0, sizeof(unsigned int) * (size_t)n_pairs, c->stream));
  for (int lvl = q.first_level; lvl >= q.last_level; lvl--) {
    ResidualArgs ra = residual_args(c, lvl);
    ra.zf = q.z_factor;
    ra.af = q.angle_factor;
    ra.gain = q.gain;
    ra.slices = lv[lvl].slices;
    ra.partials = recs;
    UpdateArgs ua = update_args(c, lvl);
    ua.partials = recs;
    ua.slices = ra.slices;
    ua.max_iters = q.max_iters;
    ua.early_exit = q.early_exit;
    ua.epsilon = q.epsilon;
    ua.gain = q.gain;
    int next_poll = c->tn.first_poll;
    int pending = -1;
    for (int k = 0; k < q.max_iters; k++) {
      ua.k = k;
      const bool poll = polls && (k + 1 == next_poll) && (k + 1 < q.max_iters);
      const int slot = c->poll_seq & 1;
      ua.active = poll ? c->d_active + slot : nullptr;
      if (poll) HIPCHK(c, hipMemsetAsync(c->d_active + slot, 0, sizeof(int), c->stream));
      arm_tail(c, ra, ua);
      uwt::launch_table_eval(c->stream, launch_sel(c), ra, lv[lvl].ta, n_pairs);
      HIPCHK(c, hipGetLastError());
      if (pending >= 0) {
        HIPCHK(c, hipEventSynchronize(c->ev_poll[pending]));
        const bool none_left = c->h_active[pending] == 0;
        pending = -1;
        if (none_left) break;
      }
      if (poll) {
        HIPCHK(c, hipMemcpyAsync(c->h_active + slot, c->d_active + slot, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_poll[slot], c->stream));
        pending = slot;
        c->poll_seq++;
        next_poll *= 2;
      }
    }
    hipLaunchKernelGGL(k_level_end, dim3(blocks), dim3(tb), 0, c->stream, c->state, n_pairs, lvl, q.handoff_scale_t, q.initial_error);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_write_out, dim3(blocks), dim3(tb), 0, c->stream, c->state, n_pairs, d_poses, d_stats);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// System::Tracking's live call for n_pairs pairs, enqueued on the context stream: the producer over the reference frames, then
// enqueue_table_estimate under feature_params, which the host never polls.  No read-back, no wait for the device.
int features_enqueue(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, const float* kp,
                     const int32_t* n_kp, float* d_poses, StatsOut* d_stats) {
  int st = check_features_args(c, what, n_pairs, ref_slots, tgt_slots, kp, n_kp);
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
  return enqueue_table_estimate(c, n_pairs, feature_params(c), &lv0, c->feat_recs, false, d_poses, d_stats);
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
  std::vector<int> cnt((size_t)n_frames);
  HIPCHK(c, hipMemcpyAsync(cnt.data(), c->feat_cnt, sizeof(int) * n_frames, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int f = 0; f < n_frames; f++) {
    counts_out[f] = cnt[(size_t)f];
    const int m = std::min(cnt[(size_t)f], cap);
    if (m > 0)
      HIPCHK(c, hipMemcpyAsync(pts_out + (size_t)f * cap * 4, c->feat_tab + (size_t)f * kFeatTableRows, (size_t)m * 16,
                               hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_track_features_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                   const float* kp, const int32_t* n_kp, float* d_poses_out, uwt_stats* d_stats_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_poses_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_track_features_batch_async: null argument");
  int st = features_enqueue(c, "uwt_track_features_batch_async", n_pairs, ref_slots, tgt_slots, kp, n_kp, d_poses_out,
                            reinterpret_cast<StatsOut*>(d_stats_out));
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int uwt_estimate_pose_features_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                     const float* kp, const int32_t* n_kp, float* poses_out, uwt_stats* stats_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !poses_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_features_batch: null argument");
  const char* what = "uwt_estimate_pose_features_batch";
  int st = features_enqueue(c, what, n_pairs, ref_slots, tgt_slots, kp, n_kp, c->d_poses, c->d_stats);
  if (st) return st;
  return read_back_pairs(c, what, n_pairs, poses_out, stats_out);
}

// ---- semi-dense tracking for a batch of pairs: candidate tables built and evaluated on the device ------------------------
namespace {

// one of the call's device buffers, at least `bytes` (its contents are not kept).  The context stream is drained first: an
// asynchronous call enqueued before may still read the old buffer.
int grow(uwt_ctx* c, void** buf, size_t* have, size_t bytes) {
  if (bytes <= *have) return UWT_OK;
  if (*buf) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(*buf));
  }
  *buf = nullptr;
  *have = 0;
  HIPCHK(c, hipMalloc(buf, bytes));
  *have = bytes;
  return UWT_OK;
}

// Tracker::ObtainCandidatePoints(previous) on levels last_level..first_level, then Tracker::EstimatePose(previous, current) over
// those tables, for n_pairs pairs, enqueued on the context stream: per level the slot-list producer (pair i's table at cand_tab +
// level offset + i * gw * gh, its count at cand_cnt[lvl * n_pairs + i]), then enqueue_table_estimate under the context's params,
// polled under early_exit.  The only waits are the early-exit polls.
int candidates_enqueue(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                       float* d_poses, StatsOut* d_stats) {
  const uwt_params& p = c->p;
  int st = check_pair_lists(c, what, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  if (!std::isfinite(threshold)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": threshold is not finite");
  if (p.weights || p.sampler)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": identity weights and the nearest sampler only; robust weights or the "
                                                            "bilinear sampler over candidate tables: uwt_estimate_pose_points");
  size_t rows = 0, work = 0, tab_off[UWT_MAX_LEVELS] = {};
  int smax = 1;
  for (int l = p.last_level; l <= p.first_level; l++) {
    const LevelK& L = c->lv[l];
    tab_off[l] = rows;
    rows += (size_t)L.gw * L.gh * n_pairs;
    work = std::max(work, candidates_work_layout(L, n_pairs).total);
    smax = std::max(smax, table_slices(L.gw * L.gh));
  }
  st = grow(c, (void**)&c->cand_tab, &c->cand_tab_bytes, rows * sizeof(float4));
  if (!st) st = grow(c, (void**)&c->cand_cnt, &c->cand_cnt_bytes, sizeof(int) * UWT_MAX_LEVELS * (size_t)n_pairs);
  if (!st) st = grow(c, &c->cand_work, &c->cand_work_bytes, work);
  if (!st) st = grow(c, (void**)&c->cand_recs, &c->cand_recs_bytes, sizeof(uint32_t) * kRecWords * (size_t)smax * n_pairs);
  if (st) return st;
  st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  st = compute_begin_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  TableLevel lv[UWT_MAX_LEVELS];
  for (int l = p.last_level; l <= p.first_level; l++) {
    float4* tab = c->cand_tab + tab_off[l];
    int* cnt = c->cand_cnt + (size_t)l * n_pairs;
    st = enqueue_candidates(c, l, n_pairs, c->d_ref, threshold, c->cand_work, tab, cnt);
    if (st) return st;
    const int cells = c->lv[l].gw * c->lv[l].gh;   // the bound every pair's count obeys
    lv[l] = {{tab, cnt, cells}, table_slices(cells)};
  }
  return enqueue_table_estimate(c, n_pairs, p, lv, c->cand_recs, p.early_exit != 0, d_poses, d_stats);
}

}  // namespace

int uwt_track_candidates_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                                     float* d_poses_out, uwt_stats* d_stats_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_poses_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_track_candidates_batch_async: null argument");
  int st = candidates_enqueue(c, "uwt_track_candidates_batch_async", n_pairs, ref_slots, tgt_slots, threshold, d_poses_out,
                              reinterpret_cast<StatsOut*>(d_stats_out));
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int uwt_estimate_pose_candidates_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, double threshold,
                                       float* poses_out, uwt_stats* stats_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !poses_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_estimate_pose_candidates_batch: null argument");
  const char* what = "uwt_estimate_pose_candidates_batch";
  int st = candidates_enqueue(c, what, n_pairs, ref_slots, tgt_slots, threshold, c->d_poses, c->d_stats);
  if (st) return st;
  return read_back_pairs(c, what, n_pairs, poses_out, stats_out);
}

// ---- descriptor matching: 2-NN both ways, ratio test, symmetry test (RobustMatcher, src/Tracker.cpp:52-102, 202-236) -----------
namespace {

static_assert(sizeof(Knn2) == sizeof(uwt_knn2) && sizeof(MatchOut) == sizeof(uwt_match), "uwt_knn2 / uwt_match layout");
static_assert(kMatchMaxRows == UWT_MATCH_MAX_ROWS && kMatchMaxWords * 4 == UWT_MATCH_MAX_ROW_BYTES, "matching limits of include/uwt.h");
static_assert(kMatchL2 == UWT_NORM_L2 && kMatchHamming == UWT_NORM_HAMMING, "uwt_norm");

// Checks the arguments, grows the scratch, uploads both descriptor sets and their counts on the context stream and enqueues
// k_knn2 behind them (dirs = 1: query -> train alone; 2: both directions).  Nothing is enqueued when a check fails.  The train
// range of a (pair, query tile, direction) is cut into parts until the launch has kMatchTargetBlocks blocks: one pair of
// 2000 x 2000 fills the chip as 1024 pairs of 500 x 500 do; the merge of the parts is exact, so the cut shows in no bit.
int match_enqueue(uwt_ctx* c, const char* what, int n_pairs, int norm, int dim, const void* query, const int32_t* n_query,
                  const void* train, const int32_t* n_train, int cap, int dirs, MatchArgs* out) {
  if (n_pairs < 1 || !query || !n_query || !train || !n_train) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list or n_pairs < 1");
  if (norm != UWT_NORM_L2 && norm != UWT_NORM_HAMMING) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": unknown norm");
  if (dim < 1 || (dim & 3)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": dim must be a positive multiple of 4");
  if (cap < 1) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": cap < 1");
  int max_q = 0, max_t = 0;
  for (int p = 0; p < n_pairs; p++) {
    if (n_query[p] < 0 || n_query[p] > cap || n_train[p] < 0 || n_train[p] > cap)
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": descriptor count outside 0..cap");
    max_q = std::max(max_q, n_query[p]);
    max_t = std::max(max_t, n_train[p]);
  }
  const int words = norm == UWT_NORM_L2 ? dim : dim / 4;
  if (cap > kMatchMaxRows || words > kMatchMaxWords)
    return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": cap above UWT_MATCH_MAX_ROWS or a row above UWT_MATCH_MAX_ROW_BYTES");
  const int rows = dirs == 2 ? std::max(max_q, max_t) : max_q, train_rows = dirs == 2 ? rows : max_t;
  const int tiles = (rows + kMatchTile - 1) / kMatchTile, train_tiles = (train_rows + kMatchTile - 1) / kMatchTile;
  const size_t blocks = (size_t)n_pairs * std::max(tiles, 1) * dirs;
  const int splits = (int)std::min<size_t>(std::min(kMatchMaxSplits, std::max(train_tiles, 1)), (kMatchTargetBlocks + blocks - 1) / blocks);
  const size_t set_bytes = sizeof(uint32_t) * words * (size_t)cap * n_pairs;
  int st = grow(c, &c->match_desc, &c->match_desc_bytes, 2 * set_bytes);
  if (!st) st = grow(c, (void**)&c->match_cnt, &c->match_cnt_bytes, sizeof(int) * 2 * (size_t)n_pairs);
  if (!st) st = grow(c, (void**)&c->match_part, &c->match_part_bytes, sizeof(Knn2) * cap * (size_t)splits * n_pairs * dirs);
  if (st) return st;
  MatchArgs a;
  a.desc[0] = (const uint32_t*)c->match_desc;
  a.desc[1] = (const uint32_t*)((const unsigned char*)c->match_desc + set_bytes);
  a.cnt[0] = c->match_cnt;
  a.cnt[1] = c->match_cnt + n_pairs;
  a.cap = cap; a.words = words; a.n_pairs = n_pairs; a.splits = splits;
  a.part = c->match_part;
  HIPCHK(c, hipMemcpyAsync(c->match_desc, query, set_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((unsigned char*)c->match_desc + set_bytes, train, set_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->match_cnt, n_query, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->match_cnt + n_pairs, n_train, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  if (rows > 0) {
    launch_knn2(c->stream, norm, a, dirs, rows);
    HIPCHK(c, hipGetLastError());
  }
  *out = a;
  return UWT_OK;
}

int match_descriptors_enqueue(uwt_ctx* c, const char* what, int n_pairs, int norm, int dim, const void* query, const int32_t* n_query,
                              const void* train, const int32_t* n_train, int cap, float ratio, MatchOut* d_matches, int* d_counts) {
  if (!std::isfinite(ratio)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": ratio is not finite");
  MatchArgs a;
  int st = match_enqueue(c, what, n_pairs, norm, dim, query, n_query, train, n_train, cap, 2, &a);
  if (st) return st;
  launch_match_filter(c->stream, a, ratio, d_matches, d_counts);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

}  // namespace

int uwt_knn_match_batch(uwt_ctx* c, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                        const void* train, const int32_t* n_train, int32_t cap, uwt_knn2* out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_knn_match_batch: null argument");
  MatchArgs a;
  int st = match_enqueue(c, "uwt_knn_match_batch", n_pairs, norm, dim, query, n_query, train, n_train, cap, 1, &a);
  if (st) return st;
  const size_t recs = (size_t)n_pairs * cap;
  st = grow(c, &c->match_out, &c->match_out_bytes, sizeof(Knn2) * recs);
  if (st) return st;
  int rows = 0;
  for (int p = 0; p < n_pairs; p++) rows = std::max(rows, n_query[p]);
  if (rows == 0) return UWT_OK;
  launch_knn2_merge(c->stream, a, rows, (Knn2*)c->match_out);
  HIPCHK(c, hipGetLastError());
  std::vector<uwt_knn2> tmp(recs);
  HIPCHK(c, hipMemcpyAsync(tmp.data(), c->match_out, sizeof(Knn2) * recs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int p = 0; p < n_pairs; p++)   // the rows past a pair's count stay as the caller left them
    std::copy(tmp.begin() + (size_t)p * cap, tmp.begin() + (size_t)p * cap + n_query[p], out + (size_t)p * cap);
  return UWT_OK;
}

int uwt_match_descriptors_batch_async(uwt_ctx* c, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                                      const void* train, const int32_t* n_train, int32_t cap, float ratio, uwt_match* d_matches_out,
                                      int32_t* d_counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_matches_out || !d_counts_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_match_descriptors_batch_async: null argument");
  return match_descriptors_enqueue(c, "uwt_match_descriptors_batch_async", n_pairs, norm, dim, query, n_query, train, n_train, cap, ratio,
                                   reinterpret_cast<MatchOut*>(d_matches_out), d_counts_out);
}

int uwt_match_descriptors_batch(uwt_ctx* c, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                                const void* train, const int32_t* n_train, int32_t cap, float ratio, uwt_match* matches_out,
                                int32_t* counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !matches_out || !counts_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_match_descriptors_batch: null argument");
  const char* what = "uwt_match_descriptors_batch";
  // (the checks of match_enqueue that the size of the result area depends on)
  if (n_pairs < 1 || cap < 1) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_pairs < 1 or cap < 1");
  if (cap > kMatchMaxRows) return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": cap above UWT_MATCH_MAX_ROWS");
  const size_t recs = (size_t)n_pairs * cap, cnt_off = (sizeof(MatchOut) * recs + 15) & ~(size_t)15;
  int st = grow(c, &c->match_out, &c->match_out_bytes, cnt_off + sizeof(int) * n_pairs);
  if (st) return st;
  MatchOut* d_matches = (MatchOut*)c->match_out;
  int* d_counts = (int*)((unsigned char*)c->match_out + cnt_off);
  st = match_descriptors_enqueue(c, what, n_pairs, norm, dim, query, n_query, train, n_train, cap, ratio, d_matches, d_counts);
  if (st) return st;
  std::vector<uwt_match> tmp(recs);
  std::vector<int32_t> cnt((size_t)n_pairs);
  HIPCHK(c, hipMemcpyAsync(cnt.data(), d_counts, sizeof(int) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tmp.data(), d_matches, sizeof(MatchOut) * recs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int p = 0; p < n_pairs; p++) {   // the rows past a pair's count stay as the caller left them
    counts_out[p] = cnt[(size_t)p];
    std::copy(tmp.begin() + (size_t)p * cap, tmp.begin() + (size_t)p * cap + cnt[(size_t)p], matches_out + (size_t)p * cap);
  }
  return UWT_OK;
}

// ---- RANSAC inlier selection (RobustMatcher::ransacTest, src/Tracker.cpp:105-169; the contract: include/uwt.h) -------------------
int uwt_default_ransac_params(uwt_ransac_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  p->distance = 3.0;      // distance_, include/Tracker.h:82
  p->confidence = 0.99;   // confidence_, include/Tracker.h:83
  p->max_hypotheses = 1000;
  p->seed = 0;
  return UWT_OK;
}

int32_t uwt_ransac_iterations(double confidence, int32_t n, int32_t inliers, int32_t max_hypotheses) {
  const int32_t H = max_hypotheses;
  if (confidence == 1.0 || inliers <= 0 || n <= 0) return H;
  const double w = (double)inliers / (double)n;
  const double w2 = w * w, w4 = w2 * w2, w8 = w4 * w4;
  const double num = std::log(1.0 - confidence);
  const double den = w8 >= 1.0 ? -HUGE_VAL : std::log(1.0 - w8);
  if (den >= 0.0 || -num >= (double)H * (-den)) return H;
  return (int32_t)std::rint(num / den);
}

namespace {

static_assert(sizeof(RansacInfo) == sizeof(uwt_ransac_info) && sizeof(uwt_ransac_info) == 88, "uwt_ransac_info layout");
static_assert(sizeof(uwt_ransac_params) == 24, "uwt_ransac_params layout");
static_assert(kRansacMaxHypotheses == UWT_RANSAC_MAX_HYPOTHESES, "RANSAC limits of include/uwt.h");

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// The checks both forms share; *rp: the parameters in force.  Nothing is enqueued when a check fails.
int ransac_check(uwt_ctx* c, const char* what, int n_pairs, int cap, const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur,
                 const int32_t* n_kp_cur, int kp_cap, const uwt_ransac_params* params, uwt_ransac_params* rp) {
  if (n_pairs < 1 || cap < 1 || kp_cap < 1 || !kp_prev || !n_kp_prev || !kp_cur || !n_kp_cur)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list, n_pairs < 1, cap < 1 or kp_cap < 1");
  if (params) *rp = *params;
  else uwt_default_ransac_params(rp);
  if (!std::isfinite(rp->distance) || rp->distance < 0.0 || !(rp->confidence > 0.0 && rp->confidence <= 1.0) || rp->max_hypotheses < 1 ||
      rp->max_hypotheses > UWT_RANSAC_MAX_HYPOTHESES)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": distance, confidence or max_hypotheses outside its range");
  for (int p = 0; p < n_pairs; p++)
    if (n_kp_prev[p] < 0 || n_kp_prev[p] > kp_cap || n_kp_cur[p] < 0 || n_kp_cur[p] > kp_cap)
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key-point count outside 0..kp_cap");
  if (cap > kMatchMaxRows || kp_cap > kMatchMaxRows) return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": cap or kp_cap above UWT_MATCH_MAX_ROWS");
  return UWT_OK;
}

// need(k) on the device for every N of `ns` (ascending, distinct, each in 8..kMatchMaxRows): the rows that are missing under
// these parameters are computed and uploaded on the context stream, one copy per run of neighbouring rows.
int ransac_need_rows(uwt_ctx* c, const uwt_ransac_params& rp, const std::vector<int>& ns) {
  if (!c->ransac_need) {
    HIPCHK(c, hipMalloc((void**)&c->ransac_need, sizeof(int) * kRansacNeedEntries));
    c->ransac_need_host.assign(kRansacNeedEntries, 0);
    c->ransac_row_done.assign((size_t)kMatchMaxRows + 1, 0);
  }
  if (c->ransac_need_confidence != rp.confidence || c->ransac_need_hypotheses != rp.max_hypotheses) {
    std::fill(c->ransac_row_done.begin(), c->ransac_row_done.end(), 0);
    c->ransac_need_confidence = rp.confidence;
    c->ransac_need_hypotheses = rp.max_hypotheses;
  }
  int run_first = 0, run_last = -1;
  auto flush = [&]() -> hipError_t {
    if (run_last < run_first) return hipSuccess;
    const size_t b = ransac_need_row(run_first), e = ransac_need_row(run_last + 1);
    return hipMemcpyAsync(c->ransac_need + b, c->ransac_need_host.data() + b, sizeof(int) * (e - b), hipMemcpyHostToDevice, c->stream);
  };
  for (int n : ns) {
    if (c->ransac_row_done[(size_t)n]) continue;
    int* row = c->ransac_need_host.data() + ransac_need_row(n);
    for (int k = 8; k <= n; k++) row[k - 8] = uwt_ransac_iterations(rp.confidence, n, k, rp.max_hypotheses);
    c->ransac_row_done[(size_t)n] = 1;
    if (run_last >= run_first && n == run_last + 1) { run_last = n; continue; }
    HIPCHK(c, flush());
    run_first = run_last = n;
  }
  HIPCHK(c, flush());
  return UWT_OK;
}

// Stages the key points, fills the rows of need(k) and enqueues k_ransac_gather + k_ransac on the context stream.  The matches and
// their counts are in device memory already; `rows`: a bound of the counts (sizes the gather's grid); ns: the values of N the call
// can meet.  `extra` bytes behind the call's own scratch are the caller's (*extra_out).
int ransac_enqueue(uwt_ctx* c, int n_pairs, int cap, const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur,
                   const int32_t* n_kp_cur, int kp_cap, const uwt_ransac_params& rp, int rows, const std::vector<int>& ns, size_t extra,
                   unsigned char** extra_out, RansacArgs* a) {
  const size_t kp_bytes = align16(sizeof(float2) * (size_t)kp_cap * n_pairs), cnt_bytes = align16(sizeof(int) * (size_t)n_pairs);
  const size_t quad_bytes = sizeof(float4) * (size_t)cap * n_pairs;
  int st = grow(c, &c->ransac_buf, &c->ransac_buf_bytes, 2 * kp_bytes + 2 * cnt_bytes + quad_bytes + extra);
  if (!st) st = ransac_need_rows(c, rp, ns);
  if (st) return st;
  unsigned char* b = (unsigned char*)c->ransac_buf;
  a->kp_prev = (const float2*)b;
  a->kp_cur = (const float2*)(b + kp_bytes);
  a->n_kp_prev = (const int*)(b + 2 * kp_bytes);
  a->n_kp_cur = (const int*)(b + 2 * kp_bytes + cnt_bytes);
  a->quads = (float4*)(b + 2 * kp_bytes + 2 * cnt_bytes);
  *extra_out = b + 2 * kp_bytes + 2 * cnt_bytes + quad_bytes;
  a->need = c->ransac_need;
  a->cap = cap; a->kp_cap = kp_cap; a->n_pairs = n_pairs;
  a->max_hypotheses = rp.max_hypotheses;
  a->seed = rp.seed;
  a->t2 = rp.distance * rp.distance;
  a->invalid_status = UWT_ERR_INVALID_ARG;
  const size_t kp_raw = sizeof(float2) * (size_t)kp_cap * n_pairs;
  HIPCHK(c, hipMemcpyAsync((void*)a->kp_prev, kp_prev, kp_raw, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((void*)a->kp_cur, kp_cur, kp_raw, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((void*)a->n_kp_prev, n_kp_prev, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((void*)a->n_kp_cur, n_kp_cur, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  return UWT_OK;
}

}  // namespace

int uwt_ransac_inliers_batch_async(uwt_ctx* c, int32_t n_pairs, const uwt_match* d_matches, const int32_t* d_n_matches, int32_t cap,
                                   const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur, const int32_t* n_kp_cur,
                                   int32_t kp_cap, const uwt_ransac_params* params, uint8_t* d_mask_out, uwt_match* d_good_out,
                                   int32_t* d_counts_out, uwt_ransac_info* d_info_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_ransac_inliers_batch_async";
  if (!c || !d_matches || !d_n_matches || !d_mask_out || !d_good_out || !d_counts_out || !d_info_out)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_ransac_params rp;
  int st = ransac_check(c, what, n_pairs, cap, kp_prev, n_kp_prev, kp_cur, n_kp_cur, kp_cap, params, &rp);
  if (st) return st;
  std::vector<int> ns;   // the counts are on the device: any N up to cap
  for (int n = kRansacMinSample; n <= cap; n++) ns.push_back(n);
  RansacArgs a;
  unsigned char* extra = nullptr;
  st = ransac_enqueue(c, n_pairs, cap, kp_prev, n_kp_prev, kp_cur, n_kp_cur, kp_cap, rp, cap, ns, 0, &extra, &a);
  if (st) return st;
  a.matches = reinterpret_cast<const MatchOut*>(d_matches);
  a.n_matches = d_n_matches;
  a.mask = d_mask_out;
  a.good = reinterpret_cast<MatchOut*>(d_good_out);
  a.counts = d_counts_out;
  a.info = reinterpret_cast<RansacInfo*>(d_info_out);
  launch_ransac(c->stream, a, cap);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

int uwt_ransac_inliers_batch(uwt_ctx* c, int32_t n_pairs, const uwt_match* matches, const int32_t* n_matches, int32_t cap,
                             const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur, const int32_t* n_kp_cur, int32_t kp_cap,
                             const uwt_ransac_params* params, uint8_t* mask_out, uwt_match* good_out, int32_t* counts_out,
                             uwt_ransac_info* info_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_ransac_inliers_batch";
  if (!c || !matches || !n_matches || !mask_out || !good_out || !counts_out || !info_out)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_ransac_params rp;
  int st = ransac_check(c, what, n_pairs, cap, kp_prev, n_kp_prev, kp_cur, n_kp_cur, kp_cap, params, &rp);
  if (st) return st;
  int rows = 0;
  std::vector<int> ns;
  for (int p = 0; p < n_pairs; p++) {
    const int n = n_matches[p];
    if (n < 0 || n > cap) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": match count outside 0..cap");
    const uwt_match* m = matches + (size_t)p * cap;
    for (int i = 0; i < n; i++)
      if (m[i].query_idx < 0 || m[i].query_idx >= n_kp_prev[p] || m[i].train_idx < 0 || m[i].train_idx >= n_kp_cur[p])
        return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": match index outside its key-point count");
    rows = std::max(rows, n);
    if (n >= kRansacMinSample) ns.push_back(n);
  }
  std::sort(ns.begin(), ns.end());
  ns.erase(std::unique(ns.begin(), ns.end()), ns.end());
  const size_t recs = (size_t)n_pairs * cap;
  const size_t match_bytes = align16(sizeof(MatchOut) * recs), cnt_bytes = align16(sizeof(int) * (size_t)n_pairs), mask_bytes = align16(recs);
  const size_t info_bytes = align16(sizeof(RansacInfo) * (size_t)n_pairs);
  RansacArgs a;
  unsigned char* x = nullptr;
  st = ransac_enqueue(c, n_pairs, cap, kp_prev, n_kp_prev, kp_cur, n_kp_cur, kp_cap, rp, rows, ns,
                      2 * match_bytes + 2 * cnt_bytes + mask_bytes + info_bytes, &x, &a);
  if (st) return st;
  a.matches = (const MatchOut*)x;
  a.good = (MatchOut*)(x + match_bytes);
  a.info = (RansacInfo*)(x + 2 * match_bytes);
  a.n_matches = (const int*)(x + 2 * match_bytes + info_bytes);
  a.counts = (int*)(x + 2 * match_bytes + info_bytes + cnt_bytes);
  a.mask = x + 2 * match_bytes + info_bytes + 2 * cnt_bytes;
  HIPCHK(c, hipMemcpyAsync((void*)a.matches, matches, sizeof(MatchOut) * recs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((void*)a.n_matches, n_matches, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  launch_ransac(c->stream, a, rows);
  HIPCHK(c, hipGetLastError());
  std::vector<uwt_match> good(recs);
  std::vector<uint8_t> mask(recs);
  std::vector<int32_t> cnt((size_t)n_pairs);
  std::vector<uwt_ransac_info> info((size_t)n_pairs);
  HIPCHK(c, hipMemcpyAsync(cnt.data(), a.counts, sizeof(int) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info.data(), a.info, sizeof(RansacInfo) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(mask.data(), a.mask, recs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(good.data(), a.good, sizeof(MatchOut) * recs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int p = 0; p < n_pairs; p++) {   // the rows past a pair's counts stay as the caller left them
    const size_t r0 = (size_t)p * cap;
    counts_out[p] = cnt[(size_t)p];
    info_out[p] = info[(size_t)p];
    std::copy(mask.begin() + r0, mask.begin() + r0 + n_matches[p], mask_out + r0);
    std::copy(good.begin() + r0, good.begin() + r0 + cnt[(size_t)p], good_out + r0);
  }
  return UWT_OK;
}

// ---- SURF detection and description (cuda::SURF_CUDA of src/Tracker.cpp:186-206; the contract: include/uwt.h) --------------------
int uwt_default_surf_params(uwt_surf_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  p->hessian_threshold = 100.0;
  p->n_octaves = 4;
  p->n_octave_layers = 2;
  p->upright = 0;
  return UWT_OK;
}

double uwt_keypoint_angle_deg(float dir_x, float dir_y) {
  double a = std::atan2((double)dir_y, (double)dir_x) * (180.0 / 3.14159265358979323846);
  if (a < 0.0) a += 360.0;
  return a >= 360.0 ? 0.0 : a;
}

static_assert(sizeof(SurfKeypoint) == sizeof(uwt_keypoint) && sizeof(uwt_keypoint) == 32, "uwt_keypoint layout");
static_assert(sizeof(uwt_surf_params) == 24, "uwt_surf_params layout");

namespace {

constexpr size_t kSurfChunkBytes = 256u << 20;   // scratch a chunk of frames may take
constexpr int kSurfMaxChunk = 4096;              // frames of a chunk at most (a launch's grid)

int surf_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap, const uwt_surf_params* params,
               uwt_surf_params* sp) {
  if (n_frames < 1 || cap < 1 || !slots) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_frames < 1, cap < 1 or a null list");
  if (cap > UWT_MATCH_MAX_ROWS) return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": cap above UWT_MATCH_MAX_ROWS");
  for (int f = 0; f < n_frames; f++)
    if (!slot_range_ok(c, slots[f], 1)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": slot out of range");
  if (params) *sp = *params;
  else uwt_default_surf_params(sp);
  if (!std::isfinite(sp->hessian_threshold)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": threshold is not finite");
  if (sp->n_octaves < 1 || sp->n_octaves > kSurfMaxOctaves || sp->n_octave_layers < 1 || sp->n_octave_layers > kSurfMaxLayers - 2)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_octaves or n_octave_layers outside 1..4");
  if (((long long)c->p.width + 1) * ((long long)c->p.height + 1) >= (1ll << 31))
    return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": the integral image has 2^31 entries or more");
  return UWT_OK;
}

// the scratch of a chunk of nf frames: [slots | raw counts | counts | integral | raw | keys | keep | key points | descriptors | extra]
struct SurfLayout {
  size_t slots, raw_count, counts, integral, raw, key, keep, kp, desc, extra, total;
};
SurfLayout surf_layout(const uwt_ctx* c, int nf, size_t raw_cap, int cap, size_t extra) {
  SurfLayout l;
  const size_t px = (size_t)(c->p.width + 1) * (size_t)(c->p.height + 1);
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += align16(bytes); return at; };
  l.slots = take(sizeof(int) * (size_t)nf);
  l.raw_count = take(sizeof(int) * (size_t)nf);
  l.counts = take(sizeof(int) * (size_t)nf);
  l.integral = take(sizeof(uint32_t) * px * nf);
  l.raw = take(sizeof(SurfKeypoint) * raw_cap * nf);
  l.key = take(sizeof(unsigned long long) * raw_cap * nf);
  l.keep = take(raw_cap * nf);
  l.kp = take(sizeof(SurfKeypoint) * (size_t)cap * nf);
  l.desc = take(sizeof(float) * 64 * (size_t)cap * nf);
  l.extra = take(extra);
  l.total = o;
  return l;
}

// frames of a chunk: as many as kSurfChunkBytes hold, one at least
int surf_chunk_frames(const uwt_ctx* c, int n_frames, size_t raw_cap, int cap) {
  const size_t per = surf_layout(c, 1, raw_cap, cap, 0).total;
  const size_t fit = std::max<size_t>(1, kSurfChunkBytes / per);
  return (int)std::min<size_t>(fit, (size_t)std::min(n_frames, kSurfMaxChunk));
}

// Grows the scratch to a chunk of nf frames, sends the chunk's slot list and enqueues the integral images.  *a describes the chunk.
int surf_begin_chunk(uwt_ctx* c, const uwt_surf_params& sp, const int32_t* slots, int nf, size_t raw_cap, int cap, size_t extra,
                     SurfArgs* a, unsigned char** extra_out) {
  const SurfLayout l = surf_layout(c, nf, raw_cap, cap, extra);
  int st = grow(c, &c->surf_buf, &c->surf_buf_bytes, l.total);
  if (st) return st;
  unsigned char* b = (unsigned char*)c->surf_buf;
  const LevelK& L = c->lv[0];
  a->img = c->img[0];
  a->frame_stride = (size_t)L.n;
  a->pitch = L.pitch;
  a->w = c->p.width;
  a->h = c->p.height;
  a->slots = (const int*)(b + l.slots);
  a->n_frames = nf;
  a->integral = (uint32_t*)(b + l.integral);
  a->threshold = sp.hessian_threshold;
  a->n_octaves = sp.n_octaves;
  a->layers = sp.n_octave_layers + 2;
  a->upright = sp.upright ? 1 : 0;
  a->raw = (SurfKeypoint*)(b + l.raw);
  a->raw_key = (unsigned long long*)(b + l.key);
  a->raw_count = (int*)(b + l.raw_count);
  a->raw_cap = (int)raw_cap;
  a->keep = b + l.keep;
  a->kp = (SurfKeypoint*)(b + l.kp);
  a->desc = (float*)(b + l.desc);
  a->counts = (int*)(b + l.counts);
  a->cap = cap;
  if (extra_out) *extra_out = b + l.extra;
  HIPCHK(c, hipMemcpyAsync((void*)a->slots, slots, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, c->stream));
  launch_surf_integral(c->stream, *a);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

// Detection (kp_in null) or the caller's key points, then orientation and descriptors, for n_frames frames in chunks.  The results
// of a chunk are in its scratch; `deliver` takes them (first frame of the chunk, the chunk's arguments) before the next chunk runs.
int surf_run(uwt_ctx* c, const uwt_surf_params& sp, int n_frames, const int32_t* slots, int cap, const uwt_keypoint* kp_in,
             const int32_t* n_in, bool want_desc, const std::function<int(int, const SurfArgs&)>& deliver) {
  int st = compute_begin_pairs(c, n_frames, slots, slots);
  if (st) return st;
  const size_t raw_cap = kp_in ? 0 : surf_raw_bound(c->p.width, c->p.height, sp.n_octaves, sp.n_octave_layers + 2);
  const int chunk = surf_chunk_frames(c, n_frames, raw_cap, cap);
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int nf = std::min(chunk, n_frames - f0);
    SurfArgs a;
    st = surf_begin_chunk(c, sp, slots + f0, nf, raw_cap, cap, 0, &a, nullptr);
    if (st) return st;
    int rows = cap;
    if (kp_in) {
      rows = 0;
      for (int f = 0; f < nf; f++) rows = std::max(rows, n_in[f0 + f]);
      HIPCHK(c, hipMemcpyAsync(a.counts, n_in + f0, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(a.kp, kp_in + (size_t)f0 * cap, sizeof(SurfKeypoint) * (size_t)cap * nf, hipMemcpyHostToDevice, c->stream));
    } else {
      HIPCHK(c, hipMemsetAsync(a.raw_count, 0, sizeof(int) * (size_t)nf, c->stream));
      launch_surf_detect(c->stream, a);
    }
    if (!want_desc) a.desc = nullptr;
    launch_surf_describe(c->stream, a, rows);
    HIPCHK(c, hipGetLastError());
    st = deliver(f0, a);
    if (st) return st;
  }
  return UWT_OK;
}

// the chunk's results to host memory: only the rows below each frame's count are written
int surf_deliver_host(uwt_ctx* c, int f0, const SurfArgs& a, uwt_keypoint* kp_out, float* desc_out, int32_t* counts_out) {
  const size_t recs = (size_t)a.n_frames * a.cap;
  std::vector<int32_t> cnt((size_t)a.n_frames);
  std::vector<uwt_keypoint> kp(recs);
  std::vector<float> desc(a.desc ? recs * 64 : 0);
  HIPCHK(c, hipMemcpyAsync(cnt.data(), a.counts, sizeof(int) * (size_t)a.n_frames, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(kp.data(), a.kp, sizeof(SurfKeypoint) * recs, hipMemcpyDeviceToHost, c->stream));
  if (a.desc) HIPCHK(c, hipMemcpyAsync(desc.data(), a.desc, sizeof(float) * 64 * recs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int f = 0; f < a.n_frames; f++) {
    const size_t r0 = (size_t)f * a.cap, g0 = (size_t)(f0 + f) * a.cap;
    const int n = std::min(std::max(cnt[(size_t)f], 0), a.cap);
    if (counts_out) counts_out[f0 + f] = n;
    std::copy(kp.begin() + r0, kp.begin() + r0 + n, kp_out + g0);
    if (a.desc) std::copy(desc.begin() + r0 * 64, desc.begin() + (r0 + n) * 64, desc_out + g0 * 64);
  }
  return UWT_OK;
}

}  // namespace

int uwt_surf_detect_describe_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params, int32_t cap,
                                   uwt_keypoint* kp_out, float* desc_out, int32_t* counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_detect_describe_batch";
  if (!c || !kp_out || !counts_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_surf_params sp;
  int st = surf_check(c, what, n_frames, slots, cap, params, &sp);
  if (st) return st;
  return surf_run(c, sp, n_frames, slots, cap, nullptr, nullptr, desc_out != nullptr,
                  [&](int f0, const SurfArgs& a) { return surf_deliver_host(c, f0, a, kp_out, desc_out, counts_out); });
}

int uwt_surf_detect_describe_batch_async(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params,
                                         int32_t cap, uwt_keypoint* d_kp_out, float* d_desc_out, int32_t* d_counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_detect_describe_batch_async";
  if (!c || !d_kp_out || !d_counts_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_surf_params sp;
  int st = surf_check(c, what, n_frames, slots, cap, params, &sp);
  if (st) return st;
  st = surf_run(c, sp, n_frames, slots, cap, nullptr, nullptr, d_desc_out != nullptr, [&](int f0, const SurfArgs& a) {
    const size_t recs = (size_t)a.n_frames * a.cap, g0 = (size_t)f0 * a.cap;
    HIPCHK(c, hipMemcpyAsync(d_counts_out + f0, a.counts, sizeof(int) * (size_t)a.n_frames, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_kp_out + g0, a.kp, sizeof(SurfKeypoint) * recs, hipMemcpyDeviceToDevice, c->stream));
    if (a.desc) HIPCHK(c, hipMemcpyAsync(d_desc_out + g0 * 64, a.desc, sizeof(float) * 64 * recs, hipMemcpyDeviceToDevice, c->stream));
    return (int)UWT_OK;
  });
  if (st) return st;
  return compute_end(c, c->dep_first, c->dep_n);
}

int uwt_surf_describe_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params,
                            const uwt_keypoint* keypoints_in, const int32_t* n_in, int32_t cap, uwt_keypoint* kp_out, float* desc_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_describe_batch";
  if (!c || !keypoints_in || !n_in || !kp_out || !desc_out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_surf_params sp;
  int st = surf_check(c, what, n_frames, slots, cap, params, &sp);
  if (st) return st;
  for (int f = 0; f < n_frames; f++) {
    if (n_in[f] < 0 || n_in[f] > cap) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key-point count outside 0..cap");
    const uwt_keypoint* k = keypoints_in + (size_t)f * cap;
    for (int i = 0; i < n_in[f]; i++)
      if (!(std::fabs(k[i].x) <= 1e6f && std::fabs(k[i].y) <= 1e6f && k[i].size > 0.f && k[i].size <= 4096.f))
        return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key point outside |x|, |y| <= 1e6, 0 < size <= 4096");
  }
  // the device keeps every row of a chunk; only the rows below a frame's count come back
  return surf_run(c, sp, n_frames, slots, cap, keypoints_in, n_in, true,
                  [&](int f0, const SurfArgs& a) { return surf_deliver_host(c, f0, a, kp_out, desc_out, nullptr); });
}

int uwt_surf_integral(uwt_ctx* c, int32_t slot, uint32_t* out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_integral";
  if (!c || !out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  uwt_surf_params sp;
  int st = surf_check(c, what, 1, &slot, 1, nullptr, &sp);
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  SurfArgs a;
  st = surf_begin_chunk(c, sp, &slot, 1, 0, 1, 0, &a, nullptr);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(out, a.integral, sizeof(uint32_t) * (size_t)(a.w + 1) * (size_t)(a.h + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_surf_response_layer(uwt_ctx* c, int32_t slot, int32_t octave, int32_t layer, double* out, int32_t* gw, int32_t* gh) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_response_layer";
  if (!c || !out || !gw || !gh) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  if (octave < 0 || octave >= kSurfMaxOctaves || layer < 0 || layer >= kSurfMaxLayers)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": octave outside 0..3 or layer outside 0..5");
  uwt_surf_params sp;
  int st = surf_check(c, what, 1, &slot, 1, nullptr, &sp);
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  const int w = c->p.width >> octave, h = c->p.height >> octave;
  const size_t n = (size_t)w * (size_t)h;
  SurfArgs a;
  unsigned char* x = nullptr;
  st = surf_begin_chunk(c, sp, &slot, 1, 0, 1, sizeof(double) * n + 16, &a, &x);
  if (st) return st;
  launch_surf_response_layer(c->stream, a, octave, layer, (double*)x);
  HIPCHK(c, hipGetLastError());
  if (n) HIPCHK(c, hipMemcpyAsync(out, x, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *gw = w;
  *gh = h;
  return UWT_OK;
}

int uwt_add_patch_points(uwt_ctx* c, int32_t lvl, const float* pts, int32_t n_pts, int32_t patch_size, float* pts_out,
                         int32_t cap, int32_t* count_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !count_out || lvl < 0 || lvl >= c->p.n_levels || n_pts < 0 || (n_pts > 0 && !pts) || cap < 0 || (cap > 0 && !pts_out) ||
      patch_size < 1)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_add_patch_points");
  const int start = (patch_size - 1) / 2;   // src/Tracker.cpp:602
  const size_t in_bytes = (size_t)n_pts * 16, out_bytes = (size_t)cap * 16;
  int st = ensure_scratch(c, 4096 + in_bytes + out_bytes + 64);
  if (st) return st;
  int* d_cnt = (int*)c->scratch;
  float4* d_in = (float4*)((uint8_t*)c->scratch + 4096);
  float4* d_out = (float4*)((uint8_t*)c->scratch + 4096 + in_bytes);
  if (n_pts) HIPCHK(c, hipMemcpyAsync(d_in, pts, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_add_patch_points, dim3(1), dim3(256), 0, c->stream, d_in, n_pts, c->lv[lvl].gw, c->lv[lvl].gh, start, d_out, cap,
                     d_cnt);
  HIPCHK(c, hipGetLastError());
  int cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *count_out = cnt;
  const int m = std::min(cnt, (int)cap);
  if (m > 0) {
    HIPCHK(c, hipMemcpyAsync(pts_out, d_out, (size_t)m * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return UWT_OK;
}

/* ---- frame ingest ------------------------------------------------------------------------------------------------- */

struct uwt_ingest {
  int in_w, in_h, out_w, out_h, device;
  double newK[4];
  std::vector<int16_t> h_map1;
  std::vector<uint16_t> h_map2;
  short2* d_map1 = nullptr;
  uint16_t* d_map2 = nullptr;
  uint8_t* d_raw = nullptr;
  uint8_t* d_und = nullptr;
  hipStream_t stream = nullptr;
};

namespace {

// cvUndistortPoints with 5 fixed iterations and no rectification/projection (normalised output), as
// icvGetRectangles calls it from cvGetOptimalNewCameraMatrix (OpenCV 3.2 calib3d).
void undistort_normalised(double u, double v, const double K[4], const double k[4], float* ox, float* oy) {
  double x = (u - K[2]) / K[0], y = (v - K[3]) / K[1];
  const double x0 = x, y0 = y;
  for (int j = 0; j < 5; j++) {
    const double r2 = x * x + y * y;
    const double icdist = 1.0 / (1.0 + ((0.0 * r2 + k[1]) * r2 + k[0]) * r2);
    const double dX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
    const double dY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
    x = (x0 - dX) * icdist;
    y = (y0 - dY) * icdist;
  }
  *ox = (float)x;
  *oy = (float)y;
}

// getOptimalNewCameraMatrix(K, dist, Size(in), alpha = 1, Size(out), nullptr, false)  (src/CameraModel.cpp:89)
void optimal_new_camera_matrix(const double K[4], const double k[4], int in_w, int in_h, double alpha, int new_w, int new_h,
                               double newK[4]) {
  const int N = 9;
  float iX0 = -3.4028235e38f, iX1 = 3.4028235e38f, iY0 = -3.4028235e38f, iY1 = 3.4028235e38f;
  float oX0 = 3.4028235e38f, oX1 = -3.4028235e38f, oY0 = 3.4028235e38f, oY1 = -3.4028235e38f;
  for (int y = 0; y < N; y++)
    for (int x = 0; x < N; x++) {
      const float px = (float)x * in_w / (N - 1), py = (float)y * in_h / (N - 1);
      float qx, qy;
      undistort_normalised(px, py, K, k, &qx, &qy);
      oX0 = std::min(oX0, qx); oX1 = std::max(oX1, qx); oY0 = std::min(oY0, qy); oY1 = std::max(oY1, qy);
      if (x == 0) iX0 = std::max(iX0, qx);
      if (x == N - 1) iX1 = std::min(iX1, qx);
      if (y == 0) iY0 = std::max(iY0, qy);
      if (y == N - 1) iY1 = std::min(iY1, qy);
    }
  const float iw = iX1 - iX0, ih = iY1 - iY0, ow = oX1 - oX0, oh = oY1 - oY0;
  const double fx0 = (float)(new_w - 1) / iw, fy0 = (float)(new_h - 1) / ih;
  const double cx0 = -fx0 * iX0, cy0 = -fy0 * iY0;
  const double fx1 = (float)(new_w - 1) / ow, fy1 = (float)(new_h - 1) / oh;
  const double cx1 = -fx1 * oX0, cy1 = -fy1 * oY0;
  newK[0] = fx0 * (1 - alpha) + fx1 * alpha;
  newK[1] = fy0 * (1 - alpha) + fy1 * alpha;
  newK[2] = cx0 * (1 - alpha) + cx1 * alpha;
  newK[3] = cy0 * (1 - alpha) + cy1 * alpha;
}

// initUndistortRectifyMap(K, dist, Mat(), newK, size, CV_16SC2, map1, map2)  (src/CameraModel.cpp:90)
void init_undistort_maps(const double K[4], const double k[4], const double newK[4], int w, int h, int16_t* map1,
                         uint16_t* map2) {
  const double ir0 = 1.0 / newK[0], ir2 = -newK[2] / newK[0], ir4 = 1.0 / newK[1], ir5 = -newK[3] / newK[1];
  for (int i = 0; i < h; i++) {
    double _x = i * 0.0 + ir2;
    const double _y = i * ir4 + ir5, _w = 1.0;
    for (int j = 0; j < w; j++, _x += ir0) {
      const double ww = 1.0 / _w, x = _x * ww, y = _y * ww;
      const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
      const double kr = (1 + ((0.0 * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((0.0 * r2 + 0.0) * r2 + 0.0) * r2);
      const double xd = (x * kr + k[2] * _2xy + k[3] * (r2 + 2 * x2));
      const double yd = (y * kr + k[2] * (r2 + 2 * y2) + k[3] * _2xy);
      const double u = K[0] * xd + K[2], v = K[1] * yd + K[3];
      const long iu = std::lrint(u * 32.0), iv = std::lrint(v * 32.0);
      const int su = std::max(-32768, std::min(32767, (int)iu >> 5)), sv = std::max(-32768, std::min(32767, (int)iv >> 5));
      map1[2 * ((size_t)i * w + j)] = (int16_t)su;
      map1[2 * ((size_t)i * w + j) + 1] = (int16_t)sv;
      map2[(size_t)i * w + j] = (uint16_t)(((int)iv & 31) * 32 + ((int)iu & 31));
    }
  }
}

#define ING_CHK(expr)                              \
  do {                                             \
    if ((expr) != hipSuccess) return UWT_ERR_HIP;  \
  } while (0)

int ingest_remap(uwt_ingest* g, const uint8_t* raw, size_t stride, int x0, int y0, int cw, int ch, uint8_t* d_dst, int dst_pitch) {
  ING_CHK(hipSetDevice(g->device));
  if (stride == (size_t)g->in_w)   // tight rows: one linear copy (a 2-D copy is issued row by row)
    ING_CHK(hipMemcpyAsync(g->d_raw, raw, (size_t)g->in_w * g->in_h, hipMemcpyHostToDevice, g->stream));
  else
    ING_CHK(hipMemcpy2DAsync(g->d_raw, g->in_w, raw, stride, g->in_w, g->in_h, hipMemcpyHostToDevice, g->stream));
  hipLaunchKernelGGL(k_remap_crop, dim3((cw * ch + kBlock - 1) / kBlock), dim3(kBlock), 0, g->stream, g->d_raw, g->in_w,
                     g->in_h, (size_t)g->in_w, g->d_map1, g->d_map2, g->out_w, x0, y0, d_dst, cw, ch, dst_pitch);
  ING_CHK(hipGetLastError());
  return UWT_OK;
}

}  // namespace

int uwt_ingest_create(const float K[4], const float dist[4], int32_t in_w, int32_t in_h, int32_t out_w, int32_t out_h,
                      int32_t device, uwt_ingest** out, float newK_out[4]) {
  if (!K || !dist || !out || in_w < 2 || in_h < 2 || out_w < 1 || out_h < 1) return UWT_ERR_INVALID_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return UWT_ERR_NO_DEVICE;
  uwt_ingest* g = new (std::nothrow) uwt_ingest();
  if (!g) return UWT_ERR_CAPACITY;
  g->in_w = in_w; g->in_h = in_h; g->out_w = out_w; g->out_h = out_h; g->device = device;
  const double Kd[4] = {K[0], K[1], K[2], K[3]}, kd[4] = {dist[0], dist[1], dist[2], dist[3]};
  optimal_new_camera_matrix(Kd, kd, in_w, in_h, 1.0, out_w, out_h, g->newK);
  g->h_map1.resize((size_t)out_w * out_h * 2);
  g->h_map2.resize((size_t)out_w * out_h);
  init_undistort_maps(Kd, kd, g->newK, out_w, out_h, g->h_map1.data(), g->h_map2.data());
  if (newK_out)
    for (int i = 0; i < 4; i++) newK_out[i] = (float)g->newK[i];
  bool ok = hipSetDevice(device) == hipSuccess && hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) == hipSuccess &&
            hipMalloc((void**)&g->d_map1, g->h_map1.size() * 2) == hipSuccess &&
            hipMalloc((void**)&g->d_map2, g->h_map2.size() * 2) == hipSuccess &&
            hipMalloc((void**)&g->d_raw, (size_t)in_w * in_h) == hipSuccess &&
            hipMalloc((void**)&g->d_und, (size_t)out_w * out_h) == hipSuccess &&
            hipMemcpy(g->d_map1, g->h_map1.data(), g->h_map1.size() * 2, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(g->d_map2, g->h_map2.data(), g->h_map2.size() * 2, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    uwt_ingest_destroy(g);
    return UWT_ERR_HIP;
  }
  *out = g;
  return UWT_OK;
}

int uwt_ingest_destroy(uwt_ingest* g) {
  if (!g) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(g->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  if (g->d_map1) (void)hipFree(g->d_map1);
  if (g->d_map2) (void)hipFree(g->d_map2);
  if (g->d_raw) (void)hipFree(g->d_raw);
  if (g->d_und) (void)hipFree(g->d_und);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  delete g;
  return UWT_OK;
}

int uwt_ingest_maps(uwt_ingest* g, int16_t* map1_out, uint16_t* map2_out) {
  if (!g || !map1_out || !map2_out) return UWT_ERR_INVALID_ARG;
  std::memcpy(map1_out, g->h_map1.data(), g->h_map1.size() * 2);
  std::memcpy(map2_out, g->h_map2.data(), g->h_map2.size() * 2);
  return UWT_OK;
}

int uwt_ingest_undistort(uwt_ingest* g, const uint8_t* raw, size_t stride, uint8_t* und_out) {
  if (!g || !raw || !und_out || stride < (size_t)g->in_w) return UWT_ERR_INVALID_ARG;
  int st = ingest_remap(g, raw, stride, 0, 0, g->out_w, g->out_h, g->d_und, g->out_w);
  if (st) return st;
  ING_CHK(hipMemcpyAsync(und_out, g->d_und, (size_t)g->out_w * g->out_h, hipMemcpyDeviceToHost, g->stream));
  ING_CHK(hipStreamSynchronize(g->stream));
  return UWT_OK;
}

int uwt_ingest_calculate_roi(uwt_ingest* g, const uint8_t* raw_first, size_t stride, int32_t roi[4]) {
  if (!g || !roi) return UWT_ERR_INVALID_ARG;
  std::vector<uint8_t> und((size_t)g->out_w * g->out_h);
  int st = uwt_ingest_undistort(g, raw_first, stride, und.data());
  if (st) return st;
  // System::CalculateROI (src/System.cpp:148-191): walk in from the four sides along the middle row / column while the
  // undistorted image is 0, then a 5-pixel margin; Rect(p1, p2) => width = p2.x - p1.x.
  const int w = g->out_w, h = g->out_h;
  const int xm = (int)((w - 1) * 0.5), ym = (int)((h - 1) * 0.5);
  int p1x = 0, p1y = 0, p2x = w - 1, p2y = h - 1;
  while (p1x < w - 1 && und[(size_t)ym * w + p1x] == 0) p1x++;
  while (p2x > 0 && und[(size_t)ym * w + p2x] == 0) p2x--;
  while (p1y < h - 1 && und[(size_t)p1y * w + xm] == 0) p1y++;
  while (p2y > 0 && und[(size_t)p2y * w + xm] == 0) p2y--;
  p1x += 5; p2x -= 5; p1y += 5; p2y -= 5;
  roi[0] = p1x; roi[1] = p1y; roi[2] = p2x - p1x; roi[3] = p2y - p1y;
  return UWT_OK;
}

int uwt_ingest_frame(uwt_ingest* g, uwt_ctx* c, int32_t slot, const uint8_t* raw, size_t stride, int32_t x0, int32_t y0) {
  if (!g || !c || !raw || stride < (size_t)g->in_w || !slot_range_ok(c, slot, 1)) return UWT_ERR_INVALID_ARG;
  const int cw = c->p.width, ch = c->p.height;
  if (x0 < 0 || y0 < 0 || x0 + cw > g->out_w || y0 + ch > g->out_h || g->device != c->p.device)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_ingest_frame: crop window outside the undistorted frame");
  // The remap runs on the ingest object's stream and writes straight into the tracker's slot: it is ordered behind the
  // tracker work still in flight on that slot (uwt_track_batch_async returns with its kernels queued), and this call
  // returns only when the slot is written, so whatever the tracker enqueues next sees the new frame.
  int st = dep_wait(c, c->busy, c->busy_next, c->busy_dropped, g->stream, slot, 1);
  if (st) return st;
  st = dep_wait(c, c->fresh, c->fresh_next, c->fresh_dropped, g->stream, slot, 1);
  if (st) return st;
  st = ingest_remap(g, raw, stride, x0, y0, cw, ch, c->img[0] + (size_t)slot * c->lv[0].n, c->lv[0].pitch);
  if (st) return st;
  ING_CHK(hipStreamSynchronize(g->stream));
  return UWT_OK;
}

static int accumulate_trajectory_impl(uwt_ctx* c, bool scan, const float* poses, int32_t n, const float start_pose[7], float t_scale,
                              int32_t reference_axes, float* traj_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !poses || !start_pose || !traj_out || n < 0) return fail(c, UWT_ERR_INVALID_ARG, "uwt_accumulate_trajectory");
  if (n == 0) return UWT_OK;
  const size_t bytes = sizeof(float) * 7 * (size_t)n;
  int st = ensure_scratch(c, 2 * bytes);
  if (st) return st;
  float* din = (float*)c->scratch;
  float* dout = din + 7 * (size_t)n;
  HIPCHK(c, hipMemcpyAsync(din, poses, bytes, hipMemcpyHostToDevice, c->stream));
  Pose P;
  for (int k = 0; k < 4; k++) P.q[k] = start_pose[k];
  for (int k = 0; k < 3; k++) P.t[k] = start_pose[4 + k];
  if (scan) hipLaunchKernelGGL(k_trajectory_scan, dim3(1), dim3(1024), 0, c->stream, din, n, P, t_scale, reference_axes, dout);
  else hipLaunchKernelGGL(k_trajectory, dim3(1), dim3(64), 0, c->stream, din, n, P, t_scale, reference_axes, dout);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(traj_out, dout, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}


int uwt_accumulate_trajectory(uwt_ctx* c, const float* poses, int32_t n, const float start_pose[7], float t_scale,
                              int32_t reference_axes, float* traj_out) {
  return accumulate_trajectory_impl(c, false, poses, n, start_pose, t_scale, reference_axes, traj_out);
}

int uwt_accumulate_trajectory_scan(uwt_ctx* c, const float* poses, int32_t n, const float start_pose[7], float t_scale,
                                   int32_t reference_axes, float* traj_out) {
  return accumulate_trajectory_impl(c, true, poses, n, start_pose, t_scale, reference_axes, traj_out);
}

}  // extern "C"
