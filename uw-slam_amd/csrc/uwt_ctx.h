// uwt_ctx.h — internal: the context behind the C ABI of include/uwt.h and what the host units of the library share (uwt_capi.hip
// and uwt_capi_*.hip): the error path, the growable device buffer, the layout carver and the helpers more than one unit calls.
#pragma once

#include "../../include/uwt.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "uwt_launch.h"

static_assert(sizeof(uwt::StatsOut) == sizeof(uwt_stats), "uwt_stats layout");

namespace uwt {

// A device buffer that grows on use (its contents are not kept).  reserve: nothing when it holds `bytes` already; else `stream` is
// drained first — work enqueued before, an asynchronous call's included, may still read the old block — then the block is freed
// and a new one allocated.  One buffer per stage: a stage's asynchronous call is never disturbed by another stage's growth.
//
// Test instrumentation (uwt_debug_guards; off unless a test turns it on, and then nothing below changes an offset, a size or a launch):
// with uwt_ctx::guard_bytes set, the block gets a guard before its first byte and one behind its last, and a carved block one behind
// every array (Carve).  reserve then remembers where the gaps are and fills them with kGuardPattern on `stream` on EVERY use, and
// uwt_debug_check_guards compares them.  The arrays themselves are never filled: only bytes no correct code reads carry the pattern.
struct GuardGap { long long at; size_t bytes; int array; };   // offset from DevBuf::p; the array in front of the gap (-1: the lead)
constexpr unsigned char kGuardPattern = 0xC7;
struct Carve;
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void* block = nullptr;          // what hipMalloc returned: p, or p minus the lead guard
  std::vector<GuardGap> gaps;     // of the last use (empty with guards off)
  int reserve(uwt_ctx* c, hipStream_t stream, size_t want, const Carve* cv = nullptr);
  int reserve(uwt_ctx* c, hipStream_t stream, const Carve& cv);                // cv.total() bytes
  int reserve(uwt_ctx* c, hipStream_t stream, const Carve& cv, size_t want);   // a site that reserves another size than total()
  // the gaps of a carve that lies INSIDE one of the block's arrays, at `base` (a per-stage entry's area behind a detector's chunk)
  int adopt(uwt_ctx* c, hipStream_t stream, const Carve& inner, const void* base);
  hipError_t release();   // the only hipFree of a buffer that can grow
};

// Carves one allocation into arrays: take<T>(n) is the offset of n elements of T, each array starting on the next multiple of
// `align` behind the one before (align may be changed between two takes); total() the bytes to reserve, the last array padded
// like the others, tight() the same without that pad; at<T>(base, offset) the array's address.  guard: uwt_ctx::guard_bytes — not 0:
// every array is followed by a gap of `guard` bytes rounded up to align (recorded in `gaps`, which DevBuf::reserve takes over).
struct Carve {
  size_t align, guard, end = 0;
  std::vector<GuardGap> gaps;
  explicit Carve(size_t a, size_t guard_bytes = 0) : align(a), guard(guard_bytes) {}
  size_t up(size_t b) const { return (b + align - 1) & ~(align - 1); }
  template <typename T> size_t take(size_t n) {
    const size_t at = up(end);
    end = at + sizeof(T) * n;
    if (guard) {
      if (!gaps.empty()) gaps.back().bytes = at - (size_t)gaps.back().at;   // (the pad in front of this array belongs to the gap before)
      const size_t stop = up(end) + up(guard);
      gaps.push_back({(long long)end, stop - end, (int)gaps.size()});
      end = stop;
    }
    return at;
  }
  size_t total() const { return up(end); }
  size_t tight() const { return end; }
  template <typename T> static T* at(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + offset); }
};

}  // namespace uwt

using namespace uwt;

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
  int32_t jacobian = UWT_JACOBIAN_REFERENCE;   // uwt_set_jacobian: every launch that forms Jw reads it through launch_sel
  hipEvent_t ev_pyramids = nullptr, ev_side_done = nullptr, ev_level[UWT_MAX_LEVELS] = {};
  // Early preparation (uwt_tuning::overlap_gradients 1 / 3): past its level 1 a dense batch call reads no plane of a
  // level >= 1, and the next call's preparation — pyramids, gradients of the levels >= 1 — writes nothing else.  A call that ends on
  // level 0 records ev_window[part] behind level 1 on each part's stream; win_open: the previous device-work entry on this context
  // was such a call and nothing has touched the context since (close_window), so the next uwt_track_batch_async may put its
  // preparation on `side` behind these events, under the previous call's level 0.  win_parts: events the call in hand recorded.
  // ev_entry: the context stream at a call's entry, i.e. the previous call's end — the level-0 gradients wait for it.
  // ev_first_end: the end of part 0 of a call that ran as parts — inside the window, and where the preparation is placed then.
  hipEvent_t ev_window[kMaxParts] = {}, ev_entry = nullptr, ev_first_end = nullptr;
  bool win_open = false;
  int win_parts = 0;
  uint8_t* img[UWT_MAX_LEVELS] = {};
  uint16_t* depth[UWT_MAX_LEVELS] = {};
  int16_t* gx[UWT_MAX_LEVELS] = {};
  int16_t* gy[UWT_MAX_LEVELS] = {};
  PairState* state = nullptr;
  // the pair lists the launches read: those of set pair_set.  Two device sets [ref(max_pairs) | tgt(max_pairs)]: an early
  // preparation reads its call's reference list while the previous call's launches still read theirs, so a call with new lists that
  // prepares early sends them to the idle set (on `side`) and makes that set the current one; every other call writes the current
  // set on the context stream, behind everything that read it.
  int* d_ref = nullptr;
  int* d_tgt = nullptr;
  int* d_pair_set[2] = {};
  int pair_set = 0;
  // pinned staging of the pair lists, a ring of kPairStages [ref(max_pairs) | tgt(max_pairs)] blocks: a new list is
  // written to a block neither device set was filled from while the asynchronous copy of an earlier one may still be reading its own
  static constexpr int kPairStages = 4;
  int* h_pairs = nullptr;
  hipEvent_t ev_pairs[kPairStages] = {};
  int pair_stage[2] = {0, 1};           // per device set: the block holding the lists that are in it ...
  int n_pairs_cached[2] = {0, 0};       // ... and how many pairs they have (0: none yet)
  int pair_stage_last = 1;              // the block written last
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
  unsigned int* hist = nullptr;         // general path: [pair][kHistBins], all-zero between evaluations
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
  size_t guard_bytes = 0;               // uwt_debug_guards: guards around and inside every DevBuf (0: none, the default)
  DevBuf scratch;                       // per-stage entry points
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
  DevBuf cand_tab, cand_cnt, cand_work, cand_recs;
  // descriptor matching (uwt_knn_match_batch, uwt_match_descriptors_batch*), each buffer grown on use to what a call needs: both
  // descriptor sets of every pair, their counts (query | train), the 2-NN parts of both directions, and the synchronous calls' results
  DevBuf match_desc, match_cnt, match_part, match_out;
  // RANSAC inlier selection (uwt_ransac_inliers_batch*): the staged key points of both frames, their counts, the (x, y, x', y')
  // table of every match and, for the synchronous call, its inputs and results — grown on use; and need(k) of the contract for
  // every N in 8..UWT_MATCH_MAX_ROWS, k in 8..N (allocated whole on first use, 33 MB; a row is filled the first time a call can
  // meet its N under the parameters the rows were computed for)
  DevBuf ransac_buf;
  int* ransac_need = nullptr;
  std::vector<int> ransac_need_host;
  std::vector<unsigned char> ransac_row_done;
  double ransac_need_confidence = 0.0;
  int ransac_need_hypotheses = 0;
  // SURF detection and description (uwt_surf_*): per chunk of frames the slot list, the counts, the integral images, the raw
  // candidates with their order keys, and the key points and descriptors before they go to the caller — grown on use
  DevBuf surf_buf;
  // ORB detection and description (uwt_orb_*): per chunk of frames the slot list, the counts, the layers above 0, the raw candidates
  // of every layer, the quota survivors, and the key points and descriptors before they go to the caller — grown on use; and the
  // sampling pattern (256 x 4 int8): the host copy, its device copy, and which of them is current (0: neither yet — the default is
  // made on first use; 1: the host copy, to be sent by the next call; 2: both)
  DevBuf orb_buf, orb_pat;
  int8_t orb_pattern[1024] = {};
  int orb_pattern_state = 0;
  // the chained tracking call (uwt_tracking_batch*, uwt_tracking_orb_batch*): per pair and side the key points, descriptors and counts
  // the detector leaves, the paths
  // and flags of the previous frames, symMatches and the RANSAC records; behind them the synchronous form's inputs and results
  DevBuf track_buf;
  // the image warp (uwt_obtain_image_transformed, uwt_warp_image_batch*, uwt_warp_mosaic): the winner planes of every pair and, for
  // the host forms, their inputs and results — grown on use
  DevBuf warp_buf;
  // the point-cloud map (uwt_point_cloud_batch*, uwt_point_cloud_points): the slot list, the per-block counts and their scan and, for
  // the host forms, their inputs and results — grown on use
  DevBuf cloud_buf;
  // pinned staging of its slot list, a ring of kPairStages blocks of max_frames slots (as h_pairs), made on first use: the caller's
  // list is copied before the call returns and the copy to the device never makes the host wait for the stream
  int* h_cloud = nullptr;
  hipEvent_t ev_cloud[kPairStages] = {};
  int cloud_stage = 0;
  // the depth sweep (uwt_sweep_depth_batch*): the slot lists, the codes, the selection's gradient_ planes and sums and, for the host
  // form, its inputs and results — grown on use; and a pinned staging ring for the lists and the codes (as h_cloud), made on first use
  DevBuf sweep_buf;
  int* h_sweep = nullptr;
  hipEvent_t ev_sweep[kPairStages] = {};
  int sweep_stage = 0;
  DevBuf stage[2];                      // uploads of frames whose rows are pitched on the device: [0] context stream, [1] copy stream
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
  // the seeded synchronous calls: the caller's host seeds (max_pairs x 7 floats) are copied here before anything is enqueued and
  // the kernels read them in place (page-locked, device-visible: no copy, no launch); a rerun of the speculative call reads them again
  float* h_seeds = nullptr;             // pinned, made on first use
  float* d_seeds = nullptr;             // its device address
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

namespace uwt {

inline int fail(uwt_ctx* c, int code, const std::string& msg) {
  if (c) c->last_error = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                                                   \
  do {                                                                                                      \
    hipError_t e_ = (expr);                                                                                 \
    if (e_ != hipSuccess)                                                                                   \
      return fail(ctx, UWT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                     \
  } while (0)

// Where a seeded call's alignments start and how their poses cross the level boundaries (uwt.h "seeded calls"): d_seeds null = the
// identity; keep = uwt_seed_options::handoff 1.  The default is every unseeded entry's.
struct Start {
  const float* d_seeds = nullptr;   // n_pairs x 7 floats in memory the device reads, or null
  int keep = 0;
  const int* d_gate = nullptr;      // table calls: per-pair counts, a pair whose count is 0 starts at the identity (k_init_state), or null
  // (handoff_scale_t is any int, non-zero = on, as the kernels always read it: only `keep` can give kHandoffKeep)
  int scale_t(const uwt_params& q) const { return keep ? kHandoffKeep : (q.handoff_scale_t != 0 ? 1 : 0); }
  // what the kernels read of it under the constants q; base: the first pair of the launch where its kernel counts from there (k_init_state)
  StartRec rec(const uwt_params& q, int base = 0) const {
    return {scale_t(q), d_seeds ? d_seeds + 7 * (size_t)base : nullptr, q.initial_error};
  }
};

// ---- helpers of uwt_capi.hip that the other host units call (described at their definitions) ------------------------------
int seed_options(uwt_ctx* c, const char* what, const uwt_seed_options* sopt_or_null, Start* out);
int seeds_clear_of(uwt_ctx* c, const char* what, const float* d_seeds, int n_pairs, const void* d_poses_out, const void* d_stats_out);
// the same against any output of a call: `bytes` bytes at `out` (null: no such output)
int seeds_clear_of_range(uwt_ctx* c, const char* what, const float* d_seeds, int n_pairs, const void* out, size_t bytes);
int stage_host_seeds(uwt_ctx* c, const float* seeds_or_null, int n_pairs, Start* start);
inline bool slot_range_ok(const uwt_ctx* c, int first, int n) { return first >= 0 && n >= 0 && (long long)first + n <= c->p.max_frames; }
template <typename T>
int launch_resize(uwt_ctx* c, const T* src, T* dst, int sw, int sh, int src_pitch, int dw, int dh, int dst_pitch, size_t sfs,
                  size_t dfs, int n_frames, const int* d_slots = nullptr, int first_slot = 0, hipStream_t on = nullptr);   // T: uint8_t, uint16_t
int launch_scharr(uwt_ctx* c, const uint8_t* src, int16_t* gx, int16_t* gy, int w, int h, int pitch, size_t fs, int n_frames,
                  const int* d_slots = nullptr, int first_slot = 0, hipStream_t on = nullptr);
LaunchSel launch_sel(const uwt_ctx* c);
int launch_residual(uwt_ctx* c, hipStream_t s, const ResidualArgs& a, int n_pairs, bool dump);
int launch_general(uwt_ctx* c, hipStream_t s, const ResidualArgs& ra, int n_pairs, bool dump);
// (q: the constants the launches run under; the table calls have their own)
UpdateRule update_rule(const uwt_params& q, bool general);
ResidualArgs residual_args(uwt_ctx* c, int lvl, const uwt_params& q);
inline ResidualArgs residual_args(uwt_ctx* c, int lvl) { return residual_args(c, lvl, c->p); }
UpdateArgs update_args(uwt_ctx* c, int lvl, const uwt_params& q, bool general);
inline UpdateArgs update_args(uwt_ctx* c, int lvl, bool general) { return update_args(c, lvl, c->p, general); }
int ensure_general_buffers(uwt_ctx* c);
void arm_tail(uwt_ctx* c, ResidualArgs& ra, const UpdateArgs& ua);
int poll_arm(uwt_ctx* c);
int poll_any_left(uwt_ctx* c, bool* left);
int dep_wait(uwt_ctx* c, const uwt_ctx::SlotDep* ring, int next, bool dropped, hipStream_t waiter, int first, int n);
// Early preparation: whatever enqueues device work on the context, reads planes back or changes its settings between two batch calls
// closes the window the first one left (uwt_ctx::win_open) — the next call is then enqueued in one piece behind it.  Called by the
// helpers such entries pass through: compute_begin / compute_begin_pairs, upload_pairs, DevBuf::reserve / adopt on any stream but
// the copy stream, the read-back helpers, and by the entries that pass through none of them.  A call refused on its arguments before it
// reaches a helper has touched nothing and may leave the window as it was (uwt.h at uwt_debug_window_open).
inline void close_window(uwt_ctx* c) { c->win_open = false; }
int compute_begin(uwt_ctx* c, int first, int n);
int compute_end(uwt_ctx* c, int first, int n);
int compute_begin_pairs(uwt_ctx* c, int n, const int32_t* slots_a, const int32_t* slots_b);
int upload_pairs(uwt_ctx* c, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots);
int read_back_pairs(uwt_ctx* c, const char* what, int n, float* poses_out, uwt_stats* stats_out);
struct RowSet { const void* d_rows; size_t elem_bytes; const int32_t* counts; void* host_out; };   // (d_rows null: nothing to deliver)
int rows_to_host(uwt_ctx* c, int cap, int n_items, std::initializer_list<RowSet> sets);
int counted_rows_to_host(uwt_ctx* c, const float4* d_rows, size_t stride, const int* d_counts, int n_items, int cap, float* pts_out,
                         int32_t* counts_out);

// ---- the stages of the chained tracking call (uwt_capi_tracking.hip): each stage's device-input form, in the stage's unit -------
// the checks of a SURF call (uwt_capi_surf.hip); *sp: the parameters in force
int surf_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap, const uwt_surf_params* params,
               uwt_surf_params* sp);
// SURF for the 2 x n_pairs frames of a tracking call, job j < n_pairs the previous frame of pair j under d_path[j] (kPathDetect /
// kPathProvided at d_prev_kp, d_n_prev / kPathNone), the others the current frames, detected: the chunk loop of every SURF call, each
// chunk's rows delivered to d_kp (2 n_pairs x cap records), d_desc (x 64 floats) and d_counts (2 n_pairs).  slots: the 2 n_pairs slots.
int surf_track_enqueue(uwt_ctx* c, const uwt_surf_params& sp, int n_pairs, const int32_t* slots, int cap, const int* d_path,
                       const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev, uwt_keypoint* d_kp, float* d_desc, int* d_counts);
// the checks of an ORB call (uwt_capi_orb.hip); *op: the parameters in force
int orb_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap, const uwt_orb_params* params, uwt_orb_params* op);
// ORB for the 2 x n_pairs frames of a tracking call, as surf_track_enqueue: the chunk loop of every ORB call under the context's
// pattern in force, each chunk's rows delivered to d_kp, d_desc (2 n_pairs x cap x 32 bytes) and d_counts
int orb_track_enqueue(uwt_ctx* c, const uwt_orb_params& op, int n_pairs, const int32_t* slots, int cap, const int* d_path,
                      const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev, uwt_keypoint* d_kp, uint8_t* d_desc, int* d_counts);
// symMatches: a matching call's checks, k_knn2 both ways and k_match_filter.  MatchIn::device: the sets and counts are device memory,
// read in place, a count outside 0..cap taken as 0 (uwt_match_descriptors_device_async); host: host memory (uwt_match_descriptors_batch*)
enum class MatchIn { host, device };
int match_descriptors_enqueue(uwt_ctx* c, const char* what, MatchIn in, int n_pairs, int norm, int dim, const void* query,
                              const int32_t* n_query, const void* train, const int32_t* n_train, int cap, float ratio, uwt_match* d_matches,
                              int32_t* d_counts);
// the range check of uwt_ransac_params
bool ransac_params_ok(const uwt_ransac_params& rp);
// ransacTest with every input in device memory: the matches and their counts, both key-point sets as n_pairs x cap uwt_keypoint
// records and their counts (in 0..cap); results as uwt_ransac_inliers_batch_async leaves them (the mask stays in the scratch)
int ransac_device_enqueue(uwt_ctx* c, int n_pairs, int cap, const uwt_ransac_params& rp, const uwt_match* d_matches,
                          const int32_t* d_n_matches, const uwt_keypoint* d_kp_prev, const int32_t* d_n_kp_prev,
                          const uwt_keypoint* d_kp_cur, const int32_t* d_n_kp_cur, uwt_match* d_good, int32_t* d_counts,
                          uwt_ransac_info* d_info);
// the live call from key points that are in device memory: features_device_begin checks the pair lists, makes the context's feat_kp
// (max_pairs x 200 float2) / feat_nkp exist and sends the lists; once the caller's kernels have filled both, features_device_enqueue
// runs the patch producer and the alignment from them (start: a seeded chain's; a pair without a key point starts at the identity)
int features_device_begin(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots);
int features_device_enqueue(uwt_ctx* c, int n_pairs, float* d_poses, uwt_stats* d_stats, const Start& start = Start());
// Tracker::ObtainCandidatePoints on level 0 for the n frames of the device slot list d_slots (uwt_capi_tables.hip: the producer of the
// batched semi-dense calls over cand_tab / cand_cnt / cand_work, grown to what the call needs), enqueued on the context stream: frame
// f's table at *tab + f * *stride, its full count at (*counts)[f]
int candidates_level0_enqueue(uwt_ctx* c, int n, const int* d_slots, double threshold, const float4** tab, size_t* stride,
                              const int** counts);
// UWT_ERR_PAIR_FAILED with the first failed pair's status in the message, or UWT_OK
int first_failure(uwt_ctx* c, const char* what, const uwt_stats* stats, int n);

// The early-exit look of the batch paths, taken one evaluation late (enqueue_estimate has the schedule and the reasons): the
// launch of an evaluation that is due counts the pairs still on the level into one of two device counters; behind it the count
// is copied to page-locked memory, and the host waits for that copy only once the next evaluation has been enqueued.
struct LatePoll {
  int next, pending = -1;   // evaluations before the next look; slot of the look not yet taken
  bool due = false;
  explicit LatePoll(int first_poll) : next(first_poll) {}
  // ahead of evaluation k's launch: the counter its update adds to, cleared on s (null: no look at this evaluation)
  int arm(uwt_ctx* c, hipStream_t s, bool polls, int k, int max_iters, int** active);
  // behind it: the look at the evaluation before (*none_left: every pair has left the level; nothing more is queued then), then
  // this evaluation's read-back on s
  int look(uwt_ctx* c, hipStream_t s, bool* none_left);
};

}  // namespace uwt
