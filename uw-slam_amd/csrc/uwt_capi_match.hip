// uwt_capi_match.hip — host side of libuwt_hip.so: descriptor matching and RANSAC inlier selection.
#include "uwt_ctx.h"
#include "uwt_match.h"
#include "uwt_ransac.h"
#include "uwt_track.h"

extern "C" {

// ---- descriptor matching: 2-NN both ways, ratio test, symmetry test (RobustMatcher, src/Tracker.cpp:52-102, 202-236) -----------
namespace {

static_assert(sizeof(Knn2) == sizeof(uwt_knn2) && sizeof(MatchOut) == sizeof(uwt_match), "uwt_knn2 / uwt_match layout");
static_assert(kMatchMaxRows == UWT_MATCH_MAX_ROWS && kMatchMaxWords * 4 == UWT_MATCH_MAX_ROW_BYTES, "matching limits of include/uwt.h");
static_assert(kMatchL2 == UWT_NORM_L2 && kMatchHamming == UWT_NORM_HAMMING, "uwt_norm");

// The checks both forms share; *words: the 32-bit words of a row.
int match_shape_check(uwt_ctx* c, const char* what, int n_pairs, int norm, int dim, int cap, int* words) {
  if (n_pairs < 1) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_pairs < 1");
  if (norm != UWT_NORM_L2 && norm != UWT_NORM_HAMMING) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": unknown norm");
  if (dim < 1 || (dim & 3)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": dim must be a positive multiple of 4");
  if (cap < 1) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": cap < 1");
  *words = norm == UWT_NORM_L2 ? dim : dim / 4;
  if (cap > kMatchMaxRows || *words > kMatchMaxWords)
    return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": cap above UWT_MATCH_MAX_ROWS or a row above UWT_MATCH_MAX_ROW_BYTES");
  return UWT_OK;
}

// k_knn2 over sets and counts that are in device memory (`a` but its parts), enqueued on the context stream (dirs = 1: query ->
// train alone; 2: both directions); rows / train_rows bound the rows the launch covers and the rows they are compared with.  The
// train range of a (pair, query tile, direction) is cut into parts until the launch has kMatchTargetBlocks blocks: one pair of
// 2000 x 2000 fills the chip as 1024 pairs of 500 x 500 do; the merge of the parts is exact, so the cut shows in no bit.
int match_core(uwt_ctx* c, MatchArgs& a, int norm, int dirs, int rows, int train_rows) {
  const int tiles = (rows + kMatchTile - 1) / kMatchTile, train_tiles = (train_rows + kMatchTile - 1) / kMatchTile;
  const size_t blocks = (size_t)a.n_pairs * std::max(tiles, 1) * dirs;
  a.splits = (int)std::min<size_t>(std::min(kMatchMaxSplits, std::max(train_tiles, 1)), (kMatchTargetBlocks + blocks - 1) / blocks);
  int st = c->match_part.reserve(c, c->stream, sizeof(Knn2) * a.cap * (size_t)a.splits * a.n_pairs * dirs);
  if (st) return st;
  a.part = (Knn2*)c->match_part.p;
  if (rows > 0) {
    launch_knn2(c->stream, norm, a, dirs, rows);
    HIPCHK(c, hipGetLastError());
  }
  return UWT_OK;
}

// The host form: both sets and their counts are uploaded on the context stream, the core's bounds are the largest counts.  Nothing is
// enqueued when an argument check fails (a failed growth of the parts, in the core, leaves the uploads queued: they touch the stage's
// scratch alone).  The counts are looked at first: one outside 0..cap is reported before a cap above the limit.
int match_enqueue(uwt_ctx* c, const char* what, int n_pairs, int norm, int dim, const void* query, const int32_t* n_query,
                  const void* train, const int32_t* n_train, int cap, int dirs, MatchArgs* a) {
  if (!query || !n_query || !train || !n_train) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list");
  int max_q = 0, max_t = 0;
  for (int p = 0; p < n_pairs; p++) {
    if (n_query[p] < 0 || n_query[p] > cap || n_train[p] < 0 || n_train[p] > cap)
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": descriptor count outside 0..cap");
    max_q = std::max(max_q, n_query[p]);
    max_t = std::max(max_t, n_train[p]);
  }
  int st = match_shape_check(c, what, n_pairs, norm, dim, cap, &a->words);
  if (st) return st;
  const size_t set_bytes = sizeof(uint32_t) * a->words * (size_t)cap * n_pairs;
  st = c->match_desc.reserve(c, c->stream, 2 * set_bytes);
  if (!st) st = c->match_cnt.reserve(c, c->stream, sizeof(int) * 2 * (size_t)n_pairs);
  if (st) return st;
  uint32_t* d_desc[2] = {(uint32_t*)c->match_desc.p, Carve::at<uint32_t>(c->match_desc.p, set_bytes)};
  int* d_cnt[2] = {(int*)c->match_cnt.p, (int*)c->match_cnt.p + n_pairs};
  a->desc[0] = d_desc[0]; a->desc[1] = d_desc[1]; a->cnt[0] = d_cnt[0]; a->cnt[1] = d_cnt[1];
  a->cap = cap; a->n_pairs = n_pairs;
  HIPCHK(c, hipMemcpyAsync(d_desc[0], query, set_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_desc[1], train, set_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_cnt[0], n_query, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_cnt[1], n_train, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  const int rows = dirs == 2 ? std::max(max_q, max_t) : max_q;
  return match_core(c, *a, norm, dirs, rows, dirs == 2 ? rows : max_t);
}

// The device form, both directions: the sets are read in place; the counts are unknown here, so k_match_counts confines them to
// 0..cap and the core's bounds are cap.  (rows = train_rows = cap >= 1: tiles = train_tiles = ceil(cap / kMatchTile) >= 1, so the
// core's formula gives the grid and the splits this form always had, and k_knn2 is always launched.)
int match_device_enqueue(uwt_ctx* c, const char* what, int n_pairs, int norm, int dim, const void* d_query, const int32_t* d_n_query,
                         const void* d_train, const int32_t* d_n_train, int cap, MatchArgs* a) {
  if (!d_query || !d_n_query || !d_train || !d_n_train) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list");
  int st = match_shape_check(c, what, n_pairs, norm, dim, cap, &a->words);
  if (!st) st = c->match_cnt.reserve(c, c->stream, sizeof(int) * 2 * (size_t)n_pairs);
  if (st) return st;
  int* d_cnt[2] = {(int*)c->match_cnt.p, (int*)c->match_cnt.p + n_pairs};
  a->desc[0] = (const uint32_t*)d_query; a->desc[1] = (const uint32_t*)d_train; a->cnt[0] = d_cnt[0]; a->cnt[1] = d_cnt[1];
  a->cap = cap; a->n_pairs = n_pairs;
  launch_match_counts(c->stream, n_pairs, cap, d_n_query, d_n_train, d_cnt[0], d_cnt[1]);
  HIPCHK(c, hipGetLastError());
  return match_core(c, *a, norm, 2, cap, cap);
}

}  // namespace

int uwt_match_descriptors_device_async(uwt_ctx* c, int32_t n_pairs, int32_t norm, int32_t dim, const void* d_query, const int32_t* d_n_query,
                                       const void* d_train, const int32_t* d_n_train, int32_t cap, float ratio, uwt_match* d_matches_out,
                                       int32_t* d_counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_matches_out || !d_counts_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_match_descriptors_device_async: null argument");
  return match_descriptors_enqueue(c, "uwt_match_descriptors_device_async", MatchIn::device, n_pairs, norm, dim, d_query, d_n_query, d_train,
                                   d_n_train, cap, ratio, d_matches_out, d_counts_out);
}

int uwt_knn_match_batch(uwt_ctx* c, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                        const void* train, const int32_t* n_train, int32_t cap, uwt_knn2* out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_knn_match_batch: null argument");
  MatchArgs a;
  int st = match_enqueue(c, "uwt_knn_match_batch", n_pairs, norm, dim, query, n_query, train, n_train, cap, 1, &a);
  if (st) return st;
  st = c->match_out.reserve(c, c->stream, sizeof(Knn2) * (size_t)n_pairs * cap);
  if (st) return st;
  int rows = 0;
  for (int p = 0; p < n_pairs; p++) rows = std::max(rows, n_query[p]);
  if (rows == 0) return UWT_OK;
  launch_knn2_merge(c->stream, a, rows, (Knn2*)c->match_out.p);
  HIPCHK(c, hipGetLastError());
  return rows_to_host(c, cap, n_pairs, {{c->match_out.p, sizeof(Knn2), n_query, out}});
}

int uwt_match_descriptors_batch_async(uwt_ctx* c, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                                      const void* train, const int32_t* n_train, int32_t cap, float ratio, uwt_match* d_matches_out,
                                      int32_t* d_counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !d_matches_out || !d_counts_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_match_descriptors_batch_async: null argument");
  return match_descriptors_enqueue(c, "uwt_match_descriptors_batch_async", MatchIn::host, n_pairs, norm, dim, query, n_query, train, n_train, cap,
                                   ratio, d_matches_out, d_counts_out);
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
  Carve cv(16, c->guard_bytes);   // [matches | counts]
  const size_t o_matches = cv.take<MatchOut>((size_t)n_pairs * cap), o_counts = cv.take<int>((size_t)n_pairs);
  int st = c->match_out.reserve(c, c->stream, cv, cv.tight());
  if (st) return st;
  uwt_match* d_matches = Carve::at<uwt_match>(c->match_out.p, o_matches);
  int* d_counts = Carve::at<int>(c->match_out.p, o_counts);
  st = match_descriptors_enqueue(c, what, MatchIn::host, n_pairs, norm, dim, query, n_query, train, n_train, cap, ratio, d_matches, d_counts);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(counts_out, d_counts, sizeof(int) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  return rows_to_host(c, cap, n_pairs, {{d_matches, sizeof(uwt_match), counts_out, matches_out}});
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

// the call's scratch: [key points of the previous frames | of the current ones | their counts | (x, y, x', y') of every match];
// the synchronous call carves its inputs and results behind these
struct RansacScratch { size_t kp_prev, kp_cur, n_kp_prev, n_kp_cur, quads; };
RansacScratch ransac_carve(Carve& cv, int n_pairs, int cap, int kp_cap) {
  RansacScratch o;
  o.kp_prev = cv.take<float2>((size_t)kp_cap * n_pairs);
  o.kp_cur = cv.take<float2>((size_t)kp_cap * n_pairs);
  o.n_kp_prev = cv.take<int>((size_t)n_pairs);
  o.n_kp_cur = cv.take<int>((size_t)n_pairs);
  o.quads = cv.take<float4>((size_t)cap * n_pairs);
  return o;
}

// The checks both forms share; *rp: the parameters in force.  Nothing is enqueued when a check fails.
int ransac_check(uwt_ctx* c, const char* what, int n_pairs, int cap, const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur,
                 const int32_t* n_kp_cur, int kp_cap, const uwt_ransac_params* params, uwt_ransac_params* rp) {
  if (n_pairs < 1 || cap < 1 || kp_cap < 1 || !kp_prev || !n_kp_prev || !kp_cur || !n_kp_cur)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list, n_pairs < 1, cap < 1 or kp_cap < 1");
  if (params) *rp = *params;
  else uwt_default_ransac_params(rp);
  if (!ransac_params_ok(*rp))
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

// the arguments that do not depend on where a call's inputs and results live (after ransac_need_rows: the triangle exists)
RansacArgs ransac_args(const uwt_ctx* c, const uwt_ransac_params& rp, int n_pairs, int cap, int kp_cap) {
  RansacArgs a = {};
  a.need = c->ransac_need;
  a.cap = cap; a.kp_cap = kp_cap; a.n_pairs = n_pairs;
  a.max_hypotheses = rp.max_hypotheses;
  a.seed = rp.seed;
  a.t2 = rp.distance * rp.distance;
  a.invalid_status = UWT_ERR_INVALID_ARG;
  return a;
}

// The staged forms: grows the scratch to the carve `cv` (ransac_carve at `o` and what the caller carved behind it), fills the rows of need(k)
// for `ns`, the values of N the call can meet, and uploads the (x, y) tables and their counts.  The caller adds the matches and the
// results, which are in device memory, and launches.
int ransac_enqueue(uwt_ctx* c, int n_pairs, int cap, const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur,
                   const int32_t* n_kp_cur, int kp_cap, const uwt_ransac_params& rp, const std::vector<int>& ns, const RansacScratch& o,
                   const Carve& cv, RansacArgs* a) {
  int st = c->ransac_buf.reserve(c, c->stream, cv);
  if (!st) st = ransac_need_rows(c, rp, ns);
  if (st) return st;
  void* b = c->ransac_buf.p;
  *a = ransac_args(c, rp, n_pairs, cap, kp_cap);
  a->kp_prev = Carve::at<float>(b, o.kp_prev);
  a->kp_cur = Carve::at<float>(b, o.kp_cur);
  a->rec_floats = 2;
  a->n_kp_prev = Carve::at<int>(b, o.n_kp_prev);
  a->n_kp_cur = Carve::at<int>(b, o.n_kp_cur);
  a->quads = Carve::at<float4>(b, o.quads);
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
  RansacArgs a;
  Carve cv(16, c->guard_bytes);
  const RansacScratch o = ransac_carve(cv, n_pairs, cap, kp_cap);
  st = ransac_enqueue(c, n_pairs, cap, kp_prev, n_kp_prev, kp_cur, n_kp_cur, kp_cap, rp, ransac_all_rows(cap), o, cv, &a);
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
  RansacArgs a;
  Carve cv(16, c->guard_bytes);   // behind the call's own: [matches | good | info | match counts | inlier counts | mask]
  const RansacScratch o = ransac_carve(cv, n_pairs, cap, kp_cap);
  const size_t o_matches = cv.take<MatchOut>(recs), o_good = cv.take<MatchOut>(recs), o_info = cv.take<RansacInfo>((size_t)n_pairs),
               o_n_matches = cv.take<int>((size_t)n_pairs), o_counts = cv.take<int>((size_t)n_pairs), o_mask = cv.take<uint8_t>(recs);
  st = ransac_enqueue(c, n_pairs, cap, kp_prev, n_kp_prev, kp_cur, n_kp_cur, kp_cap, rp, ns, o, cv, &a);
  if (st) return st;
  void* b = c->ransac_buf.p;
  a.matches = Carve::at<MatchOut>(b, o_matches);
  a.good = Carve::at<MatchOut>(b, o_good);
  a.info = Carve::at<RansacInfo>(b, o_info);
  a.n_matches = Carve::at<int>(b, o_n_matches);
  a.counts = Carve::at<int>(b, o_counts);
  a.mask = Carve::at<uint8_t>(b, o_mask);
  HIPCHK(c, hipMemcpyAsync((void*)a.matches, matches, sizeof(MatchOut) * recs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((void*)a.n_matches, n_matches, sizeof(int) * n_pairs, hipMemcpyHostToDevice, c->stream));
  launch_ransac(c->stream, a, rows);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(counts_out, a.counts, sizeof(int) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info_out, a.info, sizeof(RansacInfo) * n_pairs, hipMemcpyDeviceToHost, c->stream));
  return rows_to_host(c, cap, n_pairs, {{a.mask, 1, n_matches, mask_out}, {a.good, sizeof(MatchOut), counts_out, good_out}});
}

}  // extern "C"

// ---- what the chained tracking call uses of this unit (declared in uwt_ctx.h) -------------------------------------------------------
// symMatches of either form: the ratio test of both directions, the symmetry test and the ordered compaction behind the form's k_knn2
int uwt::match_descriptors_enqueue(uwt_ctx* c, const char* what, MatchIn in, int n_pairs, int norm, int dim, const void* query,
                                   const int32_t* n_query, const void* train, const int32_t* n_train, int cap, float ratio,
                                   uwt_match* d_matches, int32_t* d_counts) {
  if (!std::isfinite(ratio)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": ratio is not finite");
  MatchArgs a;
  int st = in == MatchIn::device ? match_device_enqueue(c, what, n_pairs, norm, dim, query, n_query, train, n_train, cap, &a)
                     : match_enqueue(c, what, n_pairs, norm, dim, query, n_query, train, n_train, cap, 2, &a);
  if (st) return st;
  launch_match_filter(c->stream, a, ratio, reinterpret_cast<MatchOut*>(d_matches), d_counts);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

bool uwt::ransac_params_ok(const uwt_ransac_params& rp) {
  return std::isfinite(rp.distance) && rp.distance >= 0.0 && rp.confidence > 0.0 && rp.confidence <= 1.0 && rp.max_hypotheses >= 1 &&
         rp.max_hypotheses <= UWT_RANSAC_MAX_HYPOTHESES;
}

// The key points are the caller's uwt_keypoint records, read in place, kp_cap = cap; scratch: [(x, y, x', y') of every match | the
// inlier mask]; need(k) for every N up to cap, as in uwt_ransac_inliers_batch_async
int uwt::ransac_device_enqueue(uwt_ctx* c, int n_pairs, int cap, const uwt_ransac_params& rp, const uwt_match* d_matches,
                               const int32_t* d_n_matches, const uwt_keypoint* d_kp_prev, const int32_t* d_n_kp_prev,
                               const uwt_keypoint* d_kp_cur, const int32_t* d_n_kp_cur, uwt_match* d_good, int32_t* d_counts,
                               uwt_ransac_info* d_info) {
  Carve cv(16, c->guard_bytes);
  const size_t o_quads = cv.take<float4>((size_t)cap * n_pairs), o_mask = cv.take<uint8_t>((size_t)cap * n_pairs);
  int st = c->ransac_buf.reserve(c, c->stream, cv);
  if (!st) st = ransac_need_rows(c, rp, ransac_all_rows(cap));
  if (st) return st;
  RansacArgs a = ransac_args(c, rp, n_pairs, cap, cap);
  static_assert(sizeof(uwt_keypoint) == 8 * sizeof(float), "uwt_keypoint: eight 32-bit fields, (x, y) first");
  a.kp_prev = reinterpret_cast<const float*>(d_kp_prev);
  a.kp_cur = reinterpret_cast<const float*>(d_kp_cur);
  a.rec_floats = 8;
  a.n_kp_prev = d_n_kp_prev;
  a.n_kp_cur = d_n_kp_cur;
  a.matches = reinterpret_cast<const MatchOut*>(d_matches);
  a.n_matches = d_n_matches;
  a.quads = Carve::at<float4>(c->ransac_buf.p, o_quads);
  a.mask = Carve::at<uint8_t>(c->ransac_buf.p, o_mask);
  a.good = reinterpret_cast<MatchOut*>(d_good);
  a.counts = d_counts;
  a.info = reinterpret_cast<RansacInfo*>(d_info);
  launch_ransac(c->stream, a, cap);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}
