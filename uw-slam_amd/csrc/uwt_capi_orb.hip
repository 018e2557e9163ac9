// uwt_capi_orb.hip — host side of libuwt_hip.so: ORB detection and description.
#include "uwt_ctx.h"
#include "uwt_orb.h"

namespace {

// mix() of the RANSAC contract (include/uwt.h)
inline uint32_t orb_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
constexpr uint32_t kOrbPatternSeed = 0x6f726221u;

bool orb_pattern_ok(const int8_t* p) {
  for (int i = 0; i < 512; i++)
    if ((int)p[2 * i] * p[2 * i] + (int)p[2 * i + 1] * p[2 * i + 1] > 225) return false;
  return true;
}

}  // namespace

extern "C" {

// ---- ORB detection and description (cuda::ORB of src/Tracker.cpp:210-223; the contract: include/uwt.h) -----------------------------
int uwt_default_orb_params(uwt_orb_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  p->n_features = 500;
  p->n_levels = 8;
  p->edge_threshold = 31;
  p->fast_threshold = 20;
  p->upright = 0;
  return UWT_OK;
}

int uwt_orb_level_quota(int32_t n_features, int32_t n_levels, int32_t* out) {
  if (!out || n_features < 0 || n_levels < 1 || n_levels > kOrbMaxLevels) return UWT_ERR_INVALID_ARG;
  const double factor = 1.0 / 1.2;
  double fp = 1.0;
  for (int l = 0; l < n_levels; l++) fp = fp * factor;
  double want = (double)n_features * (1.0 - factor) / (1.0 - fp);
  int total = 0;
  for (int l = 0; l < n_levels - 1; l++) {
    out[l] = (int32_t)std::rint(want);
    total += out[l];
    want = want * factor;
  }
  out[n_levels - 1] = std::max(n_features - total, 0);
  return UWT_OK;
}

int uwt_orb_default_pattern(int8_t* out) {
  if (!out) return UWT_ERR_INVALID_ARG;
  uint32_t n = 0;
  for (int k = 0; k < 256; k++) {
    int8_t e[4];
    do {
      for (uint32_t j = 0; j < 4; j++) e[j] = (int8_t)((int)(((uint64_t)orb_mix(kOrbPatternSeed ^ orb_mix(n + j)) * 21u) >> 32) - 10);
      n += 4;
    } while (e[0] == e[2] && e[1] == e[3]);
    std::memcpy(out + 4 * k, e, 4);
  }
  return UWT_OK;
}

int uwt_orb_layer_size(int32_t w, int32_t h, int32_t level, int32_t* lw, int32_t* lh) {
  if (!lw || !lh || w < 1 || h < 1 || level < 0 || level >= kOrbMaxLevels) return UWT_ERR_INVALID_ARG;
  *lw = orb_layer_dim(w, level);
  *lh = orb_layer_dim(h, level);
  return UWT_OK;
}

int uwt_orb_set_pattern(uwt_ctx* c, const int8_t* pattern_or_null) {
  if (!c) return UWT_ERR_INVALID_ARG;
  if (pattern_or_null && !orb_pattern_ok(pattern_or_null))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_orb_set_pattern: a point outside x^2 + y^2 <= 225");
  if (pattern_or_null) std::memcpy(c->orb_pattern, pattern_or_null, sizeof(c->orb_pattern));
  else uwt_orb_default_pattern(c->orb_pattern);
  c->orb_pattern_state = 1;   // the next ORB call sends it, on the stream behind the calls before
  return UWT_OK;
}

static_assert(sizeof(uwt_orb_params) == 20, "uwt_orb_params layout");

namespace {

// the scratch of a chunk of nf frames: [slots | raw counts | counts | layers | raw keys | raw H | kept | keep | key points | descriptors | extra]
struct OrbLayout {
  size_t slots, raw_count, counts, layers, raw_key, raw_h, kept, keep, kp, desc, extra, total;
};
OrbLayout orb_layout(Carve& cv, const OrbArgs& g, int nf, int cap, size_t extra) {
  OrbLayout l;
  l.slots = cv.take<int>((size_t)nf);
  l.raw_count = cv.take<int>((size_t)nf * kOrbMaxLevels);
  l.counts = cv.take<int>((size_t)nf);
  l.layers = cv.take<uint8_t>(g.layer_stride * nf);
  l.raw_key = cv.take<unsigned long long>(g.raw_stride * nf);
  l.raw_h = cv.take<long long>(g.raw_stride * nf);
  l.kept = cv.take<OrbKept>((size_t)g.kept_stride * nf);
  l.keep = cv.take<uint8_t>((size_t)g.kept_stride * nf);
  l.kp = cv.take<OrbKeypoint>((size_t)cap * nf);
  l.desc = cv.take<uint8_t>(32 * (size_t)cap * nf);
  l.extra = cv.take<uint8_t>(extra);
  l.total = cv.total();
  return l;
}

// the context's pattern on the device: the default one the first time, a new one behind uwt_orb_set_pattern
int orb_pattern_ready(uwt_ctx* c) {
  if (c->orb_pattern_state == 0) {
    uwt_orb_default_pattern(c->orb_pattern);
    c->orb_pattern_state = 1;
  }
  if (c->orb_pattern_state == 1) {
    int st = c->orb_pat.reserve(c, c->stream, sizeof(c->orb_pattern));
    if (st) return st;
    HIPCHK(c, hipMemcpyAsync(c->orb_pat.p, c->orb_pattern, sizeof(c->orb_pattern), hipMemcpyHostToDevice, c->stream));
    c->orb_pattern_state = 2;
  }
  return UWT_OK;
}

// the parameters in force (*op) and their checks
int orb_params_check(uwt_ctx* c, const char* what, const uwt_orb_params* params, uwt_orb_params* op) {
  if (params) *op = *params;
  else uwt_default_orb_params(op);
  if (op->n_features < 1 || op->n_features > kOrbMaxFeatures || op->n_levels < 1 || op->n_levels > kOrbMaxLevels)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_features outside 1..65536 or n_levels outside 1..8");
  if (op->edge_threshold < kOrbMinEdge || op->edge_threshold > kOrbMaxEdge || op->fast_threshold < 0 || op->fast_threshold > 255)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": edge_threshold outside 16..1024 or fast_threshold outside 0..255");
  if (c->p.width > kOrbMaxDim || c->p.height > kOrbMaxDim)
    return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": a frame wider or higher than 16384");
  return UWT_OK;
}

// One ORB call: its parameters, its geometry (g), its chunk (a), and the driver's parts over them.  With the device paths of the
// tracking call set (n_frames = 2 n_pairs; orb_track_enqueue's arguments, uwt_ctx.h) a chunk's extra scratch holds the frames' modes:
// detection runs under them (the blocks of a frame on another path return at once), k_orb_take_provided has put the provided records
// and counts where detection would have, and describe, sized by cap, serves both.
struct OrbCall {
  uwt_ctx* c;
  int cap;
  uwt_orb_params op;
  OrbArgs g, a;
  const int* d_path = nullptr;
  int n_pairs = 0;
  const uwt_keypoint* d_prev_kp = nullptr;
  const int32_t* d_n_prev = nullptr;
  int* mode = nullptr;   // the chunk's modes (a.mode) where d_path is set
  Detector d;

  OrbCall(uwt_ctx* c_, const uwt_orb_params* params, int cap_) : c(c_), cap(cap_) {
    d.prepare = [this, params](const char* what, bool detect) {
      const int st = orb_params_check(c, what, params, &op);
      return st ? st : plan(detect);
    };
    d.kp_ok = [this](const uwt_keypoint& k) {
      return orb_keypoint_ok(k.x, k.y, k.octave, op.n_levels, op.edge_threshold, c->p.width, c->p.height);
    };
    d.kp_msg = ": a key point that is not finite, has an octave outside 0..n_levels-1 or lies closer than edge_threshold to a border of "
               "its layer";
    d.chunk = &a;
    d.begin = [this](const int32_t* slots, int nf, size_t extra, unsigned char** x) { return begin(slots, nf, extra, x); };
    d.detect = [this](int f0) {
      if (d_path)
        launch_orb_take_provided(c->stream, a, f0, n_pairs, d_path, reinterpret_cast<const OrbKeypoint*>(d_prev_kp), d_n_prev, mode);
      launch_orb_detect(c->stream, a);
      return (int)UWT_OK;
    };
    d.describe = [this](int rows) { launch_orb_describe(c->stream, a, rows); };
  }
  // the geometry of a call: the layers, the quotas and, when the call detects, the bounds of the candidate lists
  int plan(bool detect) {
    detect_image(c, &g);
    g.n_levels = op.n_levels;
    g.edge = op.edge_threshold;
    g.fast_threshold = op.fast_threshold;
    g.upright = op.upright ? 1 : 0;
    int32_t quota[kOrbMaxLevels] = {};
    uwt_orb_level_quota(op.n_features, op.n_levels, quota);
    size_t loff = 0, roff = 0;
    long long kept = 0;
    for (int l = 0; l < kOrbMaxLevels; l++) {
      const bool on = l < op.n_levels;
      g.lw[l] = on ? orb_layer_dim(g.w, l) : 0;
      g.lh[l] = on ? orb_layer_dim(g.h, l) : 0;
      g.loff[l] = loff;
      if (l > 0) loff += (size_t)g.lw[l] * (size_t)g.lh[l];
      g.quota[l] = on && detect ? quota[l] : 0;
      kept += g.quota[l];
      g.raw_cap[l] = on && detect ? (int)orb_raw_bound(g.lw[l], g.lh[l], g.edge) : 0;
      g.raw_off[l] = roff;
      roff += (size_t)g.raw_cap[l];
    }
    g.layer_stride = (loff + 15) & ~(size_t)15;
    g.raw_stride = roff;
    g.kept_stride = (int)kept;
    Carve cv(16, c->guard_bytes);
    d.frame_bytes = orb_layout(cv, g, 1, cap, 0).total;
    d.rows = d_path ? cap : std::min(cap, std::max(g.kept_stride, 1));   // (a provided list may hold cap records)
    return UWT_OK;
  }
  // Grows the scratch to a chunk of nf frames, sends the chunk's slot list and the pattern, and enqueues the layers.
  int begin(const int32_t* slots, int nf, size_t extra, unsigned char** extra_out) {
    const size_t modes = d_path ? sizeof(int) * (size_t)nf : 0;   // (no call has both)
    Carve cv(16, c->guard_bytes);
    const OrbLayout l = orb_layout(cv, g, nf, cap, extra + modes);
    int st = c->orb_buf.reserve(c, c->stream, cv);
    if (st) return st;
    st = orb_pattern_ready(c);
    if (st) return st;
    unsigned char* b = (unsigned char*)c->orb_buf.p;
    a = g;
    a.slots = (const int*)(b + l.slots);
    a.n_frames = nf;
    a.layers = b + l.layers;
    a.raw_key = (unsigned long long*)(b + l.raw_key);
    a.raw_h = (long long*)(b + l.raw_h);
    a.raw_count = (int*)(b + l.raw_count);
    a.kept = (OrbKept*)(b + l.kept);
    a.keep = b + l.keep;
    a.kp = (OrbKeypoint*)(b + l.kp);
    a.desc = b + l.desc;
    a.desc_row = 32;
    a.counts = (int*)(b + l.counts);
    a.cap = cap;
    a.pattern = (const signed char*)c->orb_pat.p;
    a.mode = mode = modes ? (int*)(b + l.extra) : nullptr;
    if (extra_out) *extra_out = b + l.extra;
    HIPCHK(c, hipMemcpyAsync((void*)a.slots, slots, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(a.raw_count, 0, sizeof(int) * (size_t)nf * kOrbMaxLevels, c->stream));
    launch_orb_layers(c->stream, a);
    HIPCHK(c, hipGetLastError());
    return UWT_OK;
  }
};

}  // namespace

int uwt_orb_detect_describe_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_orb_params* params, int32_t cap,
                                  uwt_keypoint* kp_out, uint8_t* desc_out, int32_t* counts_out) {
  OrbCall o(c, params, cap);
  return detect_entry(c, "uwt_orb_detect_describe_batch", o.d, DetectForm::host, n_frames, slots, cap, nullptr, nullptr, kp_out, desc_out, counts_out);
}

int uwt_orb_detect_describe_batch_async(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_orb_params* params, int32_t cap,
                                        uwt_keypoint* d_kp_out, uint8_t* d_desc_out, int32_t* d_counts_out) {
  OrbCall o(c, params, cap);
  return detect_entry(c, "uwt_orb_detect_describe_batch_async", o.d, DetectForm::device, n_frames, slots, cap, nullptr, nullptr, d_kp_out, d_desc_out,
                      d_counts_out);
}

int uwt_orb_describe_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_orb_params* params, const uwt_keypoint* keypoints_in,
                           const int32_t* n_in, int32_t cap, uwt_keypoint* kp_out, uint8_t* desc_out) {
  OrbCall o(c, params, cap);
  return detect_entry(c, "uwt_orb_describe_batch", o.d, DetectForm::given, n_frames, slots, cap, keypoints_in, n_in, kp_out, desc_out, nullptr);
}

int uwt_orb_layer(uwt_ctx* c, int32_t slot, int32_t level, uint8_t* out, int32_t* lw, int32_t* lh) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_orb_layer";
  if (!c || !out || !lw || !lh) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  if (level < 0 || level >= kOrbMaxLevels) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": level outside 0..7");
  OrbCall o(c, nullptr, 1);
  const OrbArgs& a = o.a;
  int st = stage_begin(c, what, o.d, slot, false, 0, nullptr);
  if (st) return st;
  const size_t w = (size_t)a.lw[level], h = (size_t)a.lh[level];
  if (w && h) {
    if (level == 0)
      HIPCHK(c, hipMemcpy2DAsync(out, w, a.img + (size_t)slot * a.frame_stride, (size_t)a.pitch, w, h, hipMemcpyDeviceToHost, c->stream));
    else
      HIPCHK(c, hipMemcpyAsync(out, a.layers + a.loff[level], w * h, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *lw = (int32_t)w;
  *lh = (int32_t)h;
  return UWT_OK;
}

int uwt_orb_fast_scores(uwt_ctx* c, int32_t slot, int32_t level, int32_t* out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_orb_fast_scores";
  if (!c || !out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  if (level < 0 || level >= kOrbMaxLevels) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": level outside 0..7");
  const size_t n = (size_t)orb_layer_dim(c->p.width, level) * (size_t)orb_layer_dim(c->p.height, level);
  OrbCall o(c, nullptr, 1);
  OrbArgs& a = o.a;
  unsigned char* x = nullptr;
  int st = stage_begin(c, what, o.d, slot, true, sizeof(int) * n + 16, &x);
  if (st) return st;
  if (n) {
    HIPCHK(c, hipMemsetAsync(x, 0, sizeof(int) * n, c->stream));
    a.score_out = (int*)x;
    launch_orb_fast(c->stream, a, level);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, x, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_orb_harris(uwt_ctx* c, int32_t slot, int32_t level, const int32_t* xy, int32_t n, int64_t* H_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_orb_harris";
  if (!c || !xy || !H_out || n < 1) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument or n < 1");
  if (level < 0 || level >= kOrbMaxLevels) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": level outside 0..7");
  const int lw = orb_layer_dim(c->p.width, level), lh = orb_layer_dim(c->p.height, level);
  for (int i = 0; i < n; i++)
    if (xy[2 * i] < 4 || xy[2 * i] >= lw - 4 || xy[2 * i + 1] < 4 || xy[2 * i + 1] >= lh - 4)
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": a pixel closer than 4 to a border of the layer");
  OrbCall o(c, nullptr, 1);
  const OrbArgs& a = o.a;
  unsigned char* x = nullptr;
  Carve cv(16, c->guard_bytes);
  const size_t at_xy = cv.take<int>(2 * (size_t)n), at_h = cv.take<long long>((size_t)n);
  int st = stage_begin(c, what, o.d, slot, false, cv.total(), &x);
  if (!st) st = c->orb_buf.adopt(c, c->stream, cv, x);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(x + at_xy, xy, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
  launch_orb_harris(c->stream, a, level, (const int*)(x + at_xy), n, (long long*)(x + at_h));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(H_out, x + at_h, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

}  // extern "C"

// ---- what the chained tracking call uses of this unit (declared in uwt_ctx.h) -------------------------------------------------------
// Nothing is enqueued when a check fails.
int uwt::orb_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap, const uwt_orb_params* params,
                   uwt_orb_params* op) {
  int st = detect_check(c, what, n_frames, slots, cap);
  return st ? st : orb_params_check(c, what, params, op);
}

// The tracking call's ORB: the path of every previous frame decided on the device, delivered as the asynchronous call delivers.
int uwt::orb_track_enqueue(uwt_ctx* c, const uwt_orb_params& op, int n_pairs, const int32_t* slots, int cap, const int* d_path,
                           const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev, uwt_keypoint* d_kp, uint8_t* d_desc, int* d_counts) {
  OrbCall o(c, nullptr, cap);
  o.op = op;
  o.d_path = d_path;
  o.n_pairs = n_pairs;
  o.d_prev_kp = d_prev_kp;
  o.d_n_prev = d_n_prev;
  o.plan(true);
  return detect_run(c, o.d, 2 * n_pairs, slots, cap, nullptr, nullptr, true,
                    [&](int f0, const DetectArgs& a) { return deliver_device(c, f0, a, d_kp, d_desc, d_counts); });
}
