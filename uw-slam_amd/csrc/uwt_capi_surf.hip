// uwt_capi_surf.hip — host side of libuwt_hip.so: SURF detection and description.
#include <functional>

#include "uwt_ctx.h"
#include "uwt_surf.h"

extern "C" {

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

// the scratch of a chunk of nf frames: [slots | raw counts | counts | integral | raw | keys | keep | key points | descriptors | extra]
struct SurfLayout {
  size_t slots, raw_count, counts, integral, raw, key, keep, kp, desc, extra, total;
};
SurfLayout surf_layout(const uwt_ctx* c, int nf, size_t raw_cap, int cap, size_t extra) {
  SurfLayout l;
  const size_t px = (size_t)(c->p.width + 1) * (size_t)(c->p.height + 1);
  Carve cv(16);
  l.slots = cv.take<int>((size_t)nf);
  l.raw_count = cv.take<int>((size_t)nf);
  l.counts = cv.take<int>((size_t)nf);
  l.integral = cv.take<uint32_t>(px * nf);
  l.raw = cv.take<SurfKeypoint>(raw_cap * nf);
  l.key = cv.take<unsigned long long>(raw_cap * nf);
  l.keep = cv.take<uint8_t>(raw_cap * nf);
  l.kp = cv.take<SurfKeypoint>((size_t)cap * nf);
  l.desc = cv.take<float>(64 * (size_t)cap * nf);
  l.extra = cv.take<uint8_t>(extra);
  l.total = cv.total();
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
  int st = c->surf_buf.reserve(c, c->stream, l.total);
  if (st) return st;
  unsigned char* b = (unsigned char*)c->surf_buf.p;
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

// where a run's key points come from: nothing set, every frame is detected; else one of the two groups (kp_in wins if both are set)
struct SurfSource {
  const uwt_keypoint* kp_in = nullptr;   // the caller's lists in host memory (n_frames x cap): described as they are, no detection
  const int32_t* n_in = nullptr;         // their counts
  // the tracking call (n_frames = 2 n_pairs), a path per previous frame decided on the device: surf_track_enqueue's arguments (uwt_ctx.h)
  const int* d_path = nullptr;
  int n_pairs = 0;
  const uwt_keypoint* d_prev_kp = nullptr;
  const int32_t* d_n_prev = nullptr;
};

// Key points from `src`, then orientation and descriptors, for n_frames frames in chunks.  The results of a chunk are in its
// scratch; `deliver` takes them (first frame of the chunk, the chunk's arguments) before the next chunk runs.  With device paths a
// chunk's extra scratch holds the frames' modes: detection runs under them (the blocks of a frame on another path return at once),
// k_surf_take_provided has put the provided records and counts where detection would have, and describe, sized by cap, serves both.
int surf_run(uwt_ctx* c, const uwt_surf_params& sp, int n_frames, const int32_t* slots, int cap, const SurfSource& src, bool want_desc,
             const std::function<int(int, const SurfArgs&)>& deliver) {
  int st = compute_begin_pairs(c, n_frames, slots, slots);
  if (st) return st;
  const size_t raw_cap = src.kp_in ? 0 : surf_raw_bound(c->p.width, c->p.height, sp.n_octaves, sp.n_octave_layers + 2);
  const int chunk = surf_chunk_frames(c, n_frames, raw_cap, cap);
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int nf = std::min(chunk, n_frames - f0);
    SurfArgs a;
    unsigned char* x = nullptr;
    st = surf_begin_chunk(c, sp, slots + f0, nf, raw_cap, cap, src.d_path ? sizeof(int) * (size_t)nf : 0, &a, &x);
    if (st) return st;
    int rows = cap;
    if (src.kp_in) {
      rows = 0;
      for (int f = 0; f < nf; f++) rows = std::max(rows, src.n_in[f0 + f]);
      HIPCHK(c, hipMemcpyAsync(a.counts, src.n_in + f0, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(a.kp, src.kp_in + (size_t)f0 * cap, sizeof(SurfKeypoint) * (size_t)cap * nf, hipMemcpyHostToDevice, c->stream));
    } else {
      if (src.d_path) {
        int* mode = reinterpret_cast<int*>(x);
        a.mode = mode;
        launch_surf_take_provided(c->stream, a, f0, src.n_pairs, src.d_path, reinterpret_cast<const SurfKeypoint*>(src.d_prev_kp),
                                  src.d_n_prev, mode);
      }
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

// the chunk's results to the caller's device arrays, every row of the chunk (d_desc is not written when the chunk has no descriptors)
int surf_deliver_device(uwt_ctx* c, int f0, const SurfArgs& a, uwt_keypoint* d_kp, float* d_desc, int32_t* d_counts) {
  const size_t recs = (size_t)a.n_frames * a.cap, g0 = (size_t)f0 * a.cap;
  HIPCHK(c, hipMemcpyAsync(d_counts + f0, a.counts, sizeof(int) * (size_t)a.n_frames, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_kp + g0, a.kp, sizeof(SurfKeypoint) * recs, hipMemcpyDeviceToDevice, c->stream));
  if (a.desc) HIPCHK(c, hipMemcpyAsync(d_desc + g0 * 64, a.desc, sizeof(float) * 64 * recs, hipMemcpyDeviceToDevice, c->stream));
  return UWT_OK;
}

// the chunk's results to host memory: only the rows below each frame's count are written
int surf_deliver_host(uwt_ctx* c, int f0, const SurfArgs& a, uwt_keypoint* kp_out, float* desc_out, int32_t* counts_out) {
  std::vector<int32_t> cnt((size_t)a.n_frames);
  HIPCHK(c, hipMemcpyAsync(cnt.data(), a.counts, sizeof(int) * (size_t)a.n_frames, hipMemcpyDeviceToHost, c->stream));
  const size_t g0 = (size_t)f0 * a.cap;
  int st = rows_to_host(c, a.cap, a.n_frames, {{a.kp, sizeof(SurfKeypoint), cnt.data(), kp_out + g0},
                                                {a.desc, sizeof(float) * 64, cnt.data(), a.desc ? desc_out + g0 * 64 : nullptr}});
  if (!st && counts_out)
    for (int f = 0; f < a.n_frames; f++) counts_out[f0 + f] = std::min(std::max(cnt[(size_t)f], 0), a.cap);
  return st;
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
  return surf_run(c, sp, n_frames, slots, cap, SurfSource(), desc_out != nullptr,
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
  st = surf_run(c, sp, n_frames, slots, cap, SurfSource(), d_desc_out != nullptr,
                [&](int f0, const SurfArgs& a) { return surf_deliver_device(c, f0, a, d_kp_out, d_desc_out, d_counts_out); });
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
      if (!surf_keypoint_ok(k[i].x, k[i].y, k[i].size))
        return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key point outside |x|, |y| <= 1e6, 0 < size <= 4096");
  }
  // the device keeps every row of a chunk; only the rows below a frame's count come back
  return surf_run(c, sp, n_frames, slots, cap, SurfSource{keypoints_in, n_in}, true,
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

}  // extern "C"

// ---- what the chained tracking call uses of this unit (declared in uwt_ctx.h) -------------------------------------------------------
// Nothing is enqueued when a check fails.
int uwt::surf_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap, const uwt_surf_params* params,
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

// The tracking call's SURF: the path of every previous frame decided on the device, delivered as the asynchronous call delivers.
int uwt::surf_track_enqueue(uwt_ctx* c, const uwt_surf_params& sp, int n_pairs, const int32_t* slots, int cap, const int* d_path,
                            const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev, uwt_keypoint* d_kp, float* d_desc, int* d_counts) {
  return surf_run(c, sp, 2 * n_pairs, slots, cap, SurfSource{nullptr, nullptr, d_path, n_pairs, d_prev_kp, d_n_prev}, true,
                  [&](int f0, const SurfArgs& a) { return surf_deliver_device(c, f0, a, d_kp, d_desc, d_counts); });
}
