// uwt_capi_surf.hip — host side of libuwt_hip.so: SURF detection and description.
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

static_assert(sizeof(uwt_surf_params) == 24, "uwt_surf_params layout");

namespace {

// the scratch of a chunk of nf frames: [slots | raw counts | counts | integral | raw | keys | keep | key points | descriptors | extra]
struct SurfLayout {
  size_t slots, raw_count, counts, integral, raw, key, keep, kp, desc, extra, total;
};
SurfLayout surf_layout(const uwt_ctx* c, Carve& cv, int nf, size_t raw_cap, int cap, size_t extra) {
  SurfLayout l;
  const size_t px = (size_t)(c->p.width + 1) * (size_t)(c->p.height + 1);
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

// the parameters in force (*sp) and their checks
int surf_params_check(uwt_ctx* c, const char* what, const uwt_surf_params* params, uwt_surf_params* sp) {
  if (params) *sp = *params;
  else uwt_default_surf_params(sp);
  if (!std::isfinite(sp->hessian_threshold)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": threshold is not finite");
  if (sp->n_octaves < 1 || sp->n_octaves > kSurfMaxOctaves || sp->n_octave_layers < 1 || sp->n_octave_layers > kSurfMaxLayers - 2)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_octaves or n_octave_layers outside 1..4");
  if (((long long)c->p.width + 1) * ((long long)c->p.height + 1) >= (1ll << 31))
    return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": the integral image has 2^31 entries or more");
  return UWT_OK;
}

// One SURF call: its parameters, its chunk, and the driver's parts over them.  With the device paths of the tracking call set
// (n_frames = 2 n_pairs; surf_track_enqueue's arguments, uwt_ctx.h) a chunk's extra scratch holds the frames' modes: detection runs
// under them (the blocks of a frame on another path return at once), k_surf_take_provided has put the provided records and counts
// where detection would have, and describe, sized by cap, serves both.
struct SurfCall {
  uwt_ctx* c;
  int cap;
  uwt_surf_params sp;
  size_t raw_cap = 0;
  SurfArgs a;
  const int* d_path = nullptr;
  int n_pairs = 0;
  const uwt_keypoint* d_prev_kp = nullptr;
  const int32_t* d_n_prev = nullptr;
  int* mode = nullptr;   // the chunk's modes (a.mode) where d_path is set
  Detector d;

  SurfCall(uwt_ctx* c_, const uwt_surf_params* params, int cap_) : c(c_), cap(cap_) {
    d.prepare = [this, params](const char* what, bool detect) {
      const int st = surf_params_check(c, what, params, &sp);
      return st ? st : plan(detect);
    };
    d.kp_ok = [](const uwt_keypoint& k) { return surf_keypoint_ok(k.x, k.y, k.size); };
    d.kp_msg = ": key point outside |x|, |y| <= 1e6, 0 < size <= 4096";
    d.chunk = &a;
    d.begin = [this](const int32_t* slots, int nf, size_t extra, unsigned char** x) { return begin(slots, nf, extra, x); };
    d.detect = [this](int f0) {
      if (d_path)
        launch_surf_take_provided(c->stream, a, f0, n_pairs, d_path, reinterpret_cast<const SurfKeypoint*>(d_prev_kp), d_n_prev, mode);
      HIPCHK(c, hipMemsetAsync(a.raw_count, 0, sizeof(int) * (size_t)a.n_frames, c->stream));
      launch_surf_detect(c->stream, a);
      return (int)UWT_OK;
    };
    d.describe = [this](int rows) { launch_surf_describe(c->stream, a, rows); };
  }
  // the geometry under sp: the bound of the candidate lists when the call detects
  int plan(bool detect) {
    raw_cap = detect ? surf_raw_bound(c->p.width, c->p.height, sp.n_octaves, sp.n_octave_layers + 2) : 0;
    Carve cv(16, c->guard_bytes);
    d.frame_bytes = surf_layout(c, cv, 1, raw_cap, cap, 0).total;
    d.rows = cap;
    return UWT_OK;
  }
  // Grows the scratch to a chunk of nf frames, sends the chunk's slot list and enqueues the integral images.
  int begin(const int32_t* slots, int nf, size_t extra, unsigned char** extra_out) {
    const size_t modes = d_path ? sizeof(int) * (size_t)nf : 0;   // (no call has both)
    Carve cv(16, c->guard_bytes);
    const SurfLayout l = surf_layout(c, cv, nf, raw_cap, cap, extra + modes);
    int st = c->surf_buf.reserve(c, c->stream, cv);
    if (st) return st;
    unsigned char* b = (unsigned char*)c->surf_buf.p;
    detect_image(c, &a);
    a.slots = (const int*)(b + l.slots);
    a.n_frames = nf;
    a.integral = (uint32_t*)(b + l.integral);
    a.threshold = sp.hessian_threshold;
    a.n_octaves = sp.n_octaves;
    a.layers = sp.n_octave_layers + 2;
    a.upright = sp.upright ? 1 : 0;
    a.raw = (SurfKeypoint*)(b + l.raw);
    a.raw_key = (unsigned long long*)(b + l.key);
    a.raw_count = (int*)(b + l.raw_count);
    a.raw_cap = (int)raw_cap;
    a.keep = b + l.keep;
    a.kp = (SurfKeypoint*)(b + l.kp);
    a.desc = b + l.desc;
    a.desc_row = sizeof(float) * 64;
    a.counts = (int*)(b + l.counts);
    a.cap = cap;
    a.mode = mode = modes ? (int*)(b + l.extra) : nullptr;
    if (extra_out) *extra_out = b + l.extra;
    HIPCHK(c, hipMemcpyAsync((void*)a.slots, slots, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, c->stream));
    launch_surf_integral(c->stream, a);
    HIPCHK(c, hipGetLastError());
    return UWT_OK;
  }
};

}  // namespace

int uwt_surf_detect_describe_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params, int32_t cap,
                                   uwt_keypoint* kp_out, float* desc_out, int32_t* counts_out) {
  SurfCall s(c, params, cap);
  return detect_entry(c, "uwt_surf_detect_describe_batch", s.d, DetectForm::host, n_frames, slots, cap, nullptr, nullptr, kp_out, desc_out, counts_out);
}

int uwt_surf_detect_describe_batch_async(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params,
                                         int32_t cap, uwt_keypoint* d_kp_out, float* d_desc_out, int32_t* d_counts_out) {
  SurfCall s(c, params, cap);
  return detect_entry(c, "uwt_surf_detect_describe_batch_async", s.d, DetectForm::device, n_frames, slots, cap, nullptr, nullptr, d_kp_out, d_desc_out,
                      d_counts_out);
}

int uwt_surf_describe_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params,
                            const uwt_keypoint* keypoints_in, const int32_t* n_in, int32_t cap, uwt_keypoint* kp_out, float* desc_out) {
  SurfCall s(c, params, cap);
  return detect_entry(c, "uwt_surf_describe_batch", s.d, DetectForm::given, n_frames, slots, cap, keypoints_in, n_in, kp_out, desc_out, nullptr);
}

int uwt_surf_integral(uwt_ctx* c, int32_t slot, uint32_t* out) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_integral";
  if (!c || !out) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  SurfCall s(c, nullptr, 1);
  int st = stage_begin(c, what, s.d, slot, false, 0, nullptr);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(out, s.a.integral, sizeof(uint32_t) * (size_t)(s.a.w + 1) * (size_t)(s.a.h + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_surf_response_layer(uwt_ctx* c, int32_t slot, int32_t octave, int32_t layer, double* out, int32_t* gw, int32_t* gh) {
  if (c) (void)hipSetDevice(c->p.device);
  const char* what = "uwt_surf_response_layer";
  if (!c || !out || !gw || !gh) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  if (octave < 0 || octave >= kSurfMaxOctaves || layer < 0 || layer >= kSurfMaxLayers)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": octave outside 0..3 or layer outside 0..5");
  const int w = c->p.width >> octave, h = c->p.height >> octave;
  const size_t n = (size_t)w * (size_t)h;
  SurfCall s(c, nullptr, 1);
  unsigned char* x = nullptr;
  int st = stage_begin(c, what, s.d, slot, false, sizeof(double) * n + 16, &x);
  if (st) return st;
  launch_surf_response_layer(c->stream, s.a, octave, layer, (double*)x);
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
  int st = detect_check(c, what, n_frames, slots, cap);
  return st ? st : surf_params_check(c, what, params, sp);
}

// The tracking call's SURF: the path of every previous frame decided on the device, delivered as the asynchronous call delivers.
int uwt::surf_track_enqueue(uwt_ctx* c, const uwt_surf_params& sp, int n_pairs, const int32_t* slots, int cap, const int* d_path,
                            const uwt_keypoint* d_prev_kp, const int32_t* d_n_prev, uwt_keypoint* d_kp, float* d_desc, int* d_counts) {
  SurfCall s(c, nullptr, cap);
  s.sp = sp;
  s.d_path = d_path;
  s.n_pairs = n_pairs;
  s.d_prev_kp = d_prev_kp;
  s.d_n_prev = d_n_prev;
  s.plan(true);
  return detect_run(c, s.d, 2 * n_pairs, slots, cap, nullptr, nullptr, true,
                    [&](int f0, const DetectArgs& a) { return deliver_device(c, f0, a, d_kp, d_desc, d_counts); });
}
