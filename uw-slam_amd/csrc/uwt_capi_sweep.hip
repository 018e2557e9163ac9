// uwt_capi_sweep.hip — host side of libuwt_hip.so: the depth sweep (EXTENSION), a keyframe's depth codes from the frames tracked against
// it and their poses in device memory.  include/uwt.h states the contract, uwt_sweep_kernels.h the kernel.
#include "uwt_ctx.h"
#include "uwt_sweep.h"

namespace {

static_assert(sizeof(uwt_sweep_params) == 64 && offsetof(uwt_sweep_params, threshold) == 8 && offsetof(uwt_sweep_params, n_views) == 16 &&
                  offsetof(uwt_sweep_params, reserved) == 48, "uwt_sweep_params layout");
static_assert(sizeof(uwt_sweep_info) == 64 && sizeof(SweepInfo) == sizeof(uwt_sweep_info), "uwt_sweep_info layout");
static_assert(offsetof(uwt_sweep_info, n_outcome) == 8 && offsetof(uwt_sweep_info, sum_cost) == 40 &&
                  offsetof(uwt_sweep_info, reserved) == 56, "uwt_sweep_info layout");

constexpr int kSweepMaxJobs = 65535;   // jobs are the grid's y

bool codes_ok(const uint16_t* codes, int n) {
  for (int k = 0; k < n; k++)
    if (codes[k] < 1 || codes[k] > 32767 || (k && codes[k] <= codes[k - 1])) return false;
  return true;
}

// Every check the host can make; nothing is enqueued and no buffer grows when one fails.
int sweep_check(uwt_ctx* c, const char* what, int n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const uint16_t* codes,
                const uwt_sweep_params* p) {
  const std::string w(what);
  if (!ref_slots || !view_slots || !codes || !p) return fail(c, UWT_ERR_INVALID_ARG, w + ": null argument");
  if (n_jobs < 1 || n_jobs > c->p.max_pairs || n_jobs > kSweepMaxJobs) return fail(c, UWT_ERR_INVALID_ARG, w + ": n_jobs outside 1..max_pairs");
  if (p->lvl < 0 || p->lvl >= c->p.n_levels) return fail(c, UWT_ERR_INVALID_ARG, w + ": level out of range");
  if (p->source < 0 || p->source > 1 || p->n_views < 1 || p->n_views > kSweepMaxViews || p->n_hyp < 3 || p->n_hyp > kSweepMaxHyp ||
      p->radius < 1 || p->radius > 2 || p->refine < 0 || p->refine > 1)
    return fail(c, UWT_ERR_INVALID_ARG, w + ": source, n_views, n_hyp, radius or refine out of range");
  if (p->max_mean_abs < 1 || p->uniq_num < 1 || p->uniq_den < 1 || p->min_parallax < 2)
    return fail(c, UWT_ERR_INVALID_ARG, w + ": max_mean_abs, uniq_num or uniq_den < 1, or min_parallax < 2");
  if (p->reserved[0] || p->reserved[1] || p->reserved[2] || p->reserved[3] || !std::isfinite(p->threshold))
    return fail(c, UWT_ERR_INVALID_ARG, w + ": a non-zero reserved word or a threshold that is not finite");
  for (int i = 0; i < n_jobs; i++) {
    if (!slot_range_ok(c, ref_slots[i], 1)) return fail(c, UWT_ERR_INVALID_ARG, w + ": slot out of range");
    for (int v = 0; v < p->n_views; v++)
      if (!slot_range_ok(c, view_slots[i * p->n_views + v], 1)) return fail(c, UWT_ERR_INVALID_ARG, w + ": slot out of range");
  }
  if (!codes_ok(codes, p->n_hyp)) return fail(c, UWT_ERR_INVALID_ARG, w + ": codes not strictly increasing or outside 1..32767");
  return UWT_OK;
}

// the work area of a call at the base of sweep_buf: [ref slots | view slots | codes | gradient_ sums | gradient_ planes]
struct SweepWork {
  size_t o_ref, o_view, o_codes, o_sums, o_mag;
};
SweepWork sweep_work_layout(Carve& cv, const LevelK& L, int n_jobs, const uwt_sweep_params& p) {
  SweepWork w;
  w.o_ref = cv.take<int>((size_t)n_jobs);
  w.o_view = cv.take<int>((size_t)n_jobs * p.n_views);
  w.o_codes = cv.take<uint16_t>(kSweepMaxHyp);
  w.o_sums = cv.take<unsigned long long>(p.source == 1 ? (size_t)n_jobs : 0);
  w.o_mag = cv.take<uint8_t>(p.source == 1 ? (size_t)n_jobs * L.n : 0);
  return w;
}

// The caller's lists and codes to the device through the pinned ring (they may be temporaries: copied before this returns; the copies
// from page-locked memory are enqueued without a wait for what the stream holds).  The only wait is for the copies that read this
// block kPairStages calls ago.
int sweep_send(uwt_ctx* c, int n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const uint16_t* codes,
               const uwt_sweep_params& p, int* d_ref, int* d_view, uint16_t* d_codes) {
  const size_t block = (size_t)c->p.max_pairs * (1 + kSweepMaxViews) + kSweepMaxHyp / 2;
  if (!c->h_sweep) {
    HIPCHK(c, hipHostMalloc((void**)&c->h_sweep, sizeof(int) * block * uwt_ctx::kPairStages));
    for (hipEvent_t& e : c->ev_sweep) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  const int stage = (c->sweep_stage + 1) % uwt_ctx::kPairStages;
  HIPCHK(c, hipEventSynchronize(c->ev_sweep[stage]));
  int* h_ref = c->h_sweep + stage * block;
  int* h_view = h_ref + c->p.max_pairs;
  uint16_t* h_codes = reinterpret_cast<uint16_t*>(h_view + (size_t)c->p.max_pairs * kSweepMaxViews);
  std::memcpy(h_ref, ref_slots, sizeof(int) * (size_t)n_jobs);
  std::memcpy(h_view, view_slots, sizeof(int) * (size_t)n_jobs * p.n_views);
  std::memset(h_codes, 0, sizeof(uint16_t) * kSweepMaxHyp);
  std::memcpy(h_codes, codes, sizeof(uint16_t) * (size_t)p.n_hyp);
  c->sweep_stage = stage;
  HIPCHK(c, hipMemcpyAsync(d_ref, h_ref, sizeof(int) * (size_t)n_jobs, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_view, h_view, sizeof(int) * (size_t)n_jobs * p.n_views, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_codes, h_codes, sizeof(uint16_t) * kSweepMaxHyp, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_sweep[stage], c->stream));
  return UWT_OK;
}

// The batch call, enqueued on the context stream (the arguments have passed sweep_check; sweep_buf holds the work area w at its base).
int sweep_enqueue(uwt_ctx* c, int n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const float* d_poses, const uint16_t* codes,
                  const uwt_sweep_params& p, const SweepWork& w, const uwt_sweep_io& io) {
  int lo = c->p.max_frames, hi = 0;   // the slot range the call names
  for (int i = 0; i < n_jobs; i++) {
    lo = std::min(lo, ref_slots[i]);
    hi = std::max(hi, ref_slots[i] + 1);
  }
  for (int i = 0; i < n_jobs * p.n_views; i++) {
    lo = std::min(lo, view_slots[i]);
    hi = std::max(hi, view_slots[i] + 1);
  }
  c->dep_first = lo;
  c->dep_n = hi - lo;
  int st = compute_begin(c, c->dep_first, c->dep_n);
  if (st) return st;
  const LevelK& L = c->lv[p.lvl];
  void* b = c->sweep_buf.p;
  SweepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.L = L;
  a.img = c->img[p.lvl];
  a.ref_slots = Carve::at<int>(b, w.o_ref);
  a.view_slots = Carve::at<int>(b, w.o_view);
  a.codes = Carve::at<uint16_t>(b, w.o_codes);
  a.poses = d_poses;
  st = sweep_send(c, n_jobs, ref_slots, view_slots, codes, p, const_cast<int*>(a.ref_slots), const_cast<int*>(a.view_slots),
                  const_cast<uint16_t*>(a.codes));
  if (st) return st;
  if (p.source == 1) {   // gradient_ of the reference slots and its sums, as ObtainCandidatePoints' producer makes them
    unsigned long long* sums = Carve::at<unsigned long long>(b, w.o_sums);
    uint8_t* mag = Carve::at<uint8_t>(b, w.o_mag);
    HIPCHK(c, hipMemsetAsync(sums, 0, sizeof(unsigned long long) * (size_t)n_jobs, c->stream));
    launch_grad_mag(c->stream, L, n_jobs, a.ref_slots, c->gx[p.lvl], c->gy[p.lvl], mag, sums);
    HIPCHK(c, hipGetLastError());
    a.mag = mag;
    a.mag_sums = sums;
  }
  a.threshold = p.threshold;
  a.n_views = p.n_views;
  a.n_hyp = p.n_hyp;
  a.radius = p.radius;
  a.poor_limit = (long long)p.max_mean_abs * (2 * p.radius + 1) * (2 * p.radius + 1) * p.n_views;
  a.uniq_num = p.uniq_num;
  a.uniq_den = p.uniq_den;
  a.min_parallax = p.min_parallax;
  a.refine = p.refine;
  a.depth = io.d_depth;
  a.cost = io.d_cost;
  a.outcome = io.d_outcome;
  a.info = reinterpret_cast<SweepInfo*>(io.d_info);
  a.invalid_status = UWT_ERR_INVALID_ARG;
  HIPCHK(c, hipMemsetAsync(io.d_info, 0, sizeof(uwt_sweep_info) * (size_t)n_jobs, c->stream));
  launch_sweep(c->stream, launch_sel(c), a, n_jobs);
  HIPCHK(c, hipGetLastError());
  return compute_end(c, c->dep_first, c->dep_n);
}

}  // namespace

extern "C" {

int uwt_default_sweep_params(uwt_sweep_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  p->source = 1;
  p->threshold = 20.0;   // the GRADIENT_THRESHOLD the reference's candidate tables are made with
  p->n_views = 1;
  p->n_hyp = 32;
  p->radius = 2;
  p->max_mean_abs = 12;
  p->uniq_num = 3;
  p->uniq_den = 4;
  p->min_parallax = 4;
  p->refine = 1;
  return UWT_OK;
}

int uwt_sweep_hypotheses(double z_near, double z_far, double depth_scale, int32_t n, uint16_t* codes_out) {
  if (!codes_out || n < 3 || n > kSweepMaxHyp) return UWT_ERR_INVALID_ARG;
  if (!std::isfinite(z_near) || !std::isfinite(z_far) || !std::isfinite(depth_scale) || !(z_near > 0.0) || !(depth_scale > 0.0) ||
      !(z_near < z_far))
    return UWT_ERR_INVALID_ARG;
  uint16_t codes[kSweepMaxHyp];
  const double r0 = 1.0 / z_near, step = (1.0 / z_far - r0) / (double)(n - 1);
  for (int k = 0; k < n; k++) {
    const double rho = r0 + (double)k * step;
    const double d = std::rint(1.0 / (rho * depth_scale));
    if (!(d >= 1.0 && d <= 32767.0)) return UWT_ERR_INVALID_ARG;
    codes[k] = (uint16_t)d;
  }
  if (!codes_ok(codes, n)) return UWT_ERR_INVALID_ARG;
  std::memcpy(codes_out, codes, sizeof(uint16_t) * (size_t)n);
  return UWT_OK;
}

int uwt_sweep_depth_batch_async(uwt_ctx* c, int32_t n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const float* d_poses,
                                const uint16_t* codes, const uwt_sweep_params* params, const uwt_sweep_io* io) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (!d_poses || !io || !io->d_depth || !io->d_info) return fail(c, UWT_ERR_INVALID_ARG, "uwt_sweep_depth_batch_async: null argument");
  int st = sweep_check(c, "uwt_sweep_depth_batch_async", n_jobs, ref_slots, view_slots, codes, params);
  if (st) return st;
  Carve cv(256, c->guard_bytes);
  const SweepWork w = sweep_work_layout(cv, c->lv[params->lvl], n_jobs, *params);
  st = c->sweep_buf.reserve(c, c->stream, cv);
  if (st) return st;
  return sweep_enqueue(c, n_jobs, ref_slots, view_slots, d_poses, codes, *params, w, *io);
}

int uwt_sweep_depth_batch(uwt_ctx* c, int32_t n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const float* poses,
                          const uint16_t* codes, const uwt_sweep_params* params, uint16_t* depth_out, uint16_t* cost_out,
                          uint8_t* outcome_out, uwt_sweep_info* info_out) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (!poses || !depth_out || !info_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_sweep_depth_batch: null argument");
  int st = sweep_check(c, "uwt_sweep_depth_batch", n_jobs, ref_slots, view_slots, codes, params);
  if (st) return st;
  const LevelK& L = c->lv[params->lvl];
  const size_t planes = (size_t)L.n * n_jobs, n_poses = 7 * (size_t)n_jobs * params->n_views;
  Carve cv(256, c->guard_bytes);   // [the work area | poses | records | depth | cost | outcome]
  const SweepWork w = sweep_work_layout(cv, L, n_jobs, *params);
  const size_t o_pose = cv.take<float>(n_poses), o_info = cv.take<uwt_sweep_info>((size_t)n_jobs), o_d = cv.take<uint16_t>(planes),
               o_c = cv.take<uint16_t>(cost_out ? planes : 0), o_o = cv.take<uint8_t>(outcome_out ? planes : 0);
  st = c->sweep_buf.reserve(c, c->stream, cv);
  if (st) return st;
  void* b = c->sweep_buf.p;
  uwt_sweep_io io;
  io.d_depth = Carve::at<uint16_t>(b, o_d);
  io.d_cost = cost_out ? Carve::at<uint16_t>(b, o_c) : nullptr;
  io.d_outcome = outcome_out ? Carve::at<uint8_t>(b, o_o) : nullptr;
  io.d_info = Carve::at<uwt_sweep_info>(b, o_info);
  float* d_poses = Carve::at<float>(b, o_pose);
  HIPCHK(c, hipMemcpyAsync(d_poses, poses, sizeof(float) * n_poses, hipMemcpyHostToDevice, c->stream));
  st = sweep_enqueue(c, n_jobs, ref_slots, view_slots, d_poses, codes, *params, w, io);
  if (st) return st;
  const size_t rows = (size_t)L.ih * n_jobs;   // a job's rows follow the previous job's: one strided copy per output
  HIPCHK(c, hipMemcpy2DAsync(depth_out, 2 * (size_t)L.iw, io.d_depth, 2 * (size_t)L.pitch, 2 * (size_t)L.iw, rows, hipMemcpyDeviceToHost, c->stream));
  if (cost_out)
    HIPCHK(c, hipMemcpy2DAsync(cost_out, 2 * (size_t)L.iw, io.d_cost, 2 * (size_t)L.pitch, 2 * (size_t)L.iw, rows, hipMemcpyDeviceToHost, c->stream));
  if (outcome_out)
    HIPCHK(c, hipMemcpy2DAsync(outcome_out, L.iw, io.d_outcome, L.pitch, L.iw, rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(info_out, io.d_info, sizeof(uwt_sweep_info) * (size_t)n_jobs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n_jobs; i++)
    if (info_out[i].status != UWT_OK)
      return fail(c, UWT_ERR_PAIR_FAILED, std::string("uwt_sweep_depth_batch: at least one job failed, first status: ") +
                                              uwt_status_string(info_out[i].status));
  return UWT_OK;
}

}  // extern "C"
