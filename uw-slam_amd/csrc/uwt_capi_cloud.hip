// uwt_capi_cloud.hip — host side of libuwt_hip.so: the RGB-D point-cloud map, Visualizer::AddPointCloudFromRGBD for a batch of
// resident frames with the poses in device memory and for one explicit table, and the trajectory accumulation on device pointers that
// feeds it.  include/uwt.h states the contract, uwt_cloud_kernels.h the passes.
#include "uwt_ctx.h"
#include "uwt_cloud.h"

namespace {

static_assert(sizeof(uwt_cloud_point) == 16 && sizeof(uwt_cloud_params) == 32, "uwt_cloud_point / uwt_cloud_params layout");
static_assert(sizeof(uwt_cloud_info) == 32 && sizeof(CloudInfo) == sizeof(uwt_cloud_info), "uwt_cloud_info layout");
static_assert(offsetof(uwt_cloud_info, offset) == 16 && offsetof(uwt_cloud_info, written) == 24, "uwt_cloud_info layout");
static_assert(offsetof(uwt_cloud_params, threshold) == 16 && offsetof(uwt_cloud_params, reserved) == 24, "uwt_cloud_params layout");

constexpr int kCloudMaxFrames = 65535;   // frames are the grid's y
constexpr int kCloudMaxRows = 1 << 30;   // rows of an explicit table at most

// the range check of uwt_cloud_params (with_source: the batch calls; the explicit table ignores source and threshold)
int cloud_params_check(uwt_ctx* c, const char* what, const uwt_cloud_params* p, bool with_source) {
  if (!p) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null params");
  if (p->mode < 0 || p->mode > 1 || p->stride < 1 || p->skip_invalid < 0 || p->skip_invalid > 1 || p->reserved[0] || p->reserved[1])
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": mode or skip_invalid outside 0..1, stride < 1 or a non-zero reserved word");
  if (with_source && (p->source < 0 || p->source > 1 || !std::isfinite(p->threshold)))
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": source outside 0..1 or a threshold that is not finite");
  return UWT_OK;
}

// Every check of the batch call the host can make; nothing is enqueued and no buffer grows when one fails.
int cloud_batch_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, const uwt_cloud_params* params, const void* points,
                      int64_t cap) {
  if (!slots || cap < 0 || (cap > 0 && !points)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument or cap < 0");
  if (n_frames < 1 || n_frames > c->p.max_frames || n_frames > kCloudMaxFrames)
    return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_frames outside 1..max_frames");
  for (int i = 0; i < n_frames; i++)
    if (!slot_range_ok(c, slots[i], 1)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": slot out of range");
  return cloud_params_check(c, what, params, true);
}

// the work area of a call at the base of cloud_buf: [slot list | block counts | their scan]; `rows`: the bound of a frame's table
struct CloudWork {
  int bpf, run;
  size_t o_slots, o_counts, o_base;
};
CloudWork cloud_work_layout(Carve& cv, int rows, int stride, int n_frames) {
  CloudWork w;
  cloud_shape(rows, stride, n_frames, &w.bpf, &w.run);
  const size_t m = (size_t)w.bpf * n_frames;
  w.o_slots = cv.take<int>((size_t)n_frames);
  w.o_counts = cv.take<int>(m);
  w.o_base = cv.take<long long>(m + 1);
  return w;
}

CloudArgs cloud_args(uwt_ctx* c, const uwt_cloud_params& p, const CloudWork& w, int rows) {
  CloudArgs a;
  std::memset(&a, 0, sizeof(a));
  void* b = c->cloud_buf.p;
  a.L = c->lv[0];
  a.img = c->img[0];
  a.depth = c->p.has_depth ? c->depth[0] : nullptr;
  a.slots = Carve::at<int>(b, w.o_slots);
  a.n = rows;
  a.mode = p.mode;
  a.stride = p.stride;
  a.skip_invalid = p.skip_invalid;
  a.bpf = w.bpf;
  a.run = w.run;
  a.block_counts = Carve::at<int>(b, w.o_counts);
  a.block_base = Carve::at<long long>(b, w.o_base);
  a.invalid_status = UWT_ERR_INVALID_ARG;
  a.capacity_status = UWT_ERR_CAPACITY;
  return a;
}

// The caller's slot list to d_slots through the pinned ring (the list may be a temporary: it is copied before this returns; the copy
// from page-locked memory is enqueued without a wait for what the stream holds).  The only wait is for the copy that read this block
// kPairStages calls ago.
int cloud_send_slots(uwt_ctx* c, int n_frames, const int32_t* slots, int* d_slots) {
  const size_t block = (size_t)c->p.max_frames;
  if (!c->h_cloud) {
    HIPCHK(c, hipHostMalloc((void**)&c->h_cloud, sizeof(int) * block * uwt_ctx::kPairStages));
    for (hipEvent_t& e : c->ev_cloud) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  const int stage = (c->cloud_stage + 1) % uwt_ctx::kPairStages;
  HIPCHK(c, hipEventSynchronize(c->ev_cloud[stage]));
  int* h = c->h_cloud + stage * block;
  std::memcpy(h, slots, sizeof(int) * (size_t)n_frames);
  c->cloud_stage = stage;
  HIPCHK(c, hipMemcpyAsync(d_slots, h, sizeof(int) * (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_cloud[stage], c->stream));
  return UWT_OK;
}

// two arrays of n poses (7 floats each) share a byte
bool ranges_overlap(const float* a, const float* b, int n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = sizeof(float) * 7 * (size_t)n;
  return n > 0 && x < y + len && y < x + len;
}

// The batch call, enqueued on the context stream (the arguments have passed cloud_batch_check; cloud_buf holds the work area w at its
// base).
int cloud_batch_enqueue(uwt_ctx* c, int n_frames, const int32_t* slots, const float* d_traj, const uwt_cloud_params& p, const CloudWork& w,
                        uwt_cloud_point* d_points, int64_t cap, uwt_cloud_info* d_info) {
  int st = compute_begin_pairs(c, n_frames, slots, slots);
  if (st) return st;
  const LevelK& L = c->lv[0];
  CloudArgs a = cloud_args(c, p, w, L.gw * L.gh);
  st = cloud_send_slots(c, n_frames, slots, const_cast<int*>(a.slots));
  if (st) return st;
  if (p.source == 1) {   // the producer of the batched semi-dense calls, level 0; its counts stay on the device
    st = candidates_level0_enqueue(c, n_frames, a.slots, p.threshold, &a.tab, &a.tab_stride, &a.tab_cnt);
    if (st) return st;
  }
  a.traj = d_traj;
  a.out = reinterpret_cast<float4*>(d_points);
  a.cap = cap;
  a.info = reinterpret_cast<CloudInfo*>(d_info);
  launch_cloud(c->stream, launch_sel(c), a, n_frames, p.source == 1 || p.skip_invalid != 0);
  HIPCHK(c, hipGetLastError());
  return compute_end(c, c->dep_first, c->dep_n);
}

}  // namespace

extern "C" {

int uwt_default_cloud_params(uwt_cloud_params* p) {
  if (!p) return UWT_ERR_INVALID_ARG;
  std::memset(p, 0, sizeof(*p));
  p->stride = 100;        // src/Visualizer.cpp:437
  p->threshold = 20.0;    // the GRADIENT_THRESHOLD the reference's candidate tables are made with
  return UWT_OK;
}

int uwt_point_cloud_batch_async(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const float* d_traj, const uwt_cloud_params* params,
                                uwt_cloud_point* d_points_out, int64_t cap, uwt_cloud_info* d_info_out) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (!d_traj || !d_info_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_point_cloud_batch_async: null argument");
  int st = cloud_batch_check(c, "uwt_point_cloud_batch_async", n_frames, slots, params, d_points_out, cap);
  if (st) return st;
  Carve cv(256, c->guard_bytes);
  const CloudWork w = cloud_work_layout(cv, c->lv[0].gw * c->lv[0].gh, params->stride, n_frames);
  st = c->cloud_buf.reserve(c, c->stream, cv);
  if (st) return st;
  return cloud_batch_enqueue(c, n_frames, slots, d_traj, *params, w, d_points_out, cap, d_info_out);
}

int uwt_point_cloud_batch(uwt_ctx* c, int32_t n_frames, const int32_t* slots, const float* traj, const uwt_cloud_params* params,
                          uwt_cloud_point* points_out, int64_t cap, uwt_cloud_info* info_out) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (!traj || !info_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_point_cloud_batch: null argument");
  int st = cloud_batch_check(c, "uwt_point_cloud_batch", n_frames, slots, params, points_out, cap);
  if (st) return st;
  const int rows = c->lv[0].gw * c->lv[0].gh;
  const int64_t room = std::min<int64_t>(cap, (int64_t)n_frames * ((rows - 1) / params->stride + 1));   // records the call can write at most
  Carve cv(256, c->guard_bytes);   // [the work area | poses | records | the cloud]
  const CloudWork w = cloud_work_layout(cv, rows, params->stride, n_frames);
  const size_t o_traj = cv.take<float>(7 * (size_t)n_frames), o_info = cv.take<uwt_cloud_info>((size_t)n_frames + 1),
               o_pts = cv.take<uwt_cloud_point>((size_t)room);
  st = c->cloud_buf.reserve(c, c->stream, cv);
  if (st) return st;
  void* b = c->cloud_buf.p;
  float* d_traj = Carve::at<float>(b, o_traj);
  uwt_cloud_info* d_info = Carve::at<uwt_cloud_info>(b, o_info);
  uwt_cloud_point* d_pts = Carve::at<uwt_cloud_point>(b, o_pts);
  HIPCHK(c, hipMemcpyAsync(d_traj, traj, sizeof(float) * 7 * (size_t)n_frames, hipMemcpyHostToDevice, c->stream));
  st = cloud_batch_enqueue(c, n_frames, slots, d_traj, *params, w, d_pts, room, d_info);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(info_out, d_info, sizeof(uwt_cloud_info) * ((size_t)n_frames + 1), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uwt_cloud_info& call = info_out[n_frames];
  if (call.written > 0) {
    HIPCHK(c, hipMemcpyAsync(points_out, d_pts, sizeof(uwt_cloud_point) * (size_t)call.written, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  for (int i = 0; i < n_frames; i++)
    if (info_out[i].status != UWT_OK)
      return fail(c, UWT_ERR_PAIR_FAILED, std::string("uwt_point_cloud_batch: at least one frame failed, first status: ") +
                                              uwt_status_string(info_out[i].status));
  if (call.status != UWT_OK) return fail(c, call.status, "uwt_point_cloud_batch: the cloud holds more points than cap");
  return UWT_OK;
}

int uwt_point_cloud_points(uwt_ctx* c, int32_t slot, const float* pts, int32_t n, const float traj_pose[7], const uwt_cloud_params* params,
                           uwt_cloud_point* points_out, int64_t cap, int64_t* count_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !traj_pose || !count_out || n < 0 || (n > 0 && !pts) || cap < 0 || (cap > 0 && !points_out) || !slot_range_ok(c, slot, 1))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_point_cloud_points: null argument, n < 0, cap < 0 or a slot out of range");
  if (n > kCloudMaxRows) return fail(c, UWT_ERR_CAPACITY, "uwt_point_cloud_points: more than 2^30 rows");
  int st = cloud_params_check(c, "uwt_point_cloud_points", params, false);
  if (st) return st;
  *count_out = 0;
  for (int k = 0; k < 7; k++)
    if (!std::isfinite(traj_pose[k])) return fail(c, UWT_ERR_INVALID_ARG, "uwt_point_cloud_points: the pose has a non-finite entry");
  if (n == 0) return UWT_OK;
  const int64_t room = std::min<int64_t>(cap, (n - 1) / params->stride + 1);   // records the call can write at most
  Carve cv(256, c->guard_bytes);   // [the work area | the pose | records | the table | the cloud]
  const CloudWork w = cloud_work_layout(cv, n, params->stride, 1);
  const size_t o_traj = cv.take<float>(7), o_info = cv.take<uwt_cloud_info>(2), o_tab = cv.take<float4>((size_t)n),
               o_pts = cv.take<uwt_cloud_point>((size_t)room);
  st = c->cloud_buf.reserve(c, c->stream, cv);
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  void* b = c->cloud_buf.p;
  CloudArgs a = cloud_args(c, *params, w, n);
  float* d_traj = Carve::at<float>(b, o_traj);
  uwt_cloud_info* d_info = Carve::at<uwt_cloud_info>(b, o_info);
  uwt_cloud_point* d_pts = Carve::at<uwt_cloud_point>(b, o_pts);
  const int h_slot = slot;
  HIPCHK(c, hipMemcpyAsync((void*)a.slots, &h_slot, sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_traj, traj_pose, sizeof(float) * 7, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(Carve::at<float4>(b, o_tab), pts, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  a.tab = Carve::at<float4>(b, o_tab);
  a.tab_stride = (size_t)n;
  a.traj = d_traj;
  a.out = reinterpret_cast<float4*>(d_pts);
  a.cap = room;
  a.info = reinterpret_cast<CloudInfo*>(d_info);
  launch_cloud(c->stream, launch_sel(c), a, 1, params->skip_invalid != 0);
  HIPCHK(c, hipGetLastError());
  uwt_cloud_info info[2];
  HIPCHK(c, hipMemcpyAsync(info, d_info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
  st = compute_end(c, slot, 1);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *count_out = info[1].offset;
  const int64_t k = std::min<int64_t>(info[1].offset, cap);
  if (k > 0) {
    HIPCHK(c, hipMemcpyAsync(points_out, d_pts, sizeof(uwt_cloud_point) * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (info[1].offset > cap) return fail(c, UWT_ERR_CAPACITY, "uwt_point_cloud_points: the cloud holds more points than cap");
  return UWT_OK;
}

int uwt_accumulate_trajectory_device_async(uwt_ctx* c, const float* d_poses, int32_t n, const float start_pose[7], float t_scale,
                                           int32_t reference_axes, float* d_traj_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !d_poses || !start_pose || !d_traj_out || n < 0) return fail(c, UWT_ERR_INVALID_ARG, "uwt_accumulate_trajectory_device_async");
  if (ranges_overlap(d_poses, d_traj_out, n))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_accumulate_trajectory_device_async: d_poses and d_traj_out overlap");
  if (n == 0) return UWT_OK;
  close_window(c);   // (device work on the context stream that passes through no helper)
  Pose P;
  for (int k = 0; k < 4; k++) P.q[k] = start_pose[k];
  for (int k = 0; k < 3; k++) P.t[k] = start_pose[4 + k];
  hipLaunchKernelGGL(k_trajectory, dim3(1), dim3(64), 0, c->stream, d_poses, n, P, t_scale, reference_axes, d_traj_out);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

int uwt_accumulate_trajectory_device_from_async(uwt_ctx* c, const float* d_poses, int32_t n, const float* d_start_pose, float t_scale,
                                                int32_t reference_axes, float* d_traj_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !d_poses || !d_start_pose || !d_traj_out || n < 0)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_accumulate_trajectory_device_from_async");
  // (the start pose is 7 floats: it may not lie inside the n output poses, nor the first output pose on it)
  const uintptr_t s0 = (uintptr_t)d_start_pose, o0 = (uintptr_t)d_traj_out, one = sizeof(float) * 7;
  if (ranges_overlap(d_poses, d_traj_out, n) || (n > 0 && s0 < o0 + one * (size_t)n && o0 < s0 + one))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_accumulate_trajectory_device_from_async: d_traj_out overlaps an input");
  if (n == 0) return UWT_OK;
  close_window(c);   // (device work on the context stream that passes through no helper)
  hipLaunchKernelGGL(k_trajectory_from, dim3(1), dim3(64), 0, c->stream, d_poses, n, d_start_pose, t_scale, reference_axes, d_traj_out);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

int uwt_predict_seeds_device_async(uwt_ctx* c, int32_t n, const float* d_prev, const float* d_cur, float* d_seed_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !d_prev || !d_cur || !d_seed_out || n < 0) return fail(c, UWT_ERR_INVALID_ARG, "uwt_predict_seeds_device_async");
  if (ranges_overlap(d_prev, d_seed_out, n) || ranges_overlap(d_cur, d_seed_out, n))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_predict_seeds_device_async: d_seed_out overlaps an input");
  if (n == 0) return UWT_OK;
  close_window(c);   // (device work on the context stream that passes through no helper)
  const int tb = 64;
  hipLaunchKernelGGL(k_predict_seeds, dim3((n + tb - 1) / tb), dim3(tb), 0, c->stream, d_prev, d_cur, n, d_seed_out);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

int uwt_predict_seeds(uwt_ctx* c, int32_t n, const float* prev, const float* cur, float* seed_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !prev || !cur || !seed_out || n < 0) return fail(c, UWT_ERR_INVALID_ARG, "uwt_predict_seeds");
  if (n == 0) return UWT_OK;
  // scratch: [prev | cur | seeds]
  Carve cv(256, c->guard_bytes);
  const size_t rows = 7 * (size_t)n, o_prev = cv.take<float>(rows), o_cur = cv.take<float>(rows), o_out = cv.take<float>(rows);
  int st = c->scratch.reserve(c, c->stream, cv);
  if (st) return st;
  float* d_prev = Carve::at<float>(c->scratch.p, o_prev);
  float* d_cur = Carve::at<float>(c->scratch.p, o_cur);
  float* d_out = Carve::at<float>(c->scratch.p, o_out);
  HIPCHK(c, hipMemcpyAsync(d_prev, prev, sizeof(float) * rows, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_cur, cur, sizeof(float) * rows, hipMemcpyHostToDevice, c->stream));
  st = uwt_predict_seeds_device_async(c, n, d_prev, d_cur, d_out);
  if (st) return st;
  HIPCHK(c, hipMemcpyAsync(seed_out, d_out, sizeof(float) * rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

}  // extern "C"
