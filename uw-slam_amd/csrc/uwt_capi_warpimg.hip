// uwt_capi_warpimg.hip — host side of libuwt_hip.so: Tracker::ObtainImageTransformed for one frame's explicit table and, in its dense
// form, for a batch of pairs with poses in device memory; and the image of Tracker::DebugShowWarpedPerspective.  include/uwt.h states
// the contract, uwt_warpimg_kernels.h the two passes over the winner plane.
#include "uwt_ctx.h"
#include "uwt_warpimg.h"

namespace {

static_assert(sizeof(uwt_warp_quality) == 48 && sizeof(WarpQuality) == sizeof(uwt_warp_quality), "uwt_warp_quality layout");
static_assert(offsetof(uwt_warp_quality, sum_abs) == 16 && offsetof(uwt_warp_quality, reserved) == 40, "uwt_warp_quality layout");

WarpImageArgs warp_args(uwt_ctx* c, int lvl) {
  WarpImageArgs a;
  std::memset(&a, 0, sizeof(a));
  a.L = c->lv[lvl];
  a.img = c->img[lvl];
  a.invalid_status = UWT_ERR_INVALID_ARG;
  return a;
}

// Every check of the dense batch call the host can make; nothing is enqueued and no buffer grows when one fails.
int warp_batch_check(uwt_ctx* c, const char* what, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int lvl) {
  if (!ref_slots || !tgt_slots) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null list");
  if (n_pairs < 1 || n_pairs > c->p.max_pairs) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_pairs outside 1..max_pairs");
  if (lvl < 0 || lvl >= c->p.n_levels) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": level out of range");
  for (int i = 0; i < n_pairs; i++)
    if (!slot_range_ok(c, ref_slots[i], 1) || !slot_range_ok(c, tgt_slots[i], 1))
      return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": pair slot out of range");
  return UWT_OK;
}

// The dense batch, enqueued on the context stream (the arguments have passed warp_batch_check; warp_buf holds the winner planes at its
// base).
int warp_batch_enqueue(uwt_ctx* c, int n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int lvl, const float* d_poses,
                       const uwt_warp_image_io& io) {
  int st = compute_begin_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  st = upload_pairs(c, n_pairs, ref_slots, tgt_slots);
  if (st) return st;
  WarpImageArgs a = warp_args(c, lvl);
  a.depth = c->p.has_depth ? c->depth[lvl] : nullptr;
  a.ref_slots = c->d_ref;
  a.tgt_slots = c->d_tgt;
  a.poses = d_poses;
  a.n = a.L.gw * a.L.gh;
  a.winner = (int*)c->warp_buf.p;
  a.warped = io.d_warped;
  a.valid = io.d_valid;
  a.absdiff = io.d_absdiff;
  a.quality = reinterpret_cast<WarpQuality*>(io.d_quality);
  HIPCHK(c, hipMemsetAsync(a.winner, 0xFF, sizeof(int) * (size_t)a.L.n * n_pairs, c->stream));
  HIPCHK(c, hipMemsetAsync(io.d_quality, 0, sizeof(uwt_warp_quality) * (size_t)n_pairs, c->stream));
  launch_warp_image(c->stream, launch_sel(c), a, n_pairs);
  HIPCHK(c, hipGetLastError());
  return compute_end(c, c->dep_first, c->dep_n);
}

}  // namespace

extern "C" {

int uwt_obtain_image_transformed(uwt_ctx* c, int32_t slot, int32_t lvl, const float* pts, const float* warped, int32_t n,
                                 uint8_t* image_inout, uint8_t* valid_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !image_inout || !valid_out || n < 0 || (n > 0 && (!pts || !warped)) || lvl < 0 || lvl >= c->p.n_levels ||
      !slot_range_ok(c, slot, 1))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_obtain_image_transformed: null argument, n < 0, or a slot or level out of range");
  const LevelK& L = c->lv[lvl];
  Carve cv(256, c->guard_bytes);   // [winner | image | valid | the slot | table | warped rows]
  const size_t o_win = cv.take<int>(L.n), o_img = cv.take<uint8_t>(L.n), o_val = cv.take<uint8_t>(L.n), o_slot = cv.take<int>(1),
               o_pts = cv.take<float4>(n), o_wp = cv.take<float4>(n);
  int st = c->warp_buf.reserve(c, c->stream, cv);
  if (st) return st;
  st = compute_begin(c, slot, 1);
  if (st) return st;
  void* b = c->warp_buf.p;
  WarpImageArgs a = warp_args(c, lvl);
  a.winner = Carve::at<int>(b, o_win);
  a.warped = Carve::at<uint8_t>(b, o_img);
  a.valid = Carve::at<uint8_t>(b, o_val);
  a.ref_slots = Carve::at<int>(b, o_slot);
  a.pts = Carve::at<float4>(b, o_pts);
  a.warped_pts = Carve::at<float4>(b, o_wp);
  a.n = n;
  a.keep = 1;
  const int h_slot = slot;
  HIPCHK(c, hipMemsetAsync(a.winner, 0xFF, sizeof(int) * (size_t)L.n, c->stream));
  HIPCHK(c, hipMemsetAsync(a.warped, 0, L.n, c->stream));   // (the pad columns of the pitched rows)
  HIPCHK(c, hipMemcpy2DAsync(a.warped, L.pitch, image_inout, L.iw, L.iw, L.ih, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync((void*)a.ref_slots, &h_slot, sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (n) {
    HIPCHK(c, hipMemcpyAsync((void*)a.pts, pts, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((void*)a.warped_pts, warped, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  }
  launch_warp_image(c->stream, launch_sel(c), a, 1);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpy2DAsync(image_inout, L.iw, a.warped, L.pitch, L.iw, L.ih, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(valid_out, L.iw, a.valid, L.pitch, L.iw, L.ih, hipMemcpyDeviceToHost, c->stream));
  st = compute_end(c, slot, 1);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_warp_image_batch_async(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int32_t lvl,
                               const float* d_poses, const uwt_warp_image_io* io) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (!d_poses || !io || !io->d_quality) return fail(c, UWT_ERR_INVALID_ARG, "uwt_warp_image_batch_async: null argument");
  int st = warp_batch_check(c, "uwt_warp_image_batch_async", n_pairs, ref_slots, tgt_slots, lvl);
  if (st) return st;
  st = c->warp_buf.reserve(c, c->stream, sizeof(int) * (size_t)c->lv[lvl].n * n_pairs);
  if (st) return st;
  return warp_batch_enqueue(c, n_pairs, ref_slots, tgt_slots, lvl, d_poses, *io);
}

int uwt_warp_image_batch(uwt_ctx* c, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int32_t lvl,
                         const float* poses, uint8_t* warped_out, uint8_t* valid_out, uint8_t* absdiff_out,
                         uwt_warp_quality* quality_out) {
  if (!c) return UWT_ERR_INVALID_ARG;
  (void)hipSetDevice(c->p.device);
  if (!poses || !quality_out) return fail(c, UWT_ERR_INVALID_ARG, "uwt_warp_image_batch: null argument");
  int st = warp_batch_check(c, "uwt_warp_image_batch", n_pairs, ref_slots, tgt_slots, lvl);
  if (st) return st;
  const LevelK& L = c->lv[lvl];
  const size_t planes = (size_t)L.n * n_pairs;
  Carve cv(256, c->guard_bytes);   // [winner planes | poses | records | warped | valid | absdiff]
  cv.take<int>(planes);
  const size_t o_pose = cv.take<float>(7 * (size_t)n_pairs), o_q = cv.take<uwt_warp_quality>(n_pairs),
               o_w = cv.take<uint8_t>(warped_out ? planes : 0), o_v = cv.take<uint8_t>(valid_out ? planes : 0),
               o_d = cv.take<uint8_t>(absdiff_out ? planes : 0);
  st = c->warp_buf.reserve(c, c->stream, cv);
  if (st) return st;
  void* b = c->warp_buf.p;
  uwt_warp_image_io io;
  io.d_warped = warped_out ? Carve::at<uint8_t>(b, o_w) : nullptr;
  io.d_valid = valid_out ? Carve::at<uint8_t>(b, o_v) : nullptr;
  io.d_absdiff = absdiff_out ? Carve::at<uint8_t>(b, o_d) : nullptr;
  io.d_quality = Carve::at<uwt_warp_quality>(b, o_q);
  float* d_poses = Carve::at<float>(b, o_pose);
  HIPCHK(c, hipMemcpyAsync(d_poses, poses, sizeof(float) * 7 * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
  st = warp_batch_enqueue(c, n_pairs, ref_slots, tgt_slots, lvl, d_poses, io);
  if (st) return st;
  const size_t rows = (size_t)L.ih * n_pairs;   // a pair's rows follow the previous pair's: one strided copy per output
  for (auto pr : {std::make_pair(warped_out, io.d_warped), std::make_pair(valid_out, io.d_valid), std::make_pair(absdiff_out, io.d_absdiff)})
    if (pr.first) HIPCHK(c, hipMemcpy2DAsync(pr.first, L.iw, pr.second, L.pitch, L.iw, rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(quality_out, io.d_quality, sizeof(uwt_warp_quality) * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n_pairs; i++)
    if (quality_out[i].status != UWT_OK)
      return fail(c, UWT_ERR_PAIR_FAILED, std::string("uwt_warp_image_batch: at least one pair failed, first status: ") +
                                              uwt_status_string(quality_out[i].status));
  return UWT_OK;
}

int uwt_warp_mosaic(uwt_ctx* c, int32_t ref_slot, int32_t tgt_slot, int32_t lvl, const uint8_t* warped, uint8_t* mosaic_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !warped || !mosaic_out || lvl < 0 || lvl >= c->p.n_levels || !slot_range_ok(c, ref_slot, 1) ||
      !slot_range_ok(c, tgt_slot, 1))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_warp_mosaic: null argument, or a slot or level out of range");
  const LevelK& L = c->lv[lvl];
  Carve cv(256, c->guard_bytes);   // [warped | mosaic]
  const size_t o_w = cv.take<uint8_t>(L.n), o_m = cv.take<uint8_t>(4 * (size_t)L.iw * L.ih);
  int st = c->warp_buf.reserve(c, c->stream, cv);
  if (st) return st;
  st = compute_begin_pairs(c, 1, &ref_slot, &tgt_slot);
  if (st) return st;
  uint8_t* d_w = Carve::at<uint8_t>(c->warp_buf.p, o_w);
  uint8_t* d_m = Carve::at<uint8_t>(c->warp_buf.p, o_m);
  HIPCHK(c, hipMemcpy2DAsync(d_w, L.pitch, warped, L.iw, L.iw, L.ih, hipMemcpyHostToDevice, c->stream));
  launch_warp_mosaic(c->stream, L, c->img[lvl] + (size_t)ref_slot * L.n, c->img[lvl] + (size_t)tgt_slot * L.n, d_w, d_m);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(mosaic_out, d_m, 4 * (size_t)L.iw * L.ih, hipMemcpyDeviceToHost, c->stream));
  st = compute_end(c, c->dep_first, c->dep_n);
  if (st) return st;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

}  // extern "C"
