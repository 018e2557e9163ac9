// uwt_capi_stages.hip — host side of libuwt_hip.so: the per-stage entry points (one stage of the reference per call, synchronous,
// over the context's scratch buffer).
#include "uwt_ctx.h"

namespace {

// cv::resize(src, dst, Size(), 0.5, 0.5) of one host image of any size through pitched scratch planes (rows padded to whole
// groups of four, as the context's level planes are); dst is dw x dh = cvRound halves (even_only: exact halves, or an error)
template <typename T>
int resize_half_host(uwt_ctx* c, const char* what, bool even_only, const T* src, int sw, int sh, T* dst) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  const int dw = uwt_half_size(sw), dh = uwt_half_size(sh);
  if (!c || !src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || (even_only && ((sw | sh) & 1))) return fail(c, UWT_ERR_INVALID_ARG, what);
  const size_t sp = ((size_t)sw + 3) & ~(size_t)3, dp = ((size_t)dw + 3) & ~(size_t)3, es = sizeof(T);
  Carve cv(256, c->guard_bytes);   // [source plane | result plane]
  cv.take<T>(sp * sh);
  const size_t off = cv.take<T>(dp * dh);
  int st = c->scratch.reserve(c, c->stream, cv, cv.tight() + 64);
  if (st) return st;
  unsigned char* d = (unsigned char*)c->scratch.p;
  HIPCHK(c, hipMemcpy2DAsync(d, sp * es, src, (size_t)sw * es, (size_t)sw * es, sh, hipMemcpyHostToDevice, c->stream));
  st = launch_resize<T>(c, (const T*)d, (T*)(d + off), sw, sh, (int)sp, dw, dh, (int)dp, sp * sh, dp * dh, 1);
  if (st) return st;
  HIPCHK(c, hipMemcpy2DAsync(dst, (size_t)dw * es, d + off, dp * es, (size_t)dw * es, dh, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int run_se3_op(uwt_ctx* c, int op, const float* a, int na, const float* b, int nb, float* out, int nout, int* flag) {
  if (!c) return UWT_ERR_INVALID_ARG;
  Carve cv(256, c->guard_bytes);   // floats [0,64) a, [64,128) b, [128,256) out, [256] flag
  const size_t o_a = cv.take<float>(64), o_b = cv.take<float>(64), o_out = cv.take<float>(128), o_flag = cv.take<int>(1);
  int st = c->scratch.reserve(c, c->stream, cv, std::max<size_t>(4096, cv.total()));   // (a page: the carving needs less without guards)
  if (st) return st;
  float *da = Carve::at<float>(c->scratch.p, o_a), *db = Carve::at<float>(c->scratch.p, o_b), *dout = Carve::at<float>(c->scratch.p, o_out);
  int* dflag = Carve::at<int>(c->scratch.p, o_flag);
  HIPCHK(c, hipMemcpyAsync(da, a, sizeof(float) * na, hipMemcpyHostToDevice, c->stream));
  if (b) HIPCHK(c, hipMemcpyAsync(db, b, sizeof(float) * nb, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_se3_ops, dim3(1), dim3(1), 0, c->stream, op, da, db, dout, dflag);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, dout, sizeof(float) * nout, hipMemcpyDeviceToHost, c->stream));
  int f = 1;
  HIPCHK(c, hipMemcpyAsync(&f, dflag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (flag) *flag = f;
  return UWT_OK;
}

}  // namespace

extern "C" {

/* ---- per-stage entry points ---------------------------------------------------------------------------------- */

int uwt_half_size(int32_t n) { return (int)std::lrint((double)n * 0.5); }   // cvRound(n * 0.5): half to even

int uwt_halve_u8(uwt_ctx* c, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst) { return resize_half_host(c, "uwt_halve_u8", true, src, w, h, dst); }
int uwt_halve_u16(uwt_ctx* c, const uint16_t* src, int32_t w, int32_t h, uint16_t* dst) { return resize_half_host(c, "uwt_halve_u16", true, src, w, h, dst); }
int uwt_resize_half_u8(uwt_ctx* c, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst) { return resize_half_host(c, "uwt_resize_half_u8", false, src, w, h, dst); }
int uwt_resize_half_u16(uwt_ctx* c, const uint16_t* src, int32_t w, int32_t h, uint16_t* dst) { return resize_half_host(c, "uwt_resize_half_u16", false, src, w, h, dst); }

int uwt_scharr3(uwt_ctx* c, const uint8_t* src, int32_t w, int32_t h, int16_t* gx, int16_t* gy) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !src || !gx || !gy || w < 1 || h < 1) return fail(c, UWT_ERR_INVALID_ARG, "uwt_scharr3");
  const size_t pitch = ((size_t)w + 3) & ~(size_t)3;   // rows padded to whole groups of four, as the context's level planes are
  const size_t n = pitch * h;
  Carve cv(256, c->guard_bytes);   // [image | gx, gy]
  cv.take<uint8_t>(n);
  const size_t off = cv.take<int16_t>(2 * n);
  int st = c->scratch.reserve(c, c->stream, cv, cv.tight());
  if (st) return st;
  uint8_t* d = (uint8_t*)c->scratch.p;
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
  int st = c->scratch.reserve(c, c->stream, bytes * 2);
  if (st) return st;
  float4* din = (float4*)c->scratch.p;
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
    st = c->scratch.reserve(c, c->stream, n * (6 * 4 + 4 + 4 + 1) + 512);
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
    a.dumpJ = (float*)c->scratch.p;
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
  int st = c->scratch.reserve(c, c->stream, fl * 4);
  if (st) return st;
  float* dJ = (float*)c->scratch.p;
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

static_assert(sizeof(uwt_pair_state) == sizeof(PairState) && offsetof(uwt_pair_state, last_error) == offsetof(PairState, last_error) &&
              offsetof(uwt_pair_state, n_valid) == offsetof(PairState, n_valid), "uwt_pair_state layout");

// Test surface: one update of pairs [pair_base, pair_base + n_pairs) from the caller's records, by k_gn_update (form 0) or by the tail
// form under k_tail_fold_stage (form 1).  Every device array is indexed by the absolute pair, like an alignment's.
int uwt_gn_update_records(uwt_ctx* c, int32_t form, int32_t n_pairs, int32_t pair_base, int32_t stride, int32_t count,
                          const uint32_t* records, const uwt_pair_state* states_in, int32_t k, int32_t max_iters, int32_t early_exit,
                          float epsilon, float gain, int32_t general, uwt_pair_state* states_out, int32_t* active_out,
                          uint32_t* tickets_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  constexpr int kMaxRows = 1024, kMaxStride = 256;
  if (!c || !records || !states_in || !states_out || !active_out || (form != 0 && form != 1) || n_pairs < 1 || pair_base < 0 ||
      pair_base > kMaxRows || n_pairs > kMaxRows - pair_base || count < 1 || count > kMaxSlices || stride < count || stride > kMaxStride ||
      (form == 0 && stride != count))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_gn_update_records: a null array, form not 0 / 1, pairs outside 1..1024 rows, count outside 1..160, "
                                        "stride < count or > 256, or form 0 with stride != count");
  const size_t rows = (size_t)pair_base + n_pairs;
  Carve cv(256, c->guard_bytes);   // [records | states | active | tickets]
  const size_t o_rec = cv.take<uint32_t>(rows * stride * kRecWords), o_st = cv.take<PairState>(rows), o_act = cv.take<int>(1),
               o_tk = cv.take<unsigned int>(rows);
  int st = c->scratch.reserve(c, c->stream, cv);
  if (st) return st;
  uint32_t* d_rec = Carve::at<uint32_t>(c->scratch.p, o_rec);
  PairState* d_st = Carve::at<PairState>(c->scratch.p, o_st);
  int* d_act = Carve::at<int>(c->scratch.p, o_act);
  unsigned int* d_tk = Carve::at<unsigned int>(c->scratch.p, o_tk);
  HIPCHK(c, hipMemcpyAsync(d_rec, records, sizeof(uint32_t) * rows * stride * kRecWords, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_st, states_in, sizeof(PairState) * rows, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_act, 0, sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(d_tk, 0, sizeof(unsigned int) * rows, c->stream));
  const UpdateRule rule = {max_iters, early_exit, epsilon, gain, general ? 1 : 0, c->p.arith == UWT_ARITH_LEGACY ? 1 : 0};
  if (form == 0) {
    UpdateArgs u{};
    u.partials = d_rec;
    u.state = d_st;
    u.slices = count;
    u.k = k;
    u.rule = rule;
    u.pair_base = pair_base;
    u.active = d_act;
    hipLaunchKernelGGL(k_gn_update, dim3(n_pairs), dim3(kUpdateBlock), 0, c->stream, u);
  } else {
    ResidualArgs a{};
    a.partials = d_rec;
    a.pair_base = pair_base;
    a.slices = stride;
    a.tail.tickets = d_tk;
    a.tail.state = d_st;
    a.tail.active = d_act;
    a.tail.on = 1;
    a.tail.k = k;
    a.tail.rule = rule;
    hipLaunchKernelGGL(k_tail_fold_stage, dim3(count, n_pairs), dim3(64), 0, c->stream, a, (int)stride, (int)count);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(states_out, d_st, sizeof(PairState) * rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(active_out, d_act, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (tickets_out) HIPCHK(c, hipMemcpyAsync(tickets_out, d_tk, sizeof(unsigned int) * rows, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return UWT_OK;
}

int uwt_robust_weights(uwt_ctx* c, const float* residuals, int32_t n, int32_t kind, float* weights_out, float* median_out,
                       float* mad_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !residuals || n < 1 || (kind != kWeightsIdentity && kind != kWeightsTukeyRef))
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_robust_weights: null residuals, n < 1, or a kind other than identity / Tukey");
  const size_t bytes = sizeof(float) * (size_t)n;
  int st = c->scratch.reserve(c, c->stream, 2 * bytes + 64);
  if (st) return st;
  float* d_r = (float*)c->scratch.p;
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

int uwt_add_patch_points(uwt_ctx* c, int32_t lvl, const float* pts, int32_t n_pts, int32_t patch_size, float* pts_out,
                         int32_t cap, int32_t* count_out) {
  if (c) (void)hipSetDevice(c->p.device);
  if (!c || !count_out || lvl < 0 || lvl >= c->p.n_levels || n_pts < 0 || (n_pts > 0 && !pts) || cap < 0 || (cap > 0 && !pts_out) ||
      patch_size < 1)
    return fail(c, UWT_ERR_INVALID_ARG, "uwt_add_patch_points");
  const int start = (patch_size - 1) / 2;   // src/Tracker.cpp:602
  const size_t in_bytes = (size_t)n_pts * 16, out_bytes = (size_t)cap * 16;
  int st = c->scratch.reserve(c, c->stream, 4096 + in_bytes + out_bytes + 64);
  if (st) return st;
  int* d_cnt = (int*)c->scratch.p;
  float4* d_in = (float4*)((uint8_t*)c->scratch.p + 4096);
  float4* d_out = (float4*)((uint8_t*)c->scratch.p + 4096 + in_bytes);
  if (n_pts) HIPCHK(c, hipMemcpyAsync(d_in, pts, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_add_patch_points, dim3(1), dim3(256), 0, c->stream, d_in, n_pts, c->lv[lvl].gw, c->lv[lvl].gh, start, d_out, cap,
                     d_cnt);
  HIPCHK(c, hipGetLastError());
  return counted_rows_to_host(c, d_out, 0, d_cnt, 1, cap, pts_out, count_out);
}

static int accumulate_trajectory_impl(uwt_ctx* c, bool scan, const float* poses, int32_t n, const float start_pose[7], float t_scale,
                              int32_t reference_axes, float* traj_out) {
  if (c) (void)hipSetDevice(c->p.device);  // one context = one device; callers may have switched the thread's device
  if (!c || !poses || !start_pose || !traj_out || n < 0) return fail(c, UWT_ERR_INVALID_ARG, "uwt_accumulate_trajectory");
  if (n == 0) return UWT_OK;
  const size_t bytes = sizeof(float) * 7 * (size_t)n;
  int st = c->scratch.reserve(c, c->stream, 2 * bytes);
  if (st) return st;
  float* din = (float*)c->scratch.p;
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
