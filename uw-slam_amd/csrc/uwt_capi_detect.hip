// uwt_capi_detect.hip — host side of libuwt_hip.so: the driver SURF and ORB detection and description share (uwt_detect.h).
#include "uwt_ctx.h"
#include "uwt_detect.h"

static_assert(sizeof(Keypoint) == sizeof(uwt_keypoint) && sizeof(uwt_keypoint) == 32, "uwt_keypoint layout");

namespace uwt {

void detect_image(const uwt_ctx* c, DetectArgs* a) {
  const LevelK& L = c->lv[0];
  a->img = c->img[0];
  a->frame_stride = (size_t)L.n;
  a->pitch = L.pitch;
  a->w = c->p.width;
  a->h = c->p.height;
}

int detect_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap) {
  if (n_frames < 1 || cap < 1 || !slots) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": n_frames < 1, cap < 1 or a null list");
  if (cap > UWT_MATCH_MAX_ROWS) return fail(c, UWT_ERR_CAPACITY, std::string(what) + ": cap above UWT_MATCH_MAX_ROWS");
  for (int f = 0; f < n_frames; f++)
    if (!slot_range_ok(c, slots[f], 1)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": slot out of range");
  return UWT_OK;
}

int detect_run(uwt_ctx* c, const Detector& d, int n_frames, const int32_t* slots, int cap, const uwt_keypoint* kp_in, const int32_t* n_in,
               bool want_desc, const Deliver& deliver) {
  int st = compute_begin_pairs(c, n_frames, slots, slots);
  if (st) return st;
  const int chunk = chunk_frames(d.frame_bytes, n_frames);
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int nf = std::min(chunk, n_frames - f0);
    st = d.begin(slots + f0, nf, 0, nullptr);
    if (st) return st;
    DetectArgs* a = d.chunk;
    int rows = d.rows;
    if (kp_in) {
      rows = provided_rows(n_in + f0, nf);
      HIPCHK(c, hipMemcpyAsync(a->counts, n_in + f0, sizeof(int) * (size_t)nf, hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(a->kp, kp_in + (size_t)f0 * cap, sizeof(Keypoint) * (size_t)cap * nf, hipMemcpyHostToDevice, c->stream));
    } else {
      st = d.detect(f0);
      if (st) return st;
    }
    if (!want_desc) a->desc = nullptr;
    d.describe(rows);
    HIPCHK(c, hipGetLastError());
    st = deliver(f0, *a);
    if (st) return st;
  }
  return UWT_OK;
}

// Grid (blocks, n_frames): the rows below frame f's count (confined to 0..cap) of a fixed-stride table of `words` 32-bit words a row,
// from the chunk's scratch to the caller's table.  The rows past the count are neither read nor written.
static __global__ __launch_bounds__(256) void k_deliver_rows(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                             const int* __restrict__ counts, int cap, int words) {
  const int f = blockIdx.y;
  const size_t n = (size_t)min(max(counts[f], 0), cap) * words, base = (size_t)f * cap * words;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[base + i] = src[base + i];
}

int deliver_device(uwt_ctx* c, int f0, const DetectArgs& a, uwt_keypoint* d_kp, void* d_desc, int32_t* d_counts) {
  const size_t g0 = (size_t)f0 * a.cap;
  HIPCHK(c, hipMemcpyAsync(d_counts + f0, a.counts, sizeof(int) * (size_t)a.n_frames, hipMemcpyDeviceToDevice, c->stream));
  auto rows = [&](const void* src, void* dst, int words) {
    const int blocks = (int)std::min<size_t>(((size_t)a.cap * words + 255) / 256, 64);
    hipLaunchKernelGGL(k_deliver_rows, dim3(blocks, a.n_frames), dim3(256), 0, c->stream, (const uint32_t*)src, (uint32_t*)dst, a.counts,
                       a.cap, words);
  };
  rows(a.kp, d_kp + g0, (int)(sizeof(Keypoint) / 4));
  if (a.desc) rows(a.desc, (unsigned char*)d_desc + g0 * a.desc_row, a.desc_row / 4);
  HIPCHK(c, hipGetLastError());
  return UWT_OK;
}

int deliver_host(uwt_ctx* c, int f0, const DetectArgs& a, uwt_keypoint* kp_out, void* desc_out, int32_t* counts_out) {
  std::vector<int32_t> cnt((size_t)a.n_frames);
  HIPCHK(c, hipMemcpyAsync(cnt.data(), a.counts, sizeof(int) * (size_t)a.n_frames, hipMemcpyDeviceToHost, c->stream));
  const size_t g0 = (size_t)f0 * a.cap;
  int st = rows_to_host(c, a.cap, a.n_frames,
                        {{a.kp, sizeof(Keypoint), cnt.data(), kp_out + g0},
                         {a.desc, (size_t)a.desc_row, cnt.data(), a.desc ? (unsigned char*)desc_out + g0 * a.desc_row : nullptr}});
  if (!st && counts_out)
    for (int f = 0; f < a.n_frames; f++) counts_out[f0 + f] = std::min(std::max(cnt[(size_t)f], 0), a.cap);
  return st;
}

int detect_entry(uwt_ctx* c, const char* what, Detector& d, DetectForm form, int n_frames, const int32_t* slots, int cap,
                 const uwt_keypoint* kp_in, const int32_t* n_in, uwt_keypoint* kp_out, void* desc_out, int32_t* counts_out) {
  if (c) (void)hipSetDevice(c->p.device);
  const bool given = form == DetectForm::given, device = form == DetectForm::device;
  if (!c || !kp_out || (given ? !kp_in || !n_in || !desc_out : !counts_out)) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": null argument");
  int st = detect_check(c, what, n_frames, slots, cap);
  if (!st) st = d.prepare(what, !given);
  if (st) return st;
  for (int f = 0; given && f < n_frames; f++) {
    if (n_in[f] < 0 || n_in[f] > cap) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + ": key-point count outside 0..cap");
    const uwt_keypoint* k = kp_in + (size_t)f * cap;
    for (int i = 0; i < n_in[f]; i++)
      if (!d.kp_ok(k[i])) return fail(c, UWT_ERR_INVALID_ARG, std::string(what) + d.kp_msg);
  }
  // (given lists: the device keeps every row of a chunk; only the rows below a frame's count come back)
  st = detect_run(c, d, n_frames, slots, cap, kp_in, n_in, desc_out != nullptr, [&](int f0, const DetectArgs& a) {
    return device ? deliver_device(c, f0, a, kp_out, desc_out, counts_out) : deliver_host(c, f0, a, kp_out, desc_out, counts_out);
  });
  return st || !device ? st : compute_end(c, c->dep_first, c->dep_n);
}

int stage_begin(uwt_ctx* c, const char* what, Detector& d, int32_t slot, bool detect, size_t extra, unsigned char** x) {
  int st = detect_check(c, what, 1, &slot, 1);
  if (!st) st = d.prepare(what, detect);
  if (!st) st = compute_begin(c, slot, 1);
  return st ? st : d.begin(&slot, 1, extra, x);
}

}  // namespace uwt
