// uwt_orb_kernels.h — the kernels of ORB detection and description.  include/uwt.h states the contract; every f32 / f64 step here
// is the one operation the contract names (the unit is built with -ffp-contract=off), integers are exact.
//   k_orb_layers     layers 1 .. n - 1 of every frame from its level-0 plane: a thread per destination pixel
//   k_orb_fast       one layer: a 32 x 32 tile of the candidate band; its pixels with a four-pixel halo and its scores with a
//                    one-pixel halo in LDS; suppression from LDS; the survivors' Harris measures from the same pixels; each is
//                    appended to its layer's raw list
//   k_orb_rank       one block per (layer, frame): a candidate's rank by (H descending, y, x) is its place among the quota
//   k_orb_select     one block per frame: the cap strongest when the frame overflows, then each survivor's place by (layer, y, x)
//                    — the output is a function of the SET of candidates alone
//   k_orb_describe   one wave per key point: the patch moments over the lanes, then 64 tests per pass balloted into a word
//   k_orb_harris     the per-stage entry: a thread per given pixel
//   k_orb_take_provided  the tracking call: the modes of a chunk's frames, and the provided records where detection would have put its own
#pragma once

#include "uwt_orb.h"
#include "uwt_select.h"

namespace uwt {

// UWT_ORB_UMAX of include/uwt.h
__constant__ unsigned char kOrbUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

__device__ __forceinline__ int orb_rnd(float v) { return (int)floorf(v + 0.5f); }

// layer l of frame f: its first pixel and the bytes of a row
__device__ __forceinline__ const uint8_t* orb_layer_ptr(const OrbArgs& a, int f, int l, int* pitch) {
  if (l == 0) {
    *pitch = a.pitch;
    return a.img + (size_t)a.slots[f] * a.frame_stride;
  }
  *pitch = a.lw[l];
  return a.layers + (size_t)f * a.layer_stride + a.loff[l];
}

// ---- the scale pyramid -----------------------------------------------------------------------------------------------------------
// grid (ceil(lw[1] lh[1] / 256), n_levels - 1, n_frames): layer blockIdx.y + 1.  Sizes are at most kOrbMaxDim: (2 x + 1) w < 2^30.
__global__ __launch_bounds__(kOrbBlock) void k_orb_layers(OrbArgs a) {
  const int l = blockIdx.y + 1, f = blockIdx.z;
  const int lw = a.lw[l], lh = a.lh[l];
  const int i = blockIdx.x * kOrbBlock + threadIdx.x;
  if (i >= lw * lh) return;
  const int y = i / lw, x = i - y * lw;
  const unsigned nx = (unsigned)(2 * x + 1) * (unsigned)a.w - (unsigned)lw, ny = (unsigned)(2 * y + 1) * (unsigned)a.h - (unsigned)lh;
  const unsigned dx = 2u * (unsigned)lw, dy = 2u * (unsigned)lh;
  const int x0 = (int)(nx / dx), y0 = (int)(ny / dy);
  const unsigned fx = ((nx % dx) * 2048u) / dx, fy = ((ny % dy) * 2048u) / dy;
  const int x1 = min(x0 + 1, a.w - 1), y1 = min(y0 + 1, a.h - 1);
  const uint8_t* src = a.img + (size_t)a.slots[f] * a.frame_stride;
  const unsigned i00 = src[(size_t)y0 * a.pitch + x0], i01 = src[(size_t)y0 * a.pitch + x1];
  const unsigned i10 = src[(size_t)y1 * a.pitch + x0], i11 = src[(size_t)y1 * a.pitch + x1];
  const unsigned s = i00 * (2048u - fx) * (2048u - fy) + i01 * fx * (2048u - fy) + i10 * (2048u - fx) * fy + i11 * fx * fy + (1u << 21);
  a.layers[(size_t)f * a.layer_stride + a.loff[l] + (size_t)i] = (uint8_t)(s >> 22);
}

// ---- FAST score and Harris measure -------------------------------------------------------------------------------------------------
// the score of the pixel at p (rows of `pitch` bytes): 0 unless above thr.  No early-out: every lane does the same work.
__device__ __forceinline__ int orb_fast_score(const uint8_t* p, int pitch, int thr) {
  const int c = (int)p[0];
  int d[16];
  d[0] = (int)p[-3 * pitch] - c;
  d[1] = (int)p[-3 * pitch + 1] - c;
  d[2] = (int)p[-2 * pitch + 2] - c;
  d[3] = (int)p[-pitch + 3] - c;
  d[4] = (int)p[3] - c;
  d[5] = (int)p[pitch + 3] - c;
  d[6] = (int)p[2 * pitch + 2] - c;
  d[7] = (int)p[3 * pitch + 1] - c;
  d[8] = (int)p[3 * pitch] - c;
  d[9] = (int)p[3 * pitch - 1] - c;
  d[10] = (int)p[2 * pitch - 2] - c;
  d[11] = (int)p[pitch - 3] - c;
  d[12] = (int)p[-3] - c;
  d[13] = (int)p[-pitch - 3] - c;
  d[14] = (int)p[-2 * pitch - 2] - c;
  d[15] = (int)p[-3 * pitch - 1] - c;
  // windows of 2, 4, 8, then 9 ring pixels from i on: the minimum (bright arcs) and the maximum (dark arcs: min(-d) = -max(d))
  int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    lo2[i] = min(d[i], d[(i + 1) & 15]);
    hi2[i] = max(d[i], d[(i + 1) & 15]);
  }
#pragma unroll
  for (int i = 0; i < 16; i++) {
    lo4[i] = min(lo2[i], lo2[(i + 2) & 15]);
    hi4[i] = max(hi2[i], hi2[(i + 2) & 15]);
  }
  int bright = -256, dark_neg = 256;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int lo9 = min(min(lo4[i], lo4[(i + 4) & 15]), d[(i + 8) & 15]);
    const int hi9 = max(max(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
    bright = max(bright, lo9);
    dark_neg = min(dark_neg, hi9);
  }
  const int s = max(bright, -dark_neg);
  return s > thr ? s : 0;
}

// H of the 7 x 7 block around the pixel at p; the pixels within 4 of it are read
__device__ __forceinline__ long long orb_harris(const uint8_t* p, int pitch) {
  int a = 0, b = 0, c = 0;
  for (int dy = -3; dy <= 3; dy++)
    for (int dx = -3; dx <= 3; dx++) {
      const uint8_t* q = p + dy * pitch + dx;
      const int ix = 2 * ((int)q[1] - (int)q[-1]) + ((int)q[-pitch + 1] - (int)q[-pitch - 1]) + ((int)q[pitch + 1] - (int)q[pitch - 1]);
      const int iy = 2 * ((int)q[pitch] - (int)q[-pitch]) + ((int)q[pitch - 1] - (int)q[-pitch - 1]) + ((int)q[pitch + 1] - (int)q[-pitch + 1]);
      a += ix * ix;
      b += iy * iy;
      c += ix * iy;
    }
  return 25ll * ((long long)a * b - (long long)c * c) - (long long)(a + b) * (long long)(a + b);
}

// grid (tiles_x, tiles_y, n_frames) over the candidate band of layer l, 256 threads.  Lanes run along x.
__global__ __launch_bounds__(kOrbBlock) void k_orb_fast(OrbArgs a, int l) {
  constexpr int P = kOrbPixTile, S = kOrbScoreTile, T = kOrbTile;
  __shared__ uint8_t pix[P * P];
  __shared__ int sc[S * S];
  const int f = blockIdx.z, tid = threadIdx.x;
  if (a.mode && a.mode[f] != kPathDetect) return;   // (uniform: ahead of every barrier)
  const int lw = a.lw[l], lh = a.lh[l], e = a.edge;
  int pitch;
  const uint8_t* img = orb_layer_ptr(a, f, l, &pitch);
  const int bx0 = e + blockIdx.x * T, by0 = e + blockIdx.y * T;   // the tile's first score pixel
  for (int t = tid; t < P * P; t += kOrbBlock) {
    const int ty = t / P, tx = t - ty * P;
    const int gx = bx0 - 4 + tx, gy = by0 - 4 + ty;
    pix[t] = (gx < lw && gy < lh) ? img[(size_t)gy * pitch + gx] : (uint8_t)0;   // (gx, gy >= e - 4 >= 0)
  }
  __syncthreads();
  for (int t = tid; t < S * S; t += kOrbBlock) {
    const int sy = t / S, sx = t - sy * S;
    const int gx = bx0 - 1 + sx, gy = by0 - 1 + sy;
    int s = 0;
    if (gx >= e && gx < lw - e && gy >= e && gy < lh - e) s = orb_fast_score(pix + (sy + 3) * P + sx + 3, P, a.fast_threshold);
    sc[t] = s;
  }
  __syncthreads();
  for (int t = tid; t < T * T; t += kOrbBlock) {
    const int ly = t / T, lx = t - ly * T;
    const int gx = bx0 + lx, gy = by0 + ly;
    const int* c = sc + (ly + 1) * S + lx + 1;
    const int v = c[0];
    if (a.score_out && f == 0 && gx < lw && gy < lh) a.score_out[(size_t)gy * lw + gx] = v;
    if (v <= 0) continue;   // (a corner is inside the band: the reads below stay inside the layer)
    if (!(v > c[-S - 1] && v > c[-S] && v > c[-S + 1] && v > c[-1] && v > c[1] && v > c[S - 1] && v > c[S] && v > c[S + 1])) continue;
    const long long H = orb_harris(pix + (ly + 4) * P + lx + 4, P);
    const int at = atomicAdd(a.raw_count + f * kOrbMaxLevels + l, 1);
    if (at < a.raw_cap[l]) {   // (raw_cap is an upper bound of the candidates: always)
      const size_t r = (size_t)f * a.raw_stride + a.raw_off[l] + (size_t)at;
      a.raw_key[r] = ((unsigned long long)gy << 20) | (unsigned long long)gx;
      a.raw_h[r] = H;
    }
  }
}

// the per-stage entry: grid ceil(n / 256); xy: n x (x, y), each at least 4 from every border of the layer (checked on the host)
__global__ __launch_bounds__(kOrbBlock) void k_orb_harris(OrbArgs a, int l, const int* __restrict__ xy, int n, long long* __restrict__ out) {
  const int i = blockIdx.x * kOrbBlock + threadIdx.x;
  if (i >= n) return;
  int pitch;
  const uint8_t* img = orb_layer_ptr(a, 0, l, &pitch);
  out[i] = orb_harris(img + (size_t)xy[2 * i + 1] * pitch + xy[2 * i], pitch);
}

// ---- quota, order and capacity ---------------------------------------------------------------------------------------------------
// grid (n_levels, n_frames), 1024 threads.  Layer l keeps its quota[l] first by (H descending, key ascending); candidate i's rank
// there is its place among them, behind what the layers below keep.
__global__ __launch_bounds__(kOrbRankBlock) void k_orb_rank(OrbArgs a) {
  const int l = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  if (a.mode && a.mode[f] != kPathDetect) return;   // (uniform: ahead of every barrier)
  const int n = min(a.raw_count[f * kOrbMaxLevels + l], a.raw_cap[l]);
  int before = 0;
  for (int k = 0; k < l; k++) before += min(min(a.raw_count[f * kOrbMaxLevels + k], a.raw_cap[k]), a.quota[k]);
  const unsigned long long* key = a.raw_key + (size_t)f * a.raw_stride + a.raw_off[l];
  const long long* H = a.raw_h + (size_t)f * a.raw_stride + a.raw_off[l];
  OrbKept* out = a.kept + (size_t)f * a.kept_stride + before;
  const int q = a.quota[l];
  for (int i0 = 0; i0 < n; i0 += kOrbRankBlock) {
    const int i = i0 + tid;
    const bool mine = i < n;
    const long long hi = mine ? H[i] : 0;
    const unsigned long long ki = mine ? key[i] : 0ull;
    const int rank = select_rank<kOrbRankBlock>(n, mine, hi, ki, [&](int j) { return H[j]; }, [&](int j) { return key[j]; });
    if (mine && rank < q) {   // (before + rank < the sum of the quotas = n_features)
      out[rank].key = ((unsigned long long)l << 40) | ki;
      out[rank].H = hi;
    }
  }
}

// grid n_frames, 1024 threads.  A frame whose layers keep more than cap in all keeps the cap first by (H descending, key
// ascending); every kept candidate goes to the place its key has among the kept.
__global__ __launch_bounds__(kOrbRankBlock) void k_orb_select(OrbArgs a) {
  const int f = blockIdx.x;
  if (a.mode && a.mode[f] != kPathDetect) return;   // (uniform) the frame's count and key points come from elsewhere
  int n = 0;
  for (int k = 0; k < a.n_levels; k++) n += min(min(a.raw_count[f * kOrbMaxLevels + k], a.raw_cap[k]), a.quota[k]);
  const OrbKept* in = a.kept + (size_t)f * a.kept_stride;
  n = select_ordered<kOrbRankBlock>(
      n, a.cap, a.keep + (size_t)f * a.kept_stride, [&](int j) { return in[j].H; }, [&](int j) { return in[j].key; },
      [&](int i, int pos) {
        const unsigned long long ki = in[i].key;
        const int l = (int)(ki >> 40), gy = (int)((ki >> 20) & 0xFFFFFull), gx = (int)(ki & 0xFFFFFull);
        const long long p6 = orb_pow(6, l);
        const double p5 = (double)orb_pow(5, l);
        OrbKeypoint k;
        k.x = (float)((double)((long long)gx * p6) / p5);
        k.y = (float)((double)((long long)gy * p6) / p5);
        k.size = (float)((double)((long long)kOrbPatch * p6) / p5);
        k.response = (float)((double)in[i].H / kOrbHarrisDen);
        k.dir_x = 1.0f;
        k.dir_y = 0.0f;
        k.octave = l;
        k.laplacian = 0;
        a.kp[(size_t)f * a.cap + pos] = k;
      });
  if (threadIdx.x == 0) a.counts[f] = n;
}

// ---- the caller's key points from device memory (the tracking call) --------------------------------------------------------------
// grid (ceil(cap / 256), n_frames): take_provided of uwt_detect.h
__global__ __launch_bounds__(256) void k_orb_take_provided(OrbArgs a, int j0, int n_pairs, const int* __restrict__ path,
                                                           const OrbKeypoint* __restrict__ prev_kp, const int* __restrict__ n_prev,
                                                           int* __restrict__ mode) {
  take_provided(a, j0, n_pairs, path, prev_kp, n_prev, mode);
}

// ---- direction and descriptor ------------------------------------------------------------------------------------------------------
// grid (ceil(rows / 4), n_frames), 256 threads: wave v of block b has key point 4 b + v of its frame.  No barrier: a wave without a
// key point leaves at once.
__global__ __launch_bounds__(64 * kOrbDescWaves) void k_orb_describe(OrbArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, f = blockIdx.y;
  const int k = blockIdx.x * kOrbDescWaves + wv;
  if (k >= min(a.counts[f], a.cap)) return;   // (uniform over the wave)
  OrbKeypoint* kp = a.kp + (size_t)f * a.cap + k;
  const int l = kp->octave;
  uint8_t* desc = a.desc ? static_cast<uint8_t*>(a.desc) + ((size_t)f * a.cap + k) * 32 : nullptr;
  // what the host checks of a caller's record (detection's own always pass) holds here too: no read leaves the layer
  bool ok = l >= 0 && l < a.n_levels && fabsf(kp->x) <= 1e6f && fabsf(kp->y) <= 1e6f;
  int gx = 0, gy = 0;
  if (ok) {
    gx = orb_layer_pos(kp->x, l);
    gy = orb_layer_pos(kp->y, l);
    ok = gx >= kOrbMinEdge && gx < a.lw[l] - kOrbMinEdge && gy >= kOrbMinEdge && gy < a.lh[l] - kOrbMinEdge;
  }
  if (!ok) {   // (uniform)
    if (lane == 0) {
      kp->dir_x = 1.0f;
      kp->dir_y = 0.0f;
    }
    if (desc && lane < 4) reinterpret_cast<unsigned long long*>(desc)[lane] = 0ull;
    return;
  }
  int pitch;
  const uint8_t* c0 = orb_layer_ptr(a, f, l, &pitch) + (size_t)gy * pitch + gx;
  float c = 1.0f, s = 0.0f;
  if (!a.upright) {
    int m10 = 0, m01 = 0;
    for (int t = lane; t < 31 * 31; t += 64) {
      const int v = t / 31 - 15, u = t % 31 - 15;
      if (abs(u) <= (int)kOrbUmax[abs(v)]) {
        const int I = (int)c0[v * pitch + u];
        m10 += u * I;
        m01 += v * I;
      }
    }
    for (int m = 32; m > 0; m >>= 1) {
      m10 += __shfl_xor(m10, m, 64);
      m01 += __shfl_xor(m01, m, 64);
    }
    const float fx = (float)m10, fy = (float)m01;
    const float n = sqrtf(fx * fx + fy * fy);
    if (n != 0.f) {
      c = fx / n;
      s = fy / n;
    }
  }
  if (lane == 0) {
    kp->dir_x = c;
    kp->dir_y = s;
  }
  if (!desc) return;   // (uniform)
  unsigned long long mine = 0ull;
  for (int j = 0; j < 4; j++) {
    const char4 e = reinterpret_cast<const char4*>(a.pattern)[j * 64 + lane];
    const float x0 = (float)e.x, y0 = (float)e.y, x1 = (float)e.z, y1 = (float)e.w;
    const int px0 = orb_rnd(x0 * c - y0 * s), py0 = orb_rnd(x0 * s + y0 * c);
    const int px1 = orb_rnd(x1 * c - y1 * s), py1 = orb_rnd(x1 * s + y1 * c);
    const bool bit = c0[py0 * pitch + px0] < c0[py1 * pitch + px1];
    const unsigned long long word = __ballot(bit);
    if (lane == j) mine = word;
  }
  if (lane < 4) reinterpret_cast<unsigned long long*>(desc)[lane] = mine;
}

}  // namespace uwt
