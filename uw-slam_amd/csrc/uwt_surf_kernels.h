// uwt_surf_kernels.h — the kernels of SURF detection and description.  include/uwt.h states the contract; every f32 / f64 step here
// is the one operation the contract names (the unit is built with -ffp-contract=off), integers are exact.
//   k_surf_integral_rows / _cols   the integral image: a wave scans a row in chunks of 64, then a thread runs down each column
//   k_surf_response                one octave: a 32 x 32 tile of every layer with a one-point halo in LDS, suppression from LDS,
//                                  refinement of the survivors, which are appended to the frame's raw list with their order key
//   k_surf_select                  one block per frame: the cap strongest when the frame overflows, then each survivor's place
//                                  among the kept by its key — the output is a function of the SET of candidates alone
//   k_surf_describe                one wave per key point: orientation (109 samples over the lanes, 36 windows on 36 lanes, each
//                                  summing in sample order), then 400 samples over the lanes and one descriptor element per lane
#pragma once

#include "uwt_select.h"
#include "uwt_surf.h"

namespace uwt {

// ---- the literal tables of include/uwt.h -------------------------------------------------------------------------------------
constexpr float kSurfScale = 0.13333334f;
__constant__ float kSurfOriWeight[49] = {
  1.0f, 0.923116326f, 0.726149023f, 0.486752242f, 0.27803731f, 0.135335281f, 0.0561347641f,
  0.923116326f, 0.852143764f, 0.670320034f, 0.449328959f, 0.256660789f, 0.12493021f, 0.0518189184f,
  0.726149023f, 0.670320034f, 0.52729243f, 0.353454679f, 0.201896518f, 0.0982735828f, 0.0407622047f,
  0.486752242f, 0.449328959f, 0.353454679f, 0.236927763f, 0.135335281f, 0.0658747554f, 0.0273237228f,
  0.27803731f, 0.256660789f, 0.201896518f, 0.135335281f, 0.0773047432f, 0.0376282558f, 0.0156075582f,
  0.135335281f, 0.12493021f, 0.0982735828f, 0.0658747554f, 0.0376282558f, 0.0183156393f, 0.00759701384f,
  0.0561347641f, 0.0518189184f, 0.0407622047f, 0.0273237228f, 0.0156075582f, 0.00759701384f, 0.00315111154f};
__constant__ float kSurfOriDir[72] = {
  1.0f, 0.0f, 0.98480773f, 0.173648179f, 0.939692616f, 0.342020154f, 0.866025388f, 0.5f,
  0.766044438f, 0.642787635f, 0.642787635f, 0.766044438f, 0.5f, 0.866025388f, 0.342020154f, 0.939692616f,
  0.173648179f, 0.98480773f, 0.0f, 1.0f, -0.173648179f, 0.98480773f, -0.342020154f, 0.939692616f,
  -0.5f, 0.866025388f, -0.642787635f, 0.766044438f, -0.766044438f, 0.642787635f, -0.866025388f, 0.5f,
  -0.939692616f, 0.342020154f, -0.98480773f, 0.173648179f, -1.0f, 0.0f, -0.98480773f, -0.173648179f,
  -0.939692616f, -0.342020154f, -0.866025388f, -0.5f, -0.766044438f, -0.642787635f, -0.642787635f, -0.766044438f,
  -0.5f, -0.866025388f, -0.342020154f, -0.939692616f, -0.173648179f, -0.98480773f, 0.0f, -1.0f,
  0.173648179f, -0.98480773f, 0.342020154f, -0.939692616f, 0.5f, -0.866025388f, 0.642787635f, -0.766044438f,
  0.766044438f, -0.642787635f, 0.866025388f, -0.5f, 0.939692616f, -0.342020154f, 0.98480773f, -0.173648179f};
__constant__ float kSurfDescGauss[10] = {
  0.988587201f, 0.901851177f, 0.750541389f, 0.569815516f, 0.394651532f,
  0.249352202f, 0.143725067f, 0.0755738765f, 0.0362518989f, 0.0158638898f};

// the grid points of the radius-6 disc, j (y) outermost, both ascending
constexpr int kSurfOriSamples = 109;
struct SurfDisc {
  signed char i[kSurfOriSamples], j[kSurfOriSamples];
  constexpr SurfDisc() : i(), j() {
    int n = 0;
    for (int b = -6; b <= 6; b++)
      for (int a = -6; a <= 6; a++)
        if (a * a + b * b < 36) {
          i[n] = (signed char)a;
          j[n] = (signed char)b;
          n++;
        }
  }
};
__constant__ SurfDisc kSurfDisc = SurfDisc();

// ---- box sums ----------------------------------------------------------------------------------------------------------------
// the sum over [x0, x1) x [y0, y1), modulo 2^32; the corners are inside the (h + 1) x iw integral image
__device__ __forceinline__ long long surf_box(const uint32_t* __restrict__ I, int iw, int x0, int y0, int x1, int y1) {
  const uint32_t s = I[(size_t)y1 * iw + x1] - I[(size_t)y0 * iw + x1] - I[(size_t)y1 * iw + x0] + I[(size_t)y0 * iw + x0];
  return (long long)s;
}
__device__ __forceinline__ int surf_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ long long surf_box_clip(const uint32_t* __restrict__ I, int w, int h, int x0, int y0, int x1, int y1) {
  return surf_box(I, w + 1, surf_clamp(x0, w), surf_clamp(y0, h), surf_clamp(x1, w), surf_clamp(y1, h));
}
// (right - left, bottom - top) of the 2hh x 2hh box around the pixel corner (px, py), clipped to the image
__device__ __forceinline__ void surf_haar(const uint32_t* __restrict__ I, int w, int h, int px, int py, int hh, long long* dx,
                                          long long* dy) {
  *dx = surf_box_clip(I, w, h, px, py - hh, px + hh, py + hh) - surf_box_clip(I, w, h, px - hh, py - hh, px, py + hh);
  *dy = surf_box_clip(I, w, h, px - hh, py, px + hh, py + hh) - surf_box_clip(I, w, h, px - hh, py - hh, px + hh, py);
}
__device__ __forceinline__ int surf_rnd(float v) { return (int)floorf(v + 0.5f); }

// Dxx, Dyy, Dxy of the s x s filter centred on pixel (cx, cy); false where its window leaves the image
__device__ __forceinline__ bool surf_hessian(const uint32_t* __restrict__ I, int w, int h, int cx, int cy, int s, long long* dxx,
                                             long long* dyy, long long* dxy) {
  const int x0 = cx - (s >> 1), y0 = cy - (s >> 1);
  if (x0 < 0 || y0 < 0 || x0 + s > w || y0 + s > h) return false;
  const int iw = w + 1;
  const int p1 = (s + 4) / 9, p2 = (2 * s + 4) / 9, p3 = (3 * s + 4) / 9, p4 = (4 * s + 4) / 9, p5 = (5 * s + 4) / 9,
            p6 = (6 * s + 4) / 9, p7 = (7 * s + 4) / 9, p8 = (8 * s + 4) / 9, p9 = s;
  *dxx = surf_box(I, iw, x0, y0 + p2, x0 + p9, y0 + p7) - 3 * surf_box(I, iw, x0 + p3, y0 + p2, x0 + p6, y0 + p7);
  *dyy = surf_box(I, iw, x0 + p2, y0, x0 + p7, y0 + p9) - 3 * surf_box(I, iw, x0 + p2, y0 + p3, x0 + p7, y0 + p6);
  *dxy = surf_box(I, iw, x0 + p1, y0 + p1, x0 + p4, y0 + p4) + surf_box(I, iw, x0 + p5, y0 + p5, x0 + p8, y0 + p8) -
         surf_box(I, iw, x0 + p5, y0 + p1, x0 + p8, y0 + p4) - surf_box(I, iw, x0 + p1, y0 + p5, x0 + p4, y0 + p8);
  return true;
}
__device__ __forceinline__ double surf_response(const uint32_t* __restrict__ I, int w, int h, int cx, int cy, int s) {
  long long dxx, dyy, dxy;
  if (!surf_hessian(I, w, h, cx, cy, s, &dxx, &dyy, &dxy)) return __builtin_nan("");
  const long long num = 100 * dxx * dyy - 81 * dxy * dxy;
  const double s2 = (double)(s * s);
  return (double)num / (100.0 * s2 * s2);
}

// ---- the integral image ------------------------------------------------------------------------------------------------------
// grid (ceil((h + 1) / 4), n_frames), 256 threads: wave v of block b has row r = 4 b + v of the integral image: row 0 is zero, row
// r the running sums of image row r - 1 (column 0 zero)
__global__ __launch_bounds__(256) void k_surf_integral_rows(SurfArgs a) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6), f = blockIdx.y;
  if (r > a.h) return;
  const int iw = a.w + 1;
  uint32_t* out = a.integral + (size_t)f * (size_t)(a.h + 1) * iw + (size_t)r * iw;
  if (r == 0) {
    for (int x = lane; x < iw; x += 64) out[x] = 0u;
    return;
  }
  const uint8_t* row = a.img + (size_t)a.slots[f] * a.frame_stride + (size_t)(r - 1) * a.pitch;
  if (lane == 0) out[0] = 0u;
  uint32_t carry = 0u;
  for (int x0 = 0; x0 < a.w; x0 += 64) {
    const int x = x0 + lane;
    uint32_t v = x < a.w ? (uint32_t)row[x] : 0u;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(v, d, 64);
      if (lane >= d) v += up;
    }
    if (x < a.w) out[x + 1] = carry + v;
    carry += __shfl(v, 63, 64);
  }
}
// grid (ceil(w / 256), n_frames): a thread runs down column x + 1
__global__ __launch_bounds__(256) void k_surf_integral_cols(SurfArgs a) {
  const int x = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (x >= a.w) return;
  const int iw = a.w + 1;
  uint32_t* col = a.integral + (size_t)f * (size_t)(a.h + 1) * iw + (size_t)(x + 1);
  uint32_t acc = 0u;
  for (int y = 1; y <= a.h; y++) {
    acc += col[(size_t)y * iw];
    col[(size_t)y * iw] = acc;
  }
}

// one response layer of frame 0 on the octave's grid (the per-stage entry): grid ceil(gw * gh / 256)
__global__ __launch_bounds__(256) void k_surf_response_layer(SurfArgs a, int octave, int layer, double* __restrict__ out) {
  const int gw = a.w >> octave, gh = a.h >> octave;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= gw * gh) return;
  const int gy = i / gw, gx = i - gy * gw;
  out[i] = surf_response(a.integral, a.w, a.h, gx << octave, gy << octave, surf_filter_size(octave, layer));
}

// ---- response, suppression, refinement ------------------------------------------------------------------------------------------
// grid (tiles_x, tiles_y, n_frames) for one octave, 256 threads, dynamic LDS: layers x 34 x 34 doubles.  Lanes run along x.
__global__ __launch_bounds__(kSurfBlock) void k_surf_response(SurfArgs a, int octave) {
  extern __shared__ double lds_r[];
  constexpr int T = kSurfTile + 2;
  const int f = blockIdx.z;
  if (a.mode && a.mode[f] != kPathDetect) return;   // (uniform: ahead of every barrier)
  const uint32_t* I = a.integral + (size_t)f * (size_t)(a.h + 1) * (size_t)(a.w + 1);
  const int gx0 = blockIdx.x * kSurfTile - 1, gy0 = blockIdx.y * kSurfTile - 1;   // grid point of the tile's (0, 0), halo included
  const int L = a.layers;
  for (int t = threadIdx.x; t < L * T * T; t += kSurfBlock) {
    const int l = t / (T * T), r = t - l * T * T, ly = r / T, lx = r - ly * T;
    const int gx = gx0 + lx, gy = gy0 + ly;
    double v = __builtin_nan("");
    if (gx >= 0 && gy >= 0 && gx < (a.w >> octave) && gy < (a.h >> octave))
      v = surf_response(I, a.w, a.h, gx << octave, gy << octave, surf_filter_size(octave, l));
    lds_r[t] = v;
  }
  __syncthreads();
  const double thr = a.threshold;
  for (int t = threadIdx.x; t < (L - 2) * kSurfTile * kSurfTile; t += kSurfBlock) {
    const int l = 1 + t / (kSurfTile * kSurfTile), r = t % (kSurfTile * kSurfTile), ly = 1 + r / kSurfTile, lx = 1 + r % kSurfTile;
    const double* c = lds_r + (l * T + ly) * T + lx;
#define SURF_R(dl, dy, dx) c[((dl) * T + (dy)) * T + (dx)]
    const double v = c[0];
    if (!(v > thr)) continue;
    bool top = true;
    for (int dl = -1; dl <= 1; dl++)
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++)
          if (dl | dy | dx) top = top && (v > SURF_R(dl, dy, dx));   // an absent neighbour is NaN: the comparison fails
    if (!top) continue;
    const double gdx = (SURF_R(0, 0, 1) - SURF_R(0, 0, -1)) * 0.5;
    const double gdy = (SURF_R(0, 1, 0) - SURF_R(0, -1, 0)) * 0.5;
    const double gds = (SURF_R(1, 0, 0) - SURF_R(-1, 0, 0)) * 0.5;
    const double dxx = (SURF_R(0, 0, 1) - 2.0 * v) + SURF_R(0, 0, -1);
    const double dyy = (SURF_R(0, 1, 0) - 2.0 * v) + SURF_R(0, -1, 0);
    const double dss = (SURF_R(1, 0, 0) - 2.0 * v) + SURF_R(-1, 0, 0);
    const double dxy = (((SURF_R(0, 1, 1) - SURF_R(0, 1, -1)) - SURF_R(0, -1, 1)) + SURF_R(0, -1, -1)) * 0.25;
    const double dxs = (((SURF_R(1, 0, 1) - SURF_R(1, 0, -1)) - SURF_R(-1, 0, 1)) + SURF_R(-1, 0, -1)) * 0.25;
    const double dys = (((SURF_R(1, 1, 0) - SURF_R(1, -1, 0)) - SURF_R(-1, 1, 0)) + SURF_R(-1, -1, 0)) * 0.25;
#undef SURF_R
    const double b0 = -gdx, b1 = -gdy, b2 = -gds;
    const double p0 = dxx;
    if (p0 == 0.0) continue;
    const double m1 = dxy / p0, m2 = dxs / p0;
    const double a11 = dyy - m1 * dxy, a12 = dys - m1 * dxs, c1 = b1 - m1 * b0;
    const double a21 = dys - m2 * dxy, a22 = dss - m2 * dxs, c2 = b2 - m2 * b0;
    const double p1 = a11;
    if (p1 == 0.0) continue;
    const double m3 = a21 / p1;
    const double p2 = a22 - m3 * a12;
    if (p2 == 0.0) continue;
    const double c2b = c2 - m3 * c1;
    const double os = c2b / p2;
    const double oy = (c1 - a12 * os) / p1;
    const double ox = ((b0 - dxy * oy) - dxs * os) / p0;
    if (!(fabs(ox) <= 1.0 && fabs(oy) <= 1.0 && fabs(os) <= 1.0)) continue;
    const int gx = gx0 + lx, gy = gy0 + ly, s = surf_filter_size(octave, l);
    long long hxx = 0, hyy = 0, hxy = 0;
    surf_hessian(I, a.w, a.h, gx << octave, gy << octave, s, &hxx, &hyy, &hxy);
    const long long tr = hxx + hyy;
    SurfKeypoint k;
    k.x = (float)(((double)gx + ox) * (double)(1 << octave));
    k.y = (float)(((double)gy + oy) * (double)(1 << octave));
    k.size = (float)((double)s + os * (double)(6 << octave));
    k.response = (float)v;
    k.dir_x = 1.0f;
    k.dir_y = 0.0f;
    k.octave = octave;
    k.laplacian = tr > 0 ? 1 : (tr < 0 ? -1 : 0);
    const int at = atomicAdd(a.raw_count + f, 1);
    if (at < a.raw_cap) {   // (raw_cap is an upper bound of the candidates: always)
      a.raw[(size_t)f * a.raw_cap + at] = k;
      a.raw_key[(size_t)f * a.raw_cap + at] =
          ((unsigned long long)(octave * 8 + l) << 40) | ((unsigned long long)gy << 20) | (unsigned long long)gx;
    }
  }
}

// ---- order and capacity ------------------------------------------------------------------------------------------------------
// grid n_frames, 1024 threads.  A frame with more than cap candidates keeps the cap first by (response descending, key ascending);
// every kept candidate goes to the place its key has among the kept.
__global__ __launch_bounds__(kSurfSelectBlock) void k_surf_select(SurfArgs a) {
  const int f = blockIdx.x;
  if (a.mode && a.mode[f] != kPathDetect) return;   // (uniform) the frame's count and key points come from elsewhere
  const SurfKeypoint* raw = a.raw + (size_t)f * a.raw_cap;
  const unsigned long long* key = a.raw_key + (size_t)f * a.raw_cap;
  const int n = select_ordered<kSurfSelectBlock>(
      min(a.raw_count[f], a.raw_cap), a.cap, a.keep + (size_t)f * a.raw_cap, [&](int j) { return raw[j].response; },
      [&](int j) { return key[j]; }, [&](int i, int pos) { a.kp[(size_t)f * a.cap + pos] = raw[i]; });
  if (threadIdx.x == 0) a.counts[f] = n;
}

// ---- orientation and descriptor ---------------------------------------------------------------------------------------------------
// grid (ceil(rows / 4), n_frames), 256 threads: wave v of block b has key point 4 b + v of its frame
__global__ __launch_bounds__(64 * kSurfDescWaves) void k_surf_describe(SurfArgs a) {
  __shared__ float lds_x[kSurfDescWaves][400], lds_y[kSurfDescWaves][400];
  __shared__ float lds_n2[kSurfDescWaves][36], lds_sx[kSurfDescWaves][36], lds_sy[kSurfDescWaves][36];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, f = blockIdx.y;
  const int k = blockIdx.x * kSurfDescWaves + wv;
  if ((int)blockIdx.x * kSurfDescWaves >= min(a.counts[f], a.cap)) return;   // (uniform) a launch sized by cap: no row of this block
  const bool live = k < min(a.counts[f], a.cap);
  const uint32_t* I = a.integral + (size_t)f * (size_t)(a.h + 1) * (size_t)(a.w + 1);
  SurfKeypoint* kp = a.kp + (size_t)f * a.cap + (live ? k : 0);
  float x = 0.f, y = 0.f, sc = 0.f;
  if (live) {
    x = kp->x;
    y = kp->y;
    sc = kp->size * kSurfScale;
  }
  float c = 1.0f, s = 0.0f;
  float* px_ = lds_x[wv];
  float* py_ = lds_y[wv];
  if (!a.upright) {   // (uniform over the block: the barriers below are reached by every wave)
    if (live) {
      int hh = surf_rnd(2.0f * sc);
      hh = hh < 1 ? 1 : hh;
      for (int t = lane; t < kSurfOriSamples; t += 64) {
        const int i = kSurfDisc.i[t], j = kSurfDisc.j[t];
        const int px = surf_rnd(x + (float)i * sc), py = surf_rnd(y + (float)j * sc);
        long long dx, dy;
        surf_haar(I, a.w, a.h, px, py, hh, &dx, &dy);
        const float wgt = kSurfOriWeight[(j < 0 ? -j : j) * 7 + (i < 0 ? -i : i)];
        px_[t] = wgt * (float)dx;
        py_[t] = wgt * (float)dy;
      }
    }
    __syncthreads();
    if (live && lane < 36) {
      const int k2 = (lane + 6) % 36;
      const float ax = kSurfOriDir[2 * lane], ay = kSurfOriDir[2 * lane + 1], bx = kSurfOriDir[2 * k2], by = kSurfOriDir[2 * k2 + 1];
      float sx = 0.f, sy = 0.f;
      for (int t = 0; t < kSurfOriSamples; t++) {
        const float wx = px_[t], wy = py_[t];
        const float c0 = ax * wy - ay * wx;
        const float c1 = wx * by - wy * bx;
        if (c0 >= 0.f && c1 > 0.f) {
          sx = sx + wx;
          sy = sy + wy;
        }
      }
      lds_sx[wv][lane] = sx;
      lds_sy[wv][lane] = sy;
      lds_n2[wv][lane] = sx * sx + sy * sy;
    }
    __syncthreads();
    if (live) {
      int best = 0;
      float bn = lds_n2[wv][0];
      for (int w2 = 1; w2 < 36; w2++)
        if (lds_n2[wv][w2] > bn) {
          bn = lds_n2[wv][w2];
          best = w2;
        }
      const float bx = lds_sx[wv][best], by = lds_sy[wv][best];
      const float n = sqrtf(bx * bx + by * by);
      if (n != 0.f) {
        c = bx / n;
        s = by / n;
      }
    }
    __syncthreads();   // the sample buffers are reused below
  }
  if (live && lane == 0) {
    kp->dir_x = c;
    kp->dir_y = s;
  }
  if (!a.desc) return;   // (uniform)
  if (live) {
    int hh = surf_rnd(sc);
    hh = hh < 1 ? 1 : hh;
    for (int t = lane; t < 400; t += 64) {
      const int ty = t / 20, tx = t - ty * 20;
      const float rx = ((float)tx - 9.5f) * sc, ry = ((float)ty - 9.5f) * sc;
      const float sx = x + (rx * c - ry * s);
      const float sy = y + (rx * s + ry * c);
      long long dx, dy;
      surf_haar(I, a.w, a.h, surf_rnd(sx), surf_rnd(sy), hh, &dx, &dy);
      const float g = kSurfDescGauss[tx < 10 ? 9 - tx : tx - 10] * kSurfDescGauss[ty < 10 ? 9 - ty : ty - 10];
      const float wdx = g * (float)dx, wdy = g * (float)dy;
      px_[t] = wdx * c + wdy * s;
      py_[t] = wdy * c - wdx * s;
    }
  }
  __syncthreads();
  if (!live) return;
  const int sub = lane >> 2, comp = lane & 3, sb = sub >> 2, sa = sub & 3;
  float acc = 0.f;
  for (int v = 0; v < 5; v++)
    for (int u = 0; u < 5; u++) {
      const int t = (sb * 5 + v) * 20 + sa * 5 + u;
      const float e = (comp & 1) ? py_[t] : px_[t];
      acc = acc + ((comp & 2) ? fabsf(e) : e);
    }
  float q = acc * acc;
  for (int m = 32; m > 0; m >>= 1) q = q + __shfl_xor(q, m, 64);
  const float n = sqrtf(q);
  static_cast<float*>(a.desc)[((size_t)f * a.cap + k) * 64 + lane] = n == 0.f ? 0.f : acc / n;
}

// ---- the caller's key points from device memory (the tracking call) --------------------------------------------------------------
// grid (ceil(cap / 256), n_frames): take_provided of uwt_detect.h
__global__ __launch_bounds__(256) void k_surf_take_provided(SurfArgs a, int j0, int n_pairs, const int* __restrict__ path,
                                                            const SurfKeypoint* __restrict__ prev_kp, const int* __restrict__ n_prev,
                                                            int* __restrict__ mode) {
  take_provided(a, j0, n_pairs, path, prev_kp, n_prev, mode);
}

}  // namespace uwt
