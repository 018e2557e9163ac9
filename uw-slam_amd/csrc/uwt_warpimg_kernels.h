// uwt_warpimg_kernels.h — gfx950 kernels of Tracker::ObtainImageTransformed (src/Tracker.cpp:1473-1525) and of the image
// Tracker::DebugShowWarpedPerspective builds (:1694-1737).
//
//   k_warp_scatter   one thread per source row: where the row lands, and atomicMax of its index into the pair's winner plane
//   k_warp_resolve   one thread per group of four target pixels: the winners' source bytes, the mask, |warped - image2| and the
//                    pair's integer sums
//   k_warp_mosaic    [image1 | image2] over [blend(warped, image2) | blend(image1, image2)]
//
// The reference is a sequential scatter: among the rows that land on one pixel the LAST one in table order stays.  Here every landed
// row i does atomicMax(&winner[pixel], i) on a plane that starts at -1, and the resolve pass reads the row the plane names.  The
// maximum of a set of integers does not depend on the order in which its elements arrive, so the plane — and everything read from
// it — is the same whatever the scheduling, the batch, the pair's place in it or the launch shape: that is the whole determinism
// argument.  The sums are integers added with integer atomics, order-independent for the same reason.
#pragma once

#include "uwt_warpimg.h"

namespace uwt {

// (int)round(u) of the reference (C round: halves away from zero).  False: u is not finite or |u| >= 2^31 - 128, where the
// conversion is undefined — the row is skipped.  u - trunc(u) is exact in f32.
__device__ __forceinline__ bool warp_round_int(float u, int& r) {
  if (!(__builtin_fabsf(u) < 2147483520.0f)) return false;
  float t = __builtin_truncf(u);
  if (__builtin_fabsf(u - t) >= 0.5f) t += __builtin_copysignf(1.0f, u);
  r = (int)t;
  return true;
}

__device__ __forceinline__ bool warp_pose_finite(const float* __restrict__ q) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) ok = ok && (__builtin_fabsf(q[k]) < __builtin_inff());
  return ok;
}

// the sum of v over the block, valid in thread 0 (every thread of the block calls it)
template <typename T>
__device__ __forceinline__ T warp_block_sum(T v, T* red) {
  __syncthreads();   // the previous use of red
  red[threadIdx.x] = v;
  __syncthreads();
  for (int st = kBlock / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  return red[0];
}

// (int)pts[i][0], (int)pts[i][1] of an explicit row (truncation toward zero: -0.5 reads column 0).  False: outside the level's image
// (or not a number) — the reference would read out of bounds; the row is skipped.
__device__ __forceinline__ bool warp_source_pixel(const LevelK& L, const float4 p, int& x1, int& y1) {
  if (!(p.x > -1.0f && p.x < (float)L.iw && p.y > -1.0f && p.y < (float)L.ih)) return false;
  x1 = (int)p.x;
  y1 = (int)p.y;
  return true;
}

// Grid (ceil(n / kBlock), n_pairs).  DENSE: row i is point (x, y) = (i - y gw, i / gw) of ObtainAllPoints' grid (src/Tracker.cpp:
// 1266-1302: z = depth * zscale, a point whose depth read as int16 is <= 0 becomes [0 0 1 0], z = 1 without a depth plane), warped
// with warp_table_point and the projection lines of k_warp_table under the pair's pose.  Else row i of the table and of its warped
// rows.  A row lands iff y2 > 0 && y2 < rows && x2 > 0 && x2 < cols (:1483).
template <int AR, bool DENSE>
__global__ __launch_bounds__(kBlock) void k_warp_scatter(const WarpImageArgs a) {
  __shared__ int red[kBlock];
  const int pair = blockIdx.y;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const LevelK& L = a.L;
  int landed = 0;
  bool ok = i < a.n;
  float u = 0.f, v = 0.f;
  if constexpr (DENSE) {
    const float* q = a.poses + 7 * (size_t)pair;
    ok = ok && warp_pose_finite(q);
    if (ok) {
      const int y = i / L.gw, x = i - y * L.gw;
      float4 p = make_float4((float)x, (float)y, 1.0f, 1.0f);
      if (a.depth) {
        const int d = (int)(int16_t)a.depth[(size_t)a.ref_slots[pair] * L.n + (size_t)y * L.pitch + x];   // at<short> (:1272)
        if (d > 0) p.z = (float)d * L.zscale;
        else p = make_float4(0.f, 0.f, 1.0f, 0.f);
      }
      Pose pose;
      for (int k = 0; k < 4; k++) pose.q[k] = q[k];
      for (int k = 0; k < 3; k++) pose.t[k] = q[4 + k];
      float T[12], o[3], wq;
      pose_to_T12(pose, T);
      warp_table_point<AR>(L, T, p, o, wq);
      u = o[0] * L.fx; u = u / o[2]; u = u + L.cx;
      v = o[1] * L.fy; v = v / o[2]; v = v + L.cy;
      u = u * wq;
      v = v * wq;
    }
  } else {
    if (ok) {
      int x1, y1;
      ok = warp_source_pixel(L, a.pts[i], x1, y1);
      const float4 wp = a.warped_pts[i];
      u = wp.x;
      v = wp.y;
    }
  }
  int x2 = 0, y2 = 0;
  ok = ok && warp_round_int(u, x2) && warp_round_int(v, y2);
  int at = -1;   // the target's offset in the pair's plane
  if (ok && y2 > 0 && y2 < L.ih && x2 > 0 && x2 < L.iw) {
    at = y2 * L.pitch + x2;
    landed = 1;
  }
  // The next lane holds row i + 1.  A row whose successor lands on the same pixel cannot be that pixel's maximum, so it leaves its
  // atomic out: the plane is the same, and the lanes of a wave that would queue on one address (neighbours in x under a contracting
  // pose) do not.
  const int next = __shfl_down(at, 1);
  const bool loses = (threadIdx.x & 63) != 63 && next == at;
  if (landed && !loses) atomicMax(&a.winner[(size_t)pair * L.n + at], i);   // the largest i wins: order-independent
  if (a.quality) {
    const int total = warp_block_sum<int>(landed, red);
    if (threadIdx.x == 0 && total) atomicAdd(&a.quality[pair].n_landed, total);
  }
}

// Grid (ceil(pitch / 4 * ih / kBlock), n_pairs).  A thread owns four pixels of a row (x .. x + 3; those at x >= iw are pad columns
// of the pitched row and carry nothing).
template <bool DENSE>
__global__ __launch_bounds__(kBlock) void k_warp_resolve(const WarpImageArgs a) {
  __shared__ unsigned long long red[kBlock];
  const int pair = blockIdx.y;
  const LevelK& L = a.L;
  const int gpr = L.pitch >> 2, groups = gpr * L.ih;
  const int g = blockIdx.x * kBlock + threadIdx.x;
  bool failed = false;
  if constexpr (DENSE) failed = !warp_pose_finite(a.poses + 7 * (size_t)pair);
  unsigned long long n_cov = 0, s_abs = 0, s_sq = 0, s_un = 0;
  if (g < groups) {
    const int y = g / gpr, x = (g - y * gpr) << 2;
    const size_t at = (size_t)pair * L.n + (size_t)y * L.pitch + x;
    const int4 w4 = *reinterpret_cast<const int4*>(a.winner + at);
    const int win[4] = {w4.x, w4.y, w4.z, w4.w};
    const uint8_t* orig = a.img + (size_t)a.ref_slots[pair] * L.n;
    uint32_t keep = 0, t4 = 0, r4 = 0;
    if (a.keep) keep = *reinterpret_cast<const uint32_t*>(a.warped + at);
    if (a.tgt_slots) {
      const size_t off = (size_t)y * L.pitch + x;
      t4 = *reinterpret_cast<const uint32_t*>(a.img + (size_t)a.tgt_slots[pair] * L.n + off);   // image2
      r4 = *reinterpret_cast<const uint32_t*>(orig + off);                                     // image1 at the same pixels
    }
    uint32_t out = 0, val = 0, dif = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t b = (keep >> (8 * j)) & 255u;
      const int i = win[j];
      if (x + j < L.iw && i >= 0 && !failed) {
        int x1, y1;
        if constexpr (DENSE) {
          y1 = i / L.gw;
          x1 = i - y1 * L.gw;
        } else {
          warp_source_pixel(L, a.pts[i], x1, y1);   // a row that landed has passed this test
        }
        b = orig[(size_t)y1 * L.pitch + x1];
        val |= 1u << (8 * j);
        if (a.tgt_slots) {
          const int t = (int)((t4 >> (8 * j)) & 255u), r = (int)((r4 >> (8 * j)) & 255u);
          const int d = abs((int)b - t);
          dif |= (uint32_t)d << (8 * j);
          n_cov += 1;
          s_abs += (unsigned)d;
          s_sq += (unsigned)(d * d);
          s_un += (unsigned)abs(r - t);
        }
      }
      out |= b << (8 * j);
    }
    if (a.warped) *reinterpret_cast<uint32_t*>(a.warped + at) = out;
    if (a.valid) *reinterpret_cast<uint32_t*>(a.valid + at) = val;
    if (a.absdiff) *reinterpret_cast<uint32_t*>(a.absdiff + at) = dif;
  }
  if (a.quality) {
    WarpQuality* q = a.quality + pair;
    n_cov = warp_block_sum<unsigned long long>(n_cov, red);
    s_abs = warp_block_sum<unsigned long long>(s_abs, red);
    s_sq = warp_block_sum<unsigned long long>(s_sq, red);
    s_un = warp_block_sum<unsigned long long>(s_un, red);
    if (threadIdx.x == 0) {   // integers: order-independent
      if (n_cov) atomicAdd(&q->n_covered, (int)n_cov);
      if (s_abs) atomicAdd(reinterpret_cast<unsigned long long*>(&q->sum_abs), s_abs);
      if (s_sq) atomicAdd(reinterpret_cast<unsigned long long*>(&q->sum_sq), s_sq);
      if (s_un) atomicAdd(reinterpret_cast<unsigned long long*>(&q->sum_abs_unaligned), s_un);
      if (blockIdx.x == 0) {
        q->status = failed ? a.invalid_status : 0;
        q->n_points = failed ? 0 : a.n;
      }
    }
  }
}

// addWeighted(a, 0.5, b, 0.5, 1.0) on u8: saturate(cvRound(0.5 a + 0.5 b + 1)), cvRound to the even neighbour of a half
__device__ __forceinline__ uint8_t warp_blend(int a, int b) {
  const int s = a + b;
  int m = (s >> 1) + 1;
  if (s & 1) m += (m & 1);   // m + 0.5: the even one of m, m + 1
  return (uint8_t)min(m, 255);
}

// One thread per pixel of the 2 iw x 2 ih image (src/Tracker.cpp:1700-1727); the resize loop of :1729-1732 scales the window for the
// display and is not built.
static __global__ __launch_bounds__(kBlock) void k_warp_mosaic(const LevelK L, const uint8_t* __restrict__ image1,
                                                               const uint8_t* __restrict__ image2, const uint8_t* __restrict__ warped,
                                                               uint8_t* __restrict__ out) {
  const int W = 2 * L.iw, H = 2 * L.ih;
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= W * H) return;
  const int Y = k / W, X = k - Y * W;
  const int y = Y < L.ih ? Y : Y - L.ih, x = X < L.iw ? X : X - L.iw;
  const size_t at = (size_t)y * L.pitch + x;
  uint8_t r;
  if (Y < L.ih) r = X < L.iw ? image1[at] : image2[at];
  else r = X < L.iw ? warp_blend(warped[at], image2[at]) : warp_blend(image1[at], image2[at]);
  out[k] = r;
}

}  // namespace uwt
