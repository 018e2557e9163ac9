// uwt_sweep_kernels.h — the gfx950 kernel of the depth sweep (EXTENSION, no reference counterpart; include/uwt.h states the contract).
//
//   k_sweep   a 256-thread block owns a 32 x 8 tile of the reference image.  It forms the views' rigid matrices once (pose_to_T12, the
//             arithmetic of uwt_warp) and stages the tile with a halo of two pixels in LDS; one thread per pixel evaluates the selection
//             and the border test and writes the planes of the pixels that need no sweep; the others are compacted into an LDS list by
//             ballot.  The four waves walk the list with stride four, ONE PIXEL PER WAVE, A LANE PER HYPOTHESIS: the lane warps its row
//             through warp_table_point and the projection lines of k_warp_table, gathers the (2 r + 1) rows of every view's patch as
//             bytes packed into dwords and sums absolute differences four bytes at a time (v_sad_u8) against the reference rows read
//             from LDS in the same packing.  The decision is wave operations alone: ballots and bit scans for validity, the winner as
//             the wave minimum of cost << 6 | k (the smallest k wins a tie by construction), the competitor a second masked minimum,
//             shuffles for the winner's landing and its neighbours' costs.  Lane 0 writes.
//
// Determinism: a pixel's outcome is a function of its own inputs; the per-job counts are integer sums (LDS atomics per block, then
// integer atomics on the job's record, which the call zeroes): order-independent.  No cursor, no float atomic.
#pragma once

#include "uwt_sweep.h"

namespace uwt {

// (int)round(u), C round; false where the contract says the hypothesis does not land (not finite, or |u| >= 2^31 - 128)
__device__ __forceinline__ bool sweep_round_int(float u, int& r) {
  if (!(__builtin_fabsf(u) < 2147483520.0f)) return false;
  float t = __builtin_truncf(u);
  if (__builtin_fabsf(u - t) >= 0.5f) t += __builtin_copysignf(1.0f, u);
  r = (int)t;
  return true;
}

// bytes sh .. sh + 2 r of the eight bytes (w1 : w0): the first four in lo, the fifth (r = 2) in hi; unused positions 0
__device__ __forceinline__ void sweep_pack(uint32_t w0, uint32_t w1, int sh, int r, uint32_t& lo, uint32_t& hi) {
  const unsigned long long w = (((unsigned long long)w1 << 32) | w0) >> (8 * sh);
  lo = (uint32_t)w;
  hi = (uint32_t)(w >> 32) & 0xFFu;
  if (r == 1) { lo &= 0xFFFFFFu; hi = 0; }
}

__device__ __forceinline__ uint32_t sweep_wave_min(uint32_t v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m));
  return v;
}

template <int AR>
__global__ __launch_bounds__(kBlock) void k_sweep(const SweepArgs a) {
  constexpr int TW = kSweepTileW, TH = kSweepTileH, HALO = 2;
  constexpr int SW = 40;                     // bytes per staged row: TW + 2 HALO = 36, rounded up to whole dwords with one to spare
  constexpr int SROWS = TH + 2 * HALO;
  static_assert(TW * TH == kBlock && SW % 4 == 0 && SW >= TW + 2 * HALO + 4, "k_sweep tile");
  __shared__ uint32_t ref_w[SROWS * SW / 4];
  __shared__ float Tm[kSweepMaxViews * 12];
  __shared__ uint16_t list[kBlock];
  __shared__ int wave_cnt[kBlock / 64];
  __shared__ int cnt[8];
  __shared__ unsigned long long sums[2];
  __shared__ int s_failed;

  const LevelK& L = a.L;
  const int job = blockIdx.y;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int tiles_x = (L.iw + TW - 1) / TW;
  const int y0 = ((int)blockIdx.x / tiles_x) * TH, x0 = ((int)blockIdx.x % tiles_x) * TW;
  const int r = a.radius;
  const uint8_t* ref = a.img + (size_t)a.ref_slots[job] * L.n;

  if (t < 8) cnt[t] = 0;
  if (t < 2) sums[t] = 0;
  if (t == 0) s_failed = 0;
  __syncthreads();
  if (t < a.n_views) {   // the rigid matrix of view t, as uwt_warp forms it
    const float* q = a.poses + 7 * ((size_t)job * a.n_views + t);
    bool ok = true;
    Pose pose;
#pragma unroll
    for (int k = 0; k < 7; k++) ok = ok && (__builtin_fabsf(q[k]) < __builtin_inff());
#pragma unroll
    for (int k = 0; k < 4; k++) pose.q[k] = q[k];
#pragma unroll
    for (int k = 0; k < 3; k++) pose.t[k] = q[4 + k];
    float T[12];
    pose_to_T12(pose, T);
#pragma unroll
    for (int k = 0; k < 12; k++) Tm[12 * t + k] = T[k];
    if (!ok) atomicOr(&s_failed, 1);
  }
  {   // the tile and its halo; positions outside the image hold 0 and are never part of a patch
    uint8_t* ref_b = reinterpret_cast<uint8_t*>(ref_w);
    for (int i = t; i < SROWS * (TW + 2 * HALO); i += kBlock) {
      const int ly = i / (TW + 2 * HALO), lx = i - ly * (TW + 2 * HALO);
      const int yy = y0 - HALO + ly, xx = x0 - HALO + lx;
      uint8_t b = 0;
      if (yy >= 0 && yy < L.ih && xx >= 0 && xx < L.iw) b = ref[(size_t)yy * L.pitch + xx];
      ref_b[ly * SW + lx] = b;
    }
  }
  __syncthreads();
  const bool failed = s_failed != 0;

  // ---- selection, one thread per pixel of the tile ------------------------------------------------------------------------------
  {
    const int ty = t / TW, tx = t - ty * TW;
    const int x = x0 + tx, y = y0 + ty;
    const bool in_img = x < L.iw && y < L.ih;
    bool selected = in_img && x < L.gw && y < L.gh && !failed;
    if (selected && a.mag) {
      const double thres = (double)a.mag_sums[job] / (double)((size_t)L.iw * L.ih) + a.threshold;
      selected = (double)a.mag[(size_t)job * L.n + (size_t)y * L.pitch + x] > thres;
    }
    const bool border = selected && !(x >= r && x <= L.iw - 1 - r && y >= r && y <= L.ih - 1 - r);
    const bool work = selected && !border;
    if (in_img && !work) {
      const size_t at = (size_t)job * L.n + (size_t)y * L.pitch + x;
      a.depth[at] = 0;
      if (a.cost) a.cost[at] = 0;
      if (a.outcome) a.outcome[at] = border ? 2 : 0;
    }
    const unsigned long long bal = __ballot(work), bal_b = __ballot(border);
    if (lane == 0) {
      wave_cnt[wave] = __popcll(bal);
      if (bal_b) atomicAdd(&cnt[2], __popcll(bal_b));
    }
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += wave_cnt[w];
    if (work) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)t;
    __syncthreads();
  }
  int total = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; w++) total += wave_cnt[w];

  // ---- the sweep: one pixel per wave, a lane per hypothesis -----------------------------------------------------------------------
  const bool active = lane < a.n_hyp;
  const int code = active ? (int)a.codes[lane] : 1;
  const float z = (float)code * L.zscale;
  for (int i = wave; i < total; i += kBlock / 64) {
    const int tp = __builtin_amdgcn_readfirstlane((int)list[i]);
    const int ty = tp / TW, tx = tp - ty * TW;
    const int x = x0 + tx, y = y0 + ty;
    int x2[kSweepMaxViews], y2[kSweepMaxViews];
    bool valid = active;
#pragma unroll
    for (int v = 0; v < kSweepMaxViews; v++) {
      x2[v] = 0;
      y2[v] = 0;
      if (v < a.n_views) {
        const float4 p = make_float4((float)x, (float)y, z, 1.0f);
        float o[3], wq;
        warp_table_point<AR>(L, Tm + 12 * v, p, o, wq);
        float u = o[0] * L.fx; u = u / o[2]; u = u + L.cx;
        float vv = o[1] * L.fy; vv = vv / o[2]; vv = vv + L.cy;
        u = u * wq;
        vv = vv * wq;
        int xi = 0, yi = 0;
        bool lands = sweep_round_int(u, xi) && sweep_round_int(vv, yi) && o[2] > 0.f;
        lands = lands && xi >= r && xi <= L.iw - 1 - r && yi >= r && yi <= L.ih - 1 - r;
        if (lands) { x2[v] = xi; y2[v] = yi; }
        valid = valid && lands;
      }
    }
    const unsigned long long V = __ballot(valid);
    int outcome, out_code = 0, out_cost = 0;
    if (__popcll(V) < 3) {
      outcome = 3;
    } else {
      // the cost of a valid hypothesis
      uint32_t cost = 0;
      if (valid) {
#pragma unroll
        for (int dy = -HALO; dy <= HALO; dy++) {
          if (dy >= -r && dy <= r) {
            const int off = (ty + HALO + dy) * SW + (tx + HALO - r);
            uint32_t rlo, rhi;
            sweep_pack(ref_w[off >> 2], ref_w[(off >> 2) + 1], off & 3, r, rlo, rhi);
#pragma unroll
            for (int v = 0; v < kSweepMaxViews; v++) {
              if (v < a.n_views) {
                const uint8_t* view = a.img + (size_t)a.view_slots[job * a.n_views + v] * L.n;
                const uint32_t* row = reinterpret_cast<const uint32_t*>(view + (size_t)(y2[v] + dy) * L.pitch);
                const int at = x2[v] - r, sh = at & 3;
                const uint32_t w0 = row[at >> 2];
                const uint32_t w1 = sh + 2 * r + 1 > 4 ? row[(at >> 2) + 1] : 0u;   // (never a dword the patch does not reach)
                uint32_t vlo, vhi;
                sweep_pack(w0, w1, sh, r, vlo, vhi);
                cost = __builtin_amdgcn_sad_u8(vlo, rlo, cost);
                cost = __builtin_amdgcn_sad_u8(vhi, rhi, cost);
              }
            }
          }
        }
      }
      const int first = __builtin_ctzll(V), last = 63 - __builtin_clzll(V);
      int par = 0;
#pragma unroll
      for (int v = 0; v < kSweepMaxViews; v++)
        if (v < a.n_views) {
          par = max(par, abs(__shfl(x2[v], first) - __shfl(x2[v], last)));
          par = max(par, abs(__shfl(y2[v], first) - __shfl(y2[v], last)));
        }
      par = __builtin_amdgcn_readfirstlane(par);   // (uniform already: the branches below are scalar)
      const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)sweep_wave_min(valid ? (cost << 6) | (uint32_t)lane : 0xFFFFFFFFu));
      const int kw = (int)(key & 63u);
      const long long cw = (long long)(key >> 6);
      if (par < a.min_parallax) {
        outcome = 4;
      } else if (kw == 0 || kw == a.n_hyp - 1 || !((V >> (kw - 1)) & 1ull) || !((V >> (kw + 1)) & 1ull)) {
        outcome = 5;
      } else if (cw > a.poor_limit) {
        outcome = 6;
      } else {
        int dist = 0;
#pragma unroll
        for (int v = 0; v < kSweepMaxViews; v++)
          if (v < a.n_views) {
            dist = max(dist, abs(x2[v] - __shfl(x2[v], kw)));
            dist = max(dist, abs(y2[v] - __shfl(y2[v], kw)));
          }
        const uint32_t c2 = (uint32_t)__builtin_amdgcn_readfirstlane((int)sweep_wave_min(valid && dist >= 2 ? cost : 0xFFFFFFFFu));
        if (c2 == 0xFFFFFFFFu || !(a.uniq_den * cw < a.uniq_num * (long long)c2)) {
          outcome = 7;
        } else {
          outcome = 1;
          out_cost = (int)cw;
          out_code = __shfl(code, kw);
          const long long cm = (long long)__shfl((int)cost, kw - 1), cp = (long long)__shfl((int)cost, kw + 1);
          const long long den = cm - 2 * cw + cp;
          if (a.refine && den != 0) {
            const long long diff = cm > cp ? cm - cp : cp - cm;
            const double f = (double)diff / (double)(2 * den);
            const int n = cm > cp ? kw + 1 : kw - 1;
            const double rho_k = 1.0 / (double)out_code, rho_n = 1.0 / (double)__shfl(code, n);
            double rho = rho_n - rho_k;
            rho = f * rho;
            rho = rho_k + rho;
            const double e = __builtin_rint(1.0 / rho);
            out_code = e < 1.0 ? 1 : (e > 32767.0 ? 32767 : (int)e);
          }
        }
      }
    }
    if (lane == 0) {
      const size_t at = (size_t)job * L.n + (size_t)y * L.pitch + x;
      a.depth[at] = (uint16_t)out_code;
      if (a.cost) a.cost[at] = (uint16_t)out_cost;
      if (a.outcome) a.outcome[at] = (uint8_t)outcome;
      atomicAdd(&cnt[outcome], 1);
      if (outcome == 1) {
        atomicAdd(&sums[0], (unsigned long long)out_cost);
        atomicAdd(&sums[1], (unsigned long long)out_code);
      }
    }
  }
  __syncthreads();
  SweepInfo* info = a.info + job;   // integers: order-independent
  if (t >= 1 && t < 8 && cnt[t]) atomicAdd(&info->n_outcome[t], cnt[t]);
  if (t == 8) {
    int n = 0;
    for (int k = 1; k < 8; k++) n += cnt[k];
    if (n) atomicAdd(&info->n_selected, n);
  }
  if (t == 9 && sums[0]) atomicAdd(reinterpret_cast<unsigned long long*>(&info->sum_cost), sums[0]);
  if (t == 10 && sums[1]) atomicAdd(reinterpret_cast<unsigned long long*>(&info->sum_code), sums[1]);
  if (t == 0 && blockIdx.x == 0) info->status = failed ? a.invalid_status : 0;
}

}  // namespace uwt
