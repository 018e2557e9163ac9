// uwt_ransac_kernels.h — the kernels of the RANSAC inlier selection (RobustMatcher::ransacTest, src/Tracker.cpp:105-169) under the
// contract stated in include/uwt.h: every floating-point operation here is an IEEE f64 add, subtract, multiply, divide or compare
// (the unit is compiled with -ffp-contract=off and without fast-math), so tests/ransac_ref.py reproduces every bit.
#pragma once

#include "uwt_ransac.h"

namespace uwt {

__device__ __forceinline__ uint32_t ransac_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// the error of one match under F: the larger of the two squared distances to the epipolar lines against t2, as two compares
// (a NaN, 0 / 0, is not an inlier)
__device__ __forceinline__ bool ransac_inlier(const double (&F)[9], const float4 q, const double t2) {
  const double x = (double)q.x, y = (double)q.y, xp = (double)q.z, yp = (double)q.w;
  const double a = F[0] * x + F[1] * y + F[2];
  const double b = F[3] * x + F[4] * y + F[5];
  const double c = F[6] * x + F[7] * y + F[8];
  const double s2 = xp * a + yp * b + c;
  const double d2 = s2 * s2 / (a * a + b * b);
  const double a1 = F[0] * xp + F[3] * yp + F[6];
  const double b1 = F[1] * xp + F[4] * yp + F[7];
  const double c1 = F[2] * xp + F[5] * yp + F[8];
  const double s1 = x * a1 + y * b1 + c1;
  const double d1 = s1 * s1 / (a1 * a1 + b1 * b1);
  return d1 <= t2 && d2 <= t2;
}

__device__ __forceinline__ bool ransac_match_ok(const MatchOut m, int nq, int nt, int kp_cap) {
  return m.query_idx >= 0 && m.query_idx < nq && m.query_idx < kp_cap && m.train_idx >= 0 && m.train_idx < nt && m.train_idx < kp_cap;
}

// grid: x = pair * chunks + chunk of 256 matches.  The (x, y, x', y') of every match in a table of its own: k_ransac reads it
// at addresses that are the same for every lane (scalar loads).  Both key-point sets are records of a.rec_floats floats that begin
// with (x, y): the staged tables (2) or uwt_keypoint (8).  A match with an index outside its key points reads nothing and leaves
// zeros; k_ransac reports the pair.
static __global__ __launch_bounds__(256) void k_ransac_gather(RansacArgs a, int chunks) {
  const int p = blockIdx.x / chunks, i = (blockIdx.x - p * chunks) * 256 + threadIdx.x;
  const int n = a.n_matches[p];
  if (n < 0 || n > a.cap || i >= n) return;
  const MatchOut m = a.matches[(size_t)p * a.cap + i];
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ransac_match_ok(m, a.n_kp_prev[p], a.n_kp_cur[p], a.kp_cap)) {
    const float* u = a.kp_prev + ((size_t)p * a.kp_cap + m.query_idx) * a.rec_floats;
    const float* v = a.kp_cur + ((size_t)p * a.kp_cap + m.train_idx) * a.rec_floats;
    q = make_float4(u[0], u[1], v[0], v[1]);
  }
  a.quads[(size_t)p * a.cap + i] = q;
}

// One block per pair, one hypothesis per lane, in rounds of kRansacBlock hypotheses.  A lane draws its sample, eliminates its
// 8 x 9 matrix — which is indexed by run-time pivots and therefore lives in LDS, element-major (element e of lane t at
// e * kRansacBlock + t: whatever element a lane addresses, its bank is its own) — and counts its inliers over the pair's matches,
// every lane reading the same match at the same time.  After a round, thread 0 replays the contract's sequential selection over
// the round's counts in hypothesis order (only the lanes that beat the best of the round's start can be accepted, so it walks
// those alone); the block stops once the round's end has reached `limit`, so the work past the sequential stop is at most one
// round and the result is the sequential one.  The tail recomputes the mask of the best hypothesis, and writes the kept matches in
// order (the compaction of k_match_filter).
static __global__ __launch_bounds__(kRansacBlock) void k_ransac(RansacArgs a) {
  __shared__ double sM[72 * kRansacBlock];
  __shared__ double sF[9];
  __shared__ int sCnt[kRansacBlock];
  __shared__ unsigned long long sCand[kRansacBlock / 64];
  __shared__ int sWave[kRansacBlock / 64];
  __shared__ int sBest, sBestH, sLimit, sRoundJ;
  constexpr int kWaves = kRansacBlock / 64;
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.n_matches[p];
  const size_t row0 = (size_t)p * a.cap;
  const bool n_bad = n < 0 || n > a.cap;
  int bad = n_bad ? 1 : 0;
  if (!n_bad) {
    const int nq = a.n_kp_prev[p], nt = a.n_kp_cur[p];
    for (int i = tid; i < n; i += kRansacBlock) bad |= ransac_match_ok(a.matches[row0 + i], nq, nt, a.kp_cap) ? 0 : 1;
  }
  bad = __syncthreads_or(bad);
  if (bad || n < kRansacMinSample) {
    if (!n_bad)
      for (int i = tid; i < n; i += kRansacBlock) a.mask[row0 + i] = 0;
    if (tid == 0) {
      RansacInfo r;
      r.status = bad ? a.invalid_status : 0; r.n_inliers = 0; r.best_hypothesis = -1; r.hypotheses_run = 0;
      for (int k = 0; k < 9; k++) r.F[k] = 0.0;
      a.info[p] = r;
      a.counts[p] = 0;
    }
    return;
  }
  const float4* __restrict__ Q = a.quads + row0;
  const int* __restrict__ need = a.need + ransac_need_row(n) - 8;   // need[k], k = 8..n
  const int H = a.max_hypotheses;
  const double t2 = a.t2;
  if (tid == 0) { sBest = 0; sBestH = -1; sLimit = H; }
  __syncthreads();
#define UWT_RM(r, c) sM[((r) * 9 + (c)) * kRansacBlock + tid]
  int run = 0;
  for (int base = 0;; base += kRansacBlock) {
    const int limit = sLimit, best0 = sBest;
    if (base >= limit) {   // the sequential loop has stopped at the first h >= limit behind the last accepted hypothesis
      run = limit > sBestH + 1 ? limit : sBestH + 1;
      break;
    }
    const int h = base + tid;
    int cnt = 0;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; k++) F[k] = 0.0;
    bool valid = h < H;
    if (valid) {
      // the sample: eight distinct indices from (seed, h, n); `taken` stays sorted
      int taken[8];
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const uint32_t u = ransac_mix(a.seed ^ ransac_mix((uint32_t)(8 * h + s)));
        int j = (int)(((unsigned long long)u * (unsigned long long)(uint32_t)(n - s)) >> 32);
#pragma unroll
        for (int e = 0; e < s; e++) j += j >= taken[e] ? 1 : 0;
        const float4 q = Q[j];
        const double x = (double)q.x, y = (double)q.y, xp = (double)q.z, yp = (double)q.w;
        UWT_RM(s, 0) = xp * x; UWT_RM(s, 1) = xp * y; UWT_RM(s, 2) = xp;
        UWT_RM(s, 3) = yp * x; UWT_RM(s, 4) = yp * y; UWT_RM(s, 5) = yp;
        UWT_RM(s, 6) = x; UWT_RM(s, 7) = y; UWT_RM(s, 8) = 1.0;
        int v = j;
#pragma unroll
        for (int e = 0; e < s; e++) {
          const int t = taken[e];
          if (t > v) { taken[e] = v; v = t; }
        }
        taken[s] = v;
      }
      // Gauss-Jordan elimination with full pivoting
      unsigned rused = 0, cused = 0;
      unsigned long long row_of_col = 0;
#pragma unroll 1
      for (int step = 0; step < 8; step++) {
        double best = 0.0;
        int br = -1, bc = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) {
#pragma unroll
          for (int c = 0; c < 9; c++) {
            const double v = __builtin_fabs(UWT_RM(r, c));
            if (!((rused >> r) & 1u) && !((cused >> c) & 1u) && v > best) { best = v; br = r; bc = c; }
          }
        }
        if (br < 0) break;
        if (best == __builtin_huge_val()) { valid = false; break; }
        const double piv = UWT_RM(br, bc);
        double row[9];
#pragma unroll
        for (int c = 0; c < 9; c++) { row[c] = UWT_RM(br, c) / piv; UWT_RM(br, c) = row[c]; }
#pragma unroll 1
        for (int r = 0; r < 8; r++) {
          if (r == br) continue;
          const double g = UWT_RM(r, bc);
#pragma unroll
          for (int c = 0; c < 9; c++) UWT_RM(r, c) = UWT_RM(r, c) - g * row[c];
        }
        rused |= 1u << br; cused |= 1u << bc;
        row_of_col |= (unsigned long long)br << (4 * bc);
      }
      if (valid) {
        const int cs = __ffs((int)(~cused & 0x1ffu)) - 1;
#pragma unroll
        for (int c = 0; c < 9; c++) {
          double f = c == cs ? 1.0 : 0.0;
          if ((cused >> c) & 1u) f = -UWT_RM((int)((row_of_col >> (4 * c)) & 15ull), cs);
          F[c] = f;
        }
      }
    }
    // every lane walks the matches together (an invalid lane scores its zero F and drops the count)
#pragma unroll 4
    for (int i = 0; i < n; i++) cnt += ransac_inlier(F, Q[i], t2) ? 1 : 0;
    if (!valid) cnt = 0;
    sCnt[tid] = cnt;
    const unsigned long long cand = __ballot(cnt > (best0 > 7 ? best0 : 7));
    if (lane == 0) sCand[wv] = cand;
    __syncthreads();
    if (tid == 0) {
      int best = best0, lim = limit, bh = sBestH, rj = -1;
      for (int w = 0; w < kWaves && base + w * 64 < lim; w++) {
        unsigned long long m = sCand[w];
        while (m) {
          const int j = w * 64 + __ffsll((long long)m) - 1;
          m &= m - 1;
          if (base + j >= lim) { m = 0; break; }
          const int c = sCnt[j];
          if (c > best) {
            best = c; bh = base + j; rj = j;
            const int nd = need[c];
            lim = nd < lim ? nd : lim;
          }
        }
      }
      sBest = best; sBestH = bh; sLimit = lim; sRoundJ = rj;
    }
    __syncthreads();
    if (tid == sRoundJ) {
#pragma unroll
      for (int k = 0; k < 9; k++) sF[k] = F[k];
    }
    __syncthreads();
  }
#undef UWT_RM
  // the mask of the best hypothesis and the matches it keeps, in order
  const bool have = sBestH >= 0;
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = have ? sF[k] : 0.0;
  int kept_before = 0;
  for (int i0 = 0; i0 < n; i0 += kRansacBlock) {
    const int i = i0 + tid;
    const bool keep = have && i < n && ransac_inlier(F, Q[i < n ? i : 0], t2);
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) sWave[wv] = __popcll(kept);
    __syncthreads();
    int off = kept_before, total = 0;
    for (int w = 0; w < kWaves; w++) {
      const int c = sWave[w];
      total += c;
      off += w < wv ? c : 0;
    }
    if (i < n) a.mask[row0 + i] = keep ? 1 : 0;
    if (keep) a.good[row0 + off + __popcll(kept & ((1ull << lane) - 1ull))] = a.matches[row0 + i];
    kept_before += total;
    __syncthreads();
  }
  if (tid == 0) {
    RansacInfo r;
    r.status = 0; r.n_inliers = kept_before; r.best_hypothesis = sBestH; r.hypotheses_run = run;
    for (int k = 0; k < 9; k++) r.F[k] = F[k];
    a.info[p] = r;
    a.counts[p] = kept_before;
  }
}

}  // namespace uwt
