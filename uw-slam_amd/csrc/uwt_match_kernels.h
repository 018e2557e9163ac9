// uwt_match_kernels.h — gfx950 kernels of descriptor matching: cv::DescriptorMatcher::knnMatch(query, train, 2) of the brute-force
// L2 / Hamming matchers in both directions, RobustMatcher::ratioTest and ::symmetryTest (src/Tracker.cpp:52-102, 202-236).
//
//   k_knn2<NORM>      all-pairs distances of a 64 x 64 tile per step, the two nearest train rows of every query row
//   k_knn2_merge      the parts of a row's train range folded into the caller's record (uwt_knn_match_batch)
//   k_match_filter    ratio test both ways, symmetry as a lookup, matches written in ascending query order
//
// The arithmetic contract (include/uwt.h): dist(i, j) = sqrtf(s), s = s + d * d over k in order, d = a[k] - b[k], all f32 and no
// FMA (-ffp-contract=off); or the popcount of the XOR as a float.  What is free is everything but the order of one element's
// additions, so a thread owns a 4 x 4 block of (i, j) elements, each with its own sequential s: sixteen independent chains, two
// per packed f32 instruction (v_pk_add_f32 / v_pk_mul_f32: exact per half, twice the rate of the scalar forms).  No matrix cores:
// the |a|^2 + |b|^2 - 2ab expansion is a different function.  (a - b)^2 = (b - a)^2 exactly, so the swapped direction sees the
// same bits.
// The 2-NN under "lowest index wins" is the two smallest keys (dist, j) in lexicographic order: associative and commutative, so
// the in-thread scan (ascending j, strict <), the merge across the 16 threads of a row and the merge across the parts of the
// train range give the same records in any grouping.
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "uwt_match.h"

namespace uwt {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr float kMatchInf = __builtin_inff();

// the running pair under a scan in ascending j: a tie leaves the earlier (lower) index in place
__device__ __forceinline__ void knn2_push(float d, int j, float& d0, int& j0, float& d1, int& j1) {
  const bool c1 = d < d1, c0 = d < d0;
  d1 = c0 ? d0 : (c1 ? d : d1);
  j1 = c0 ? j0 : (c1 ? j : j1);
  d0 = c0 ? d : d0;
  j0 = c0 ? j : j0;
}

__device__ __forceinline__ bool knn2_key_lt(float d, int j, float e, int k) { return (d < e) | ((d == e) & (j < k)); }

// the same in any order of arrival: keys compared whole
__device__ __forceinline__ void knn2_insert(float d, int j, float& d0, int& j0, float& d1, int& j1) {
  const bool c1 = knn2_key_lt(d, j, d1, j1), c0 = knn2_key_lt(d, j, d0, j0);
  d1 = c0 ? d0 : (c1 ? d : d1);
  j1 = c0 ? j0 : (c1 ? j : j1);
  d0 = c0 ? d : d0;
  j0 = c0 ? j : j0;
}

// 64 rows of a set from row0 on into the k-major LDS image dst[k][64] (a thread's four rows of one k are 16 contiguous bytes: one
// ds_read_b128, and the 16 threads of a wave that differ in their rows cover one 256-byte bank row).  Rows past the set are zeros.
// A lane takes 16 bytes of its own row, so the 64 lanes of a wave write 64 consecutive words per k: no bank conflict.
__device__ __forceinline__ void match_stage_tile(uint32_t* __restrict__ dst, const uint32_t* __restrict__ set, int row0, int rows, int W,
                                                 int tid) {
  if ((W & 3) == 0) {
    const int n4 = kMatchTile * (W >> 2);
    for (int e = tid; e < n4; e += 256) {
      const int r = e & (kMatchTile - 1), kq = e >> 6, row = row0 + r;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row < rows) v = *reinterpret_cast<const uint4*>(set + (size_t)row * W + kq * 4);
      uint32_t* d = dst + kq * 4 * kMatchTile + r;
      d[0] = v.x; d[kMatchTile] = v.y; d[2 * kMatchTile] = v.z; d[3 * kMatchTile] = v.w;
    }
  } else {   // Hamming rows that are not whole groups of 16 bytes
    const int n1 = kMatchTile * W;
    for (int e = tid; e < n1; e += 256) {
      const int r = e & (kMatchTile - 1), k = e >> 6, row = row0 + r;
      dst[k * kMatchTile + r] = row < rows ? set[(size_t)row * W + k] : 0u;
    }
  }
}

// grid: x = pair * tiles + query tile, z = direction * splits + part of the train range.  Direction 0 matches set 0 (query)
// against set 1 (train), direction 1 the reverse.  Dynamic LDS: 2 x W x 64 words.
template <int NORM>
__global__ __launch_bounds__(256) void k_knn2(MatchArgs a, int tiles) {
  extern __shared__ __attribute__((aligned(16))) uint32_t match_lds[];
  const int W = a.words;
  uint32_t* sA = match_lds;
  uint32_t* sB = match_lds + W * kMatchTile;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int dir = blockIdx.z / a.splits, sp = blockIdx.z - dir * a.splits;
  const int p = blockIdx.x / tiles, q0 = (blockIdx.x - p * tiles) * kMatchTile;
  const int n = (dir ? a.cnt[1] : a.cnt[0])[p], m = (dir ? a.cnt[0] : a.cnt[1])[p];
  if (q0 >= n) return;
  const size_t set_off = (size_t)p * a.cap * W;
  const uint32_t* A = (dir ? a.desc[1] : a.desc[0]) + set_off;
  const uint32_t* B = (dir ? a.desc[0] : a.desc[1]) + set_off;
  const int nt = (m + kMatchTile - 1) / kMatchTile, per = (nt + a.splits - 1) / a.splits;
  const int t_begin = sp * per, t_end = min(nt, t_begin + per);

  float d0[4], d1[4];
  int j0[4], j1[4];
#pragma unroll
  for (int r = 0; r < 4; r++) { d0[r] = d1[r] = kMatchInf; j0[r] = j1[r] = INT_MAX; }

  if (t_begin < t_end) match_stage_tile(sA, A, q0, n, W, tid);
  for (int t = t_begin; t < t_end; t++) {
    __syncthreads();   // the last tile's reads are done
    match_stage_tile(sB, B, t * kMatchTile, m, W, tid);
    __syncthreads();
    float dist[4][4];
    if (NORM == kMatchL2) {
      f32x2 acc[4][2];
#pragma unroll
      for (int r = 0; r < 4; r++) { acc[r][0] = f32x2{0.f, 0.f}; acc[r][1] = f32x2{0.f, 0.f}; }
#pragma unroll 4
      for (int k = 0; k < W; k++) {
        const uint4 au = *reinterpret_cast<const uint4*>(sA + k * kMatchTile + ty * 4);
        const uint4 bu = *reinterpret_cast<const uint4*>(sB + k * kMatchTile + tx * 4);
        const float av[4] = {__uint_as_float(au.x), __uint_as_float(au.y), __uint_as_float(au.z), __uint_as_float(au.w)};
        const f32x2 blo = {__uint_as_float(bu.x), __uint_as_float(bu.y)};
        const f32x2 bhi = {__uint_as_float(bu.z), __uint_as_float(bu.w)};
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const f32x2 ar = {av[r], av[r]};
          const f32x2 e0 = ar - blo, e1 = ar - bhi;
          acc[r][0] = acc[r][0] + e0 * e0;
          acc[r][1] = acc[r][1] + e1 * e1;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        dist[r][0] = sqrtf(acc[r][0].x); dist[r][1] = sqrtf(acc[r][0].y);
        dist[r][2] = sqrtf(acc[r][1].x); dist[r][3] = sqrtf(acc[r][1].y);
      }
    } else {
      uint32_t acc[4][4];
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0u;
#pragma unroll 4
      for (int k = 0; k < W; k++) {
        const uint4 au = *reinterpret_cast<const uint4*>(sA + k * kMatchTile + ty * 4);
        const uint4 bu = *reinterpret_cast<const uint4*>(sB + k * kMatchTile + tx * 4);
        const uint32_t av[4] = {au.x, au.y, au.z, au.w}, bv[4] = {bu.x, bu.y, bu.z, bu.w};
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
          for (int c = 0; c < 4; c++) acc[r][c] += (uint32_t)__builtin_popcount(av[r] ^ bv[c]);
      }
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) dist[r][c] = (float)acc[r][c];
    }
    // the ragged edge: a column past the train set is +inf, which the strict < never takes
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int j = t * kMatchTile + tx * 4 + c;
      const bool in = j < m;
#pragma unroll
      for (int r = 0; r < 4; r++) knn2_push(in ? dist[r][c] : kMatchInf, j, d0[r], j0[r], d1[r], j1[r]);
    }
  }
  // the 16 threads of a row are 16 consecutive lanes of one wave
#pragma unroll
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int mask = 1; mask < 16; mask <<= 1) {
      const float e0 = __shfl_xor(d0[r], mask), e1 = __shfl_xor(d1[r], mask);
      const int k0 = __shfl_xor(j0[r], mask), k1 = __shfl_xor(j1[r], mask);
      knn2_insert(e0, k0, d0[r], j0[r], d1[r], j1[r]);
      knn2_insert(e1, k1, d0[r], j0[r], d1[r], j1[r]);
    }
    const int row = q0 + ty * 4 + r;
    if (tx == 0 && row < n) {
      Knn2 rec;
      rec.idx0 = j0[r]; rec.idx1 = j1[r]; rec.d0 = d0[r]; rec.d1 = d1[r];
      a.part[((size_t)(dir * a.n_pairs + p) * a.splits + sp) * a.cap + row] = rec;
    }
  }
}

// a row's record over the whole train range, in the caller's form (an absent neighbour: idx = -1, d = 0)
__device__ __forceinline__ Knn2 knn2_merged(const MatchArgs& a, int dir, int p, int row) {
  const Knn2* q = a.part + (size_t)(dir * a.n_pairs + p) * a.splits * a.cap + row;
  Knn2 r = q[0];
  for (int s = 1; s < a.splits; s++) {
    const Knn2 t = q[(size_t)s * a.cap];
    knn2_insert(t.d0, t.idx0, r.d0, r.idx0, r.d1, r.idx1);
    knn2_insert(t.d1, t.idx1, r.d0, r.idx0, r.d1, r.idx1);
  }
  if (r.idx0 == INT_MAX) { r.idx0 = -1; r.d0 = 0.f; }
  if (r.idx1 == INT_MAX) { r.idx1 = -1; r.d1 = 0.f; }
  return r;
}

// RobustMatcher::ratioTest (src/Tracker.cpp:52-72): a row with two neighbours is removed when d0 / d1 > ratio — the negated form
// keeps the row whose two nearest are both at distance 0 (0 / 0 is NaN), as the reference does
__device__ __forceinline__ bool knn2_survives(const Knn2& r, float ratio) { return r.idx1 >= 0 && !(r.d0 / r.d1 > ratio); }

// grid: x = pair * chunks + chunk of 256 rows
static __global__ __launch_bounds__(256) void k_knn2_merge(MatchArgs a, int chunks, Knn2* __restrict__ out) {
  const int p = blockIdx.x / chunks, i = (blockIdx.x - p * chunks) * 256 + threadIdx.x;
  if (i < a.cnt[0][p]) out[(size_t)p * a.cap + i] = knn2_merged(a, 0, p, i);
}

// One block of 1024 threads per pair, the query rows in chunks of 1024 in order (cap <= kMatchMaxRows: four chunks at most).  A
// row is kept when it survives the ratio test, the train row it points to survives it in the other direction, and that row
// points back (RobustMatcher::symmetryTest, src/Tracker.cpp:74-102, as a lookup).  Ordered compaction: the kept rows of a wave
// by ballot, the waves of a chunk by their counts in LDS, the chunks by the running base.
static __global__ __launch_bounds__(1024) void k_match_filter(MatchArgs a, float ratio, MatchOut* __restrict__ out, int* __restrict__ counts) {
  __shared__ int wave_kept[16];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = a.cnt[0][p];
  int base = 0;
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + tid;
    bool keep = false;
    Knn2 f = {};
    if (i < n) {
      f = knn2_merged(a, 0, p, i);
      if (knn2_survives(f, ratio)) {
        const Knn2 b = knn2_merged(a, 1, p, f.idx0);
        keep = knn2_survives(b, ratio) && b.idx0 == i;
      }
    }
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) wave_kept[wv] = __popcll(kept);
    __syncthreads();
    int off = base, total = 0;
    for (int w = 0; w < 16; w++) {
      const int c = wave_kept[w];
      total += c;
      off += w < wv ? c : 0;
    }
    if (keep) {
      MatchOut mo;
      mo.query_idx = i; mo.train_idx = f.idx0; mo.distance = f.d0;
      out[(size_t)p * a.cap + off + __popcll(kept & ((1ull << lane) - 1ull))] = mo;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) counts[p] = base;
}

}  // namespace uwt
