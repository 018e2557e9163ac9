// uwt_select.h — internal: the ordered selection SURF and ORB share.  A block of B threads orders n candidates, each with a score and a
// key: candidate i is beaten by candidate j when s_j > s_i || (s_j == s_i && k_j < k_i) (a NaN score beats nothing and is beaten
// by nothing), and what is kept goes to the place its key has among the kept — the output is a function of the SET of candidates
// alone.  The candidates every thread compares its own with pass through LDS in tiles of one per thread (all lanes read the same
// entry).  score(j), key(j), kept(j): callables over 0 <= j < n.  Every thread of the block calls, with the same n.
#pragma once

#include <hip/hip_runtime.h>

namespace uwt {

// the key tile both routines use, one after the other: a kernel that calls both holds it once
template <int B> __device__ __forceinline__ unsigned long long* select_key_tile() {
  __shared__ unsigned long long t_key[B];
  return t_key;
}

// rank: the candidates that beat this thread's own (mine: it has one; its score si and key ki)
template <int B, typename S, typename ScoreOf, typename KeyOf>
__device__ __forceinline__ int select_rank(int n, bool mine, S si, unsigned long long ki, ScoreOf score, KeyOf key) {
  __shared__ S t_score[B];   // (S: float for SURF's responses, long long for ORB's Harris measures)
  unsigned long long* t_key = select_key_tile<B>();
  const int tid = threadIdx.x;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += B) {
    __syncthreads();
    if (j0 + tid < n) {
      t_key[tid] = key(j0 + tid);
      t_score[tid] = score(j0 + tid);
    }
    __syncthreads();
    const int m = min(B, n - j0);
    if (mine)
      for (int q = 0; q < m; q++) rank += (t_score[q] > si || (t_score[q] == si && t_key[q] < ki)) ? 1 : 0;
  }
  return rank;
}

// place: the kept candidates whose key is below this thread's own
template <int B, typename KeptOf, typename KeyOf>
__device__ __forceinline__ int select_place(int n, bool mine, unsigned long long ki, KeptOf kept, KeyOf key) {
  __shared__ unsigned char t_keep[B];
  unsigned long long* t_key = select_key_tile<B>();
  const int tid = threadIdx.x;
  int pos = 0;
  for (int j0 = 0; j0 < n; j0 += B) {
    __syncthreads();   // (also: what kept() reads of the other threads' writes before the call has been written)
    if (j0 + tid < n) {
      t_key[tid] = key(j0 + tid);
      t_keep[tid] = kept(j0 + tid);
    }
    __syncthreads();
    const int m = min(B, n - j0);
    if (mine)
      for (int q = 0; q < m; q++) pos += (t_keep[q] && t_key[q] < ki) ? 1 : 0;
  }
  return pos;
}

// The capacity cut and the order of a frame: more than cap candidates keep the cap first by rank (keep[]: n bytes of work area),
// then emit(i, pos) for every kept candidate i, pos < cap its place.  Returns the count kept.
template <int B, typename ScoreOf, typename KeyOf, typename Emit>
__device__ __forceinline__ int select_ordered(int n, int cap, unsigned char* keep, ScoreOf score, KeyOf key, Emit emit) {
  const int tid = threadIdx.x;
  const bool over = n > cap;
  if (over) {
    for (int i0 = 0; i0 < n; i0 += B) {
      const int i = i0 + tid;
      const bool mine = i < n;
      const int rank = select_rank<B>(n, mine, mine ? score(i) : decltype(score(0))(), mine ? key(i) : 0ull, score, key);
      if (mine) keep[i] = rank < cap ? 1 : 0;
    }
  }
  for (int i0 = 0; i0 < n; i0 += B) {
    const int i = i0 + tid;
    const bool mine = i < n && (!over || keep[i]);   // (keep[i] is this thread's own write)
    const int pos = select_place<B>(n, mine, mine ? key(i) : 0ull, [&](int j) { return over ? keep[j] : (unsigned char)1; }, key);
    if (mine && pos < cap) emit(i, pos);
  }
  return over ? cap : n;
}

}  // namespace uwt
