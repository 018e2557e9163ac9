// uwt_match.h — internal: the records, limits and launchers of descriptor matching (uwt_knn_match_batch,
// uwt_match_descriptors_batch*; include/uwt.h).  The kernels are in uwt_match_kernels.h, their only launches in
// uwt_launch_match.hip; uwt_capi_match.hip sees this header alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uwt {

constexpr int kMatchL2 = 0, kMatchHamming = 1;   // uwt_norm
constexpr int kMatchTile = 64;         // rows of a query tile and of a train tile: 16 x 16 threads, 4 x 4 elements each
constexpr int kMatchMaxRows = 4096;    // descriptors of a set at most (cap)
constexpr int kMatchMaxWords = 128;    // 32-bit words of a descriptor at most: 128 floats (SURF extended), 512 bytes
constexpr int kMatchMaxSplits = 16;    // parts the train rows of one (pair, query tile, direction) are cut into at most
constexpr int kMatchTargetBlocks = 1024;   // blocks the split aims at: four per CU

// a row's two nearest neighbours.  In the partial records of k_knn2 an absent neighbour is (+inf, INT_MAX): the largest key; in
// the records a caller sees (uwt_knn2) it is idx = -1, d = 0.
struct Knn2 { int idx0, idx1; float d0, d1; };
struct MatchOut { int query_idx, train_idx; float distance; };

struct MatchArgs {
  const uint32_t* desc[2];   // [0] the query sets, [1] the train sets: n_pairs x cap rows of `words` 32-bit words
  const int* cnt[2];         // rows of each pair's sets
  int cap, words, n_pairs;
  int splits;                // parts of the train rows; part s of pair p, direction d at part + (((d * n_pairs) + p) * splits + s) * cap
  Knn2* part;
};

// k_knn2: direction 0 (query -> train) alone (dirs = 1) or both (dirs = 2), rows: the largest count of the batch
void launch_knn2(hipStream_t s, int norm, const MatchArgs& a, int dirs, int rows);
// the parts of direction 0 merged into the caller's records: pair p's row i at out[p * cap + i]
void launch_knn2_merge(hipStream_t s, const MatchArgs& a, int rows, Knn2* out);
// ratio test of both directions, symmetry test, ordered compaction: pair p's matches at out[p * cap ...], their number at counts[p]
void launch_match_filter(hipStream_t s, const MatchArgs& a, float ratio, MatchOut* out, int* counts);

}  // namespace uwt
