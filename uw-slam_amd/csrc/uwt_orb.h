// uwt_orb.h — internal: the limits, records and launchers of ORB detection and description (uwt_orb_*; include/uwt.h states the
// contract).  The kernels are in uwt_orb_kernels.h, their only launches in uwt_launch_orb.hip; uwt_capi_orb.hip sees this header
// alone.
#pragma once

#include <math.h>

#include "uwt_detect.h"

namespace uwt {

constexpr int kOrbMaxLevels = 8;
constexpr int kOrbPatch = 31;          // the patch a key point's size scales; its radius is 15
constexpr int kOrbMinEdge = 16;        // edge_threshold at least: every read of a key point stays within 15 of it, the Harris block within 4
constexpr int kOrbMaxEdge = 1024;
constexpr int kOrbMaxDim = 16384;      // width and height at most: the pyramid's index arithmetic is 32-bit
constexpr int kOrbMaxFeatures = 65536;
constexpr int kOrbTile = 32;           // score tile along x and y; scores have a one-pixel halo, pixels a four-pixel halo
constexpr int kOrbPixTile = kOrbTile + 8, kOrbScoreTile = kOrbTile + 2;
constexpr int kOrbBlock = 256;
constexpr int kOrbRankBlock = 1024;
constexpr int kOrbDescWaves = 4;       // key points of a describe block: one wave each
constexpr double kOrbHarrisDen = 25.0 * 7140.0 * 7140.0 * 7140.0 * 7140.0;   // exact: 2^8 * 25 * 1785^4

using OrbKeypoint = Keypoint;
struct OrbKept { unsigned long long key; long long H; };   // key: (layer << 40) | (gy << 20) | gx, the contract's order

__host__ __device__ inline long long orb_pow(int base, int level) {
  long long p = 1;
  for (int i = 0; i < level; i++) p *= base;
  return p;
}
// w_l = (w 5^l + 6^l / 2) / 6^l
__host__ __device__ inline int orb_layer_dim(int n, int level) {
  const long long p6 = orb_pow(6, level), p5 = orb_pow(5, level);
  return (int)(((long long)n * p5 + p6 / 2) / p6);
}
// the layer position of a level-0 coordinate: rnd of the inverse scaling, in double (the caller has checked |v| <= 1e6)
__host__ __device__ inline int orb_layer_pos(float v, int level) {
  return (int)floor((double)v * (double)orb_pow(5, level) / (double)orb_pow(6, level) + 0.5);
}
// the range of a key point a caller provides (host lists: uwt_orb_describe_batch; device lists: k_track_predicate) on a w x h frame:
// |x|, |y| <= 1e6, the octave in 0 .. n_levels - 1, the layer position at least `edge` from every border of its layer.  Comparisons
// and orb_layer_pos only, so a NaN fails.
__host__ __device__ inline bool orb_keypoint_ok(float x, float y, int octave, int n_levels, int edge, int w, int h) {
  if (!(fabsf(x) <= 1e6f && fabsf(y) <= 1e6f && octave >= 0 && octave < n_levels)) return false;
  const int gx = orb_layer_pos(x, octave), gy = orb_layer_pos(y, octave);
  return gx >= edge && gx < orb_layer_dim(w, octave) - edge && gy >= edge && gy < orb_layer_dim(h, octave) - edge;
}
// candidates a layer's band holds at most: a strict maximum of its 3 x 3 has no candidate beside it
inline size_t orb_raw_bound(int lw, int lh, int edge) {
  const long long bw = (long long)lw - 2 * edge, bh = (long long)lh - 2 * edge;
  if (bw < 1 || bh < 1) return 0;
  return (size_t)((bw + 1) / 2) * (size_t)((bh + 1) / 2);
}

struct OrbArgs : DetectArgs {   // (desc: n_frames x cap x 32 bytes)
  int n_levels, edge, fast_threshold, upright;
  int kept_stride;               // the sum of the quotas: entries of a frame in kept and keep
  int lw[kOrbMaxLevels], lh[kOrbMaxLevels];
  size_t loff[kOrbMaxLevels];    // layer l >= 1 of a frame within its block of tight layers (layer 0 is the slot's plane)
  size_t layer_stride;           // bytes of a frame's block
  uint8_t* layers;               // n_frames blocks
  int quota[kOrbMaxLevels];
  int raw_cap[kOrbMaxLevels];    // orb_raw_bound: never exceeded
  size_t raw_off[kOrbMaxLevels]; // a layer's candidates within the frame's raw_stride entries
  size_t raw_stride;
  unsigned long long* raw_key;   // n_frames x raw_stride: (gy << 20) | gx, in the order the candidates happened to arrive
  long long* raw_h;              // their Harris measures
  int* raw_count;                // n_frames x kOrbMaxLevels, zero before the score launches
  OrbKept* kept;                 // n_frames x kept_stride: the layers' quota survivors, layer after layer
  unsigned char* keep;           // n_frames x kept_stride: work area of the capacity cut
  const signed char* pattern;    // 256 x (x0, y0, x1, y1)
  int* score_out = nullptr;      // the per-stage entry: the dense score map of frame 0's layer, lw x lh, zero before the launch
  const int* mode = nullptr;     // n_frames, or null: every frame is detected.  Else the frame's path, decided on the device: only a
                                 // frame with kPathDetect runs detection (k_orb_fast, k_orb_rank, k_orb_select return at once for the
                                 // others, whose kp and counts come from k_orb_take_provided)
};

// layers 1 .. n_levels - 1 of every frame of the chunk, one launch
void launch_orb_layers(hipStream_t s, const OrbArgs& a);
// scores, suppression and Harris measures of one layer (a.score_out set: the scores of frame 0 as well)
void launch_orb_fast(hipStream_t s, const OrbArgs& a, int level);
// every layer that has a band, then the quota of each layer and the ordered selection: a.kp (directions (1, 0)), a.counts
void launch_orb_detect(hipStream_t s, const OrbArgs& a);
// directions (unless a.upright) and descriptors of a.kp[f * cap .. + counts[f]); rows: the largest count the batch can hold
void launch_orb_describe(hipStream_t s, const OrbArgs& a, int rows);
// The chunk's frames are jobs j0 .. j0 + n_frames - 1 of a tracking call over n_pairs pairs (take_provided, uwt_detect.h): writes
// a.mode, and for a frame that is not detected its count and the provided records into a.kp.  a.mode must be set.
void launch_orb_take_provided(hipStream_t s, const OrbArgs& a, int j0, int n_pairs, const int* path, const OrbKeypoint* prev_kp,
                              const int* n_prev, int* mode);
// H at n pixels (x, y) of frame 0's layer: the per-stage entry
void launch_orb_harris(hipStream_t s, const OrbArgs& a, int level, const int* xy, int n, long long* out);

}  // namespace uwt
