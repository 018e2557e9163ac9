// uwt_surf.h — internal: the records, limits and launchers of SURF detection and description (uwt_surf_*; include/uwt.h states
// the contract).  The kernels are in uwt_surf_kernels.h, their only launches in uwt_launch_surf.hip; uwt_capi_surf.hip sees this header
// alone.
#pragma once

#include "uwt_detect.h"

namespace uwt {

constexpr int kSurfMaxOctaves = 4;
constexpr int kSurfMaxLayers = 6;      // response layers of an octave at most: n_octave_layers (1..4) + 2
constexpr int kSurfTile = 32;          // grid points of a response tile along x and y; the tile in LDS has a one-point halo
constexpr int kSurfBlock = 256;
constexpr int kSurfSelectBlock = 1024;
constexpr int kSurfDescWaves = 4;      // key points of a describe block: one wave each

using SurfKeypoint = Keypoint;

// the range of a key point a caller provides (host lists: uwt_surf_describe_batch; device lists: k_track_predicate): |x|, |y| <= 1e6,
// 0 < size <= 4096.  Comparisons only, so a NaN fails.
__host__ __device__ inline bool surf_keypoint_ok(float x, float y, float size) {
  return fabsf(x) <= 1e6f && fabsf(y) <= 1e6f && size > 0.f && size <= 4096.f;
}

constexpr int surf_filter_size(int octave, int layer) { return (9 + 6 * layer) << octave; }

// an upper bound on a frame's candidates: a strict maximum of its 3 x 3 has no candidate beside it, so a middle layer holds at most
// ceil(gw / 2) x ceil(gh / 2) of them
inline size_t surf_raw_bound(int w, int h, int n_octaves, int layers) {
  size_t n = 0;
  for (int o = 0; o < n_octaves; o++) n += (size_t)(layers - 2) * (size_t)(((w >> o) + 1) / 2) * (size_t)(((h >> o) + 1) / 2);
  return n < 64 ? 64 : n;
}

struct SurfArgs : DetectArgs {   // (desc: n_frames x cap x 64 floats)
  uint32_t* integral;        // n_frames x (h + 1) x (w + 1)
  double threshold;
  int n_octaves, layers, upright;
  SurfKeypoint* raw;         // n_frames x raw_cap: the refined candidates in the order they happened to arrive
  unsigned long long* raw_key;   // their places in the contract's order: ((octave * 8 + layer) << 40) | (gy << 20) | gx
  int* raw_count;            // n_frames, zero before the response launches
  int raw_cap;               // surf_raw_bound: never exceeded
  unsigned char* keep;       // n_frames x raw_cap: work area of the selection
  const int* mode = nullptr; // n_frames, or null: every frame is detected.  Else the frame's path, decided on the device: only a
                             // frame with kPathDetect runs detection (k_surf_response, k_surf_select return at once for the others)
};

// both passes of the integral image of every frame of the chunk
void launch_surf_integral(hipStream_t s, const SurfArgs& a);
// response + suppression + refinement of every octave that fits, then the ordered selection: a.kp, a.counts
void launch_surf_detect(hipStream_t s, const SurfArgs& a);
// one response layer of frame 0 of the chunk on the octave's (w >> octave) x (h >> octave) grid, NaN where none exists
void launch_surf_response_layer(hipStream_t s, const SurfArgs& a, int octave, int layer, double* out);
// orientation (unless a.upright) and descriptors of a.kp[f * cap .. + counts[f]); rows: the largest count the batch can hold
void launch_surf_describe(hipStream_t s, const SurfArgs& a, int rows);
// The chunk's frames are jobs j0 .. j0 + n_frames - 1 of a tracking call over n_pairs pairs (job j < n_pairs: the previous frame of
// pair j, whose path is path[j]; the others: current frames, always detected): writes a.mode, and for a frame that is not detected
// its count (the provided one, or 0) and the provided records into a.kp.  a.mode must be set.
void launch_surf_take_provided(hipStream_t s, const SurfArgs& a, int j0, int n_pairs, const int* path, const SurfKeypoint* prev_kp,
                               const int* n_prev, int* mode);

}  // namespace uwt
