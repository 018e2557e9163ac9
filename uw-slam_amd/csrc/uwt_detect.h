// uwt_detect.h — internal: what SURF and ORB detection and description share.  For the kernels: the key-point record and the leading
// fields of a chunk's arguments.  For the host: the driver between "a frame is resident in a slot" and "key points and descriptors are
// where the caller wants them", written once against DetectArgs; a detector hands it the parts of a Detector and nothing else.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <functional>

struct uwt_ctx;
struct uwt_keypoint;

namespace uwt {

struct Keypoint { float x, y, size, response, dir_x, dir_y; int octave, laplacian; };   // uwt_keypoint of include/uwt.h

// the fields the argument blocks of both detectors begin with: a chunk of frames and where its results go
struct DetectArgs {
  const uint8_t* img;        // the level-0 image plane of slot 0
  size_t frame_stride;       // bytes from one slot's plane to the next
  int pitch, w, h;
  const int* slots;          // the chunk's slots (device)
  int n_frames;
  Keypoint* kp;              // n_frames x cap: the key points in contract order
  int* counts;               // n_frames
  int cap;
  void* desc;                // n_frames x cap rows of desc_row bytes, or null
  int desc_row;              // SURF: 64 floats, ORB: 32 bytes
};

// a frame's path in a tracking call (SurfArgs::mode, OrbArgs::mode), decided on the device: detection; the caller's key points; no
// key points
constexpr int kPathDetect = 0, kPathProvided = 1, kPathNone = 2;

// The caller's key points from device memory (k_surf_take_provided, k_orb_take_provided), grid (ceil(cap / 256), n_frames), 256
// threads.  The chunk's frames are jobs j0 .. of a tracking call over n_pairs pairs (job j < n_pairs: the previous frame of pair j, whose
// path is path[j]; the others: current frames, always detected): writes the chunk's modes, and for a frame that is not detected its
// count (the provided one, or 0) and the provided records into a.kp.  A provided count is in 0..cap (k_track_predicate refused the pair
// otherwise).
__device__ __forceinline__ void take_provided(const DetectArgs& a, int j0, int n_pairs, const int* __restrict__ path,
                                              const Keypoint* __restrict__ prev_kp, const int* __restrict__ n_prev, int* __restrict__ mode) {
  const int f = blockIdx.y, j = j0 + f, i = blockIdx.x * 256 + threadIdx.x;
  const int m = j < n_pairs ? path[j] : kPathDetect;
  if (i == 0) mode[f] = m;
  if (m == kPathDetect) return;
  const int n = m == kPathProvided ? min(max(n_prev[j], 0), a.cap) : 0;
  if (i == 0) a.counts[f] = n;
  if (i < n) a.kp[(size_t)f * a.cap + i] = prev_kp[(size_t)j * a.cap + i];
}

// ---- the pure host rules -----------------------------------------------------------------------------------------------------
constexpr size_t kChunkBytes = 256u << 20;   // scratch a chunk of frames may take
constexpr int kMaxChunk = 4096;              // frames of a chunk at most (a launch's grid)

// frames of a chunk: as many as kChunkBytes hold of `per` bytes a frame, one at least
inline int chunk_frames(size_t per, int n_frames) {
  const size_t fit = std::max<size_t>(1, kChunkBytes / per);
  return (int)std::min<size_t>(fit, (size_t)std::min(n_frames, kMaxChunk));
}

// rows a describe launch covers when the caller provides the lists: the largest count of the chunk's nf frames
inline int provided_rows(const int32_t* n_in, int nf) {
  int rows = 0;
  for (int f = 0; f < nf; f++) rows = std::max(rows, n_in[f]);
  return rows;
}

// ---- the driver (uwt_capi_detect.hip) ----------------------------------------------------------------------------------------
// A detector's parts, bound to one call: the closures hold its parameters and its chunk's arguments.
struct Detector {
  std::function<int(const char* what, bool detect)> prepare;   // its parameter check, then the call's geometry (detect: false when the
                                                                // call only describes): sets frame_bytes and rows
  std::function<bool(const uwt_keypoint&)> kp_ok;              // a provided key point is in range; kp_msg: the message when one is not
  const char* kp_msg = "";
  size_t frame_bytes = 0;    // the scratch of a chunk of one frame: its layout's total
  int rows = 0;              // rows a describe launch covers behind detection
  DetectArgs* chunk = nullptr;   // the chunk's arguments (the detector's own block derives from them), filled by begin
  // begin chunk: carve the family's buffer for nf frames (and `extra` bytes behind, *extra_out), send the slot list and what else the
  // chunk needs, enqueue the integral images or the layers
  std::function<int(const int32_t* slots, int nf, size_t extra, unsigned char** extra_out)> begin;
  std::function<int(int f0)> detect;         // enqueue detection of the chunk, whose first frame is f0 of the call
  std::function<void(int rows)> describe;    // enqueue orientation and descriptors (none where the chunk's desc is null)
};
using Deliver = std::function<int(int f0, const DetectArgs& a)>;

void detect_image(const uwt_ctx* c, DetectArgs* a);   // the level-0 plane of the context's slots: img, frame_stride, pitch, w, h
// list, cap, UWT_MATCH_MAX_ROWS, slot range.  Nothing is enqueued when a check fails.
int detect_check(uwt_ctx* c, const char* what, int n_frames, const int32_t* slots, int cap);
// Key points (detected, or the caller's host lists kp_in / n_in: n_frames x cap, described as they are), then orientation and
// descriptors, for n_frames frames in chunks.  The results of a chunk are in its scratch; `deliver` takes them (first frame of the
// chunk, the chunk's arguments) before the next chunk runs.  d is prepared.
int detect_run(uwt_ctx* c, const Detector& d, int n_frames, const int32_t* slots, int cap, const uwt_keypoint* kp_in, const int32_t* n_in,
               bool want_desc, const Deliver& deliver);
// the chunk's results to the caller's device arrays: the counts, and the rows below each frame's count, in 32-bit words (d_desc is not
// written when the chunk has no descriptors); the rows past a count keep what they held, as the header says
int deliver_device(uwt_ctx* c, int f0, const DetectArgs& a, uwt_keypoint* d_kp, void* d_desc, int32_t* d_counts);
// the chunk's results to host memory: only the rows below each frame's count are written
int deliver_host(uwt_ctx* c, int f0, const DetectArgs& a, uwt_keypoint* kp_out, void* desc_out, int32_t* counts_out);
// A public entry, `what` its name: the null checks, detect_check, d.prepare, then by form — host: detection and description to host
// memory (desc_out may be null); device: the same to device memory, the call left on the stream; given: the caller's lists kp_in /
// n_in, each record checked with d.kp_ok, described and returned to host memory (counts_out unused).
enum class DetectForm { host, device, given };
int detect_entry(uwt_ctx* c, const char* what, Detector& d, DetectForm form, int n_frames, const int32_t* slots, int cap,
                 const uwt_keypoint* kp_in, const int32_t* n_in, uwt_keypoint* kp_out, void* desc_out, int32_t* counts_out);
// one frame's chunk for a per-stage entry: the checks, the stream order and d.begin with cap 1 (`extra` bytes behind, *x)
int stage_begin(uwt_ctx* c, const char* what, Detector& d, int32_t slot, bool detect, size_t extra, unsigned char** x);

}  // namespace uwt
