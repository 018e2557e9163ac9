// uwt_cloud_kernels.h — gfx950 kernels of the RGB-D point-cloud map: Visualizer::AddPointCloudFromRGBD (src/Visualizer.cpp:421-446)
// for a batch of frames, the cloud one array of 16-byte records in frame order and, inside a frame, in row order.
//
//   k_cloud_count   per block the number of selected rows it keeps (wave-64 ballot + popcount, folded through LDS)
//   k_cloud_scan    one block: the exclusive scan of those counts over frames x blocks, the call's total behind it
//   k_cloud_write   the points: the predicate again, a lane's rank from the ballot mask below it, the wave's base from LDS, the
//                   block's base from the scan (or closed-form), one 16-byte store per point; block 0 of a frame writes its record
//
// Where a record goes is a function of the counts alone: no cursor is advanced with an atomic and no float is added with one, so
// neither the order of the records nor a bit of them depends on how the blocks were scheduled.  When every selected row is emitted
// and the row counts are known on the host (skip_invalid 0, dense or explicit rows) the offsets are closed-form — frame f starts
// ceil(N / stride) records behind every earlier frame with a finite pose — and k_cloud_write runs alone.
#pragma once

#include "uwt_cloud.h"

namespace uwt {

constexpr int kCloudWaves = kBlock / 64;

__device__ __forceinline__ bool cloud_pose_finite(const float* __restrict__ q) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 7; k++) ok = ok && (__builtin_fabsf(q[k]) < __builtin_inff());
  return ok;
}

// rows of frame f's table (a counted table's count lives on the device; outside 0..n it is clamped)
template <int SRC>
__device__ __forceinline__ int cloud_rows(const CloudArgs& a, int f) {
  if constexpr (SRC == kCloudTable) {
    if (a.tab_cnt) return min(max(a.tab_cnt[f], 0), a.n);
  }
  return a.n;
}

// selected rows of a table of `rows` rows: i = 0, stride, 2 stride, ... < rows
__device__ __forceinline__ int cloud_selected(int rows, int stride) { return rows > 0 ? (rows - 1) / stride + 1 : 0; }

// Row i (< rows) of frame f.  Dense: point (x, y) = (i - y gw, i / gw) of ObtainAllPoints' grid (src/Tracker.cpp:1266-1302: z = depth *
// zscale, a point whose depth read as int16 is <= 0 becomes [0 0 1 0], z = 1 without a depth plane) — the table is never built.
template <int SRC>
__device__ __forceinline__ float4 cloud_row(const CloudArgs& a, int f, int slot, int i) {
  if constexpr (SRC == kCloudDense) {
    const LevelK& L = a.L;
    const int y = i / L.gw, x = i - y * L.gw;
    float4 p = make_float4((float)x, (float)y, 1.0f, 1.0f);
    if (a.depth) {
      const int d = (int)(int16_t)a.depth[(size_t)slot * L.n + (size_t)y * L.pitch + x];   // at<short> (:1272)
      if (d > 0) p.z = (float)d * L.zscale;
      else p = make_float4(0.f, 0.f, 1.0f, 0.f);
    }
    return p;
  } else {
    return a.tab[(size_t)f * a.tab_stride + i];
  }
}

// image[(int)y][(int)x] of the frame's level-0 image (truncation toward zero: -0.5 reads column 0); 0 outside it or for a coordinate
// that is not a number
__device__ __forceinline__ uint32_t cloud_intensity(const CloudArgs& a, int slot, const float4 p) {
  const LevelK& L = a.L;
  if (!(p.x > -1.0f && p.x < (float)L.iw && p.y > -1.0f && p.y < (float)L.ih)) return 0u;
  return a.img[(size_t)slot * L.n + (size_t)(int)p.y * L.pitch + (int)p.x];
}

// One record.  The unprojection is warp_table_point's (pixel_ray, then * z, in f32).  mode 0: (-X - tx, -Z - tz, -Y - ty) with the
// pose's translation unpermuted (src/Visualizer.cpp:440-442).  mode 1: the first three rows of T [X Y Z w] by the f64 row product of
// the OpenCV set, in BOTH arithmetic sets.
template <int AR>
__device__ __forceinline__ float4 cloud_point(const CloudArgs& a, const float* q, const float4 p, uint32_t tag) {
  const LevelK& L = a.L;
  float X = pixel_ray<AR, float>(p.x, L.cx, L.invfx, L.bx);
  float Y = pixel_ray<AR, float>(p.y, L.cy, L.invfy, L.by);
  X = X * p.z;
  Y = Y * p.z;
  float4 o;
  if (a.mode == 0) {
    o.x = (-X) - q[4];
    o.y = (-p.z) - q[6];
    o.z = (-Y) - q[5];
  } else {
    Pose pose;
    for (int k = 0; k < 4; k++) pose.q[k] = q[k];
    for (int k = 0; k < 3; k++) pose.t[k] = q[4 + k];
    float T[12];
    pose_to_T12(pose, T);
    const double Xd = (double)X, Yd = (double)Y, zd = (double)p.z, wd = (double)p.w;
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double Td[4] = {(double)T[4 * k], (double)T[4 * k + 1], (double)T[4 * k + 2], (double)T[4 * k + 3]};
      r[k] = rigid_row_f64(Td, Xd, Yd, zd, wd);
    }
    o.x = r[0]; o.y = r[1]; o.z = r[2];
  }
  o.w = __uint_as_float(tag);
  return o;
}

// Grid (bpf, n_frames).  Block b of frame f owns the selected rows b * run .. (b + 1) * run - 1 that exist; a frame whose pose is not
// finite has none.
template <int SRC>
__global__ __launch_bounds__(kBlock) void k_cloud_count(const CloudArgs a) {
  __shared__ int wave_n[kCloudWaves];
  const int f = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows = cloud_pose_finite(a.traj + 7 * (size_t)f) ? cloud_rows<SRC>(a, f) : 0;
  const long long n_sel = cloud_selected(rows, a.stride);
  const long long s0 = (long long)b * a.run, s1 = min(s0 + a.run, n_sel);
  const int slot = a.slots[f];
  int kept = 0;   // of this wave
  for (long long sb = s0; sb < s1; sb += kBlock) {
    const long long sel = sb + threadIdx.x;
    bool keep = sel < s1;
    if (keep && a.skip_invalid) keep = !(cloud_row<SRC>(a, f, slot, (int)(sel * a.stride)).w == 0.f);
    kept += __popcll(__ballot(keep));
  }
  if (lane == 0) wave_n[wave] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int k = 0; k < kCloudWaves; k++) total += wave_n[k];
    a.block_counts[(size_t)f * a.bpf + b] = total;
  }
}

// One block: base[i] = counts[0] + ... + counts[i - 1] for i = 0..m (base[m]: the total).  Every thread sums a run of counts, a
// Hillis-Steele scan over the kBlock run sums, then every thread replays its run behind its prefix.
static __global__ __launch_bounds__(kBlock) void k_cloud_scan(const int* __restrict__ counts, long long* __restrict__ base, int m) {
  __shared__ long long part[kBlock];
  const int t = threadIdx.x, per = (m + kBlock - 1) / kBlock, i0 = min(t * per, m), i1 = min(i0 + per, m);
  long long s = 0;
  for (int i = i0; i < i1; i++) s += counts[i];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const long long v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long long at = part[t] - s;
  for (int i = i0; i < i1; i++) {
    base[i] = at;
    at += counts[i];
  }
  if (t == kBlock - 1) base[m] = part[t];
}

// Grid (bpf, n_frames).  COMPACT: the block's first record is block_base[f bpf + b].  Else every selected row is emitted and a frame
// with a finite pose holds ceil(n / stride) records: the block counts the finite poses ahead of its frame.
template <int AR, int SRC, bool COMPACT>
__global__ __launch_bounds__(kBlock) void k_cloud_write(const CloudArgs a) {
  __shared__ int wave_n[kCloudWaves];
  __shared__ int s_before;
  const int f = blockIdx.y, b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float q[7];
#pragma unroll
  for (int k = 0; k < 7; k++) q[k] = a.traj[7 * (size_t)f + k];
  const bool pose_ok = cloud_pose_finite(q);
  const int rows = pose_ok ? cloud_rows<SRC>(a, f) : 0;
  const long long n_sel = cloud_selected(rows, a.stride);
  const long long s0 = (long long)b * a.run, s1 = min(s0 + a.run, n_sel);
  long long frame_base, n_points;
  if constexpr (COMPACT) {
    frame_base = a.block_base[(size_t)f * a.bpf];
    n_points = a.block_base[(size_t)(f + 1) * a.bpf] - frame_base;
  } else {
    if (threadIdx.x == 0) s_before = 0;
    __syncthreads();
    int cnt = 0;
    for (int g = threadIdx.x; g < f; g += kBlock) cnt += cloud_pose_finite(a.traj + 7 * (size_t)g) ? 1 : 0;
    if (cnt) atomicAdd(&s_before, cnt);   // an integer sum in LDS: the same whatever the order
    __syncthreads();
    frame_base = (long long)s_before * cloud_selected(a.n, a.stride);
    n_points = n_sel;
  }
  if (b == 0 && threadIdx.x == 0) {
    CloudInfo r;
    r.status = pose_ok ? 0 : a.invalid_status;
    r.n_rows = rows;
    r.n_selected = (int)n_sel;
    r.n_points = (int)n_points;
    r.offset = frame_base;
    r.written = min(max(a.cap - frame_base, 0ll), n_points);
    a.info[f] = r;
    if (f == (int)gridDim.y - 1) {   // the call's record
      const long long total = frame_base + n_points;
      r.status = total > a.cap ? a.capacity_status : 0;
      r.n_rows = (int)gridDim.y;
      r.n_selected = 0;
      r.n_points = 0;
      r.offset = total;
      r.written = min(total, a.cap);
      a.info[gridDim.y] = r;
    }
  }
  const int slot = a.slots[f];
  long long at;   // the record of the block's next kept row
  if constexpr (COMPACT) at = a.block_base[(size_t)f * a.bpf + b];
  else at = frame_base + s0;
  for (long long sb = s0; sb < s1; sb += kBlock) {   // (the bounds are the block's: every thread takes every turn)
    const long long sel = sb + threadIdx.x;
    bool keep = sel < s1;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (keep) {
      p = cloud_row<SRC>(a, f, slot, (int)(sel * a.stride));
      if (a.skip_invalid && p.w == 0.f) keep = false;
    }
    long long idx;
    if constexpr (COMPACT) {
      const unsigned long long m = __ballot(keep);
      const int rank = __popcll(m & ((1ull << lane) - 1ull));   // kept rows of this wave below this lane
      if (lane == 0) wave_n[wave] = __popcll(m);
      __syncthreads();
      int below = 0, all = 0;
#pragma unroll
      for (int k = 0; k < kCloudWaves; k++) {
        const int c = wave_n[k];
        if (k < wave) below += c;
        all += c;
      }
      __syncthreads();   // wave_n is written again on the next turn
      idx = at + below + rank;
      at += all;
    } else {
      idx = at + threadIdx.x;
      at += kBlock;
    }
    if (keep && idx < a.cap) {
      const uint32_t tag = cloud_intensity(a, slot, p) | ((uint32_t)f << 8);
      a.out[idx] = cloud_point<AR>(a, q, p, tag);   // one 16-byte store
    }
  }
}

}  // namespace uwt
