// uwt_cloud.h — internal: the records and launchers of the RGB-D point-cloud map on the device (Visualizer::AddPointCloudFromRGBD;
// uwt_point_cloud_batch*, uwt_point_cloud_points; include/uwt.h states what the calls compute).  The kernels are in
// uwt_cloud_kernels.h, their only launches in uwt_launch_cloud.hip.
#pragma once

#include <algorithm>

#include "uwt_launch.h"

namespace uwt {

// uwt_cloud_info as the kernels write it
struct CloudInfo {
  int status, n_rows, n_selected, n_points;
  long long offset, written;
};

constexpr int kCloudDense = 0, kCloudTable = 1;   // where a frame's rows come from
constexpr int kCloudMaxBlocks = 2048;             // blocks of one launch at most: a memory-bound pass strides over the rest

// One cloud call over n_frames frames.  A frame's SELECTED rows are rows 0, stride, 2 stride, ... of its table; the frame's selected
// rows are cut into bpf runs of `run` rows (a multiple of kBlock), one block each, walked kBlock rows at a time in order.
struct CloudArgs {
  LevelK L;                  // level 0
  const uint8_t* img;        // slot 0 of the level's image plane
  const uint16_t* depth;     // slot 0 of the level's depth plane, or null: z = 1 (dense source)
  const int* slots;          // n_frames (device): the frame the intensities (and, dense, the depths) are read from
  const float* traj;         // n_frames x 7 (device)
  const float4* tab;         // table source: frame f's rows at tab + f * tab_stride
  size_t tab_stride;
  const int* tab_cnt;        // table source: frame f's row count (device), clamped to 0..n; null: every frame has n rows
  int n;                     // rows per frame: dense gw * gh, an explicit table's n, the capacity of a counted table
  int mode, stride, skip_invalid;
  int bpf, run;              // blocks per frame; selected rows per block
  int* block_counts;         // n_frames x bpf: rows a block keeps (compacting form)
  long long* block_base;     // n_frames x bpf + 1: their exclusive scan, the call's total behind it
  float4* out;               // the cloud: uwt_cloud_point records
  long long cap;             // records `out` holds
  CloudInfo* info;           // n_frames + 1
  int invalid_status, capacity_status;
};

// The cut of a frame's selected rows (those of `rows` rows at most) into blocks: bpf blocks per frame, kCloudMaxBlocks per launch at
// most, `run` rows each, whole turns of kBlock.
inline void cloud_shape(int rows, int stride, int n_frames, int* bpf, int* run) {
  const long long sel = rows > 0 ? (rows - 1) / stride + 1 : 0;
  const long long want = (sel + kBlock - 1) / kBlock;
  const long long b = std::max(1ll, std::min(want, (long long)std::max(1, kCloudMaxBlocks / n_frames)));
  *bpf = (int)b;
  *run = (int)std::max(1ll, ((sel + b - 1) / b + kBlock - 1) / kBlock) * kBlock;
}

// compact = false: k_cloud_write alone, every offset closed-form (tab_cnt null and skip_invalid 0).  compact = true: k_cloud_count,
// k_cloud_scan, k_cloud_write.  Grid (bpf, n_frames).
void launch_cloud(hipStream_t s, const LaunchSel& sel, const CloudArgs& a, int n_frames, bool compact);

}  // namespace uwt
