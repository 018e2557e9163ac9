// uwt_launch.h — internal: the launch dispatchers of the heavy kernel templates, one translation unit per family so that the
// library builds in parallel (uwt_launch_residual.hip, uwt_launch_general.hip, uwt_launch_flow.hip, uwt_launch_points.hip; the image
// warp's are in uwt_warpimg.h / uwt_launch_warpimg.hip, the point cloud's in uwt_cloud.h / uwt_launch_cloud.hip).  The metric Jacobian
// mode's instantiations of all four families are in uwt_launch_metric.hip: each dispatcher hands a call with LaunchSel::metric set to
// its twin there before it looks at anything else, so that no reference-mode unit holds a metric kernel.
// A dispatcher picks the instantiation from run-time facts (arithmetic set, depth plane, level width, intrinsics, factors) and
// enqueues it; it reports nothing — the caller checks hipGetLastError().
#pragma once

#include "uwt_kernels.h"

namespace uwt {

struct LaunchSel {
  int arith;           // kArithOpenCV / kArithLegacy (uwt_params::arith)
  bool depth;          // the context has a depth plane
  bool acc64;          // f64 normal-equation sums (uwt_params::accumulate_f64)
  bool compute_only;   // the diagnostic twin (uwt_profile_enable bit 2)
  bool metric;         // uwt_set_jacobian(UWT_JACOBIAN_METRIC): the kernels' ARJ = arith | kJacMetric
};

// A level's rows are pitched to whole groups of four pixels and walked in such groups.  level_ragged: the grid's rows are not
// whole groups (46 wide in rows of 48; every level of an odd-sized frame): the RAGGED instantiations mask the positions of a
// row's last group that lie beyond the point grid (residual_core: colm).
inline bool level_ragged(const LevelK& L) { return L.gw != L.pitch; }
inline bool level_plain(const ResidualArgs& a) { return a.zf == 1.0f && a.af == 1.0f && a.L.fx == a.L.fy; }

// k_residual, identity weights / nearest sampler (and the per-stage dump form)
void launch_residual(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, bool dump);
// the scale pass (weights != 0: k_resid_hist_v) and the weighted / bilinear k_residual of one evaluation (dump: its per-stage dump
// form)
void launch_general(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, int sampler, int weights,
                    unsigned int* hist, PairScale* scale, bool dump);

// The sparse point producers and device-resident tables (uwt_launch_points.hip); the only launches of the producers, for the
// batched calls and the per-stage entries alike.  Frame f of a producer is slot slots[f] (a device list).
// ObtainPatchesPoints for a batch of frames, one block each (k_patch_points_batch), and one evaluation of a batch of tables with the
// update in its tail (k_table_eval; grid a.slices x n_pairs)
void launch_patch_points_batch(hipStream_t s, int n_frames, const float2* kp, const int* n_kp, const int* slots,
                               const uint16_t* depth0, size_t slot_elems, int pitch, int w, int h, float4* out, int stride,
                               int* counts);
void launch_table_eval(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, int n_pairs);
// the same on the general path (uwt_table_options): k_table_hist (weights != 0; the pairs' bins are all-zero before and after), then
// k_table_general with the update in its tail
void launch_table_general(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, const GeneralArgs& ga,
                          int n_pairs);
// gradient_ of one level for a batch of frames (k_grad_mag_slots): frame f's plane at mag + f * L.n, its sum added to sums[f]
// (cleared by the caller)
void launch_grad_mag(hipStream_t s, const LevelK& L, int n_frames, const int* slots, const int16_t* gx, const int16_t* gy, uint8_t* mag,
                     unsigned long long* sums);
// Tracker::ObtainCandidatePoints on one level for a batch of frames: launch_grad_mag, k_candidates_slots<false>, k_scan_counts,
// k_candidates_slots<true>.  w: the producer's work area (candidates_work_layout; its per-frame sums cleared by the caller), frame
// f's table at out + f * gw * gh, its count at counts[f]
struct CandidatesWork {
  unsigned long long* sums;   // n_frames
  uint8_t* mag;               // n_frames x L.n: gradient_
  int* cells;                 // n_frames x gw x bands: the (x, band) counts ...
  int* offsets;               // ... and their exclusive scan
  int bands;                  // row bands per column
};
void launch_candidates_slots(hipStream_t s, const LevelK& L, int n_frames, const int* slots, const int16_t* gx, const int16_t* gy,
                             const uint16_t* depth, double threshold, const CandidatesWork& w, float4* out, int* counts);

// the chained flow of a few pairs: k_iterate, k_coarse (up to kCoarseMaxLevels levels in one launch), k_finish
void launch_iterate(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const IterArgs& ia, int n_pairs);
void launch_coarse_chain(hipStream_t s, const LaunchSel& sel, const CoarseArgs& ca, int n_pairs);
void launch_finish(hipStream_t s, const IterArgs& ia, int n_pairs, float* d_poses, StatsOut* d_stats);
// the chained flow under robust weights: the pending update + the scale pass in one launch (k_hist_iterate); the weighted pass
// behind it is launch_general's second half (launch_weighted)
void launch_hist_iterate(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const IterArgs& ia, int n_pairs, int sampler,
                         int weights, unsigned int* hist, PairScale* scale);
void launch_weighted(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, int sampler, int weights);
// one coarse level of a batch, one block per pair: k_coarse_w4 (identity weights) / k_coarse_weighted
void launch_coarse_level(hipStream_t s, const LaunchSel& sel, const CoarseArgs& ca, int cnt, int weights);

// The metric mode's twins of the dispatchers above that launch a kernel which forms Jw (uwt_launch_metric.hip).  Every one takes the
// general Jacobian form — factors multiplied in, no square-pixel sharing, untyped plane loads — whatever the intrinsics, the factors and
// the plane-load switches of the tuning are: what they choose in reference mode never shows in a result, and the metric Jw has no
// coinciding products to share.  compute_only is ignored (the diagnostic twin is the production kernel's).
namespace metric {
void launch_residual(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, bool dump);
void launch_weighted(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, int sampler, int weights, bool dump);
void launch_iterate(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const IterArgs& ia, int n_pairs);
void launch_coarse_chain(hipStream_t s, const LaunchSel& sel, const CoarseArgs& ca, int n_pairs);
void launch_coarse_level(hipStream_t s, const LaunchSel& sel, const CoarseArgs& ca, int cnt, int weights);
void launch_table_eval(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, int n_pairs);
void launch_table_general(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, const GeneralArgs& ga, int n_pairs);
}  // namespace metric

// runs the statements with AR a compile-time constant
#define UWT_WITH_AR(arith, ...)                                              \
  do {                                                                       \
    if ((arith) == kArithLegacy) { constexpr int AR = kArithLegacy; __VA_ARGS__; }  \
    else { constexpr int AR = kArithOpenCV; __VA_ARGS__; }                   \
  } while (0)
// the same with ARJ = the arithmetic set | kJacMetric
#define UWT_WITH_ARJ_METRIC(arith, ...)                                      \
  do {                                                                       \
    if ((arith) == kArithLegacy) { constexpr int ARJ = kArithLegacy | kJacMetric; __VA_ARGS__; }  \
    else { constexpr int ARJ = kArithOpenCV | kJacMetric; __VA_ARGS__; }     \
  } while (0)

}  // namespace uwt
