// uwt_launch_metric.hip — dispatch of every kernel that forms Jw in the metric Jacobian mode (uwt.h: UWT_JACOBIAN_METRIC; jw_terms<METRIC>):
// the twins of launch_residual, launch_weighted (and its dump form), launch_iterate, launch_coarse_chain, launch_coarse_level,
// launch_table_eval and launch_table_general.  The mode is bit 1 of the kernels' arithmetic argument (kJacMetric), so these are
// instantiations of their own and the reference-mode ones are not touched.
//
// One shape of Jacobian: the general form (UNIT_FACTORS = false, SQUARE = false) — the contract multiplies the factors in always and
// the metric Jw has no coinciding products for square pixels.  Plain plane loads (no typed twin; a streamed one on the main path only).  Where the reference
// mode keeps a whole-row and a RAGGED instantiation, the metric mode keeps both only on its main path (f64 sums, identity weights,
// nearest sampler: k_residual and k_iterate); everything else takes the RAGGED one (or, in k_coarse, the one that decides per level), whose mask is a no-op on whole rows.  None of
// these choices shows in a result: the sums are folded the same way in every form (DESIGN.md "the metric Jacobian").
#include "uwt_launch.h"

namespace uwt {
namespace metric {
namespace {

template <int ARJ, bool DEPTH, bool DUMP>
void residual_t(hipStream_t s, const ResidualArgs& a, int n_pairs, bool acc64) {
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  if constexpr (!DUMP) {
    if (acc64 && !level_ragged(a.L)) {   // the main path on whole rows, and its streamed twin for a batch whose planes exceed the caches
      if (a.stream_planes) hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double, false, 0, 0, false, kLoadsStream>), grid, blk, 0, s, a);
      else hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double>), grid, blk, 0, s, a);
      return;
    }
  }
  if (acc64) hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double, false, 0, 0, false, 0, true>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, float, false, 0, 0, false, 0, true>), grid, blk, 0, s, a);
}

// the weighted / bilinear sums (f64 whatever accumulate_f64 says, as in reference mode) and their per-stage dump form
template <int ARJ, bool DEPTH, bool DUMP>
void weighted_t(hipStream_t s, const ResidualArgs& a, int n_pairs, int sampler, int weights) {
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  switch (sampler * 3 + weights) {
    case 1: hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double, false, 0, 1, false, 0, true>), grid, blk, 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double, false, 0, 2, false, 0, true>), grid, blk, 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double, false, 1, 0, false, 0, true>), grid, blk, 0, s, a); break;
    default: hipLaunchKernelGGL((k_residual<ARJ, 4, DEPTH, false, DUMP, double, false, 1, 2, false, 0, true>), grid, blk, 0, s, a); break;
  }
}

template <int ARJ, bool DEPTH>
void iterate_t(hipStream_t s, const ResidualArgs& a, const IterArgs& ia, int n_pairs) {
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  // up to three pairs on whole rows: the blocks alone on their CUs (one reduction pass); else four blocks per CU, masking
  if (n_pairs > 3 || level_ragged(a.L)) hipLaunchKernelGGL((k_iterate<ARJ, 4, DEPTH, false, false, 14, true>), grid, blk, 0, s, a, ia);
  else hipLaunchKernelGGL((k_iterate<ARJ, 4, DEPTH, false>), grid, blk, 0, s, a, ia);
}

// One coarse level of a batch under identity weights, one block per pair: coarse_body at PASS 14 (35 KB of LDS, several blocks per CU, as
// k_coarse_w4) instantiated for kCoarseMaxLevels levels with the masking decided per level, run on the one level of the call.  Neither
// k_coarse_w4's cap of 128 registers (under which the metric terms would spill) nor the one-level form (which runs out of scalar
// registers and parks some in scratch): no metric kernel has scratch.  For the same reason there is no metric k_coarse_weighted —
// that kernel keeps 20 bytes of scratch per lane in every form, the reference mode's included: the host leaves the coarse levels of
// a robust metric alignment on the per-evaluation launches (uwt_capi.hip: coarse_weighted_on), and `weights` is 0 here.
template <int ARJ, bool DEPTH>
void coarse_level_t(hipStream_t s, const CoarseArgs& ca, int cnt) {
  hipLaunchKernelGGL((k_coarse<ARJ, DEPTH, false, 14, kCoarseMaxLevels, 0>), dim3(cnt), dim3(kBlock), 0, s, ca);
}

}  // namespace

void launch_residual(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, bool dump) {
  UWT_WITH_ARJ_METRIC(sel.arith,
    if (sel.depth && dump) residual_t<ARJ, true, true>(s, a, n_pairs, sel.acc64);
    else if (sel.depth) residual_t<ARJ, true, false>(s, a, n_pairs, sel.acc64);
    else if (dump) residual_t<ARJ, false, true>(s, a, n_pairs, sel.acc64);
    else residual_t<ARJ, false, false>(s, a, n_pairs, sel.acc64));
}

void launch_weighted(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, int n_pairs, int sampler, int weights, bool dump) {
  UWT_WITH_ARJ_METRIC(sel.arith,
    if (sel.depth && dump) weighted_t<ARJ, true, true>(s, a, n_pairs, sampler, weights);
    else if (sel.depth) weighted_t<ARJ, true, false>(s, a, n_pairs, sampler, weights);
    else if (dump) weighted_t<ARJ, false, true>(s, a, n_pairs, sampler, weights);
    else weighted_t<ARJ, false, false>(s, a, n_pairs, sampler, weights));
}

void launch_iterate(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const IterArgs& ia, int n_pairs) {
  UWT_WITH_ARJ_METRIC(sel.arith,
    if (sel.depth) iterate_t<ARJ, true>(s, a, ia, n_pairs);
    else iterate_t<ARJ, false>(s, a, ia, n_pairs));
}

// the coarsest levels of a few pairs in one launch: the form that decides the masking per level
void launch_coarse_chain(hipStream_t s, const LaunchSel& sel, const CoarseArgs& ca, int n_pairs) {
  const dim3 grid(n_pairs), blk(kBlock);
  UWT_WITH_ARJ_METRIC(sel.arith,
    if (sel.depth) hipLaunchKernelGGL((k_coarse<ARJ, true, false, kIteratePass, kCoarseMaxLevels, 0>), grid, blk, 0, s, ca);
    else hipLaunchKernelGGL((k_coarse<ARJ, false, false, kIteratePass, kCoarseMaxLevels, 0>), grid, blk, 0, s, ca));
}

void launch_coarse_level(hipStream_t s, const LaunchSel& sel, const CoarseArgs& ca, int cnt, int weights) {
  (void)weights;   // 0: see coarse_level_t
  UWT_WITH_ARJ_METRIC(sel.arith,
    if (sel.depth) coarse_level_t<ARJ, true>(s, ca, cnt);
    else coarse_level_t<ARJ, false>(s, ca, cnt));
}

void launch_table_eval(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, int n_pairs) {
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  UWT_WITH_ARJ_METRIC(sel.arith,
    if (sel.acc64) hipLaunchKernelGGL((k_table_eval<ARJ, false, double>), grid, blk, 0, s, a, ta);
    else hipLaunchKernelGGL((k_table_eval<ARJ, false, float>), grid, blk, 0, s, a, ta));
}

void launch_table_general(hipStream_t s, const LaunchSel& sel, const ResidualArgs& a, const TableArgs& ta, const GeneralArgs& ga, int n_pairs) {
  const dim3 grid(a.slices, n_pairs), blk(kBlock);
  UWT_WITH_ARJ_METRIC(sel.arith, hipLaunchKernelGGL((k_table_general<ARJ, false>), grid, blk, 0, s, a, ta, ga));
}

}  // namespace metric
}  // namespace uwt
