/*
 * uwt.h — C ABI of the MI355X-native direct SE(3) tracker (libuwt_hip.so).
 *
 * Drop-in boundary for UW-SLAM's per-frame direct-tracking hot path.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repo).  Plain pointers and sizes only; every call
 * returns an int status (UWT_OK == 0).  The caller owns all host buffers; a uwt_ctx owns its device buffers
 * and its HIP stream.  One ctx per host thread per GPU.  Calls are synchronous unless named *_async.
 *
 * The library is HIP-only: there is no CPU fallback.  uwt_create() fails with UWT_ERR_NO_DEVICE when no
 * gfx950 device is visible.
 */
#ifndef UWT_H
#define UWT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UWT_MAX_LEVELS 8
/* The domain of the dense warp ("the dense warp's division" below): what a caller may pass.  Outside it the entries that can refuse, do. */
#define UWT_TRANSLATION_MAX 0x1p125f   /* |tx|, |ty|, |tz| of a seed at most */
#define UWT_DEPTH_MAX 0x1p100          /* depth_scale * 32767: the largest depth of level 0, at most */
#define UWT_DEPTH_MIN 0x1p-100         /* depth_scale / 2^(n_levels - 1): the smallest depth of the coarsest level, at least */
#define UWT_ABI_VERSION 4   /* 2: uwt_params::arith; 3: uwt_tuning (no environment variables are read any more); 4: any frame size
                               (uwt_level::img_w / img_h / pitch, uwt_resize_half_*) */

enum uwt_status_code {
  UWT_OK = 0,
  UWT_ERR_INVALID_ARG = 1,
  UWT_ERR_NO_VALID_POINTS = 2, /* reference: cv::Exception from the empty Mat product, src/Tracker.cpp:501 */
  UWT_ERR_HIP = 3,
  UWT_ERR_NO_DEVICE = 4,
  UWT_ERR_CAPACITY = 5,
  UWT_ERR_PAIR_FAILED = 6      /* batch ran; at least one pair has a non-zero status in its uwt_stats */
};

enum uwt_plane { UWT_PLANE_IMAGE = 0, UWT_PLANE_DEPTH = 1, UWT_PLANE_GRADX = 2, UWT_PLANE_GRADY = 3 };

/* Arithmetic of the OpenCV steps on the path (the reference pins no OpenCV build; "3.2", README.md:15).
 * UWT_ARITH_OPENCV: what OpenCV 3.x's generic (non-BLAS, non-IPP) code computes for the reference's expressions —
 *   - every cv::gemm on CV_32F accumulates in double and rounds to float once (matmul.cpp GEMMSingleMul<float,double>):
 *     rigid * points.t() (src/Tracker.cpp:1450) = (float)(T0*X + ((T1*Y + T2*Z) + T3*w)) — the A*Bt branch folds its four
 *     partial sums with "s0 += s1 + s2 + s3;" —, Jl * Jw (:479) = (float)((0 + g0*Jw0k) + g1*Jw1k), and the N-long JtJ / Jtr /
 *     rtr sums (:501, :560-561);
 *   - "(col - cx) * invfx" (:1439, :1443) is folded by the MatExpr algebra (matop.cpp MatOp_AddEx::multiply) into one scaled
 *     convert: x * invfx + (float)(-(double)cx * invfx);
 *   - "A.inv() * b" (:564) is MatOp_Invert::matmul -> cv::solve(A, b, DECOMP_LU) = hal::LU32f(A, 6, b, 1): elimination on
 *     the right-hand side and f32 back substitution, no inverse and no product.
 * UWT_ARITH_LEGACY: rounds 1-3 of this library: the 4-/2-term products as f32 FMA chains, (x - cx) * invfx as written, the
 *   inverse formed and multiplied with f64 accumulation.  Cheaper; differs from the above by <= 1 ulp per pixel term. */
enum uwt_arith { UWT_ARITH_OPENCV = 0, UWT_ARITH_LEGACY = 1 };

/* All solver constants the reference hard-codes as locals of Tracker::EstimatePose* (src/Tracker.cpp:364-372,
 * 634-640) and as link-time globals (src/Options.cpp:26-28), as one POD. */
typedef struct uwt_params {
  int32_t width, height;     /* level-0 size (w_, h_ of src/System.cpp:123: the ROI size of :186-190 when the camera is
                                distorted — any size, as long as (size >> (n_levels-1)) >= 1)                             */
  float fx, fy, cx, cy;      /* level-0 intrinsics = K passed to Tracker::InitializePyramid              */
  int32_t n_levels;          /* PYRAMID_LEVELS, src/Options.cpp:26 (5)                                   */
  int32_t first_level;       /* coarsest level iterated, src/Tracker.cpp:368 (4)                         */
  int32_t last_level;        /* finest level iterated,   src/Tracker.cpp:369 (1)                         */
  int32_t max_iters;         /* src/Tracker.cpp:366 (50)                                                 */
  float epsilon;             /* src/Tracker.cpp:364 (1e-3)                                               */
  float gain;                /* residual gain, src/Tracker.cpp:559 (50)                                  */
  float z_factor;            /* src/Tracker.cpp:371 (1)                                                  */
  float angle_factor;        /* src/Tracker.cpp:372 (1)                                                  */
  float depth_scale;         /* src/Tracker.cpp:1261 (0.0002)                                            */
  float initial_error;       /* last_error seed, src/Tracker.cpp:393 (50000)                             */
  int32_t early_exit;        /* 1: reference exit test src/Tracker.cpp:508; 0: exactly max_iters updates */
  int32_t has_depth;         /* Tracker(bool _depth_available)                                           */
  int32_t handoff_scale_t;   /* 0: EstimatePose (:580-590); 1: EstimatePoseFeatures (:856)               */
  int32_t accumulate_f64;    /* 1 (default): JᵀJ/Jᵀr summed in f64 like cv::gemm on CV_32F (:560-561);  */
                             /* 0: f32 per-thread partial sums (faster, not bit-reproducing the oracle)  */
  int32_t sampler;           /* 0: nearest neighbour, round() (:472, reference); 1: bilinear (north-star extension)  */
  int32_t weights;           /* 0: IdentityWeights (:495, :1621); 1: TukeyFunctionWeights with the reference's      */
                             /* histogram medians (:496, :1571-1654); 2: Huber, k = 1.345 (extension)                */
  int32_t max_frames;        /* frame-slot capacity of the context                                       */
  int32_t max_pairs;         /* largest batch of pairs per call                                          */
  int32_t device;            /* HIP device ordinal                                                       */
  int32_t arith;             /* uwt_arith: UWT_ARITH_OPENCV (default) or UWT_ARITH_LEGACY                */
} uwt_params;

/* per-level camera model = the vectors Tracker::InitializePyramid fills (include/Tracker.h:516-528), and the size of the
 * level's images.  The two sizes differ where the level-0 size is not divisible by 2^lvl (the reference's EUROC path crops to a
 * data-dependent ROI, src/System.cpp:148-191):
 *   w, h          w_[lvl], h_[lvl] = size >> lvl (src/Tracker.cpp:312-313): the point grid ObtainAllPoints walks (:1267-1268);
 *   img_w, img_h  images_[lvl].cols / rows: the chain of cv::resize(.., Size(), 0.5, 0.5) (src/System.cpp:246-251), each step
 *                 cvRound(size * 0.5) — half to even: 733 -> 366, 735 -> 368; what the bounds test of src/Tracker.cpp:450 reads
 *                 and what uwt_get_plane returns; img_w >= w, img_h >= h;
 *   pitch         elements per row of the level's planes in device memory (img_w rounded up to a multiple of 4): what a producer
 *                 that writes frames in place through uwt_plane_device_ptr must honour — a slot is pitch * img_h elements.  Equal to
 *                 the width for every width that is a multiple of 4. */
typedef struct uwt_level {
  int32_t w, h;
  float fx, fy, cx, cy, invfx, invfy;
  int32_t img_w, img_h;
  int32_t pitch;
} uwt_level;

typedef struct uwt_stats {
  int32_t status;     /* per-pair uwt_status_code */
  int32_t iterations; /* residual evaluations over all levels */
  int32_t n_valid;    /* valid points of the last evaluation */
  float error;        /* error of the last evaluation (src/Tracker.cpp:499-502) */
} uwt_stats;

/* normal-equation accumulators of one residual evaluation (the 28 LS accumulators, src/LeastSquares.cpp:151-199,
 * plus the constraint count): A upper triangle row-major (A00 A01 .. A05 A11 .. A55), jtr = +Σ J·r (un-gained). */
typedef struct uwt_accum {
  double A[21];
  double jtr[6];
  int64_t sum_r2;
  int32_t n_valid;
  int32_t pad;
} uwt_accum;

typedef struct uwt_ctx uwt_ctx;

/* Launch-shape switches of a context: HOW the same arithmetic is laid out in launches, never WHAT is computed — every
 * setting gives the same poses bit for bit (tests/test_gpu_production.py runs the forms against each other).  The library reads
 * no environment variable; a context starts with the defaults below (uwt_get_tuning returns them), and the parity suite and the
 * A/B tools change them through uwt_set_tuning.  No reference counterpart (the reference has one form of everything). */
typedef struct uwt_tuning {
  int32_t split;             /* parts a large fixed-schedule batch is cut into, each on a stream of its own (1..4) [2]      */
  int32_t split_min;         /* pairs per part at least [8]                                                                 */
  int64_t split_min_px;      /* level-0 pixels of the whole batch from which the split pays [32 * 640 * 480]                */
  int64_t stream_bytes;      /* a level whose planes over the whole batch exceed this is read non-temporally [200 MiB]      */
  int32_t tail_update;       /* Gauss-Newton update in the tail of the evaluation's own launch: 0 never, 1 split batches,
                                2 always [1]                                                                                */
  int32_t target_blocks;     /* blocks per residual launch the batch-dependent slicing aims at; 0: automatic [0]            */
  int32_t coarse;            /* a few pairs: the coarsest levels in one launch (k_coarse) [1]                               */
  int32_t coarse_batch_px;   /* batches: levels of up to this many pixels run one block per pair, one launch per level;
                                0: never [6144]                                                                             */
  int32_t coarse_weighted;   /* the same for robust weights over the nearest sampler (k_coarse_weighted) [1]                */
  int32_t overlap_gradients; /* uwt_track_batch_async, from 768 pairs on: finer levels' gradients on a side stream beside the
                                first, coarse iterations, and the call's pyramids and gradients of the levels >= 1 under the
                                level 0 of the batch call enqueued before it (early preparation).  0: neither, 1: both,
                                2: the side stream without the early preparation, 3: both at any batch size [1]            */
  int32_t first_poll;        /* early-exit schedules: evaluations of a level before the host first looks [3]                */
  int32_t chained;           /* -1: update chained into the next evaluation's launch for a few pairs; 1 / 0: always / never
                                [-1]                                                                                        */
  int32_t speculation;       /* one or two pairs, early exit: launch without read-backs, run again if cut short [1]         */
  int32_t fused_stages;      /* a few frames: whole pyramid / all gradient levels in one launch each [1]                    */
  int32_t pyramid_batch;     /* batches: pyramid levels 1..3 in one pass over level 0 [1]                                   */
  int32_t typed_loads;       /* the dominant kernel reads gradients and depth through typed buffer loads (the texture path
                                converts int16 to float: three vector conversions per pixel less) [1]                       */
  int32_t reserved[4];
} uwt_tuning;

/* ---- lifecycle -------------------------------------------------------------------------------------------- */

/* Fills the reference's EstimatePose constants (src/Tracker.cpp:364-372) for a w x h camera. */
int uwt_default_params(uwt_params* p, int32_t width, int32_t height, float fx, float fy, float cx, float cy);

/* new Tracker(depth) + Tracker::InitializePyramid(w, h, K)  (src/System.cpp:121-122, src/Tracker.cpp:272, 297-340) */
int uwt_create(const uwt_params* p, uwt_ctx** out);
/* Changes the solver constants of a live context — the locals the reference re-declares at the top of each
 * EstimatePose* variant (src/Tracker.cpp:364-372, 634-640, 877-885): first/last level, max_iters, epsilon, gain, z_factor,
 * angle_factor, initial_error, early_exit, handoff_scale_t, accumulate_f64, sampler, weights, arith.  Geometry and capacity
 * (size, intrinsics, n_levels, has_depth, max_frames, max_pairs, device) must equal the context's. */
int uwt_update_params(uwt_ctx* ctx, const uwt_params* p);
/* the context's current parameters */
int uwt_get_params(const uwt_ctx* ctx, uwt_params* out);
/* the context's launch-shape switches (uwt_tuning); uwt_set_tuning waits for the context's work in flight and applies to every
 * later call.  A value outside its range (split 1..4, split_min >= 1, split_min_px >= 1, stream_bytes >= 0, tail_update 0..2,
 * target_blocks 0..2^20, coarse_batch_px 0..2^24, first_poll 1..2^20, chained -1..1) returns UWT_ERR_INVALID_ARG and changes
 * nothing; the on / off switches take any non-zero value as 1, overlap_gradients a value outside 0..3 as 1. */
int uwt_get_tuning(const uwt_ctx* ctx, uwt_tuning* out);
int uwt_set_tuning(uwt_ctx* ctx, const uwt_tuning* t);
/* Tracker::~Tracker (src/Tracker.cpp:280-293) */
int uwt_destroy(uwt_ctx* ctx);
/* reads back w_/h_/fx_/fy_/cx_/cy_/invfx_/invfy_[lvl] (include/Tracker.h:516-526) */
int uwt_level_info(const uwt_ctx* ctx, int32_t lvl, uwt_level* out);
const char* uwt_status_string(int status);
const char* uwt_last_error(const uwt_ctx* ctx);
int uwt_abi_version(void);
/* sha256 (hex) of the sources and compiler flags this library was built from (csrc/Makefile puts it in at build time; hipcc's
 * output is not byte-reproducible, the sources are).  No reference counterpart: measurement hygiene — bench.py quotes the
 * counter-derived facts under profiles/ only while the loaded library reports the id they were collected on. */
const char* uwt_source_id(void);

/* ---- frames (the Frame data the tracker borrows: images_, depths_, gradientX_, gradientY_; include/System.h:85-89) */

/* Frame::images_[0] / depths_[0] of one frame from host memory with row strides in BYTES (cv::Mat::step).
 * Replaces the imread result handed to the pyramid loop in System::AddFrame (src/System.cpp:228, 243).  A strided image (a view
 * into a wider one: images_[0] = distortion(ROI), src/System.cpp:235) crosses as ONE copy of the span its rows cover — first byte
 * of the first row to last byte of the last, the bytes between the rows included: they must be readable, as they are inside a
 * parent image — while the stride is at most four times the row; beyond that as a 2-D copy (slow: issued row by row). */
int uwt_set_frame(uwt_ctx* ctx, int32_t slot, const uint8_t* gray, size_t row_stride,
                  const uint16_t* depth_or_null, size_t depth_row_stride);
/* n tightly packed frames (w*h elements each) into slots first_slot .. first_slot+n-1 */
int uwt_upload_frames(uwt_ctx* ctx, int32_t first_slot, int32_t n, const uint8_t* gray, const uint16_t* depth_or_null);
/* The same copy, asynchronous, on the context's copy stream: the per-frame ingest of System::AddFrame
 * (src/System.cpp:225-251) overlapped with the tracking of the frames already on the device.  `gray` / `depth` must be
 * page-locked (uwt_host_alloc) and stay untouched until a later uwt_sync, or until the tracker call that consumes these
 * slots has been followed by a uwt_sync.  The context orders the copy behind the tracker work still in flight on the
 * same slots and every later tracker call on these slots behind the copy; nothing else waits.  depth may be null even
 * on a context with a depth plane (the tracker reads depth of reference frames only, src/Tracker.cpp:1266-1272). */
int uwt_upload_frames_async(uwt_ctx* ctx, int32_t first_slot, int32_t n, const uint8_t* gray, const uint16_t* depth_or_null);
/* page-locked host memory for uwt_upload_frames_async (hipHostMalloc / hipHostFree) */
int uwt_host_alloc(size_t bytes, void** out);
int uwt_host_free(void* p);
/* device pointer of a plane of a slot (so a producer can write level-0 frames in place, inputs resident in HBM): img_h rows of
 * uwt_level::pitch elements, the first img_w of each row the image (tight rows whenever the width is a multiple of 4) */
int uwt_plane_device_ptr(uwt_ctx* ctx, int32_t slot, int32_t lvl, int32_t plane, void** out);
/* copy one plane of one slot back to the host: img_h x img_w elements, tight rows */
int uwt_get_plane(uwt_ctx* ctx, int32_t slot, int32_t lvl, int32_t plane, void* host_out);

/* the resize loop of System::AddFrame for levels 1..n_levels-1 (src/System.cpp:246-251), n frames at once */
int uwt_build_pyramids(uwt_ctx* ctx, int32_t first_slot, int32_t n);
/* Tracker::ApplyGradient(Frame*) (src/Tracker.cpp:1127-1134) for n frames at once */
int uwt_apply_gradient(uwt_ctx* ctx, int32_t first_slot, int32_t n);

/* ---- tracking --------------------------------------------------------------------------------------------- */

/* Tracker::EstimatePose(previous, current) (src/Tracker.cpp:362-597) for n_pairs independent pairs.
 * poses_out: n_pairs x 7 floats (qx qy qz qw tx ty tz) = previous_frame->rigid_transformation_ (:595).
 * Dense points (Tracker::ObtainAllPoints, :1259-1310) are implicit: the pixel grid is never materialised.
 * Synchronous.  How the launches are laid out follows the batch (same results either way): a few pairs per call take
 * the chained flow (one launch per evaluation, the coarsest levels in one launch, results written straight into
 * page-locked memory; one or two pairs of an early-exit schedule are launched without read-backs, each level with a budget of
 * evaluations, and run again with twice the budget — then with read-backs — if a level was cut short), batches take one
 * residual and one update launch per evaluation (coarse levels one launch per level, one block per pair), large fixed-schedule
 * batches run as two halves on two streams with the update in the tail of the residual launch. */
int uwt_estimate_pose_batch(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                            float* poses_out, uwt_stats* stats_out_or_null);

/* Alignment of device pointers.  Every pointer to DEVICE memory an entry point takes must be aligned to the widest access a kernel
 * makes through it, stated at the entry ("alignment:"), and needs no more than that: a buffer may start anywhere such a multiple falls,
 * e.g. inside a larger allocation of the caller's.  In short: 4 bytes for poses (rows of 7 floats), uwt_stats, uwt_keypoint, uwt_match,
 * uwt_tracking_info, counts and the u8 planes of uwt_warp_image_io (written four pixels at a time); 1 byte for the RANSAC mask; 8 bytes
 * for the records that hold 64-bit fields (uwt_ransac_info, uwt_warp_quality, uwt_cloud_info); 16 bytes for uwt_cloud_point (one
 * 16-byte store per point) and for the descriptor sets uwt_match_descriptors_device_async reads (16-byte loads).  No entry point
 * writes or reads outside the extents it documents: not a row past the last pair's cap, not a pose past n_pairs, not a record past a
 * cloud's cap; and no result depends on bytes outside those extents or on the rows past a count (tests/test_gpu_guard_bands.py). */

/* Whole per-frame path for a resident batch: pyramids of slots [first_slot, first_slot+n_frames), gradients of
 * the same slots, then EstimatePose for the pairs — enqueued on the context stream, results written to DEVICE
 * memory (d_poses_out: n_pairs x 7 floats, d_stats_out_or_null: n_pairs uwt_stats).  uwt_sync() to wait.
 * grad_refs_only != 0: the planes the tracker reads of the reference frame only — gradients (src/Tracker.cpp:407-408)
 * and the depth pyramid levels 1.. (:1266-1272) — are built for the pairs' ref_slots alone (wherever they lie);
 * the image pyramids still cover the whole slot range.  0 prepares every frame of the range fully, as
 * System::AddFrame / System::Tracking do for each new frame.
 * Asynchronous with early_exit = 0 (fixed iteration counts: nothing in the call waits for the device).  With
 * early_exit = 1 — the reference's schedule, uwt_default_params' setting — the call itself waits for the device a few
 * times per level above 6144 pixels (after evaluations 3, 6, 12, ... it reads back how many pairs are still iterating — each
 * look taken while the next evaluation already runs — and stops launching for a level every pair has left; smaller levels
 * decide on the device), so it returns only once the last level's first iterations are queued.
 * Ordering against uwt_upload_frames_async covers every slot the call touches: the prepared range AND every slot the pair
 * lists name (they may lie outside the range).
 * Early preparation (uwt_tuning::overlap_gradients): when the entry before this one on the context was a dense batch call of a fixed
 * schedule that ends on level 0 (identity weights, first_level >= 1, no profiling), this call's pyramids and its gradients of the
 * levels >= 1 may run before that call has ended — past its level 1 it reads level-0 planes alone, whatever slots the two calls
 * name.  Any other entry between the two, uwt_plane_device_ptr and uwt_stream included, is ordered as it always was: the call after
 * it is enqueued in one piece behind it.  Results never depend on it.  Level-0 frames a producer writes in place must be complete
 * (the producer waited for) before the call that reads them is made; work merely enqueued on uwt_stream does not order them.
 * alignment: d_poses_out 4 bytes, d_stats_out_or_null 4 bytes. */
int uwt_track_batch_async(uwt_ctx* ctx, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only,
                          int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                          float* d_poses_out, uwt_stats* d_stats_out_or_null);
/* The same call with the results copied behind it into host buffers (page-locked: uwt_host_alloc) and a ticket to wait
 * on: the streaming form — while this batch is aligned the caller uploads the next one into other slots
 * (uwt_upload_frames_async) and only waits for the batch before. */
int uwt_track_batch_host_async(uwt_ctx* ctx, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only,
                               int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                               float* h_poses_out, uwt_stats* h_stats_out_or_null, int64_t* ticket_out);
/* blocks until the call that returned `ticket` (and its result copy) has completed; later calls keep running */
int uwt_wait_ticket(uwt_ctx* ctx, int64_t ticket);
int uwt_sync(uwt_ctx* ctx);
/* Deferred stage calls (off by default).  on = 1: uwt_build_pyramids and uwt_apply_gradient return once their kernels are
 * enqueued on the context's stream; every later call of the context runs behind them, and the calls that hand results to
 * the host (uwt_estimate_pose_*, uwt_get_plane, uwt_sync, ...) wait as before — the per-frame sequence of
 * System::AddFrame + System::Tracking (src/System.cpp:193-251) then waits once per frame, in EstimatePose, instead of
 * three times.  A kernel failure of a deferred call is reported by the next waiting call.  A consumer that reads
 * uwt_plane_device_ptr planes on a stream of its own must uwt_sync first. */
int uwt_set_deferred(uwt_ctx* ctx, int32_t on);
/* the HIP stream (hipStream_t) the context launches on, for event timing by the caller */
int uwt_stream(uwt_ctx* ctx, void** out);
/* average device time in ms of the residual/Jacobian/reduction kernel launches and their count since the last
 * reset (HIP events on the context stream; only recorded while profiling is enabled).
 * `on` is a bit mask: 1 = record the events; 2 (diagnostic) = the dense residual launches run their compute-only twin —
 * the same instruction stream with every memory operation of the loop replaced by register arithmetic.  Poses computed
 * with bit 2 set are meaningless; the launch durations are the kernel's own instruction-issue floor (bench.py's
 * roofline.valu).  0 switches both off. */
int uwt_profile_enable(uwt_ctx* ctx, int32_t on);
int uwt_profile_read(uwt_ctx* ctx, double* residual_ms_total, int64_t* residual_launches, int64_t* residual_pixels);
/* the same durations and launch counts by pyramid level (arrays of n_levels entries) */
int uwt_profile_read_levels(uwt_ctx* ctx, double* ms_by_level, int64_t* launches_by_level, int32_t n_levels);
/* Shader clock (GHz) the chip held inside the last profiled k_residual launch: blocks of a profiled launch leave their
 * s_memtime (shader cycles) and s_memrealtime (100 MHz) deltas in their records.  Diagnostic; synchronises. */
int uwt_profile_clock(uwt_ctx* ctx, double* shader_ghz);

/* ---- per-stage entry points (each kernel parity-testable alone; host buffers, synchronous) ------------------ */

/* cv::resize(src, dst, Size(), 0.5, 0.5) as used at src/System.cpp:247 / :249, even sizes (dst: w/2 x h/2) */
int uwt_halve_u8(uwt_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst);
int uwt_halve_u16(uwt_ctx* ctx, const uint16_t* src, int32_t w, int32_t h, uint16_t* dst);
/* the same call on ANY size: dst is uwt_half_size(w) x uwt_half_size(h) = cvRound(size * 0.5) (half to even); whole 2 x 2 cells
 * (a + b + c + d + 2) >> 2, the half cells of a partial last column and every cell of a partial last row by resizeAreaFast's
 * generic tail: the mean of the pixels that exist, rounded half to even */
int uwt_half_size(int32_t n);
int uwt_resize_half_u8(uwt_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, uint8_t* dst);
int uwt_resize_half_u16(uwt_ctx* ctx, const uint16_t* src, int32_t w, int32_t h, uint16_t* dst);
/* cv::Scharr(src, dst, CV_16S, 1|0, 0|1, scale=3, 0, BORDER_DEFAULT) as used at src/Tracker.cpp:1133-1134 */
int uwt_scharr3(uwt_ctx* ctx, const uint8_t* src, int32_t w, int32_t h, int16_t* gx, int16_t* gy);
/* The dense warp's division.  Every entry that walks a level's point GRID (uwt_residual_jacobian*, uwt_estimate_pose_batch*,
 * uwt_track_batch*; not the explicit tables, the image warp or the sweep, which divide with the IEEE operator) forms the three quotients of
 * a pixel — u' = (x' fx) / z2, v' = (y' fy) / z2 (src/Tracker.cpp:1455, :1460) and inv_z2 = 1 / z2 (:447) — from ONE hardware reciprocal:
 *     r0 = v_rcp_f32(z2);   e = fma(-z2, r0, 1);   r = fma(e, r0, r0)                                  -> inv_z2 = r
 *     q = n * r;   e = fma(-z2, q, n);   q = fma(e, r, q);   e = fma(-z2, q, n);   q = fma(e, r, q)     -> n / z2
 * which is the sequence the compiler emits for the IEEE `/` without its scaling of the operands into range (div_scale / div_fixup).
 * Where the two agree — derived from the sequence, measured by tests/test_gpu_validity.py's range cases on gfx950:
 *   - v_rcp_f32 is accurate to 1 ulp for a normal operand with a normal result and FLUSHES subnormals on both sides: a subnormal z2 is
 *     read as zero (r0 infinite, r = NaN), and 1 / z2 for |z2| > 2^126, a subnormal number, comes back as a zero of z2's sign.
 *   - For 2^-126 <= |z2| <= 2^126 every step of the first line scales exactly with the exponent of z2 (r0 by 2^-k, e not at all), so r is
 *     the same function of the mantissa at every exponent: the correctly rounded 1 / z2 for all 2^23 mantissas (checked exhaustively at
 *     nine exponents and both signs).  inv_z2 equals the IEEE quotient on exactly that range.
 *   - Given such an r, the second line is Markstein's correction: the result is the correctly rounded n / z2 as long as no
 *     intermediate leaves the normal range — n = 0 (every step is an exact zero), or |n| and |n / z2| in [2^-100, 2^126]: the residuals
 *     e are about 2^-24 |n| and must keep their bits.  A quotient that underflows against cx (|n / z2| < 2^-126: u = cx either way) is
 *     covered by the measurement at |z2| = 2^125 and 2^126, not by the derivation.
 *   - z2 = 0, infinite or NaN: r is NaN here and the quotients NaN, where IEEE gives infinities or NaN: the pixel fails 0 < u < cols
 *     either way, which is all the loop asks; uwt_warp (an IEEE division) shows the reference's own values.
 * Outside 2^-126 <= |z2| <= 2^126 the dense entries differ from the reference: for |z2| > 2^126 inv_z2 is +-0 instead of a subnormal
 * (a pixel stays valid, its Jacobian row is zero where the reference's is about 1e-33 times the gradient, and a negative z2 leaves
 * zeros of the other sign in the dumps of the legacy set); for a subnormal z2 the pixel is invalid where the reference's is valid.
 * From the range to what a caller passes.  The derivation has three CONDITIONS which the library does not test:
 *   (a) the rays are moderate: |(col - cx) / fx|, |(row - cy) / fy| <= r_max = 2^20 over the image (uwt_create does not compare the
 *       size with the focal lengths);
 *   (b) the rotation is one: |R_ij| <= 3, true of a quaternion of norm at most 1 + 2^-3 — a seed's quaternion is read as it is and
 *       its norm is not tested;
 *   (c) the bound on the translation holds for the pose in front of EVERY evaluation, not only the seed: the solver's own updates move
 *       it, and under handoff 0 with uwt_params::handoff_scale_t = 1 the hand-off doubles t at every level boundary — a seed with
 *       |tz| = 2^125 is 2^127 two levels further down.  There a caller keeps |t| <= 2^(125 - (first_level - last_level)).
 * Under them |z2| <= |R20 X| + |R21 Y| + |R22 z| + |tz| <= 9 * 2^20 * z_max + |tz|, so
 *     |tx|, |ty|, |tz| <= UWT_TRANSLATION_MAX = 2^125   and   z_max = depth_scale * 32767 <= UWT_DEPTH_MAX = 2^100
 * give |z2| <= 9 * 2^120 + 2^125 < 2^126 (the same sum bounds x' and y'; a valid pixel has |n / z2| < cols + |cx|); and
 *     z_min = depth_scale / 2^(n_levels - 1) >= UWT_DEPTH_MIN = 2^-100   (depth code 1 on the coarsest level; without depth z = 1)
 * keeps every depth, every X = ray * z and every numerator that is not an exact zero normal with 24 bits to spare.  A z2 that CANCELS
 * to a subnormal (z2 = R22 z + tz + ... within 2^-126 of zero without being zero) needs an operand below 2^-102 and is excluded by
 * the same bounds for a pose whose translation entries are zero or at least 2^-100 in magnitude; the library does not test that either.
 * What the library does test — two necessary conditions, not the whole domain: uwt_create refuses (UWT_ERR_INVALID_ARG) a context with
 * has_depth != 0 whose depth_scale is not finite or, being non-zero, breaks one of the two depth bounds (both tested in double:
 * fabs(depth_scale) * 32767 and fabs(depth_scale) / 2^(n_levels - 1)); uwt_update_params cannot change depth_scale.  A SEED whose
 * translation exceeds UWT_TRANSLATION_MAX in magnitude fails its pair like a seed with a non-finite entry ("seeded calls" below); the
 * pose behind the seed is not tested again.  The per-stage entries take their pose as given. */
/* Tracker::WarpFunction(points, T, lvl) (src/Tracker.cpp:1417-1471): n x 4 in, n x 4 out */
int uwt_warp(uwt_ctx* ctx, int32_t lvl, const float* pts, int32_t n, const float pose[7], float* warped_out);
/* one pass of the per-point loop of EstimatePose (src/Tracker.cpp:432-490) + the reduction, for one pair at one
 * level under `pose`.  Optional per-point dumps (the level's w x h point grid, row-major): J_out (x6), r_out, valid_out. */
int uwt_residual_jacobian(uwt_ctx* ctx, int32_t ref_slot, int32_t tgt_slot, int32_t lvl, const float pose[7],
                          uwt_accum* acc_out, float* J_out_or_null, float* r_out_or_null, uint8_t* valid_out_or_null);
/* Same under the context's sampler / weights (general path): additionally returns the per-pixel robust weights
 * (Tracker::TukeyFunctionWeights, src/Tracker.cpp:1626-1654), the scale 1/MAD, the error numerator Σ r·(r·w) and the
 * accumulators of the weighted system (J <- w·J, r <- gain·r; :554-561): acc_out->jtr then holds Σ(wJ)·(gain·r·w). */
int uwt_residual_jacobian_weighted(uwt_ctx* ctx, int32_t ref_slot, int32_t tgt_slot, int32_t lvl, const float pose[7],
                                   uwt_accum* acc_out, double* err_num_out, float* inv_mad_out, float* J_out_or_null,
                                   float* r_out_or_null, uint8_t* valid_out_or_null, float* w_out_or_null);
/* LS::initialize + n x LS::update(J, r, w) + LS::finishNoDivide / finish  (src/LeastSquares.cpp:30-37, 204-209,
 * 39-146).  Every accumulator is the f32 chain the reference's loop forms, in call order (one GPU thread per chain: the 28 chains
 * are independent) — the reference's floats bit for bit, not a re-associated sum.  A: 36 row-major, b: 6 (stored sign:
 * b = -Σ w r J), error, count. */
int uwt_ls_accumulate(uwt_ctx* ctx, const float* J, const float* r, const float* w_or_null, int32_t n, int32_t divide,
                      float A[36], float b[6], float* error, int32_t* num_constraints);
/* LS::initialize + (n/4) x LS::updateSSE + LS::finishNoDivide / finish (src/LeastSquares.cpp:148-202): the 4-wide form's
 * product association ((J_i·w)·J_j, (r·w)·J_i, (r·w)·r); n must be a multiple of 4.  count_quirk != 0 reproduces
 * "num_constraints += 6" per four points (:201); 0 counts 4. */
int uwt_ls_accumulate_sse(uwt_ctx* ctx, const float* J, const float* r, const float* w, int32_t n, int32_t divide,
                          int32_t count_quirk, float A[36], float b[6], float* error, int32_t* num_constraints);
/* Sophus::SE3f::exp (thirdparty/sophus/se3.hpp:723-744) */
int uwt_se3_exp(uwt_ctx* ctx, const float xi[6], float pose_out[7]);
/* SE3f::operator* (se3.hpp:285-321) */
int uwt_se3_mul(uwt_ctx* ctx, const float a[7], const float b[7], float out[7]);
/* SE3f::matrix() (se3.hpp:253-268), row-major 4x4 */
int uwt_se3_matrix(uwt_ctx* ctx, const float pose[7], float T_out[16]);
/* level hand-off of EstimatePose (src/Tracker.cpp:580-590) */
int uwt_se3_handoff(uwt_ctx* ctx, float pose_inout[7], int32_t scale_t);
/* deltaMat = A.inv() * b (src/Tracker.cpp:564); Ainv_out_or_null receives cv::Mat::inv()'s result */
int uwt_solve_delta(uwt_ctx* ctx, const float A[36], const float b[6], float delta_out[6], float* Ainv_out_or_null,
                    int32_t* nonsingular_out_or_null);

/* The state of one pair inside an alignment, as the update kernels keep it: pose (quaternion x y z w, translation), the error of the
 * last accepted step and of this evaluation, level_done / status (uwt_stats::status), evaluations so far, valid points of the last one. */
typedef struct uwt_pair_state {
  float pose[7];
  float last_error, error;
  int32_t level_done, status, iters, n_valid;
} uwt_pair_state;   /* 52 bytes */

/* Test surface: the tail of one Gauss-Newton iteration (src/Tracker.cpp:495-574: fold of the evaluation's block records, error, exit
 * test, b, A.inv() * b, pose <- pose * exp(delta)) on records the CALLER wrote, through either of the library's two fold forms.  No
 * alignment call uses this entry.
 *   form 0   the block form (k_gn_update as the alignments launch it: 256 threads per pair); needs stride == count.  A pair that arrives
 *            with level_done or status set is returned unchanged.
 *   form 1   the tail form: `count` one-wave blocks per pair draw the pair's ticket, the last one folds and updates, as in the tail of a
 *            residual or table launch.  Those launches draw no ticket for a finished pair; here every pair is updated.
 * Every array is indexed by the absolute pair: pairs pair_base .. pair_base + n_pairs - 1 are updated, rows below pair_base travel to
 * the device and back untouched.  With rows = pair_base + n_pairs:
 *   records      rows x stride x 64 words, a pair's first `count` records folded (1 <= count <= stride, count <= 160, stride <= 256).
 *                A record: 27 f64 sums (21 of A's upper triangle, row-major, 6 of J^T r) in words 0-53 | valid points, u32, word 54 |
 *                sum of r^2, u64, words 56-57 | the error numerator, f64, words 58-59 (general != 0) | the rest not part of any sum.
 *   states_in, states_out   rows records each.
 *   k, max_iters, early_exit, epsilon, gain, general   as an alignment passes them (general != 0: records of the weighted / bilinear
 *                kind: gain already applied, error from the error numerator).  The solve is the context's arithmetic set's.
 *   active_out   the number of pairs that took a step.
 *   tickets_out_or_null   rows words: the ticket words after the call (form 0: zeros; form 1: zero again after a correct run).
 * rows > 1024 or any other argument out of range: UWT_ERR_INVALID_ARG, the outputs untouched. */
int uwt_gn_update_records(uwt_ctx* ctx, int32_t form, int32_t n_pairs, int32_t pair_base, int32_t stride, int32_t count,
                          const uint32_t* records, const uwt_pair_state* states_in, int32_t k, int32_t max_iters, int32_t early_exit,
                          float epsilon, float gain, int32_t general, uwt_pair_state* states_out, int32_t* active_out,
                          uint32_t* tickets_out_or_null);

/* ---- sparse point tables (Frame::candidatePoints_[lvl]) -------------------------------------------- */

/* Tracker::EstimatePose / EstimatePoseFeatures over explicit per-level point tables (src/Tracker.cpp:401, 669): tables[l]
 * is an n_points[l] x 4 host array [x y z w] for every level l in [last_level, first_level] (other entries ignored).
 * With the EstimatePoseFeatures constants (first = last = 0, max_iters 10, gain 1, z_factor 0.002, handoff_scale_t 1;
 * src/Tracker.cpp:634-640, 834, 856) this is the reference's live tracking call.  uwt_params::weights and ::sampler apply as in
 * the dense call.  A row whose reference position ((int)y, (int)x) lies outside the level is dropped (the reference's
 * Mat::at would read outside the image, :474-477).
 * The call is a batch of one pair over the kernels of the batched table calls below: the tables are copied to the device, their
 * rows grouped by 1024 per block and the blocks folded in slice order, the update in each evaluation's tail; with early_exit = 1
 * the early exits are polled as uwt_track_candidates_batch_async polls them.  Pose and uwt_stats are the same bits as theirs for
 * the same tables under either accumulate_f64.  (This call used to group its rows by 8192: under accumulate_f64 = 0 on the
 * identity path, whose f32 sums follow the grouping, the last bits of a pose may differ from what it gave then.  The default's
 * f64 sums and every pose under weights or the bilinear sampler have not moved.)  Like the batched calls, it is ordered behind
 * uwt_upload_frames_async into its two slots. */
int uwt_estimate_pose_points(uwt_ctx* ctx, int32_t ref_slot, int32_t tgt_slot, const float* const* tables,
                             const int32_t* n_points, float pose_out[7], uwt_stats* stats_out_or_null);
/* Tracker::MedianMat (src/Tracker.cpp:1571-1594), MedianAbsoluteDeviation (:1607-1619), IdentityWeights (:1621-1624) and
 * TukeyFunctionWeights (:1626-1654) on an explicit N x 1 residual vector (host pointers).  kind: 0 identity, 1 Tukey.
 * median_out = MedianMat(residuals) (256-bin histogram of the rounded values saturated to u8, first bin whose cumulative
 * count exceeds float(n / 2)); mad_out = 1.4826 * MedianMat(|residuals - median|); weights_out (n floats, or NULL when
 * only the statistics are wanted): ones, or (1 - (x / 4.6851)^2)^2 for |x| <= 4.6851 and 0 beyond, x = r / MAD (MAD = 1
 * when it is 0). */
int uwt_robust_weights(uwt_ctx* ctx, const float* residuals, int32_t n, int32_t kind, float* weights_out,
                       float* median_out_or_null, float* mad_out_or_null);

/* frame->gradient_[lvl] (src/Tracker.cpp:1136-1142): u8 plane copied to the host */
int uwt_gradient_magnitude(uwt_ctx* ctx, int32_t slot, int32_t lvl, uint8_t* mag_out);
/* Tracker::ObtainCandidatePoints for one level (src/Tracker.cpp:1314-1362): gradient_ > mean + threshold
 * (GRADIENT_THRESHOLD = 20, src/Options.cpp:27), x-major order; needs uwt_apply_gradient on the slot first.
 * Writes min(count, cap) points; *count_out is the full count.
 * The comparison is one of doubles, strict: a cell whose magnitude equals fl(mean + threshold) is not a candidate; the mean is the
 * integer sum of the level's img_w x img_h image (not of its pitched rows, not of the point grid) divided once.  A frame's table has
 * at most w x h rows, and exactly that many when every cell passes (any threshold below -255 on a context without a depth plane).
 * threshold must be finite, here and in uwt_obtain_candidate_points_batch as in the batched tracking calls: NaN or an infinity is
 * UWT_ERR_INVALID_ARG with nothing enqueued (+-1e300 is finite: no cell, every cell). */
int uwt_obtain_candidate_points(uwt_ctx* ctx, int32_t slot, int32_t lvl, double threshold, float* pts_out, int32_t cap,
                                int32_t* count_out);
/* The same for frames first_slot .. first_slot + n_frames - 1 in one call (many blocks per frame: per-column counts by
 * row band, an exclusive scan in the reference's x-major order, ordered write).  pts_out: n_frames x cap x 4 floats (frame
 * f's points start at f * cap * 4), counts_out: n_frames full counts. */
int uwt_obtain_candidate_points_batch(uwt_ctx* ctx, int32_t first_slot, int32_t n_frames, int32_t lvl, double threshold,
                                      float* pts_out, int32_t cap, int32_t* counts_out);
/* Tracker::ObtainPatchesPoints (src/Tracker.cpp:1178-1257): 11x11 level-0 patches around <= 200 key points (x, y).
 * The key-point domain, of this entry and of every call that takes key points for patches (uwt_obtain_patch_points_batch, the
 * uwt_estimate_pose_features_batch / uwt_track_features_batch family): 0 <= x < w and 0 <= y < h of level 0, -0.0 accepted as 0; the
 * depth is read at ((int)y, (int)x), by truncation.  A used key point outside the domain (x == w, a negative coordinate, a NaN) is
 * UWT_ERR_INVALID_ARG with nothing enqueued; key points past the first 200 are not looked at.  Inside the domain a patch may reach
 * over any border: its cells with 0 < i < w and 0 < j < h are kept (column 0 and row 0 never are), from (int)(x - 5) while
 * (float)i <= x + 5.  The depth is a signed short: 0 drops the key point, 0x8000..0xffff give a negative z. */
int uwt_obtain_patch_points(uwt_ctx* ctx, int32_t slot, const float* keypoints_xy, int32_t n_keypoints, float* pts_out,
                            int32_t cap, int32_t* count_out);
/* Tracker::AddPatchPointsFeatures(candidatePoints, lvl) (src/Tracker.cpp:599-629; include/Tracker.h:126; its only call,
 * :672, is commented out in the reference): the N x 4 table followed, point by point, by the cells of the patch_size x
 * patch_size patch around each rounded point that lie inside the level (i > 0, j > 0) and are not the centre, with the
 * point's z and w = 1.  The reference's patch_size_ is 5 (:274).  count_out: the full count (n_pts + cells), of which at
 * most cap rows are written. */
int uwt_add_patch_points(uwt_ctx* ctx, int32_t lvl, const float* pts, int32_t n_pts, int32_t patch_size, float* pts_out,
                         int32_t cap, int32_t* count_out);

/* ---- the live call for a batch of pairs (tables built and consumed on the device) ------------------------------------ */

/* Tracker::ObtainPatchesPoints (src/Tracker.cpp:1178-1257) for n_frames frames at once (1 <= n_frames <= max_pairs).
 * keypoints_xy: n_frames x 200 x 2 floats (frame f's key points at f*400); n_keypoints[f]: how many, only the first 200 used.
 * pts_out: frame f's table at f * cap * 4 (min(count, cap) rows written); counts_out[f]: its full count.  Synchronous. */
int uwt_obtain_patch_points_batch(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const float* keypoints_xy,
                                  const int32_t* n_keypoints, float* pts_out, int32_t cap, int32_t* counts_out);
/* System::Tracking's live call (src/System.cpp:214-219) for n_pairs pairs: ObtainPatchesPoints(previous) then
 * EstimatePoseFeatures(previous, current) with the reference's own constants (src/Tracker.cpp:634-640, 834, 856): level 0 only,
 * 10 iterations, epsilon 1e-3, last_error 50000 (:661), gain 1, z_factor 0.002, no angle factor, the early exit of :782,
 * identity weights (:769), round() sampling (:746).  previous = ref_slots[i] (its key points and its depth), current =
 * tgt_slots[i]; key points as in uwt_obtain_patch_points_batch.
 * Geometry, intrinsics, arith, has_depth and accumulate_f64 come from the context; its first_level, last_level, max_iters,
 * epsilon, gain, z_factor, angle_factor, initial_error, early_exit, weights and sampler are ignored and left as they are (no
 * uwt_update_params round trip; the live call under robust weights or the bilinear sampler: uwt_track_features_batch_opt_async /
 * uwt_estimate_pose_features_batch_opt below, which take them as options of the call).  1 <= n_pairs <= max_pairs, slots in range and every used key point inside level 0, or
 * UWT_ERR_INVALID_ARG with nothing enqueued.  A pair with no valid point (no key points, every key point on zero depth) gets
 * UWT_ERR_NO_VALID_POINTS in its own uwt_stats; the other pairs are unaffected.  The tables, their counts and the solver state
 * never leave the device: one producer launch, then one launch per Gauss-Newton evaluation with the update in its tail.
 * A pair's pose does not depend on the batch it runs in.  The caller may reuse every host array once the call returns.
 * Results go to DEVICE memory, as in uwt_track_batch_async (d_poses_out: n_pairs x 7 floats, d_stats_out_or_null: n_pairs
 * uwt_stats), ordered against uwt_upload_frames_async like it.  The call never waits for the device; uwt_sync() to wait.
 * alignment: d_poses_out 4 bytes, d_stats_out_or_null 4 bytes (the same in the _opt form). */
int uwt_track_features_batch_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                   const float* keypoints_xy, const int32_t* n_keypoints,
                                   float* d_poses_out, uwt_stats* d_stats_out_or_null);
/* The same, synchronous, results in host memory (the uwt_estimate_pose_batch counterpart: UWT_ERR_PAIR_FAILED when a pair
 * failed, its status in its uwt_stats). */
int uwt_estimate_pose_features_batch(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                     const float* keypoints_xy, const int32_t* n_keypoints,
                                     float* poses_out, uwt_stats* stats_out_or_null);

/* ---- robust weights and the bilinear sampler in the batched table calls ---------------------------------------------- */

/* The options of one batched table call.  They are the call's own: the context's weights and sampler are neither read nor changed. */
typedef struct uwt_table_options {
  int32_t weights;      /* as uwt_params::weights: 0 identity, 1 Tukey (the reference's TukeyFunctionWeights and medians), 2 Huber */
  int32_t sampler;      /* as uwt_params::sampler: 0 round(), 1 bilinear */
  int32_t reserved[6];  /* zero */
} uwt_table_options;    /* 32 bytes */
int uwt_default_table_options(uwt_table_options* o);   /* {0, 0} */

/* uwt_track_features_batch_async / uwt_estimate_pose_features_batch under the call's own weights and sampler; everything else
 * (the reference's constants of the live call, the arguments and their checks, ordering against uploads, asynchrony, failure per
 * pair in the pair's own uwt_stats) as documented there.  opt_or_null null or {0, 0}: the code of the entries above, the same
 * bytes.  weights outside 0..2, sampler outside 0..1 or a non-zero reserved word: UWT_ERR_INVALID_ARG with nothing enqueued.
 * Otherwise, for every pair, pose and uwt_stats are what uwt_obtain_patch_points + uwt_estimate_pose_points give on a context whose
 * params carry the live call's constants and these weights and sampler: per row the residual of either sampler, the weight from
 * the pair's scale (median and MAD of the rounded residuals' 511 signed bins), w J, (r gain) w and the error numerator
 * sum r (r w); f64 sums whatever accumulate_f64 says.  Weights and sampler combine freely here (Tukey over the bilinear sampler bins
 * the rounded residual, as Huber does).  The tables never leave the device: with weights an evaluation is two launches (the
 * scale pass, whose last block per pair derives the scale, then the weighted pass with the update in its tail), with the bilinear
 * sampler alone one; the pairs' histograms are cleared once per call.  The rows are grouped by 1024 per block by the pair's own
 * count and the blocks folded in slice order: a pair's bits depend neither on the batch it runs in, nor on its place there, nor
 * on uwt_tuning. */
int uwt_track_features_batch_opt_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                       const float* keypoints_xy, const int32_t* n_keypoints, const uwt_table_options* opt_or_null,
                                       float* d_poses_out, uwt_stats* d_stats_out_or_null);
int uwt_estimate_pose_features_batch_opt(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                         const float* keypoints_xy, const int32_t* n_keypoints, const uwt_table_options* opt_or_null,
                                         float* poses_out, uwt_stats* stats_out_or_null);

/* ---- semi-dense tracking for a batch of pairs (candidate tables built and consumed on the device) --------------------- */

/* Tracker::ObtainCandidatePoints(previous) (src/Tracker.cpp:1314-1362) on levels last_level..first_level, then
 * Tracker::EstimatePose(previous, current) (:362-597) over those tables (read at :401), for n_pairs pairs.  previous =
 * ref_slots[i], current = tgt_slots[i]; the reference frames must have had uwt_build_pyramids and uwt_apply_gradient, as
 * uwt_obtain_candidate_points requires.  threshold: GRADIENT_THRESHOLD (20, src/Options.cpp:27).
 * Tables are built for the iterated levels alone, each on the gw x gh grid the reference's loops walk, with the depth test and
 * z of uwt_obtain_candidate_points (the reference's at<uchar> read of the 16-bit plane).  The call runs under the context's
 * first_level, last_level, max_iters, epsilon, gain, z_factor, angle_factor, initial_error, early_exit, handoff_scale_t, arith and
 * accumulate_f64 — the constants uwt_estimate_pose_points honours — and reads the params without changing them.
 * weights != 0 or sampler != 0: UWT_ERR_INVALID_ARG with nothing enqueued (robust weights and the bilinear sampler over
 * candidate tables: uwt_track_candidates_batch_opt_async / uwt_estimate_pose_candidates_batch_opt below, or the per-pair path,
 * uwt_obtain_candidate_points + uwt_estimate_pose_points).  So are 1 <= n_pairs <= max_pairs violated, a slot
 * out of range, a null list and a non-finite threshold.
 * For every pair, pose and uwt_stats are the bits uwt_obtain_candidate_points per level followed by uwt_estimate_pose_points
 * give on the same context, under either accumulate_f64 (one grouping, 1024 rows per block, serves both calls).  A pair's pose
 * depends neither on the batch it runs in, nor on its place there, nor on uwt_tuning.  A pair with no valid point on a level (a
 * flat reference frame, every candidate on a zero depth byte) gets its status in its own uwt_stats, as
 * uwt_estimate_pose_points reports it; the other pairs are unaffected.
 * The tables, their counts and the solver state never leave the device: per level a producer pass (gradient_ and its mean,
 * per-column counts, an exclusive scan, the ordered write), then per level one launch per Gauss-Newton evaluation with the
 * update in its tail, k_level_end between levels.  The caller may reuse the pair lists once the call returns.
 * Results go to DEVICE memory, as in uwt_track_batch_async (d_poses_out: n_pairs x 7 floats, d_stats_out_or_null: n_pairs
 * uwt_stats), ordered against uwt_upload_frames_async like it.  With early_exit = 0 the call never waits for the device.  With
 * early_exit = 1 it waits at the early-exit polls as uwt_track_batch_async does (after evaluations first_poll, then twice as
 * many, ..., of each level, each look taken while the next evaluation runs; no launch for a level once every pair has left
 * it).  uwt_sync() to wait for the results.
 * alignment: d_poses_out 4 bytes, d_stats_out_or_null 4 bytes (the same in the _opt form). */
int uwt_track_candidates_batch_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                     double threshold, float* d_poses_out, uwt_stats* d_stats_out_or_null);
/* The same, synchronous, results in host memory (UWT_ERR_PAIR_FAILED when a pair failed, its status in its uwt_stats). */
int uwt_estimate_pose_candidates_batch(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                       double threshold, float* poses_out, uwt_stats* stats_out_or_null);
/* The same under the call's own weights and sampler (uwt_table_options, above): the context's weights and sampler are neither read
 * nor changed, and the call does not refuse on them; the context's schedule and solver constants, the early-exit polls, the
 * arguments and their checks, ordering against uploads, asynchrony and failure per pair are those of the entries above.
 * opt_or_null null or {0, 0}: the code of the entries above, the same bytes.  A bad option: UWT_ERR_INVALID_ARG with nothing
 * enqueued.  Otherwise, for every pair, pose and uwt_stats are what uwt_obtain_candidate_points per level followed by
 * uwt_estimate_pose_points give on a context whose params carry these weights and sampler (f64 sums whatever accumulate_f64
 * says, as there); launches per evaluation, grouping and the independence of batch, place and uwt_tuning as described at
 * uwt_track_features_batch_opt_async. */
int uwt_track_candidates_batch_opt_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                         double threshold, const uwt_table_options* opt_or_null, float* d_poses_out,
                                         uwt_stats* d_stats_out_or_null);
int uwt_estimate_pose_candidates_batch_opt(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                           double threshold, const uwt_table_options* opt_or_null, float* poses_out,
                                           uwt_stats* stats_out_or_null);

/* ---- descriptor matching for a batch of pairs: the matching half of RobustMatcher::DetectAndTrackFeatures -------------- */

/* System::Tracking's second call, robust_matcher_->DetectAndTrackFeatures(previous, current, usekeypoints) (src/System.cpp:203,
 * src/Tracker.cpp:171-258), has four parts.  Built here: matcher->knnMatch(.., 2) in both directions (:202-203, :224-225), the two
 * ratioTest calls and symmetryTest (:52-102, :229-236), and, since round 10, ransacTest (:106-169) as the inlier selection of
 * uwt_ransac_inliers_batch below — under a contract of this library's own, because cv::findFundamentalMat draws from OpenCV's RNG
 * and cannot be pinned.  Detection and description with cuda::SURF_CUDA (:184-206), since round 11, are uwt_surf_detect_describe_batch
 * and uwt_surf_describe_batch further below, under a contract of the same kind, and with cuda::ORB (:207-222), since round 16,
 * uwt_orb_detect_describe_batch and uwt_orb_describe_batch behind them, whose 32-byte rows are matched under UWT_NORM_HAMMING.
 * getGoodKeypoints (:260-270) is a host gather in the mirrors (include/uw_tracker.hpp, uw-slam_amd/tracker.py).
 *
 * Per pair: a query set A (n rows, the previous frame) and a train set B (m rows, the current frame) of descriptors of `dim`
 * elements.
 * Distance, as cv::DMatch::distance, a float:
 *   UWT_NORM_L2       dim floats per row (SURF: 64, extended 128):  s = 0.f; for k = 0 .. dim-1 { d = a[k] - b[k]; s = s + d * d; }
 *                     dist = sqrtf(s) — every step in f32, in that order, no FMA, sqrtf correctly rounded.  OpenCV's CUDA
 *                     brute-force matcher sums the same squared differences in an order of its own, which is not pinned here (no
 *                     OpenCV build is): its distances may differ from these in the last bits.  The |a|^2 + |b|^2 - 2ab
 *                     expansion is NOT used: on real descriptors it is a different function.
 *   UWT_NORM_HAMMING  dim bytes per row (ORB: 32): the popcount of the XOR, converted to float.  Exact.
 * 2-NN, knnMatch(query, train, k = 2): for query row i, idx0 = argmin_j dist(i, j), idx1 = argmin_{j != idx0} dist(i, j); a tie goes
 * to the LOWEST j in both (a sequential scan with <).  With m < 2 the row has fewer than two neighbours: idx1 = -1, d1 = 0 (and
 * idx0 = -1, d0 = 0 when m = 0).  dist(i, j) is the same bits seen from either direction.  Non-finite distances (NaN or infinite
 * descriptors, squares that overflow) are the caller's error: unspecified.
 * Ratio test: a row survives iff it has two neighbours and !(d0 / d1 > ratio), an f32 division (the reference's ratio_ is 0.65f).
 * The negated form matters: a row whose two nearest are both at distance 0 (0 / 0 is NaN) SURVIVES, as in the reference.
 * Symmetry test: (i, j, d0) for every surviving forward row i with idx0 = j whose backward row j (query B, train A) survives with
 * idx0 = i; ascending i, at most one entry per i; distance is the forward d0.
 *
 * query / train: HOST arrays of n_pairs x cap x dim elements, pair p's rows from p * cap * dim on (the fixed-stride layout of
 * keypoints_xy); n_query[p], n_train[p] in 0..cap.  A pair with n < 2 or m < 2 has no match (count 0: one direction has no second
 * neighbour); that is no error.
 * UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: n_pairs < 1, cap < 1, a null list, a count outside 0..cap,
 * dim < 1, a dim that is not a multiple of 4 (floats for L2, bytes for Hamming), a non-finite ratio, an unknown norm.
 * UWT_ERR_CAPACITY likewise: cap > UWT_MATCH_MAX_ROWS or a row longer than UWT_MATCH_MAX_ROW_BYTES.  n_pairs is NOT bounded by
 * max_pairs.  The calls are independent of the context's frame geometry and params and change neither.  Scratch (both descriptor
 * sets, the 2-NN records of both directions) belongs to the context, grows on demand and is freed by uwt_destroy.  Uploads and
 * launches go on the context's stream in order.  A pair's output depends neither on the batch it runs in, nor on its place there,
 * nor on uwt_tuning. */
enum uwt_norm { UWT_NORM_L2 = 0, UWT_NORM_HAMMING = 1 };
#define UWT_MATCH_MAX_ROWS 4096       /* descriptors per set (cap) at most */
#define UWT_MATCH_MAX_ROW_BYTES 512   /* bytes per descriptor at most: 128 floats (SURF extended), 512 bytes of a binary descriptor */

typedef struct uwt_match { int32_t query_idx, train_idx; float distance; } uwt_match;   /* cv::DMatch without imgIdx */
typedef struct uwt_knn2 { int32_t idx0, idx1; float d0, d1; } uwt_knn2;                 /* -1: no such neighbour */

/* matcher->knnMatch(descQ, descT, matches, 2) for n_pairs pairs — the per-stage entry.  out: n_pairs x cap records, pair p's row i
 * at out[p * cap + i]; the rows past n_query[p] are not written. */
int uwt_knn_match_batch(uwt_ctx* ctx, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                        const void* train, const int32_t* n_train, int32_t cap, uwt_knn2* out);
/* knnMatch both ways + ratioTest both ways + symmetryTest (src/Tracker.cpp:202-236).  matches_out: n_pairs x cap, pair p's
 * counts_out[p] matches from matches_out[p * cap] on; the rows past the count are not written. */
int uwt_match_descriptors_batch(uwt_ctx* ctx, int32_t n_pairs, int32_t norm, int32_t dim, const void* query, const int32_t* n_query,
                                const void* train, const int32_t* n_train, int32_t cap, float ratio, uwt_match* matches_out,
                                int32_t* counts_out);
/* The same without waiting: results in DEVICE memory (d_matches_out: n_pairs x cap uwt_match, d_counts_out: n_pairs), on the
 * context's stream; uwt_sync() to wait.  Host arrays from uwt_host_alloc are read when the copy runs and must stay untouched until
 * then; any other host array may be reused once the call returns (the runtime has staged it).  The context's scratch is reused by
 * the next matching call, which the stream orders behind this one.
 * alignment: d_matches_out 4 bytes, d_counts_out 4 bytes. */
int uwt_match_descriptors_batch_async(uwt_ctx* ctx, int32_t n_pairs, int32_t norm, int32_t dim, const void* query,
                                      const int32_t* n_query, const void* train, const int32_t* n_train, int32_t cap, float ratio,
                                      uwt_match* d_matches_out, int32_t* d_counts_out);

/* ---- RANSAC inlier selection for a batch of pairs: RobustMatcher::ransacTest -------------------------------------------- */

/* RobustMatcher::ransacTest(symMatches, keypoints1, keypoints2, goodMatches) (src/Tracker.cpp:105-169, called at :237).  The only
 * output of ransacTest that reaches the tracker is the INLIER SUBSET of the matches (goodMatches, :131-140): the fundamental matrix
 * it computes goes to a local that shadows the returned one (:110 / :124), and so does the 8-point refit of refineF_ (:141-166) —
 * the refit therefore has no device form, and the hypothesis solver only has to rank hypotheses by their inlier count.  The
 * semantics and constants of ransacTest are kept: distance_ = 3.0 to the epipolar line, confidence_ = 0.99 (include/Tracker.h:82-83),
 * the larger of the two squared point-to-line distances as the error, the adaptive iteration count, "a model needs more than
 * modelPoints - 1 inliers and strictly more than the best so far".  Which samples OpenCV draws and how its 7-point solver rounds is
 * not pinned (no OpenCV build is); instead this is the contract, complete, in which EVERY operation on the device is an
 * IEEE f64 add, subtract, multiply, divide or compare, or integer arithmetic (no square root, no SVD, no transcendental; no FMA),
 * so that tests/ransac_ref.py restates it in numpy and the device agrees with it bit for bit.
 *
 * Per pair: N matches (q_i, t_i); (x_i, y_i) = kp_prev[q_i], (x'_i, y'_i) = kp_cur[t_i], f32 converted to f64.  Parameters:
 * uwt_ransac_params.  N < 8: no inliers (OpenCV's 7-point solver would take N = 7; this contract does not).
 * Sample of hypothesis h (h = 0, 1, ...): mix(x) on uint32 is x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
 *   x ^= x >> 16.  For slot s = 0..7: u = mix(seed ^ mix(8 * h + s)), j = (u * (N - s)) >> 32 (64-bit product), then j steps past
 *   the indices already taken, in ascending order (for e in sorted(taken): if j >= e: j += 1).  Eight distinct indices that depend
 *   on (seed, h, N) alone.
 * Hypothesis: the 8 x 9 matrix M with rows [x'x, x'y, x', y'x, y'y, y', x, y, 1] (each product one multiply).  Gauss-Jordan
 *   elimination with full pivoting, at most eight steps.  A step scans the rows and columns not yet used, rows outermost, both
 *   ascending, from best = 0; an entry v takes over iff |v| > best (ties: lowest row, then lowest column; a NaN never wins).  If no
 *   entry takes over, the elimination ends early (the sample is rank-deficient).  An infinite pivot makes the hypothesis invalid
 *   (inlier count 0).  Otherwise the pivot's row is divided by the pivot (all nine columns), and from EVERY other row r — used or
 *   not — g * row is subtracted, g = M[r, c] read before the row changes: element by element one multiply, one subtract.  Then the
 *   free column c* is the lowest unused column: f[c*] = 1, f = 0 in the other unused columns, f[c] = -M[r_c, c*] for each pivot
 *   (r_c, c).  F = f, row-major 3 x 3.  No rank-2 enforcement, no normalisation.
 * Error of match i under F, every expression left to right:
 *   a = F0*x + F1*y + F2;  b = F3*x + F4*y + F5;  c = F6*x + F7*y + F8;  s2 = x'*a + y'*b + c;  d2 = s2*s2 / (a*a + b*b);
 *   a1 = F0*x' + F3*y' + F6;  b1 = F1*x' + F4*y' + F7;  c1 = F2*x' + F5*y' + F8;  s1 = x*a1 + y*b1 + c1;  d1 = s1*s1 / (a1*a1 + b1*b1);
 *   t2 = distance * distance;  inlier iff d1 <= t2 && d2 <= t2 (a NaN is not an inlier).  count_h = the number of inliers.
 * Selection, sequential by definition: best = 0; limit = H; for h = 0, 1, ... while h < limit: if count_h > max(best, 7):
 *   best = count_h, best_h = h, limit = min(limit, need(best)).  need(k) = uwt_ransac_iterations(confidence, N, k, H), computed on
 *   the host.  hypotheses_run = the h at which the loop stops.
 * Output per pair: the inlier mask of best_h (one byte per match: 1 / 0), the matches it keeps in their order, their count, and a
 *   uwt_ransac_info.  N < 8 or no hypothesis accepted: mask all 0, count 0, best_hypothesis -1, F all 0, status UWT_OK (the
 *   reference's inliers vector is zero-initialised, :122: goodMatches is empty there too); hypotheses_run is 0 for N < 8. */
#define UWT_RANSAC_MAX_HYPOTHESES 65536
typedef struct uwt_ransac_params {
  double distance;          /* distance_, pixels to the epipolar line (3.0); finite, >= 0        */
  double confidence;        /* confidence_ (0.99); in (0, 1]; 1: every one of max_hypotheses runs */
  int32_t max_hypotheses;   /* H: 1..UWT_RANSAC_MAX_HYPOTHESES (1000)                             */
  uint32_t seed;            /* of the sample sequence (0)                                         */
} uwt_ransac_params;
typedef struct uwt_ransac_info {
  int32_t status;           /* uwt_status_code of this pair */
  int32_t n_inliers, best_hypothesis, hypotheses_run;
  double F[9];              /* of best_hypothesis, row-major, scaled as the elimination leaves it (one entry is 1) */
} uwt_ransac_info;

/* {3.0, 0.99, 1000, 0}: distance_ and confidence_ of include/Tracker.h:82-83; 1000 hypotheses at most */
int uwt_default_ransac_params(uwt_ransac_params* p);
/* need(k) of the contract above: a host function, no context, no device.  H = max_hypotheses.  Returns H if confidence == 1 or
 * inliers <= 0 or n <= 0; else, in double: w = inliers / n, w8 = ((w*w)^2)^2 by three squarings, num = log(1 - confidence),
 * den = log(1 - w8), taken as -infinity when w8 >= 1; H if den >= 0 or -num >= H * (-den); else rint(num / den) (half to even;
 * 0 when every match is an inlier).  The shape of OpenCV's RANSACUpdateNumIters. */
int32_t uwt_ransac_iterations(double confidence, int32_t n, int32_t inliers, int32_t max_hypotheses);
/* ransacTest for n_pairs pairs, host in, host out, synchronous.  matches: n_pairs x cap uwt_match, pair p's n_matches[p] matches
 * from matches[p * cap] on (what uwt_match_descriptors_batch wrote); kp_prev / kp_cur: n_pairs x kp_cap x 2 floats (x, y), pair
 * p's n_kp_prev[p] / n_kp_cur[p] key points from p * kp_cap * 2 on; params: null for the defaults.  mask_out: n_pairs x cap
 * bytes, pair p's first n_matches[p] written; good_out: n_pairs x cap uwt_match, the first counts_out[p] written; info_out:
 * n_pairs records.  UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: n_pairs < 1, cap < 1, kp_cap < 1, a null
 * pointer, a count outside 0..cap / 0..kp_cap, a match index outside its key-point count, a parameter outside its range.
 * UWT_ERR_CAPACITY likewise: cap or kp_cap above UWT_MATCH_MAX_ROWS.  n_pairs is NOT bounded by max_pairs; the call is independent
 * of the context's geometry and params.  A pair's output depends neither on the batch it runs in nor on its place there.  The
 * table of need(k) is built on the host per distinct N, kept by the context and handed to the kernel. */
int uwt_ransac_inliers_batch(uwt_ctx* ctx, int32_t n_pairs, const uwt_match* matches, const int32_t* n_matches, int32_t cap,
                             const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur, const int32_t* n_kp_cur,
                             int32_t kp_cap, const uwt_ransac_params* params, uint8_t* mask_out, uwt_match* good_out,
                             int32_t* counts_out, uwt_ransac_info* info_out);
/* The same without waiting: d_matches / d_n_matches are read from DEVICE memory (what uwt_match_descriptors_batch_async wrote)
 * and the four results are left in DEVICE memory, on the context's stream; uwt_sync() to wait.  Key points and their counts are
 * host arrays, staged as in uwt_match_descriptors_batch_async.  The match indices cannot be checked on the host: the kernel checks
 * them, and a pair with an index outside its key-point count (or a match count outside 0..cap) gets UWT_ERR_INVALID_ARG in its
 * own info.status and no inliers; the other pairs are unaffected.  need(k) is not known per pair on the host here: the context
 * builds it for every N up to cap the first time these parameters are used (cap * cap / 2 logarithms, once).
 * alignment: d_matches 4 bytes, d_n_matches 4, d_mask_out 1 (byte stores), d_good_out 4, d_counts_out 4, d_info_out 8 (it holds doubles). */
int uwt_ransac_inliers_batch_async(uwt_ctx* ctx, int32_t n_pairs, const uwt_match* d_matches, const int32_t* d_n_matches,
                                   int32_t cap, const float* kp_prev, const int32_t* n_kp_prev, const float* kp_cur,
                                   const int32_t* n_kp_cur, int32_t kp_cap, const uwt_ransac_params* params, uint8_t* d_mask_out,
                                   uwt_match* d_good_out, int32_t* d_counts_out, uwt_ransac_info* d_info_out);

/* ---- SURF detection and description: the first part of RobustMatcher::DetectAndTrackFeatures --------------------------------- */

/* cuda::SURF_CUDA surf; surf(img, mask, keypoints, descriptors, useProvided) (src/Tracker.cpp:186-206; the tracker is built with
 * RobustMatcher(0), :273, so SURF is the live detector).  SURF_CUDA's internals (its scaled Haar patterns, fastAtan2, its own
 * interpolation) are not reproducible from the reference tree and no OpenCV build is pinned; as with ransacTest this is
 * SURF — Bay et al.'s fast-Hessian detector and 64-element descriptor — under a contract of this library's own, complete here, built
 * only from integer arithmetic and IEEE f32 / f64 add, subtract, multiply, divide, compare, floorf and sqrtf (no FMA, no angle
 * function), so that tests/surf_ref.py restates it in numpy and the device agrees with it bit for bit.  Parameters:
 * uwt_surf_params, defaults those of SURF_CUDA (hessianThreshold 100, 4 octaves, 2 layers per octave, not extended, not upright).
 * Not built: masks, the extended 128-element descriptor.  ORB is the section after this one.
 *
 * Integral image.  From the level-0 u8 plane of a slot (w x h): I is (h + 1) x (w + 1) uint32, I[y][x] = the sum of the pixels
 *   above and left of (x, y), modulo 2^32.  box(x0, y0, x1, y1) = I[y1][x1] - I[y0][x1] - I[y1][x0] + I[y0][x0] in uint32 arithmetic,
 *   then widened to int64: the sum over [x0, x1) x [y0, y1).  A CLIPPED box first clamps x0, x1 to [0, w] and y0, y1 to [0, h].
 * Layers.  L = n_octave_layers + 2 response layers per octave.  Octave o, layer i has filter size s = (9 + 6 i) << o on the grid of
 *   step 1 << o: gw = w >> o by gh = h >> o points, point (gx, gy) centred on pixel (gx << o, gy << o).  Its window is the s x s
 *   pixels from (cx - (s >> 1), cy - (s >> 1)) on (an even size has its centre at window pixel s / 2); a response exists only where
 *   the whole window lies inside the image.  An octave whose largest filter, (9 + 6 (L - 1)) << o, exceeds min(w, h) is skipped.
 * Response.  The 9 x 9 box patterns are scaled to the nearest pixel: pattern coordinate c = 0..9 is window coordinate
 *   p(c) = (c s + 4) / 9 (integer division; s is a multiple of 3, so no tie arises).  In window coordinates (x0, y0, x1, y1):
 *     Dxx = box(p0, p2, p9, p7) - 3 box(p3, p2, p6, p7)        Dyy = box(p2, p0, p7, p9) - 3 box(p2, p3, p7, p6)
 *     Dxy = box(p1, p1, p4, p4) + box(p5, p5, p8, p8) - box(p5, p1, p8, p4) - box(p1, p5, p4, p8)
 *   (32 corners) in int64; num = 100 Dxx Dyy - 81 Dxy Dxy in int64; response = (double)num / (100.0 * s2 * s2), s2 = (double)(s s):
 *   one conversion, one f64 division (the denominator is exact).  Laplacian sign = the sign of Dxx + Dyy: 1, -1 or 0.
 * Candidates.  A point of a middle layer (i = 1 .. L - 2) with response > hessian_threshold and strictly greater than all 26
 *   neighbours (layers i - 1 .. i + 1, gx - 1 .. gx + 1, gy - 1 .. gy + 1), every one of which must exist.
 * Refinement, in f64, R(dl, dy, dx) the neighbour's response, v = R(0, 0, 0), every expression left to right:
 *     gx' = (R(0,0,1) - R(0,0,-1)) * 0.5    gy' = (R(0,1,0) - R(0,-1,0)) * 0.5    gs' = (R(1,0,0) - R(-1,0,0)) * 0.5
 *     dxx = (R(0,0,1) - 2.0 * v) + R(0,0,-1)    dyy = (R(0,1,0) - 2.0 * v) + R(0,-1,0)    dss = (R(1,0,0) - 2.0 * v) + R(-1,0,0)
 *     dxy = (((R(0,1,1) - R(0,1,-1)) - R(0,-1,1)) + R(0,-1,-1)) * 0.25
 *     dxs = (((R(1,0,1) - R(1,0,-1)) - R(-1,0,1)) + R(-1,0,-1)) * 0.25
 *     dys = (((R(1,1,0) - R(1,-1,0)) - R(-1,1,0)) + R(-1,-1,0)) * 0.25
 *   and [dxx dxy dxs; dxy dyy dys; dxs dys dss] (ox, oy, os)^T = (b0, b1, b2) = (-gx', -gy', -gs') is solved by elimination without
 *   pivoting in the order x, y, layer:
 *     p0 = dxx;  m1 = dxy / p0;  m2 = dxs / p0;
 *     a11 = dyy - m1 * dxy;  a12 = dys - m1 * dxs;  c1 = b1 - m1 * b0;  a21 = dys - m2 * dxy;  a22 = dss - m2 * dxs;  c2 = b2 - m2 * b0;
 *     p1 = a11;  m3 = a21 / p1;  p2 = a22 - m3 * a12;  c2 = c2 - m3 * c1;
 *     os = c2 / p2;  oy = (c1 - a12 * os) / p1;  ox = ((b0 - dxy * oy) - dxs * os) / p0.
 *   The candidate is dropped if p0, p1 or p2 is 0 or unless |ox| <= 1, |oy| <= 1 and |os| <= 1 (a NaN drops it).  Then, each rounded
 *   to f32 once: x = ((double)gx + ox) * (double)(1 << o), y likewise, size = (double)s + os * (double)(6 << o), response = v.
 *   octave = o; laplacian = the Laplacian sign at (i, gx, gy).
 * Order and capacity.  Survivors are ordered by (octave, layer i, gy, gx) ascending.  If there are more than cap, the cap first by
 *   (the f32 response descending, order ascending) are kept, and reported in the order above.
 * Orientation (upright: the direction is (1, 0)).  sc = size * 0.13333334f (1.2 / 9).  rnd(v) = (int)floorf(v + 0.5f).
 *   haar(px, py, hh): dx = clipped box(px, py - hh, px + hh, py + hh) - clipped box(px - hh, py - hh, px, py + hh) (right minus left),
 *   dy = clipped box(px - hh, py, px + hh, py + hh) - clipped box(px - hh, py - hh, px + hh, py) (bottom minus top), int64, each
 *   converted to f32 once.  hh = max(1, rnd(2.0f * sc)) (side 4 sigma).  Samples: the grid points (i, j), -6 <= i, j <= 6,
 *   i i + j j < 36, j outermost, both ascending (109 of them): (dx, dy) = haar(rnd(x + (float)i * sc), rnd(y + (float)j * sc), hh),
 *   wx = W[|j|][|i|] * dx, wy = W[|j|][|i|] * dy with UWT_SURF_ORI_WEIGHT (exp(-(i i + j j) / 12.5): sigma 2.5), row-major 7 x 7:
 *   1.0f, 0.923116326f, 0.726149023f, 0.486752242f, 0.27803731f, 0.135335281f, 0.0561347641f,
 *   0.923116326f, 0.852143764f, 0.670320034f, 0.449328959f, 0.256660789f, 0.12493021f, 0.0518189184f,
 *   0.726149023f, 0.670320034f, 0.52729243f, 0.353454679f, 0.201896518f, 0.0982735828f, 0.0407622047f,
 *   0.486752242f, 0.449328959f, 0.353454679f, 0.236927763f, 0.135335281f, 0.0658747554f, 0.0273237228f,
 *   0.27803731f, 0.256660789f, 0.201896518f, 0.135335281f, 0.0773047432f, 0.0376282558f, 0.0156075582f,
 *   0.135335281f, 0.12493021f, 0.0982735828f, 0.0658747554f, 0.0376282558f, 0.0183156393f, 0.00759701384f,
 *   0.0561347641f, 0.0518189184f, 0.0407622047f, 0.0273237228f, 0.0156075582f, 0.00759701384f, 0.00315111154f
 *   Windows: UWT_SURF_ORI_DIR, U[k] = (cos, sin)(10 k degrees), k = 0..35:
 *   1.0f, 0.0f, 0.98480773f, 0.173648179f, 0.939692616f, 0.342020154f, 0.866025388f, 0.5f,
 *   0.766044438f, 0.642787635f, 0.642787635f, 0.766044438f, 0.5f, 0.866025388f, 0.342020154f, 0.939692616f,
 *   0.173648179f, 0.98480773f, 0.0f, 1.0f, -0.173648179f, 0.98480773f, -0.342020154f, 0.939692616f,
 *   -0.5f, 0.866025388f, -0.642787635f, 0.766044438f, -0.766044438f, 0.642787635f, -0.866025388f, 0.5f,
 *   -0.939692616f, 0.342020154f, -0.98480773f, 0.173648179f, -1.0f, 0.0f, -0.98480773f, -0.173648179f,
 *   -0.939692616f, -0.342020154f, -0.866025388f, -0.5f, -0.766044438f, -0.642787635f, -0.642787635f, -0.766044438f,
 *   -0.5f, -0.866025388f, -0.342020154f, -0.939692616f, -0.173648179f, -0.98480773f, 0.0f, -1.0f,
 *   0.173648179f, -0.98480773f, 0.342020154f, -0.939692616f, 0.5f, -0.866025388f, 0.642787635f, -0.766044438f,
 *   0.766044438f, -0.642787635f, 0.866025388f, -0.5f, 0.939692616f, -0.342020154f, 0.98480773f, -0.173648179f
 *   Sample (wx, wy) belongs to window k iff U[k].x * wy - U[k].y * wx >= 0 and wx * U[k+6].y - wy * U[k+6].x > 0 (k + 6 modulo 36;
 *   each cross product two f32 multiplies and one subtract).  Per window, from 0: sx = sx + wx, sy = sy + wy over its samples in
 *   sample order; n2 = sx * sx + sy * sy.  The window with the largest n2 wins, the lowest k on a tie.  n = sqrtf(sx * sx + sy * sy);
 *   (dir_x, dir_y) = (sx / n, sy / n), or (1, 0) when n == 0.
 * Descriptor.  (c, s) = (dir_x, dir_y); hh = max(1, rnd(sc)) (side 2 sigma).  Sample (tx, ty), 0 <= tx, ty < 20, of the 20 sigma
 *   window: rx = ((float)tx - 9.5f) * sc, ry = ((float)ty - 9.5f) * sc; at pixel corner (rnd(x + (rx * c - ry * s)),
 *   rnd(y + (rx * s + ry * c))) (dx, dy) = haar(.., hh); g = G[k(tx)] * G[k(ty)], k(t) = t < 10 ? 9 - t : t - 10, with
 *   UWT_SURF_DESC_GAUSS (exp(-(k + 0.5)^2 / (2 * 3.3^2))):
 *   0.988587201f, 0.901851177f, 0.750541389f, 0.569815516f, 0.394651532f,
 *   0.249352202f, 0.143725067f, 0.0755738765f, 0.0362518989f, 0.0158638898f
 *   wdx = g * dx, wdy = g * dy; rotated into the key point's frame: ex = wdx * c + wdy * s, ey = wdy * c - wdx * s.  Sub-region (a, b),
 *   0 <= a, b < 4, holds tx = 5 a + u, ty = 5 b + v; from 0, over v outermost and u innermost: sum = sum + e for e = ex, ey, |ex|,
 *   |ey|: elements 4 (4 b + a) + 0..3.  Norm: q[l] = d[l] * d[l]; for m = 32, 16, 8, 4, 2, 1: q[l] = q[l] + q[l ^ m] (all l at
 *   once); n = sqrtf(q[0]); the descriptor is d[l] / n, or 64 zeros when n == 0.
 * A frame's output depends neither on the batch it is in, nor on its place there, nor on uwt_tuning, nor on the order in which the
 * device happens to find the candidates. */
typedef struct uwt_keypoint {
  float x, y, size, response, dir_x, dir_y;   /* pixels; the filter size; the Hessian response; the unit direction        */
  int32_t octave, laplacian;                   /* 0..3; the sign of the Laplacian: 1, -1, 0                                */
} uwt_keypoint;
typedef struct uwt_surf_params {
  double hessian_threshold;   /* 100; finite                                                 */
  int32_t n_octaves;          /* 4; 1..4                                                     */
  int32_t n_octave_layers;    /* 2; 1..4: n_octave_layers + 2 response layers per octave     */
  int32_t upright;            /* 0; != 0: no orientation, every direction is (1, 0)          */
} uwt_surf_params;

/* {100.0, 4, 2, 0} */
int uwt_default_surf_params(uwt_surf_params* p);
/* cv::KeyPoint::angle of a direction: atan2(dir_y, dir_x) in double, in degrees in [0, 360).  A host function, outside the bit
 * contract. */
double uwt_keypoint_angle_deg(float dir_x, float dir_y);
/* Detection and description of the frames resident in slots[0 .. n_frames), host out, synchronous.  params: null for the defaults.
 * kp_out: n_frames x cap records, frame f's counts_out[f] key points from kp_out[f * cap] on; desc_out_or_null: n_frames x cap x 64
 * floats, the fixed-stride layout uwt_match_descriptors_batch takes as query / train (null: detection only, directions included).
 * The rows past a frame's count are not written.  A frame too small for octave 0, or a flat one, has count 0; that is no error.
 * UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: n_frames < 1, cap < 1, a null list or output, a slot out of
 * range, a non-finite threshold, n_octaves or n_octave_layers outside 1..4.  UWT_ERR_CAPACITY likewise: cap > UWT_MATCH_MAX_ROWS.
 * n_frames is NOT bounded by max_frames (a slot may appear twice).  Scratch (integral images, the candidates, the results) belongs to
 * the context, grows on demand and is sized per chunk of frames: a large batch runs as several chunks. */
int uwt_surf_detect_describe_batch(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params_or_null,
                                   int32_t cap, uwt_keypoint* kp_out, float* desc_out_or_null, int32_t* counts_out);
/* The same without waiting: results in DEVICE memory (d_kp_out: n_frames x cap, d_desc_out_or_null: n_frames x cap x 64,
 * d_counts_out: n_frames) on the context's stream, ordered against uwt_upload_frames_async; uwt_sync() to wait.  As in the host form, the
 * rows past a frame's count are not written: they keep what they held.
 * alignment: d_kp_out 4 bytes, d_desc_out_or_null 4 bytes (a set that goes on to uwt_match_descriptors_device_async needs its 16),
 * d_counts_out 4 bytes. */
int uwt_surf_detect_describe_batch_async(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params_or_null,
                                         int32_t cap, uwt_keypoint* d_kp_out, float* d_desc_out_or_null, int32_t* d_counts_out);
/* useProvidedKeypoints (src/Tracker.cpp:192-195): orientation and descriptors at the caller's key points.  keypoints_in: n_frames x
 * cap records, frame f's n_in[f] (0..cap) from keypoints_in[f * cap] on; x, y and size are read (finite, |x|, |y| <= 1e6,
 * 0 < size <= 4096, else UWT_ERR_INVALID_ARG), response, octave and laplacian pass through.  kp_out (may be keypoints_in): the same
 * records with their directions; desc_out: n_frames x cap x 64 floats.  Errors as above. */
int uwt_surf_describe_batch(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const uwt_surf_params* params_or_null,
                            const uwt_keypoint* keypoints_in, const int32_t* n_in, int32_t cap, uwt_keypoint* kp_out,
                            float* desc_out);
/* Per-stage entries.  The integral image of a slot: (h + 1) x (w + 1) uint32 to host memory. */
int uwt_surf_integral(uwt_ctx* ctx, int32_t slot, uint32_t* out);
/* One response layer (octave 0..3, layer 0..5) on its octave's grid: *gw x *gh doubles (w >> octave by h >> octave) to host
 * memory, NaN where no response exists. */
int uwt_surf_response_layer(uwt_ctx* ctx, int32_t slot, int32_t octave, int32_t layer, double* out, int32_t* gw, int32_t* gh);

/* ---- ORB detection and description: RobustMatcher(1) ------------------------------------------------------------------------ */

/* cuda::ORB::create() and orb->detectAndCompute(img, mask, keypoints, descriptors, useProvided) on both frames, followed by a
 * NORM_HAMMING brute-force matcher (src/Tracker.cpp:210-223; RobustMatcher(int detector), :38-46, chooses it with detector = 1).
 * cuda::ORB cannot be pinned: no OpenCV build is, and its learned table of 256 sampling pairs is not in the reference
 * tree.  As with ransacTest and SURF this is ORB — Rublee et al.'s FAST-9/16 corners on a 1.2 x scale pyramid, Harris ranking,
 * intensity-centroid orientation and a 256-bit steered BRIEF descriptor — under a contract of this library's own, complete here,
 * built only from integer arithmetic and IEEE f32 / f64 add, subtract, multiply, divide, compare, floorf and sqrtf (no FMA, no angle
 * function), so that tests/orb_ref.py restates it in numpy and the device agrees with it bit for bit.  Parameters: uwt_orb_params,
 * defaults those of cuda::ORB::create(): 500 features, scale 1.2, 8 levels, edge threshold 31, first level 0, WTA_K 2, Harris score,
 * patch 31, FAST threshold 20, no blur before description.  The sampling pattern is DATA of the context (uwt_orb_set_pattern): the
 * default is the recipe below, not OpenCV's table — the one distance from OpenCV a caller who has that table can close themselves.
 * Not built: masks, WTA_K 3 / 4, FAST-score ranking, blur before description, a scale other than 1.2, a first level other than 0.
 * Built since round 18: an ORB branch of uwt_tracking_batch — uwt_tracking_orb_batch, in the section after this one (the SURF call's
 * params struct is pinned at 56 bytes, so the branch has a record and entry points of its own).
 *
 * Scale pyramid.  Integer, every layer from the level-0 u8 plane of the slot (w x h) alone; independent of the context's tracking
 *   pyramid.  The scale of layer l = 0 .. n_levels - 1 is the exact rational 6^l / 5^l.  Layer width w_l = (w 5^l + 6^l / 2) / 6^l
 *   in int64, rounding down; h_l likewise from h (uwt_orb_layer_size).  Layer 0 is the plane itself.  Layer l > 0 is a bilinear
 *   resampling with pixel-centre alignment and 11-bit weights: for destination x, N = (2 x + 1) w - w_l, x0 = N / (2 w_l),
 *   fx = ((N mod 2 w_l) * 2048) / (2 w_l), x1 = min(x0 + 1, w - 1); y0, fy, y1 likewise from y, h, h_l (integer divisions); the value is
 *   (I[y0][x0] (2048 - fx)(2048 - fy) + I[y0][x1] fx (2048 - fy) + I[y1][x0] (2048 - fx) fy + I[y1][x1] fx fy + 2^21) >> 22 in
 *   uint32 (it cannot overflow).  With w_l = w the formula gives the pixel itself.
 * Candidate band.  Only pixels at least edge_threshold from every border of their layer are candidates: e <= x < w_l - e and
 *   e <= y < h_l - e.  A layer with w_l or h_l below 2 e + 1 (2 * 31 + 1 by default) has none.  edge_threshold is at least 16, so
 *   every later read (ring, 7 x 7 Harris block plus 1, radius-15 patch, rotated pattern) is inside the layer by construction.
 * FAST.  The Bresenham ring of 16 at radius 3, (dx, dy) clockwise from the top — UWT_ORB_RING:
 *   (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3)
 *   With p the pixel and r_i the ring, d_i = r_i - p (int).  bright = max over i = 0..15 of min(d_i, d_{i+1}, .., d_{i+8}) (indices
 *   modulo 16: the 16 arcs of 9 contiguous ring pixels); dark = the same with -d_i; score = max(bright, dark).  A candidate is a
 *   corner iff score > fast_threshold; the score map S holds the score of a corner and 0 everywhere else (non-corners, pixels
 *   off the band): uwt_orb_fast_scores.  Non-maximum suppression keeps a corner iff S there is strictly greater than S at all 8
 *   neighbours.
 * Harris measure of a kept corner (x, y), in integers: at each of the 49 pixels (u, v) of the 7 x 7 block centred on it,
 *   Ix = 2 (I[v][u+1] - I[v][u-1]) + (I[v-1][u+1] - I[v-1][u-1]) + (I[v+1][u+1] - I[v+1][u-1]),
 *   Iy = 2 (I[v+1][u] - I[v-1][u]) + (I[v+1][u-1] - I[v-1][u-1]) + (I[v+1][u+1] - I[v-1][u+1]);  a = sum Ix Ix, b = sum Iy Iy,
 *   c = sum Ix Iy;  H = 25 (a b - c c) - (a + b)(a + b) in int64 (|Ix|, |Iy| <= 1020: it cannot overflow; the factor is Harris
 *   k = 0.04 = 1 / 25).  uwt_orb_harris.
 * Quota.  Layer l keeps its n_l best corners by (H descending, y ascending, x ascending); n_l = uwt_orb_level_quota, a host
 *   function in double with + - * / and rint (half to even) only: factor = 1.0 / 1.2; fp = 1.0, multiplied by factor n_levels
 *   times; want = n_features * (1.0 - factor) / (1.0 - fp); for l = 0 .. n_levels - 2: n_l = rint(want), want = want * factor; the
 *   last layer takes the remainder max(n_features - sum, 0).  The shape of OpenCV's geometric split.
 * Order and capacity.  The survivors of all layers are ordered by (layer, y, x) ascending.  If there are more than cap, the cap
 *   first by (H descending, then that order) are kept, and reported in that order (layer, y, x).
 * Key-point record of layer position (gx, gy) on layer l, each f32 rounded once: x = (double)(gx 6^l) / (double)5^l, y likewise,
 *   size = (double)(31 6^l) / (double)5^l, response = (double)H / (25.0 * 7140^4) (7140 = 7 * 1020: the denominator, 2^8 * 25 *
 *   1785^4, is exact in double), octave = l, laplacian = 0, the direction below.
 * Provided key points (useProvidedKeypoints, src/Tracker.cpp:216-218): x, y and octave are read; the layer position is
 *   gx = (int)floor((double)x * (double)5^l / (double)6^l + 0.5), gy likewise — which returns the (gx, gy) of a record this
 *   contract wrote.  Direction and descriptor are recomputed there; the other fields pass through.
 * Orientation (upright: the direction is (1, 0)).  Over the circular patch of radius 15 around (gx, gy) — row v = -15 .. 15 holds
 *   u = -U[|v|] .. U[|v|] with UWT_ORB_UMAX, U = 15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3 — the integer sums
 *   m10 = sum u I[gy+v][gx+u], m01 = sum v I[gy+v][gx+u] (both below 2^24: the conversion to f32 is exact).  fx = (float)m10,
 *   fy = (float)m01, n = sqrtf(fx * fx + fy * fy); (dir_x, dir_y) = (fx / n, fy / n), or (1, 0) when n == 0.  There is no angle;
 *   uwt_keypoint_angle_deg stays the host convenience it is.
 * Descriptor.  (c, s) = (dir_x, dir_y); rnd(v) = (int)floorf(v + 0.5f).  Test k = 0..255 has pattern entry (x0, y0, x1, y1), int8
 *   converted to f32: p0 = (rnd(x0 * c - y0 * s), rnd(x0 * s + y0 * c)), p1 likewise from (x1, y1) (each two f32 multiplies and one
 *   subtract or add); bit k = I[gy + p0.y][gx + p0.x] < I[gy + p1.y][gx + p1.x] on the layer image; it goes into byte k / 8 at
 *   position k % 8.  32 bytes, the row layout uwt_match_descriptors_batch(UWT_NORM_HAMMING, 32, ..) takes.
 * Pattern.  256 x 4 int8 held by the context; valid iff every point has x x + y y <= 225.  The default, uwt_orb_default_pattern:
 *   with mix() of the RANSAC contract above and the counter n = 0, draw(n) = (int)((mix(0x6f726221 ^ mix(n)) * 21) >> 32) - 10
 *   (64-bit product: a coordinate in [-10, 10]); entry k = 0..255 in turn takes (draw(n), draw(n + 1), draw(n + 2), draw(n + 3))
 *   and n += 4, again while its two points coincide.
 * A frame's output depends neither on the batch it is in, nor on its place there, nor on uwt_tuning, nor on the order in which the
 * device happens to find the candidates. */
typedef struct uwt_orb_params {
  int32_t n_features;       /* 500; 1..65536: what the layers' quotas sum to (*)              */
  int32_t n_levels;         /* 8; 1..8                                                         */
  int32_t edge_threshold;   /* 31; 16..1024                                                    */
  int32_t fast_threshold;   /* 20; 0..255                                                      */
  int32_t upright;          /* 0; != 0: no orientation, every direction is (1, 0)              */
} uwt_orb_params;

/* (*) where the rounding of the first layers overshoots, the last layer's max(.., 0) leaves the sum one above n_features: of all
 * n_features below 3000 and every n_levels this happens once, for 7 features over 8 layers (2, 1, 1, 1, 1, 1, 1, 0). */
/* {500, 8, 31, 20, 0} */
int uwt_default_orb_params(uwt_orb_params* p);
/* Host functions of the contract above; no context, no device.  n_l for l = 0 .. n_levels - 1 (n_features >= 0, n_levels 1..8). */
int uwt_orb_level_quota(int32_t n_features, int32_t n_levels, int32_t* out);
/* the default pattern: 256 x (x0, y0, x1, y1) */
int uwt_orb_default_pattern(int8_t* out_1024);
/* (w_l, h_l) of layer `level` (0..7) of a w x h frame */
int uwt_orb_layer_size(int32_t w, int32_t h, int32_t level, int32_t* lw, int32_t* lh);
/* Loads another pattern into the context (OpenCV's, for a caller who has it), for every ORB call after this one; null restores
 * the default.  UWT_ERR_INVALID_ARG, the pattern in force unchanged, if a point has x x + y y > 225. */
int uwt_orb_set_pattern(uwt_ctx* ctx, const int8_t* pattern_1024_or_null);
/* Detection and description of the frames resident in slots[0 .. n_frames), host out, synchronous.  params: null for the defaults.
 * kp_out: n_frames x cap records, frame f's counts_out[f] key points from kp_out[f * cap] on; desc_out_or_null: n_frames x cap x 32
 * bytes, the fixed-stride layout uwt_match_descriptors_batch takes as query / train (null: detection only, directions included).
 * The rows past a frame's count are not written.  A frame too small for layer 0's band, or a flat one, has count 0; that is no
 * error.  UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: n_frames < 1, cap < 1, a null list or output, a slot
 * out of range, a parameter outside the range stated at uwt_orb_params.  UWT_ERR_CAPACITY likewise: cap > UWT_MATCH_MAX_ROWS, a
 * frame wider or higher than 16384.  n_frames is NOT bounded by max_frames (a slot may appear twice).  Scratch (the layers, the
 * candidates, the results) belongs to the context, grows on demand and is sized per chunk of frames: a large batch runs as several
 * chunks.  Uploads and launches go on the context's stream in order. */
int uwt_orb_detect_describe_batch(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const uwt_orb_params* params_or_null,
                                  int32_t cap, uwt_keypoint* kp_out, uint8_t* desc_out_or_null, int32_t* counts_out);
/* The same without waiting: results in DEVICE memory (d_kp_out: n_frames x cap, d_desc_out_or_null: n_frames x cap x 32,
 * d_counts_out: n_frames) on the context's stream, ordered against uwt_upload_frames_async; uwt_sync() to wait.  As in the host form, the
 * rows past a frame's count are not written: they keep what they held.
 * alignment: d_kp_out 4 bytes, d_desc_out_or_null 4 bytes (a set that goes on to uwt_match_descriptors_device_async needs its 16),
 * d_counts_out 4 bytes. */
int uwt_orb_detect_describe_batch_async(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const uwt_orb_params* params_or_null,
                                        int32_t cap, uwt_keypoint* d_kp_out, uint8_t* d_desc_out_or_null, int32_t* d_counts_out);
/* useProvidedKeypoints: direction and descriptors at the caller's key points.  keypoints_in: n_frames x cap records, frame f's
 * n_in[f] (0..cap) from keypoints_in[f * cap] on.  A record is UWT_ERR_INVALID_ARG, with nothing enqueued, if x or y is not finite
 * or beyond 1e6 in magnitude, if its octave is outside 0 .. n_levels - 1, or if its layer position is closer than edge_threshold
 * to a border of its layer; the key points a detection on a frame of the same size kept always pass.  kp_out (may be
 * keypoints_in): the same records with their directions; desc_out: n_frames x cap x 32 bytes.  Errors as above. */
int uwt_orb_describe_batch(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const uwt_orb_params* params_or_null,
                           const uwt_keypoint* keypoints_in, const int32_t* n_in, int32_t cap, uwt_keypoint* kp_out,
                           uint8_t* desc_out);
/* Per-stage entries, host out, synchronous, under the default parameters.  One layer (level 0..7) of a slot: *lw x *lh bytes, tight
 * rows (at most w x h). */
int uwt_orb_layer(uwt_ctx* ctx, int32_t slot, int32_t level, uint8_t* out, int32_t* lw, int32_t* lh);
/* The dense score map S of a layer, after the border rule and before suppression: w_l x h_l int32. */
int uwt_orb_fast_scores(uwt_ctx* ctx, int32_t slot, int32_t level, int32_t* out);
/* H at n pixels of a layer; xy: n x (x, y), each at least 4 from every border of the layer (else UWT_ERR_INVALID_ARG). */
int uwt_orb_harris(uwt_ctx* ctx, int32_t slot, int32_t level, const int32_t* xy, int32_t n, int64_t* H_out);

/* ---- System::Tracking for a batch of pairs in one device-resident call ---------------------------------------------------------- */

/* The five calls of System::Tracking() (src/System.cpp:193-223) for n_pairs pairs, chained on the device: nothing travels to the
 * host between the stages and the asynchronous form never waits for the device.  previous = ref_slots[p], current = tgt_slots[p];
 * the frames must be in the state uwt_track_features_batch_async expects (resident, pyramids built, gradients applied), and
 * 1 <= n_pairs <= max_pairs as there.  cap: rows of every per-pair list (1..UWT_MATCH_MAX_ROWS).  Per pair p:
 *   1. use = d_prev_kp != null && d_n_prev[p] >= 1 && d_n_prev[p] >= min_matches: `usekeypoints` of src/System.cpp:195-209 together
 *      with the mirrors' "and it has some" (a frame's n_matches_ is the number of key points it kept, so the device count decides).
 *   2. The query set Q: use ? what uwt_surf_describe_batch gives at the provided records (src/Tracker.cpp:192-195) : what
 *      uwt_surf_detect_describe_batch gives on the previous frame with capacity cap.  The train set T: detection on the current
 *      frame with capacity cap.  A per-frame predicate on the device picks the path: the blocks of the other path return at once.
 *   3. symMatches = uwt_match_descriptors_batch(UWT_NORM_L2, 64, Q, T, cap, ratio).
 *   4. goodMatches and uwt_ransac_info = uwt_ransac_inliers_batch on symMatches and the (x, y) of Q and T under params.ransac.
 *   5. kept_prev[i] = Q.kp[good[i].query_idx], kept_cur[i] = T.kp[good[i].train_idx]: getGoodKeypoints (src/Tracker.cpp:260-270) on
 *      whole uwt_keypoint records.
 *   6. Pose and uwt_stats = uwt_estimate_pose_features_batch for (previous, current) with the (x, y) of the first
 *      min(n_matches, 200) rows of kept_prev.  No good match: UWT_ERR_NO_VALID_POINTS in that pair's stats, as there; the other
 *      pairs are unaffected.
 * The contract: every output of pair p is bit for bit what that staged sequence of entry points gives on the same context — no new
 * arithmetic contract.  A pair's outputs depend neither on the batch it is in, nor on its place there, nor on uwt_tuning, nor on
 * scheduling.
 * Hand-over: d_kept_cur / d_n_matches of one call are valid d_prev_kp / d_n_prev of the next call on the same context with the same
 * cap; the stream orders the calls, no uwt_sync between them.  The inputs and outputs of ONE call must not overlap (the caller keeps
 * two sets of buffers): d_prev_kp equal to d_kept_prev or d_kept_cur, or d_n_prev equal to d_n_matches, is UWT_ERR_INVALID_ARG.
 * The asynchronous call performs no device-to-host copy; the only host waits are those for a block of a pinned staging ring (the
 * pair lists), as in uwt_track_features_batch_async.
 * UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: a null list or a null required output, n_pairs outside
 * 1..max_pairs, a slot out of range, cap < 1, a SURF or RANSAC parameter outside the range its stage states, a non-finite ratio,
 * min_matches < 0, exactly one of d_prev_kp / d_n_prev null.  UWT_ERR_CAPACITY likewise: cap > UWT_MATCH_MAX_ROWS.
 * What only the device can see — a provided count outside 0..cap; a used provided record that is not finite or outside |x|, |y| <=
 * 1e6, 0 < size <= 4096; one of the first 200 kept (x, y) outside level 0 — puts UWT_ERR_INVALID_ARG into that pair's info.status
 * and uwt_stats; its n_matches is 0 and its pose the identity, as a failed pair's is.  (A pair refused for its provided list runs
 * neither path on its previous frame: n_kp_prev = n_symmetric = 0, best_hypothesis = -1.)  Every other pair is unaffected, nothing
 * faults, and uwt_tracking_batch returns UWT_ERR_PAIR_FAILED.
 * Scratch (the key points, descriptors and counts of both sides of every pair, symMatches, the RANSAC records) belongs to the
 * context, grows on demand — also under a queued asynchronous call, which is drained first — and is freed by uwt_destroy. */
typedef struct uwt_tracking_params {
  uwt_surf_params   surf;         /* uwt_default_surf_params                                         */
  uwt_ransac_params ransac;       /* uwt_default_ransac_params                                       */
  float             ratio;        /* ratio_, 0.65f (include/Tracker.h:80); finite                    */
  int32_t           min_matches;  /* 110 (src/System.cpp:208); >= 0                                  */
} uwt_tracking_params;            /* 56 bytes */

typedef struct uwt_tracking_info {   /* per pair, 32 bytes */
  int32_t status;                    /* uwt_status_code of the front end of this pair */
  int32_t used_provided;             /* 1: the previous frame was described at the provided key points */
  int32_t n_kp_prev, n_kp_cur;       /* rows of the query / train set */
  int32_t n_symmetric;               /* symMatches.size() */
  int32_t n_matches;                 /* goodMatches.size() = Frame::n_matches_ of both frames */
  int32_t best_hypothesis, hypotheses_run;   /* of uwt_ransac_info */
} uwt_tracking_info;

typedef struct uwt_tracking_io {     /* every pointer is DEVICE memory, 4-byte aligned (no record here holds a wider field) */
  const uwt_keypoint* d_prev_kp;     /* in, may be null: n_pairs x cap, what the previous frame kept */
  const int32_t*      d_n_prev;      /* in, null iff d_prev_kp is: n_pairs counts */
  float*              d_poses;       /* out: n_pairs x 7 */
  uwt_stats*          d_stats;       /* out, may be null */
  uwt_tracking_info*  d_info;        /* out: n_pairs */
  uwt_match*          d_good;        /* out: n_pairs x cap, goodMatches */
  uwt_keypoint*       d_kept_prev;   /* out: n_pairs x cap, previous->surf_keypoints_ after the call */
  uwt_keypoint*       d_kept_cur;    /* out: n_pairs x cap, current->surf_keypoints_ after the call */
  int32_t*            d_n_matches;   /* out: n_pairs (= info.n_matches; the count of both kept lists) */
} uwt_tracking_io;

/* {uwt_default_surf_params, uwt_default_ransac_params, 0.65f, 110} */
int uwt_default_tracking_params(uwt_tracking_params* p);
/* Enqueued on the context's stream, ordered against uwt_upload_frames_async as uwt_track_features_batch_async is; uwt_sync() to
 * wait.  The rows past a pair's count in d_good / d_kept_prev / d_kept_cur are not written. */
int uwt_tracking_batch_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                             const uwt_tracking_params* params_or_null, int32_t cap, const uwt_tracking_io* io);
/* The same, synchronous, HOST in and out (prev_kp_or_null: n_pairs x cap, n_prev_or_null: n_pairs, both or neither); the rows past
 * a count are not written.  UWT_ERR_PAIR_FAILED when a pair failed, its status in its uwt_stats (and, for the front end, its info). */
int uwt_tracking_batch(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                       const uwt_tracking_params* params_or_null, int32_t cap,
                       const uwt_keypoint* prev_kp_or_null, const int32_t* n_prev_or_null,
                       float* poses_out, uwt_stats* stats_out_or_null, uwt_tracking_info* info_out, uwt_match* good_out,
                       uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out);
/* The same chain for RobustMatcher(1): ORB and the Hamming matcher (src/Tracker.cpp:210-223).  uwt_tracking_params is pinned and holds
 * SURF's parameters, so this detector has a record of its own; uwt_tracking_io, uwt_tracking_info and the uwt_keypoint records are
 * those above.  The contract is that of uwt_tracking_batch, steps 1-6, with these substitutions:
 *   Q: use ? what uwt_orb_describe_batch gives at the provided records : what uwt_orb_detect_describe_batch gives on the previous
 *      frame with capacity cap.  T: uwt_orb_detect_describe_batch on the current frame with capacity cap.  Both under the context's
 *      pattern in force (uwt_orb_set_pattern) and params.orb.
 *   symMatches = uwt_match_descriptors_batch(UWT_NORM_HAMMING, 32, Q, T, cap, ratio).
 * No new arithmetic: every output of a pair is bit for bit what that staged sequence gives on the same context, and depends neither on
 * the batch, nor on the pair's place there, nor on uwt_tuning, nor on scheduling.  Hand-over and aliasing: as above (d_kept_cur /
 * d_n_matches of one call are valid d_prev_kp / d_n_prev of the next, no uwt_sync between them; the inputs and outputs of one call
 * must not overlap).
 * Host-side refusals, nothing enqueued and the outputs untouched: those of uwt_tracking_batch with the ranges of uwt_orb_params in
 * place of SURF's; UWT_ERR_CAPACITY also for a frame wider or higher than 16384.
 * What only the device can see is handled as above (UWT_ERR_INVALID_ARG in that pair's info.status and uwt_stats, n_matches 0, the
 * identity pose, neither path run on its previous frame, its neighbours untouched, UWT_ERR_PAIR_FAILED from the synchronous call): a
 * provided count outside 0..cap; one of the first 200 kept (x, y) outside level 0; and a USED provided record that
 * uwt_orb_describe_batch would refuse on the host — x or y not finite or beyond 1e6 in magnitude, an octave outside 0 .. n_levels - 1,
 * a layer position closer than edge_threshold (the parameter) to a border of its layer.
 * A frame too small for layer 0's band is no front-end error: its counts are 0, info.status is UWT_OK and the pair's uwt_stats carry
 * UWT_ERR_NO_VALID_POINTS. */
typedef struct uwt_tracking_orb_params {
  uwt_orb_params    orb;          /* uwt_default_orb_params                                          */
  uwt_ransac_params ransac;       /* uwt_default_ransac_params                                       */
  float             ratio;        /* 0.65f; finite                                                   */
  int32_t           min_matches;  /* 110; >= 0                                                       */
} uwt_tracking_orb_params;        /* 56 bytes (orb: 20, 4 of padding, ransac: 24) */

/* {uwt_default_orb_params, uwt_default_ransac_params, 0.65f, 110} */
int uwt_default_tracking_orb_params(uwt_tracking_orb_params* p);
int uwt_tracking_orb_batch_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                 const uwt_tracking_orb_params* params_or_null, int32_t cap, const uwt_tracking_io* io);
int uwt_tracking_orb_batch(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                           const uwt_tracking_orb_params* params_or_null, int32_t cap,
                           const uwt_keypoint* prev_kp_or_null, const int32_t* n_prev_or_null,
                           float* poses_out, uwt_stats* stats_out_or_null, uwt_tracking_info* info_out, uwt_match* good_out,
                           uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out);
/* uwt_match_descriptors_batch_async with both descriptor sets and their counts already in DEVICE memory (d_query / d_train: n_pairs x
 * cap x dim elements, d_n_query / d_n_train: n_pairs), read in place: nothing is uploaded.  The launch is bounded by cap instead of
 * the counts (blocks past a pair's counts return at once; the merge of the train parts is exact, so the different cut shows in no
 * bit): the results are those of uwt_match_descriptors_batch.  A device count outside 0..cap is taken as 0: that pair has count 0.
 * Host-side errors as there (the counts cannot be checked on the host).
 * alignment: d_query and d_train 16 bytes (rows that are a multiple of 16 bytes long — every L2 row, Hamming rows of 16, 32, ... bytes —
 * are read with 16-byte loads; other rows a 32-bit word at a time); d_n_query, d_n_train, d_matches_out and d_counts_out 4 bytes. */
int uwt_match_descriptors_device_async(uwt_ctx* ctx, int32_t n_pairs, int32_t norm, int32_t dim, const void* d_query,
                                       const int32_t* d_n_query, const void* d_train, const int32_t* d_n_train, int32_t cap, float ratio,
                                       uwt_match* d_matches_out, int32_t* d_counts_out);

/* ---- did the alignment work: Tracker::ObtainImageTransformed and DebugShowWarpedPerspective ---------------------------------- */

/* Tracker::ObtainImageTransformed(original, candidatePoints N x 4, warpedPoints N x 4, output) (src/Tracker.cpp:1473-1525; live code
 * inside FastEstimatePose, :930) carries a frame into another frame's view and returns the mask of the pixels it covered.  The contract:
 * for rows i = 0..N-1 IN ORDER, x1 = (int)pts[i][0], y1 = (int)pts[i][1] (truncation toward zero), x2 = (int)round(warped[i][0]),
 * y2 = (int)round(warped[i][1]) (C round: halves away from zero).
 *   - A row LANDS iff y2 > 0 && y2 < rows && x2 > 0 && x2 < cols (:1483, the reference's own test: row 0 and column 0 are never
 *     written).  rows x cols: the level's image, img_h x img_w.
 *   - On landing output[y2, x2] = original[y1, x1] and valid[y2, x2] = 1.
 *   - Pixels no row lands on keep what `output` held; their valid is 0.
 *   - Ordering rule: among the rows that land on one pixel the one with the largest i wins (the reference is a sequential scatter).
 * The device form is two passes over an int32 winner plane per pair that starts at -1: every landed row does atomicMax(winner[y2, x2], i),
 * then one pass reads original[y1, x1] of each pixel's winner.  An integer maximum does not depend on the order of its operands, so the
 * result is the same bits on every run and depends neither on the batch, nor on the pair's place in it, nor on uwt_tuning, nor on
 * scheduling.
 * Deviations (in the style of SURVEY C-3):
 *   - A row whose (x1, y1) lies outside the level's image (or is not a number) is skipped: the reference would read out of bounds there.
 *   - A row whose warped u or v is not finite, or has magnitude >= 2^31 - 128, is skipped: the conversion to int is undefined there.
 * Tracker::DebugShowWarpedPerspective(image1, image2, imageWarped, lvl) (src/Tracker.cpp:1694-1737) builds the four-panel image
 *   [ image1 | image2 ] over [ blend(imageWarped, image2) | blend(image1, image2) ],  2 img_w x 2 img_h u8,
 * blend(a, b) = addWeighted(a, 0.5, b, 0.5, 1.0) = saturate_u8(cvRound(0.5 a + 0.5 b + 1)), cvRound to the even neighbour of a half: with
 * s = a + b, s / 2 + 1 for an even s, the even one of (s - 1) / 2 + 1 and (s - 1) / 2 + 2 for an odd s, capped at 255.  The reference's
 * "resize x2 while _lvl > 1" (:1729-1732) scales the window for the display and is not built; imshow / waitKey are the caller's. */
typedef struct uwt_warp_quality {   /* per pair, 48 bytes, all integers: exact and order-independent */
  int32_t status;          /* uwt_status_code of this pair */
  int32_t n_points;        /* rows considered (dense: w*h of the level's grid) */
  int32_t n_landed;        /* rows that passed the landing test */
  int32_t n_covered;       /* pixels with valid = 1 (<= n_landed; the difference is the rows that lost) */
  int64_t sum_abs;         /* over covered pixels: |warped - image2| */
  int64_t sum_sq;          /* over covered pixels: (warped - image2)^2 */
  int64_t sum_abs_unaligned; /* over the SAME covered pixels: |image1 - image2| (the "noalign" panel's content) */
  int64_t reserved;
} uwt_warp_quality;

typedef struct uwt_warp_image_io {   /* every pointer is DEVICE memory, 4-byte aligned; planes are n_pairs x pitch x img_h u8 */
  uint8_t*          d_warped;        /* out, may be null: image1 in image2's view; 0 where no row landed */
  uint8_t*          d_valid;         /* out, may be null: 1 where a row landed */
  uint8_t*          d_absdiff;       /* out, may be null: |warped - image2| where a row landed, else 0 */
  uwt_warp_quality* d_quality;       /* out, required: n_pairs records; 8-byte aligned (64-bit sums) */
} uwt_warp_image_io;

/* The reference's signature on host arrays for one frame: original = the image plane of `slot` at `lvl` (resident, pyramids built),
 * pts / warped: n x 4 floats, image_inout / valid_out: img_w x img_h u8, tight.  image_inout is honoured as input (pixels not landed on
 * keep its content).  n = 0 is UWT_OK: the image is untouched and the mask all zero.  Synchronous. */
int uwt_obtain_image_transformed(uwt_ctx* ctx, int32_t slot, int32_t lvl, const float* pts, const float* warped, int32_t n,
                                 uint8_t* image_inout, uint8_t* valid_out);
/* The dense form for a batch of pairs, ObtainAllPoints -> WarpFunction -> ObtainImageTransformed in one call: the rows are the level's
 * w x h point grid in ObtainAllPoints' order (i = y * w + x; z = depth * depth_scale / 2^lvl of the reference slot's depth plane, a point
 * whose depth read as int16 is <= 0 becomes [0 0 1 0], z = 1 without a depth plane; src/Tracker.cpp:1266-1302), warped by uwt_warp's
 * arithmetic under the pair's pose d_poses[p] (n_pairs x 7, DEVICE memory: uwt_tracking_io::d_poses and the pose buffers of the _async
 * table calls are valid inputs with no uwt_sync between the calls, the stream orders them); original = ref_slots[p]'s image plane at lvl,
 * image2 = tgt_slots[p]'s.  Pixels no row lands on are 0 in d_warped and d_absdiff.  Every output of a pair is bit for bit what
 * uwt_obtain_image_transformed gives on that table and uwt_warp's rows.
 * 1 <= n_pairs <= max_pairs; the frames must be resident with pyramids built (gradients are not needed).  Enqueued on the context's
 * stream, ordered against uwt_upload_frames_async as the other batch calls are; uwt_sync() to wait.
 * UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: a null list, a null d_poses, io or d_quality, n_pairs outside
 * 1..max_pairs, a slot or level out of range.  A pose with a non-finite entry puts UWT_ERR_INVALID_ARG into that pair's status with all
 * counts 0 and its planes zero; its neighbours are untouched.
 * alignment: d_poses 4 bytes; io: at uwt_warp_image_io (planes 4 bytes, d_quality 8). */
int uwt_warp_image_batch_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int32_t lvl,
                               const float* d_poses, const uwt_warp_image_io* io);
/* The same, synchronous, HOST in and out: poses n_pairs x 7; warped_out / valid_out / absdiff_out n_pairs x img_w x img_h u8, tight,
 * each may be null; quality_out n_pairs, required.  UWT_ERR_PAIR_FAILED when a pair failed, its status in its record. */
int uwt_warp_image_batch(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots, int32_t lvl,
                         const float* poses, uint8_t* warped_out, uint8_t* valid_out, uint8_t* absdiff_out,
                         uwt_warp_quality* quality_out);
/* The image of DebugShowWarpedPerspective for one pair: image1 = ref_slot's image plane at lvl, image2 = tgt_slot's, warped: img_w x
 * img_h u8 (host), mosaic_out: 2 img_w x 2 img_h u8 (host).  Synchronous. */
int uwt_warp_mosaic(uwt_ctx* ctx, int32_t ref_slot, int32_t tgt_slot, int32_t lvl, const uint8_t* warped, uint8_t* mosaic_out);

/* ---- the map: Visualizer::AddPointCloudFromRGBD and Map::AddPointCloudFromRGBD ------------------------------------------------- */

/* Visualizer::AddPointCloudFromRGBD(Frame*) (src/Visualizer.cpp:421-446) unprojects the frame's level-0 candidatePoints_ table, takes
 * every 100th row, offsets it by the accumulated pose's translation and appends it to point_cloud_; Map::AddPointCloudFromRGBD(Frame*)
 * (src/Map.cpp:33-45) keeps the x y z columns of that table as recent_cloud_points_.  The contract of the device form:
 * A cloud is a sequence of 16-byte records uwt_cloud_point { x, y, z, tag }, tag = intensity | (frame_index_in_call << 8), intensity =
 * image[(int)y][(int)x] (truncation toward zero: -0.5 reads column 0) at level 0 of the frame's slot, 0 where that pixel lies outside the
 * image or the coordinate is not a number.  The geometry never reads the image.
 * Frame f of a call has a level-0 table of N rows [x, y, z, w] and a pose traj[f] = qx qy qz qw tx ty tz.
 *   - Selection: rows i = 0, stride, 2 stride, ... < N IN THAT ORDER (the loop "for (i = 0; i < rows; i += 100)", :437); stride >= 1, the
 *     reference's is 100.  skip_invalid = 0 (the reference): every selected row is emitted, the [0 0 1 0] rows of zero depth included —
 *     the reference emits them, a quirk reproduced.  skip_invalid = 1 (extension): a selected row with w == 0 is dropped, the others keep
 *     their order.
 *   - Unprojection: X = ((x - cx) invfx) z, Y = ((y - cy) invfy) z with level 0's intrinsics, exactly uwt_warp's under the context's
 *     arith: the MatExpr-folded x * invfx + (float)(-(double)cx * invfx) in the OpenCV set, as written in the legacy set, then * z, all
 *     in f32.  Z = z.
 *   - mode 0, the reference's visualiser (:440-442): point = (-X - tx, -Z - tz, -Y - ty), each one f32 subtraction, t = traj[f]'s
 *     translation UNPERMUTED: the reference reads previous_pose_.translation(), not the published position, so the caller passes the
 *     accumulation made with reference_axes = 0.
 *   - mode 1, world (extension, no counterpart in the reference): point = the first three rows of T(traj[f]) [X Y Z w], T =
 *     uwt_se3_matrix's matrix, each row (float)(T0 X + ((T1 Y + T2 Z) + T3 w)) formed in f64.  This one definition holds in BOTH
 *     arithmetic sets (the legacy set's f32 chain is not used here).
 *   - Order: the cloud of a call is frame 0's points, then frame 1's, ..., each in row order — what successive push_backs give.
 *   - Independence: the bytes of a frame's points depend neither on the batch, nor on the frame's place in it (the tag's frame index
 *     apart), nor on uwt_tuning, nor on the run: where a record goes follows from counts and a scan, never from an atomic cursor.
 * Deviations (in the style of SURVEY C-3): a frame whose pose has a non-finite entry contributes no points; its record carries
 * UWT_ERR_INVALID_ARG with n_rows, n_selected and n_points 0; its neighbours are untouched. */
typedef struct uwt_cloud_point {   /* 16 bytes */
  float x, y, z;
  uint32_t tag;              /* intensity | (frame_index_in_call << 8) */
} uwt_cloud_point;

typedef struct uwt_cloud_params {   /* 32 bytes */
  int32_t mode;              /* 0: the reference's visualiser; 1: world */
  int32_t stride;            /* >= 1; the reference: 100 */
  int32_t skip_invalid;      /* 0: the reference; 1: drop selected rows with w == 0 */
  int32_t source;            /* 0: ObtainAllPoints' dense level-0 table; 1: ObtainCandidatePoints' under `threshold` */
  double  threshold;         /* source 1 only; finite */
  int32_t reserved[2];       /* must be zero */
} uwt_cloud_params;

typedef struct uwt_cloud_info {   /* 32 bytes; n_frames records for the frames, then ONE for the call */
  int32_t status;            /* a frame: UWT_OK or UWT_ERR_INVALID_ARG (its pose); the call: UWT_OK or UWT_ERR_CAPACITY */
  int32_t n_rows;            /* a frame: N; the call: n_frames */
  int32_t n_selected;        /* a frame: rows selected, ceil(N / stride); the call: 0 */
  int32_t n_points;          /* a frame: records it emits (skip_invalid 0: n_selected); the call: 0 */
  int64_t offset;            /* a frame: its first record in the cloud; the call: the total number of points, the FULL count */
  int64_t written;           /* records actually written: a frame's inside cap; the call: min(total, cap) */
} uwt_cloud_info;

/* {0, 100, 0, 0, 20.0, {0, 0}}: the reference's call */
int uwt_default_cloud_params(uwt_cloud_params* params);
/* The cloud of n_frames resident frames, every pointer DEVICE memory: d_traj n_frames x 7 (the output of
 * uwt_accumulate_trajectory_device_async goes straight in), d_points_out `cap` records, d_info_out n_frames + 1 records.
 *   source 0: frame f's table is ObtainAllPoints' dense level-0 table of slots[f] (src/Tracker.cpp:1259-1310), rows i = y w + x, z and the
 *     invalid rule exactly as uwt_warp_image_batch documents them; it is never materialised (2 bytes of depth and 1 of the image are
 *     read per selected pixel, 16 written).  With skip_invalid 0 every offset is closed-form and the call is one launch.
 *   source 1: ObtainCandidatePoints' level-0 table of slots[f] under `threshold`: bit for bit the rows of
 *     uwt_obtain_candidate_points(slots[f], 0, threshold).  The frames need gradients (uwt_apply_gradient).
 * Points beyond cap are not written — the records beyond it stay as they were — and UWT_ERR_CAPACITY goes into the call's record, which
 * still holds the full count, as uwt_obtain_candidate_points writes min(count, cap) rows and returns the full count.
 * Enqueued on the context's stream, ordered against uwt_upload_frames_async as the other batch calls are; it never waits for the device
 * (uwt_sync() to wait).  1 <= n_frames <= max_frames (and <= 65535).
 * UWT_ERR_INVALID_ARG with nothing enqueued and the outputs untouched: a null argument (d_points_out may be null with cap 0), cap < 0, n_frames
 * out of range, a slot out of range, a mode or source outside 0..1, skip_invalid outside 0..1, stride < 1, a non-zero reserved word, a
 * non-finite threshold.
 * alignment: d_traj 4 bytes, d_points_out 16 bytes (one 16-byte store per point), d_info_out 8 bytes (64-bit fields). */
int uwt_point_cloud_batch_async(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const float* d_traj, const uwt_cloud_params* params,
                                uwt_cloud_point* d_points_out, int64_t cap, uwt_cloud_info* d_info_out);
/* The same, synchronous, HOST arrays: traj n_frames x 7, points_out cap records (those below the call's `written` are delivered),
 * info_out n_frames + 1.  UWT_ERR_PAIR_FAILED when a frame failed (its status in its record), else UWT_ERR_CAPACITY when cap was too
 * small; the records are valid in both cases. */
int uwt_point_cloud_batch(uwt_ctx* ctx, int32_t n_frames, const int32_t* slots, const float* traj, const uwt_cloud_params* params,
                          uwt_cloud_point* points_out, int64_t cap, uwt_cloud_info* info_out);
/* The reference's call on ONE explicit host table: pts n x 4 floats of any producer, `slot` serves the intensities only, traj_pose 7
 * floats; params->source and threshold are ignored.  The tag's frame index is 0.  *count_out: the full count; min(count, cap) records are
 * written.  n = 0 is UWT_OK with count 0.  UWT_ERR_CAPACITY when count > cap, UWT_ERR_INVALID_ARG for a non-finite pose (count 0).
 * The batch form over the same rows gives the same bytes.  Synchronous. */
int uwt_point_cloud_points(uwt_ctx* ctx, int32_t slot, const float* pts, int32_t n, const float traj_pose[7],
                           const uwt_cloud_params* params, uwt_cloud_point* points_out, int64_t cap, int64_t* count_out);

/* ---- next to the path: frame ingest---------------------------------------------------------------- */

typedef struct uwt_ingest uwt_ingest;

/* CameraModel::GetCameraModel's rectification setup (src/CameraModel.cpp:84-90): getOptimalNewCameraMatrix(K, dist,
 * Size(in), 1.0, Size(out)) and initUndistortRectifyMap(K, dist, Mat(), newK, Size(out), CV_16SC2, map1, map2), computed
 * once on the host and kept on the device.  K and newK_out are (fx, fy, cx, cy); dist is (k1, k2, p1, p2). */
int uwt_ingest_create(const float K[4], const float dist[4], int32_t in_w, int32_t in_h, int32_t out_w, int32_t out_h,
                      int32_t device, uwt_ingest** out, float newK_out[4]);
int uwt_ingest_destroy(uwt_ingest* ing);
/* the fixed-point maps (out_h x out_w x 2 int16, out_h x out_w uint16), for inspection */
int uwt_ingest_maps(uwt_ingest* ing, int16_t* map1_out, uint16_t* map2_out);
/* remap(raw, undistorted, map1, map2, INTER_LINEAR) of a whole frame (src/System.cpp:152, :233) to host memory */
int uwt_ingest_undistort(uwt_ingest* ing, const uint8_t* raw, size_t row_stride, uint8_t* undistorted_out);
/* System::CalculateROI (src/System.cpp:148-191) on a raw first frame: roi_out = x, y, w, h */
int uwt_ingest_calculate_roi(uwt_ingest* ing, const uint8_t* raw_first, size_t row_stride, int32_t roi_out[4]);
/* remap + crop of System::AddFrame (src/System.cpp:231-235) fused on the GPU: the ctx->width x ctx->height window of the
 * undistorted frame starting at (x0, y0) lands directly in frame slot `slot` of `ctx` (level 0, image plane). */
int uwt_ingest_frame(uwt_ingest* ing, uwt_ctx* ctx, int32_t slot, const uint8_t* raw, size_t row_stride, int32_t x0,
                     int32_t y0);

/* ---- next to the path: trajectory accumulation (Visualizer::UpdateMessages, src/Visualizer.cpp:304-325) --------- */

/* final_i = final_{i-1} * SE3(q_i, t_scale * t_i), start = previous_pose_ (identity or the ground-truth start,
 * src/Visualizer.cpp:240-258).  reference_axes != 0 additionally publishes position as (-z, -x, -y) (:318-320).
 * The reference uses t_scale = 40, reference_axes = 1; (1, 0) is the plain SE(3) prefix product.
 * poses: n x 7 host floats (per-pair poses from uwt_estimate_pose_batch); traj_out: n x 7 host floats. */
int uwt_accumulate_trajectory(uwt_ctx* ctx, const float* poses, int32_t n, const float start_pose[7], float t_scale,
                              int32_t reference_axes, float* traj_out);
/* The same accumulation as a parallel prefix product (one block: per-thread runs, a scan over the run products, replay).
 * SE(3) composition is associative; in floats the grouping shows in the last bits, so results agree with the sequential
 * form to rounding, not bit for bit — the clean default for long trajectories; the reference-visualiser mode
 * (t_scale 40, reference_axes 1) that has to reproduce src/Visualizer.cpp:304-325 exactly stays sequential. */
int uwt_accumulate_trajectory_scan(uwt_ctx* ctx, const float* poses, int32_t n, const float start_pose[7], float t_scale,
                                   int32_t reference_axes, float* traj_out);
/* uwt_accumulate_trajectory with d_poses and d_traj_out (n x 7 each) in DEVICE memory: the same sequential kernel launched on them on the
 * context's stream, no copy and no wait, the results bit for bit the same.  d_poses may be uwt_tracking_io::d_poses of a call enqueued
 * before and d_traj_out the d_traj of uwt_point_cloud_batch_async enqueued behind: tracking -> trajectory -> cloud with one uwt_sync()
 * at the end.  n = 0: nothing is enqueued.  start_pose: host.  d_poses and d_traj_out must not overlap (the kernel reads and writes
 * through restrict pointers; accumulating in place is refused): UWT_ERR_INVALID_ARG with nothing enqueued.
 * alignment: d_poses and d_traj_out 4 bytes (and d_start_pose of the form below). */
int uwt_accumulate_trajectory_device_async(uwt_ctx* ctx, const float* d_poses, int32_t n, const float start_pose[7], float t_scale,
                                           int32_t reference_axes, float* d_traj_out);
/* The same behind a previous pose that is in DEVICE memory: d_start_pose, 7 floats as an accumulation with reference_axes = 0 stores
 * them (a row of an earlier call's d_traj_out).  A live loop accumulates one pose per frame with it — row k from row k - 1 — at a
 * constant cost per frame and still without a wait; the rows are bit for bit those of one call over all poses.  d_traj_out must
 * overlap neither d_poses nor d_start_pose: UWT_ERR_INVALID_ARG with nothing enqueued. */
int uwt_accumulate_trajectory_device_from_async(uwt_ctx* ctx, const float* d_poses, int32_t n, const float* d_start_pose, float t_scale,
                                                int32_t reference_axes, float* d_traj_out);

/* ---- seeded calls: an alignment that starts from a given pose (keyframe tracking, a motion-model prediction, a refinement) ------- */

/* Every alignment above starts at the identity, as Tracker::EstimatePose* does (src/Tracker.cpp:385, :647).  The entries below are
 * their counterparts with a start pose per pair, a SEED: 7 floats qx qy qz qw tx ty tz that stand where that identity stood — the pose
 * in front of the first evaluation of the first iterated level, used exactly as given: nothing normalises, scales or pre-compensates
 * it (the intended sources are this library's own poses).  Everything behind it is the existing loop under the existing constants.  No
 * reference counterpart: the reference's System carries current_keyframe_ / keyframes_ / AddKeyFrame (src/System.cpp:264-278) and
 * never tracks against them.
 * The reference's level hand-off doubles q.xyz behind every level that is not level 0 (:580-590), so a rotation carried in by a seed
 * is multiplied too (twice doubled over three levels); hence the option of the seeded calls:
 *   handoff 0  the reference's hand-off (uwt_se3_handoff under uwt_params::handoff_scale_t; the live call's :856) — the default;
 *   handoff 1  keep: the pose crosses every level boundary unchanged, the last one included; last_error is re-armed as before.
 * Rules, the same in every seeded entry (each takes the arguments and the checks of its unseeded counterpart, then the tail
 * seeds_or_null, sopt_or_null):
 *   - seeds_or_null null: every pair starts at the identity; with handoff 0 the results are the unseeded entry's byte for byte.
 *     sopt_or_null null: {0}.  handoff outside 0..1 or a non-zero reserved word: UWT_ERR_INVALID_ARG with nothing enqueued.
 *   - per-pair failure: a seed with a non-finite entry, or with |tx|, |ty| or |tz| above UWT_TRANSLATION_MAX (2^125: beyond it the dense
 *     warp's division leaves the reference's arithmetic, see "the dense warp's division"), gives that pair alone uwt_stats {UWT_ERR_INVALID_ARG, iterations 0, n_valid 0,
 *     error 0} and the identity as its pose (a non-finite value is never echoed); the pair runs no evaluation, the other pairs' bits
 *     are what they are without it, and the synchronous forms return UWT_ERR_PAIR_FAILED.  The test is made on the device (device
 *     seeds are invisible to the host), in the synchronous forms too.  Every other failure is reported as in the unseeded entry.
 *   - synchronous forms: seeds are n_pairs x 7 HOST floats, copied into the context before anything is enqueued; a rerun of the
 *     speculative one- or two-pair call starts from that copy again.
 *   - _async forms: seeds are n_pairs x 7 floats in DEVICE memory, alignment 4 bytes, not a byte outside that extent is read.  They are
 *     read on the context's stream: the pose buffer of a call enqueued before on the same context may go in without a wait; it must
 *     stay untouched until this call has completed.  The seed range must overlap no output of the same call (d_poses_out,
 *     d_stats_out): UWT_ERR_INVALID_ARG with nothing enqueued — an alignment may be evaluated by launches that run after results
 *     were written, and each must find the seed.
 *   - a pair's bits depend neither on the batch, nor on its place in it, nor on uwt_tuning. */
typedef struct uwt_seed_options {
  int32_t handoff;      /* 0: the reference's hand-off (default); 1: keep */
  int32_t reserved[7];  /* zero */
} uwt_seed_options;     /* 32 bytes */
int uwt_default_seed_options(uwt_seed_options* o);   /* {0} */

/* uwt_estimate_pose_batch from seeds (host seeds, host results; every launch form of the unseeded call). */
int uwt_estimate_pose_batch_seeded(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                   float* poses_out, uwt_stats* stats_out_or_null, const float* seeds_or_null,
                                   const uwt_seed_options* sopt_or_null);
/* uwt_track_batch_async from seeds in device memory, ordered against uploads exactly as the unseeded call.
 * alignment: d_poses_out, d_stats_out_or_null and d_seeds_or_null 4 bytes. */
int uwt_track_batch_seeded_async(uwt_ctx* ctx, int32_t first_slot, int32_t n_frames, int32_t grad_refs_only, int32_t n_pairs,
                                 const int32_t* ref_slots, const int32_t* tgt_slots, float* d_poses_out, uwt_stats* d_stats_out_or_null,
                                 const float* d_seeds_or_null, const uwt_seed_options* sopt_or_null);
/* The live call (uwt_track_features_batch_opt_async / uwt_estimate_pose_features_batch_opt) from seeds: level 0 only, so a seed is
 * what lets it follow a motion its ten iterations cannot absorb from the identity.  The hand-off is the live call's (:856).
 * alignment: as uwt_track_features_batch_async, d_seeds_or_null 4 bytes. */
int uwt_track_features_batch_seeded_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                          const float* keypoints_xy, const int32_t* n_keypoints, const uwt_table_options* opt_or_null,
                                          float* d_poses_out, uwt_stats* d_stats_out_or_null, const float* d_seeds_or_null,
                                          const uwt_seed_options* sopt_or_null);
int uwt_estimate_pose_features_batch_seeded(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                            const float* keypoints_xy, const int32_t* n_keypoints, const uwt_table_options* opt_or_null,
                                            float* poses_out, uwt_stats* stats_out_or_null, const float* seeds_or_null,
                                            const uwt_seed_options* sopt_or_null);
/* Semi-dense tracking (uwt_track_candidates_batch_opt_async / uwt_estimate_pose_candidates_batch_opt) from seeds.
 * alignment: as uwt_track_candidates_batch_async, d_seeds_or_null 4 bytes. */
int uwt_track_candidates_batch_seeded_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                            double threshold, const uwt_table_options* opt_or_null, float* d_poses_out,
                                            uwt_stats* d_stats_out_or_null, const float* d_seeds_or_null,
                                            const uwt_seed_options* sopt_or_null);
int uwt_estimate_pose_candidates_batch_seeded(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                              double threshold, const uwt_table_options* opt_or_null, float* poses_out,
                                              uwt_stats* stats_out_or_null, const float* seeds_or_null,
                                              const uwt_seed_options* sopt_or_null);

/* The chained tracking calls (uwt_tracking_batch_async / uwt_tracking_orb_batch_async) from seeds in device memory: uwt_tracking_io
 * stays as it is, the seeds are arguments — a live loop passes the previous call's io.d_poses.  The front end is untouched: info, good
 * and the kept lists are the unseeded chain's.  A pair that reaches the live call without a key point — every pair the front end fails —
 * starts at the identity whatever its seed row holds, and keeps the unseeded call's record and the identity pose.  The seeds must
 * overlap no output of io (d_poses, d_stats, d_info, d_good, d_kept_prev, d_kept_cur, d_n_matches, each in its full n_pairs [x cap]
 * extent): UWT_ERR_INVALID_ARG with nothing enqueued.  alignment: as the unseeded chains, d_seeds_or_null 4 bytes. */
int uwt_tracking_batch_seeded_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                    const uwt_tracking_params* params_or_null, int32_t cap, const uwt_tracking_io* io,
                                    const float* d_seeds_or_null, const uwt_seed_options* sopt_or_null);
int uwt_tracking_orb_batch_seeded_async(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                        const uwt_tracking_orb_params* params_or_null, int32_t cap, const uwt_tracking_io* io,
                                        const float* d_seeds_or_null, const uwt_seed_options* sopt_or_null);

/* The synchronous chains (uwt_tracking_batch / uwt_tracking_orb_batch) from HOST seeds, everything else as there: what the language
 * mirrors' TrackingBatch(..., seeds) calls. */
int uwt_tracking_batch_seeded(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                              const uwt_tracking_params* params_or_null, int32_t cap, const uwt_keypoint* prev_kp_or_null,
                              const int32_t* n_prev_or_null, float* poses_out, uwt_stats* stats_out_or_null, uwt_tracking_info* info_out,
                              uwt_match* good_out, uwt_keypoint* kept_prev_out, uwt_keypoint* kept_cur_out, const float* seeds_or_null,
                              const uwt_seed_options* sopt_or_null);
int uwt_tracking_orb_batch_seeded(uwt_ctx* ctx, int32_t n_pairs, const int32_t* ref_slots, const int32_t* tgt_slots,
                                  const uwt_tracking_orb_params* params_or_null, int32_t cap, const uwt_keypoint* prev_kp_or_null,
                                  const int32_t* n_prev_or_null, float* poses_out, uwt_stats* stats_out_or_null,
                                  uwt_tracking_info* info_out, uwt_match* good_out, uwt_keypoint* kept_prev_out,
                                  uwt_keypoint* kept_cur_out, const float* seeds_or_null, const uwt_seed_options* sopt_or_null);

/* The constant-velocity motion model in keyframe coordinates, on the device: seed_i = (cur_i * prev_i^-1) * cur_i with prev = the pose
 * keyframe -> frame p - 1, cur = keyframe -> frame p, the seed for keyframe -> frame p + 1.  (Frame-to-frame tracking needs no kernel:
 * its constant-velocity seed IS the previous call's pose buffer.)  The library's own contract, the same in both arithmetic sets:
 *   inverse of prev = (q, t):  qi = (-qx, -qy, -qz, qw), the conjugate;  R = the rotation uwt_se3_matrix gives for qi (f32, as there);
 *     ti[k] = (float)(-(((double)R[3k] * t[0] + (double)R[3k+1] * t[1]) + (double)R[3k+2] * t[2])) — each row in f64, products exact,
 *     added in this order, negated, rounded once (contraction cannot change it);
 *   rel = uwt_se3_mul(cur, (qi, ti));  seed = uwt_se3_mul(rel, cur) — the bits of uwt_se3_mul.
 * A row with a non-finite entry in prev or cur gives an all-NaN seed row, which a seeded call then refuses for that pair.
 * d_prev, d_cur, d_seed_out: n x 7 floats in device memory, alignment 4 bytes; d_seed_out must overlap neither input:
 * UWT_ERR_INVALID_ARG with nothing enqueued.  Enqueued on the context's stream, no wait; n = 0: nothing is enqueued. */
int uwt_predict_seeds_device_async(uwt_ctx* ctx, int32_t n, const float* d_prev, const float* d_cur, float* d_seed_out);
/* The same kernel on host arrays (n x 7 floats each), staged through the context's scratch; synchronous; the same bits. */
int uwt_predict_seeds(uwt_ctx* ctx, int32_t n, const float* prev, const float* cur, float* seed_out);

/* ---- the metric Jacobian (EXTENSION; no reference counterpart) ------------------------------------------------------------------ */

/* The reference forms Jw (src/Tracker.cpp:455-467) with the warped PIXEL coordinates x2, y2 where the warped 3-D point's X, Y belong,
 * so columns 2..5 of every Jacobian row are off by factors of 10^2 to 10^5 and the tracker estimates little but an image-plane shift.
 * UWT_JACOBIAN_REFERENCE (the default of a new context) reproduces that bit for bit.  UWT_JACOBIAN_METRIC puts X = xn * z2, Y = yn * z2
 * in, written in normalised coordinates; signs and column order are the reference's.
 *
 * The contract.  Inputs: the values the reference-mode Jw reads — x2, y2, iz behind the validity test and iz <- max(1 / z2, 0); the
 * level's fx, fy, cx, cy, invfx, invfy (uwt_level); the factors zf = z_factor, af = angle_factor.  Everything f32, every operation
 * rounded once, in the written order, no contraction; the same in both arithmetic sets:
 *   xn = (x2 - cx) * invfx                                 yn = (y2 - cy) * invfy
 *   row 0:  a0 = fx * iz      0      a2 = -(((fx * xn) * iz) * zf)   a3 = -(((fx * xn) * yn) * af)
 *           a4 = (fx * (1 + xn * xn)) * af                            a5 = -((fx * yn) * af)
 *   row 1:  0      b1 = fy * iz      b2 = -(((fy * yn) * iz) * zf)   b3 = -((fy * (1 + yn * yn)) * af)
 *           b4 = ((fy * xn) * yn) * af                                b5 = (fy * xn) * af
 * Everything else keeps the bits it has under the context's arith, accumulate_f64, weights and sampler: Jacobian_row = Jl * Jw in the
 * arithmetic set's own form, validity and the residual, the robust scale and weights, the 28 sums and their fold, the exit test, the
 * solve, exp and the composition.  Which kernel forms serve the mode (uwt_tuning, the level's shape) never shows in a result.
 *
 * The mode is state of the context (uwt_params and UWT_ABI_VERSION are unchanged).  uwt_set_jacobian, like uwt_set_tuning, waits for
 * the context's work in flight and applies to every later call that forms a Jacobian: the dense calls in every launch form and all
 * their seeded forms, uwt_estimate_pose_points, the batched table calls (features and candidates; plain, _opt, _seeded), both tracking
 * chains, and the per-stage uwt_residual_jacobian / uwt_residual_jacobian_weighted.  Any other value: UWT_ERR_INVALID_ARG and nothing
 * changes.  uwt_update_params neither reads nor resets the mode.
 * One exception to "the call's own constants": the live call's z_factor = 0.002 (src/Tracker.cpp:640) is the reference's compensation
 * for the pixel coordinate in column 2; in metric mode the live call, and the chains through it, run with z_factor = 1.  Its other
 * constants stay.
 * Metric mode is meant to run with handoff = 1 (keep) of the seeded entries (a null seed starts at the identity): with rotations that
 * are real, the reference's q.xyz *= 2 hand-off overshoots and diverges on some pairs. */
enum uwt_jacobian { UWT_JACOBIAN_REFERENCE = 0, UWT_JACOBIAN_METRIC = 1 };
int uwt_set_jacobian(uwt_ctx* ctx, int32_t mode);
int uwt_get_jacobian(const uwt_ctx* ctx, int32_t* out);

/* ---- EXTENSION: depth from tracked motion, a plane sweep over resident frames -------------------------------------------------- */

/* No reference counterpart: the reference has depth only where a sensor delivers it (src/Tracker.cpp:1266-1302).  Given a reference
 * slot, 1..4 view slots and the poses a tracking call left (X_view = T * X_ref, the tracker's own convention: the pose buffers of
 * uwt_track_batch_async, uwt_track_batch_seeded_async and uwt_tracking_io::d_poses go straight in), the sweep tries n_hyp depth CODES
 * on every considered pixel of the reference slot and writes the code under which the views agree best.  A code d is what a depth
 * plane holds: at level lvl it means the table row [x, y, z(d), 1] ObtainAllPoints makes for a pixel whose depth plane holds d,
 * z(d) = (float)d * (float)(depth_scale / 2^lvl) as ObtainAllPoints computes it (src/Tracker.cpp:1266) (lvl = 0 is the intended
 * level; lvl >= 1 reproduces the reference's / 2^lvl quirk and nothing more).  The row is warped by uwt_warp's arithmetic in the
 * context's arithmetic set, the matching costs are integers, the only other floating point is the f64 refinement of step 10: the
 * result is the same bytes on every run, in any batch, and the depth written is exactly the depth under which the tracker,
 * uwt_warp_image_batch and uwt_point_cloud_batch compute the same landing pixels.
 *
 * A JOB is one reference slot and n_views view slots, 1 <= n_views <= 4 (the same for every job of a call), view v of job j under the
 * pose d_poses[j * n_views + v].  The hypotheses are n_hyp codes d_0 < d_1 < ... < d_{n_hyp-1}, 3 <= n_hyp <= 64, each in 1..32767
 * (what the tracker's (int16)depth > 0 accepts); they are host data of the call.
 * Pixels considered: source = 0 the level's w x h point grid; source = 1 the pixels (x, y) of the rows
 * uwt_obtain_candidate_points(slot, lvl, threshold) returns on a context without a depth plane: gradient_ > mean + threshold over the
 * point grid (gradients must have been applied to the reference slot).  The sweep never reads a depth plane, so the zero-depth test
 * ObtainCandidatePoints makes on a context WITH a depth plane is not part of the selection.
 * For a considered pixel (x, y), patch radius r in {1, 2}, img_w x img_h the level's image:
 *    1. BORDER unless r <= x <= img_w-1-r and r <= y <= img_h-1-r.
 *    2. Landing, for hypothesis k and view v: [u, v', Z', .] = uwt_warp(lvl, [x, y, z(d_k), 1], T_v); x2 = (int)round(u), y2 =
 *       (int)round(v') (C round); u or v' not finite or of magnitude >= 2^31 - 128 does not land (the image warp's rule).  It LANDS iff
 *       Z' > 0 and r <= x2 <= img_w-1-r and r <= y2 <= img_h-1-r.  k is VALID iff it lands in every view.
 *    3. FEW: fewer than 3 valid hypotheses.
 *    4. cost[k] = sum over views and dy, dx in [-r, r] of | view_v[y2+dy, x2+dx] - ref[y+dy, x+dx] | on the u8 image planes: the
 *       reference patch translated, not warped per pixel.  At most 25 * 255 * 4.
 *    5. dist(a, b) = max over views of max(|x2_a - x2_b|, |y2_a - y2_b|).  LOW_PARALLAX when dist(first valid, last valid) <
 *       min_parallax: the motion does not separate the hypotheses.
 *    6. The winner is the valid k of least cost, the smallest such k on equal cost.
 *    7. EDGE when the winner is 0 or n_hyp-1 or a neighbour k-1, k+1 is not valid.
 *    8. POOR when cost[k] > max_mean_abs * (2r+1)^2 * n_views.
 *    9. c2 = the least cost over valid j with dist(j, k) >= 2.  AMBIGUOUS when there is no such j, or unless
 *       uniq_den * cost[k] < uniq_num * c2 (strict, 64-bit integers).
 *   10. ESTIMATED.  With refine = 0, or den = c- - 2 c0 + c+ equal to 0 (c-, c0, c+ the costs of k-1, k, k+1), the code is d_k.  Else,
 *       in f64, every operation rounded once, no contraction: a = (double)|c- - c+| / (double)(2 den); n = k+1 when c- > c+, else k-1;
 *       rho_j = 1.0 / (double)d_j; rho = rho_k + a * (rho_n - rho_k); code = (int)rint(1.0 / rho) (ties to even), clamped to 1..32767.
 * Outputs, job j's plane j * pitch * img_h elements behind job 0's, laid out like a slot's plane (pitch x img_h; columns >= img_w
 * are never written): d_depth (u16) the code where ESTIMATED and 0 at every other pixel of the image; d_cost (u16) the winner's cost
 * where ESTIMATED, else 0; d_outcome (u8) the values of uwt_sweep_outcome; d_info one record per job.  A job's bytes depend neither
 * on the batch, nor on the job's place in it, nor on uwt_tuning, nor on the run: minima and sums of integers, no cursor, no float
 * atomic.  The sweep never reads a depth plane: for a ONE-job call uwt_plane_device_ptr(ctx, ref_slot, lvl, UWT_PLANE_DEPTH) is a
 * valid d_depth, which is how a keyframe gets its depth in place.
 * What consumes a semi-dense level-0 plane (zeros where nothing was estimated) as it is: the live call
 * (uwt_estimate_pose_features_batch: a key point on a zero is dropped), uwt_point_cloud_batch with skip_invalid = 1,
 * uwt_warp_image_batch at level 0, and alignments that iterate level 0 alone (zero-depth points are [0 0 1 0] rows, never valid).
 * uwt_build_pyramids averages the zeros in, as the reference's resize does: the coarser levels of such a plane are the
 * caller's business. */
enum uwt_sweep_outcome { UWT_SWEEP_NOT_SELECTED = 0, UWT_SWEEP_ESTIMATED = 1, UWT_SWEEP_BORDER = 2, UWT_SWEEP_FEW = 3,
                         UWT_SWEEP_LOW_PARALLAX = 4, UWT_SWEEP_EDGE = 5, UWT_SWEEP_POOR = 6, UWT_SWEEP_AMBIGUOUS = 7 };

typedef struct uwt_sweep_params {   /* 64 bytes */
  int32_t lvl;            /* the level swept */
  int32_t source;         /* 0: the point grid, 1: the candidate pixels */
  double  threshold;      /* source 1: GRADIENT_THRESHOLD; finite */
  int32_t n_views;        /* 1..4 */
  int32_t n_hyp;          /* 3..64 */
  int32_t radius;         /* 1 or 2 */
  int32_t max_mean_abs;   /* >= 1: step 8 */
  int32_t uniq_num;       /* >= 1: step 9 */
  int32_t uniq_den;       /* >= 1 */
  int32_t min_parallax;   /* >= 2: step 5 */
  int32_t refine;         /* 0 or 1: step 10 */
  int32_t reserved[4];    /* must be zero */
} uwt_sweep_params;

typedef struct uwt_sweep_info {   /* per job, 64 bytes, all integers: exact and order-independent */
  int32_t status;          /* uwt_status_code of this job */
  int32_t n_selected;      /* pixels considered = the sum of n_outcome[1..7] */
  int32_t n_outcome[8];    /* by uwt_sweep_outcome; [0] is 0 */
  int64_t sum_cost;        /* over the estimated pixels: the winner's cost */
  int64_t sum_code;        /* over the estimated pixels: the code written */
  int64_t reserved;
} uwt_sweep_info;

typedef struct uwt_sweep_io {   /* every pointer is DEVICE memory; planes are n_jobs x pitch x img_h elements */
  uint16_t*       d_depth;      /* out, required; 2-byte aligned */
  uint16_t*       d_cost;       /* out, may be null; 2-byte aligned */
  uint8_t*        d_outcome;    /* out, may be null */
  uwt_sweep_info* d_info;       /* out, required: n_jobs records; 8-byte aligned (64-bit sums) */
} uwt_sweep_io;

/* {0, 1, 20.0, 1, 32, 2, 12, 3, 4, 4, 1, {0}} */
int uwt_default_sweep_params(uwt_sweep_params* out);
/* HOST helper, no context: n codes uniform in inverse depth from z_near to z_far, in f64: rho_k = 1/z_near + k (1/z_far - 1/z_near) /
 * (n - 1), d_k = rint(1 / (rho_k * depth_scale)).  UWT_ERR_INVALID_ARG: a null pointer, n outside 3..64, z_near, z_far or depth_scale
 * not finite or not > 0, z_near >= z_far, or codes that are not strictly increasing or leave 1..32767 (codes_out is then untouched). */
int uwt_sweep_hypotheses(double z_near, double z_far, double depth_scale, int32_t n, uint16_t* codes_out);
/* The sweep for a batch of jobs.  ref_slots: n_jobs; view_slots: n_jobs x n_views; d_poses: DEVICE memory, n_jobs x n_views x 7
 * floats; codes: n_hyp host values (copied before the call returns).  The frames must be resident with pyramids built, source = 1
 * needs the reference slots' gradients.  Enqueued on the context's stream, ordered against uwt_upload_frames_async on every slot
 * named as the other batch calls are; it never waits for the device; uwt_sync() to wait.
 * UWT_ERR_INVALID_ARG with nothing enqueued and every output untouched: a null list, d_poses, codes, params, io, d_depth or d_info;
 * n_jobs outside 1..max_pairs; a slot or level out of range; source outside 0..1, n_views outside 1..4, n_hyp outside 3..64, radius
 * outside 1..2, refine outside 0..1; uniq_num, uniq_den or max_mean_abs < 1; min_parallax < 2; a non-zero reserved word; a threshold
 * that is not finite; codes that are not strictly increasing or leave 1..32767.
 * A pose with a non-finite entry puts UWT_ERR_INVALID_ARG into that job's status with all counts 0 and its planes zero; its
 * neighbours are untouched.
 * alignment: d_poses 4 bytes; io: at uwt_sweep_io. */
int uwt_sweep_depth_batch_async(uwt_ctx* ctx, int32_t n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const float* d_poses,
                                const uint16_t* codes, const uwt_sweep_params* params, const uwt_sweep_io* io);
/* The same, synchronous, HOST in and out: poses n_jobs x n_views x 7; depth_out (required) / cost_out n_jobs x img_w x img_h u16,
 * outcome_out n_jobs x img_w x img_h u8, tight, the latter two may be null; info_out n_jobs, required.  UWT_ERR_PAIR_FAILED when a job
 * failed, its status in its record. */
int uwt_sweep_depth_batch(uwt_ctx* ctx, int32_t n_jobs, const int32_t* ref_slots, const int32_t* view_slots, const float* poses,
                          const uint16_t* codes, const uwt_sweep_params* params, uint16_t* depth_out, uint16_t* cost_out,
                          uint8_t* outcome_out, uwt_sweep_info* info_out);

/* ---- test instrumentation: guards inside the context's own scratch ------------------------------------------------------------ */

/* Not part of the tracker: these two serve tests/test_gpu_guard_bands.py, which uses them to see whether a kernel writes outside an
 * array of the context's growable scratch (the staging of every synchronous entry point and the work areas of the asynchronous ones:
 * one block per stage, cut into arrays).  No reference counterpart.
 * uwt_debug_guards(ctx, guard_bytes): waits for everything the context has enqueued, releases every growable block (each is made again
 * on its next use, like any growth) and, for guard_bytes > 0, makes every such block from then on with a gap of guard_bytes (rounded
 * up to the array alignment of the stage) behind EVERY array, one in front of the first and one behind the last; each use of a block
 * fills its gaps with a byte pattern on the context's stream.  0 (the default of a new context) turns the guards off again: offsets,
 * sizes and launches are then exactly those of a context that never had them.  Results do not depend on the setting.  guard_bytes
 * outside 0..2^24: UWT_ERR_INVALID_ARG.
 *   - Only the gaps carry the pattern; the arrays are never filled.  A pattern in scratch that a latent error reads as an index or a
 *     count could turn a silent error into a wild access; the gaps are read by no correct code, so what they hold cannot matter.
 *   - The allocations uwt_create makes once (planes, pair state, histograms, the live call's tables) are outside this.
 * uwt_debug_check_guards(ctx, damaged_bytes_out): waits for the context's streams, compares every gap recorded by the last use of
 * every block, and returns UWT_OK with *damaged_bytes_out = the number of damaged bytes (0: none).  On damage uwt_last_error names the
 * stage's block, the index of the array in front of the first damaged gap (-1: the gap in front of the first array) and the first
 * damaged byte's offset in that gap. */
int uwt_debug_guards(uwt_ctx* ctx, int64_t guard_bytes);
int uwt_debug_check_guards(uwt_ctx* ctx, int64_t* damaged_bytes_out);

/* uwt_debug_window_open(ctx, out): *out = 1 while the early-preparation window of the last uwt_track_batch_async /
 * uwt_track_batch_seeded_async is open (a fixed-schedule batch call that ended on level 0, and no entry since that enqueues device
 * work on the context stream, reads a plane back or changes a setting), else 0.  Serves tests/test_gpu_history.py, which asserts that
 * every such entry leaves it closed.  A call refused on its arguments alone, before anything is enqueued, read back or changed
 * (UWT_ERR_CAPACITY for n_pairs > max_pairs or a cap above UWT_MATCH_MAX_ROWS, a null argument), has not touched the context and may
 * leave it as it was; uwt_sync and uwt_wait_ticket only wait and leave it too.  Host only: it reads one flag, enqueues nothing, waits for nothing and changes nothing.  No
 * reference counterpart.  A null argument: UWT_ERR_INVALID_ARG. */
int uwt_debug_window_open(const uwt_ctx* ctx, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif
