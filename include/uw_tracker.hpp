// uw_tracker.hpp — header-only C++ mirror of the reference's direct-tracking class surface over the C ABI (uwt.h).
//
// Same class / method names, argument meaning and call order as the reference's include/Tracker.h:90-170,
// include/LeastSquares.h:26-50 and the Frame members of include/System.h:63-103 that the path touches, so that
// System::InitializeSystem / System::Tracking (src/System.cpp:121-123, 193-223) read the same against this header:
//
//     tracker_ = new uw::Tracker(depth_available_);
//     tracker_->InitializePyramid(w_, h_, K_);
//     ...
//     tracker_->ApplyGradient(previous_frame_);  tracker_->ApplyGradient(current_frame_);
//     tracker_->ObtainAllPoints(previous_frame_);
//     tracker_->EstimatePose(previous_frame_, current_frame_);   // -> previous_frame_->rigid_transformation_
//
// OpenCV / Eigen / Sophus are not required: images are passed as uw::ImageView (data, rows, cols, step — the four
// cv::Mat fields the path reads); define UW_WITH_OPENCV before including to get the cv::Mat overloads, UW_WITH_EIGEN to make
// uw::Mat61f / uw::Mat66f (LS::A, LS::b, LS::update's Jacobian) the reference's Eigen types instead of the stand-ins below.
// Neither branch has been compiled in the image this repository is developed in (it has no OpenCV and no Eigen).
// Every numeric step runs in libuwt_hip.so on the GPU; a non-zero status becomes a std::runtime_error (the reference
// surfaces misuse as cv::Exception / SOPHUS_ENSURE aborts).
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "uwt.h"

#ifdef __SSE__
#include <xmmintrin.h>
#endif

#ifdef UW_WITH_OPENCV
#include <opencv2/core.hpp>
#endif
#ifdef UW_WITH_EIGEN
#include <Eigen/Cholesky>
#include <Eigen/Core>
#endif

namespace uw {

constexpr int PYRAMID_LEVELS = 5;  // src/Options.cpp:26

// Storage of Sophus::SE3f: unit quaternion (x y z w) + translation.
struct SE3 {
  float q[4] = {0.f, 0.f, 0.f, 1.f};
  float t[3] = {0.f, 0.f, 0.f};
  const float* data() const { return q; }  // 7 contiguous floats
  float* data() { return q; }
};
static_assert(sizeof(SE3) == 7 * sizeof(float), "SE3 must be 7 packed floats");

namespace detail {
// The context a default-constructed LS folds on ("LS ls;", src/Tracker.cpp:537): LS::bind(ctx), the first Tracker's
// context, or — when neither exists — a minimal context created for the reductions alone.
inline uwt_ctx*& ls_default_ctx() { static uwt_ctx* c = nullptr; return c; }
inline uwt_ctx* ls_context() {
  uwt_ctx*& d = ls_default_ctx();
  if (!d) {   // nothing bound and no tracker yet: a minimal context for the reductions (lives for the process)
    uwt_params p;
    int st = uwt_default_params(&p, 64, 48, 64.f, 64.f, 31.5f, 23.5f);
    if (st == UWT_OK) {
      p.n_levels = 1; p.first_level = 0; p.last_level = 0; p.max_frames = 2; p.max_pairs = 1;
      st = uwt_create(&p, &d);
    }
    if (st != UWT_OK) throw std::runtime_error(std::string("LS: no context: ") + uwt_status_string(st));
  }
  return d;
}
}  // namespace detail

// include/Options.h:146-147.  With UW_WITH_EIGEN these ARE the reference's Eigen types; without Eigen, stand-ins with the
// members the path's code uses (operator(), data(), unary minus, ldlt().solve()).  The stand-in's solve() is the library's
// 6x6 solve on the GPU (uwt_solve_delta: the LU inverse of the live path, src/Tracker.cpp:564) — no host factorisation.
#ifdef UW_WITH_EIGEN
typedef Eigen::Matrix<float, 6, 1> Mat61f;
typedef Eigen::Matrix<float, 6, 6> Mat66f;
#else
struct Mat61f {
  float v[6] = {0, 0, 0, 0, 0, 0};
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
  float* data() { return v; }
  const float* data() const { return v; }
  Mat61f operator-() const { Mat61f r; for (int i = 0; i < 6; i++) r.v[i] = -v[i]; return r; }
};
struct Mat66f {
  float v[36] = {};   // row-major (A is symmetric: reads the same column-major)
  float& operator()(int r, int c) { return v[6 * r + c]; }
  float operator()(int r, int c) const { return v[6 * r + c]; }
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
  float* data() { return v; }
  const float* data() const { return v; }
  struct Solver {
    const Mat66f* A;
    Mat61f solve(const Mat61f& b) const {
      Mat61f x;
      const int st = uwt_solve_delta(detail::ls_context(), A->v, b.v, x.v, nullptr, nullptr);
      if (st != UWT_OK) throw std::runtime_error(std::string("Mat66f::ldlt().solve: ") + uwt_status_string(st));
      return x;
    }
  };
  Solver ldlt() const { return Solver{this}; }
};
#endif

struct ImageView {
  const void* data = nullptr;
  int rows = 0, cols = 0;
  size_t step = 0;  // bytes per row (cv::Mat::step)
  ImageView() = default;
  ImageView(const void* d, int r, int c, size_t s) : data(d), rows(r), cols(c), step(s) {}
#ifdef UW_WITH_OPENCV
  ImageView(const cv::Mat& m) : data(m.data), rows(m.rows), cols(m.cols), step(m.step) {}
#endif
};

struct Size {  // cv::Size() as System::AddFrame passes it to resize (src/System.cpp:247)
  int width = 0, height = 0;
};

// cv::resize(src, dst, Size(), 0.5, 0.5) of System::AddFrame's pyramid loop (src/System.cpp:246-251).  The pixels of
// levels 1.. are produced on the GPU when the tracker binds the frame (uwt_build_pyramids: the same 2x2 round-half-up
// mean); here the destination view only takes its shape, with no host pixels (data == nullptr), so the loop compiles
// and reads as it does in the reference.
inline void resize(const ImageView& src, ImageView& dst, Size /*dsize*/, double fx, double fy) {
  dst = ImageView(nullptr, (int)(src.rows * fy + 0.5), (int)(src.cols * fx + 0.5), 0);
}

class Tracker;

// include/System.h:63-103 — the members the tracker reads or writes.
class Frame {
 public:
  Frame() = default;
  ~Frame();                       // releases the device slot the frame holds, if any
  Frame(const Frame&) = delete;   // a bound frame is known to its tracker by address
  Frame& operator=(const Frame&) = delete;

  int idFrame_ = 0;
  std::vector<ImageView> images_ = std::vector<ImageView>(PYRAMID_LEVELS);  // [0]: CV_8UC1 host pixels; [1..]: shapes only
  std::vector<ImageView> depths_ = std::vector<ImageView>(PYRAMID_LEVELS);  // [0]: CV_16UC1 host pixels (optional)
  bool depth_available_ = false;
  bool obtained_gradients_ = false;
  bool obtained_candidatePoints_ = false;
  SE3 rigid_transformation_;
  std::vector<float> keypoints_;                         // x0 y0 x1 y1 ... (cv::KeyPoint::pt of Frame::keypoints_)
  int n_matches_ = 0;                                    // include/System.h:93
  std::vector<uwt_keypoint> surf_keypoints_;             // the same key points as cv::KeyPoint holds them (size, response, direction,
                                                         // octave): what useProvidedKeypoints describes again in the next call
  std::vector<uwt_keypoint> orb_keypoints_;              // the same under RobustMatcher(tracker, 1): ORB's records
  std::vector<float> candidatePoints_[PYRAMID_LEVELS];   // N x 4 [x y z w] per level when a sparse producer ran
  int slot_ = -1;                 // device frame slot while bound; -1 again once the slot has gone to another frame
  Tracker* tracker_ = nullptr;    // the tracker that holds the slot
};

class RobustMatcher;

class Tracker {
  friend class RobustMatcher;   // DetectAndTrackFeatures binds both frames

 public:
  // include/Tracker.h:97.  `overrides` lets a caller change the constants the reference hard-codes as locals of
  // EstimatePose (src/Tracker.cpp:364-372); by default they are exactly those.
  explicit Tracker(bool _depth_available, int max_frames = 16, int device = 0)
      : depth_available_(_depth_available), max_frames_(max_frames < 2 ? 2 : max_frames), device_(device),
        owner_((size_t)(max_frames < 2 ? 2 : max_frames), nullptr), last_use_((size_t)(max_frames < 2 ? 2 : max_frames), 0) {}
  ~Tracker() {
    for (Frame* f : owner_)
      if (f) { f->slot_ = -1; f->tracker_ = nullptr; f->obtained_gradients_ = false; }
    if (ctx_ && detail::ls_default_ctx() == ctx_) detail::ls_default_ctx() = nullptr;
    if (ctx_) uwt_destroy(ctx_);
  }
  // a frame that goes away (System::FreeFrames, src/System.cpp:352-355) gives its slot back
  void forget(Frame* f) {
    if (f->slot_ >= 0 && f->slot_ < (int)owner_.size() && owner_[(size_t)f->slot_] == f) owner_[(size_t)f->slot_] = nullptr;
    f->slot_ = -1;
    f->tracker_ = nullptr;
  }
  Tracker(const Tracker&) = delete;
  Tracker& operator=(const Tracker&) = delete;

  uwt_params& params() { return params_; }  // valid after InitializePyramid's defaults; edit before first use

  // include/Tracker.h:112; K row-major 3x3 (fx 0 cx; 0 fy cy; 0 0 1)
  void InitializePyramid(int _width, int _height, const float K[9]) {
    check(uwt_default_params(&params_, _width, _height, K[0], K[4], K[2], K[5]), "uwt_default_params");
    params_.n_levels = PYRAMID_LEVELS;
    params_.has_depth = depth_available_ ? 1 : 0;
    params_.max_frames = max_frames_;
    params_.max_pairs = max_frames_ > 1 ? max_frames_ / 2 : 1;
    params_.device = device_;
  }
#ifdef UW_WITH_OPENCV
  void InitializePyramid(int _width, int _height, const cv::Mat& _K) {
    const float K[9] = {_K.at<float>(0, 0), 0, _K.at<float>(0, 2), 0, _K.at<float>(1, 1), _K.at<float>(1, 2), 0, 0, 1};
    InitializePyramid(_width, _height, K);
  }
#endif
  void InitializeMasks() {}  // src/Tracker.cpp:342-359 builds masks nothing reads

  void ApplyGradient(Frame* _frame) {  // include/Tracker.h:137
    const int slot = bind(_frame);
    check(uwt_apply_gradient(ctx(), slot, 1), "uwt_apply_gradient");
    _frame->obtained_gradients_ = true;
  }
  void ObtainAllPoints(Frame* _frame) {  // include/Tracker.h:153 — the dense table is implicit on the GPU
    bind(_frame);
    _frame->obtained_candidatePoints_ = true;
  }
  // include/Tracker.h:170: N x 4 points in, N x 4 out
  std::vector<float> WarpFunction(const std::vector<float>& _points2warp, const SE3& _rigid_transformation, int _lvl) {
    std::vector<float> out(_points2warp.size());
    check(uwt_warp(ctx(), _lvl, _points2warp.data(), (int)(_points2warp.size() / 4), _rigid_transformation.data(), out.data()),
          "uwt_warp");
    return out;
  }
  // include/Tracker.h:126 (src/Tracker.cpp:599-629): the N x 4 table followed by the patch cells around every point
  // (patch_size_ = 5, :274).  Its only call in the reference is commented out (:672).
  std::vector<float> AddPatchPointsFeatures(const std::vector<float>& candidatePoints, int lvl) {
    const int n = (int)(candidatePoints.size() / 4), cap = n * patch_size_ * patch_size_;
    std::vector<float> out((size_t)(cap > 0 ? cap : 1) * 4);
    int32_t count = 0;
    check(uwt_add_patch_points(ctx(), lvl, candidatePoints.data(), n, patch_size_, out.data(), cap, &count), "uwt_add_patch_points");
    out.resize((size_t)(count < cap ? count : cap) * 4);
    return out;
  }
  // include/Tracker.h:178 (src/Tracker.cpp:1596-1605): 6 x 1 [w1 w2 w3 x1 x2 x3] -> SE3(SO3::exp(w), x); the translation
  // is taken as it is (not through V(w)), so the rotation is exp's of the tangent (0, w) and t is copied.
  SE3 Mat2SE3(const float _input[6]) {
    const float xi[6] = {0.f, 0.f, 0.f, _input[0], _input[1], _input[2]};
    SE3 T;
    check(uwt_se3_exp(ctx(), xi, T.data()), "uwt_se3_exp");
    T.t[0] = _input[3]; T.t[1] = _input[4]; T.t[2] = _input[5];
    return T;
  }
#ifdef UW_WITH_OPENCV
  SE3 Mat2SE3(const cv::Mat& _input) {
    const float v[6] = {_input.at<float>(0, 0), _input.at<float>(1, 0), _input.at<float>(2, 0),
                        _input.at<float>(3, 0), _input.at<float>(4, 0), _input.at<float>(5, 0)};
    return Mat2SE3(v);
  }
#endif
  // include/Tracker.h:122
  void EstimatePose(Frame* _previous_frame, Frame* _current_frame) {
    const int32_t a = bind(_previous_frame), b = bind(_current_frame);
    if (!_previous_frame->obtained_gradients_)
      throw std::runtime_error("EstimatePose: ApplyGradient(previous) not called (or its slot was reused since)");
    check(uwt_estimate_pose_batch(ctx(), 1, &a, &b, _previous_frame->rigid_transformation_.data(), &last_stats_),
          "uwt_estimate_pose_batch");
  }
  // EstimatePose from a start pose (uwt_estimate_pose_batch_seeded; no reference counterpart: the reference always starts at the
  // identity, src/Tracker.cpp:385): _seed is the pose in front of the first evaluation, used as given — a keyframe's prediction
  // (PredictSeeds), the previous pair's pose, another stage's result.  handoff 0: the reference's level hand-off; 1: the pose crosses
  // the levels unchanged (uwt_seed_options).  A seed with a non-finite entry, or with |tx|, |ty| or |tz| above UWT_TRANSLATION_MAX (2^125,
  // the range of the dense warp's division, uwt.h), is refused: the call throws with UWT_ERR_PAIR_FAILED, UWT_ERR_INVALID_ARG in last_stats_.
  void EstimatePoseSeeded(Frame* _previous_frame, Frame* _current_frame, const SE3& _seed, int32_t handoff = 0) {
    const int32_t a = bind(_previous_frame), b = bind(_current_frame);
    if (!_previous_frame->obtained_gradients_)
      throw std::runtime_error("EstimatePoseSeeded: ApplyGradient(previous) not called (or its slot was reused since)");
    const SE3 seed = _seed;   // (the seed may be the previous frame's own rigid_transformation_, which the call writes)
    const uwt_seed_options so = seed_options(handoff);
    check(uwt_estimate_pose_batch_seeded(ctx(), 1, &a, &b, _previous_frame->rigid_transformation_.data(), &last_stats_, seed.data(), &so),
          "uwt_estimate_pose_batch_seeded");
  }
  // The constant-velocity motion model in keyframe coordinates (uwt_predict_seeds): _prev = the poses keyframe -> frame p - 1, _cur =
  // keyframe -> frame p, n x 7 floats each; returns the seeds (cur * prev^-1) * cur for keyframe -> frame p + 1.
  std::vector<float> PredictSeeds(const std::vector<float>& _prev, const std::vector<float>& _cur) {
    if (_prev.size() != _cur.size() || _prev.size() % 7) throw std::invalid_argument("PredictSeeds: n x 7 floats each");
    std::vector<float> out(_cur.size());
    check(uwt_predict_seeds(ctx(), (int32_t)(_cur.size() / 7), _prev.data(), _cur.data(), out.data()), "uwt_predict_seeds");
    return out;
  }
  static uwt_seed_options seed_options(int32_t handoff) {
    uwt_seed_options so;
    uwt_default_seed_options(&so);
    so.handoff = handoff;
    return so;
  }
  // include/Tracker.h:124 — the vectorised prototype's schedule: levels PYRAMID_LEVELS-1 .. 0, <= 50 iterations, gain 50,
  // epsilon 1e-3, no z / angle factor applied (src/Tracker.cpp:877-885, 1082).  The reference BODY is not reproduced: its
  // residual ignores the warp (:933-944) and column 0 of Jw1 is zeroed by a typo (:986); this runs the same per-point
  // terms as EstimatePose under that schedule.
  void FastEstimatePose(Frame* _previous_frame, Frame* _current_frame) {
    const int32_t a = bind(_previous_frame), b = bind(_current_frame);
    if (!_previous_frame->obtained_gradients_)
      throw std::runtime_error("FastEstimatePose: ApplyGradient(previous) not called (or its slot was reused since)");
    uwt_params saved;
    check(uwt_get_params(ctx(), &saved), "uwt_get_params");
    uwt_params f = saved;
    f.first_level = f.n_levels - 1; f.last_level = 0; f.max_iters = 50; f.gain = 50.0f; f.epsilon = 0.001f;
    f.z_factor = 1.0f; f.angle_factor = 1.0f; f.early_exit = 1; f.handoff_scale_t = 0;
    check(uwt_update_params(ctx(), &f), "uwt_update_params");
    const int st = uwt_estimate_pose_batch(ctx(), 1, &a, &b, _previous_frame->rigid_transformation_.data(), &last_stats_);
    uwt_update_params(ctx(), &saved);
    check(st, "uwt_estimate_pose_batch");
  }
  // host copy of one level of a bound frame's planes (Frame::images_/depths_/gradientX_/gradientY_[lvl] in the reference)
  void GetFrameLevel(Frame* _frame, int _lvl, int _plane, void* _host_out) {
    check(uwt_get_plane(ctx(), bind(_frame), _lvl, _plane, _host_out), "uwt_get_plane");
  }
  // include/Tracker.h:188 (src/Tracker.cpp:1473-1525): _outputImage[round(warped)] = _originalImage[(int)point] for every row in
  // order, the last row on a pixel winning; _outputImage (tight rows of the level's image) is written in place — pixels no row lands
  // on keep their content — and validPixel returned.  _originalImage is the plane of a bound frame: (frame, level), or a view of
  // level-0 pixels — those of a bound frame (by address), else uploaded as a frame of the tracker's own, which takes the
  // least-recently-used slot.  (Levels 1.. exist on the device only: name them by frame and level.)
  std::vector<uint8_t> ObtainImageTransformed(Frame* _originalFrame, int _lvl, const std::vector<float>& _candidatePoints,
                                              const std::vector<float>& _warpedPoints, std::vector<uint8_t>& _outputImage) {
    const int slot = bind(_originalFrame);
    const uwt_level L = level(_lvl);
    if (_candidatePoints.size() != _warpedPoints.size() || _outputImage.size() != (size_t)L.img_w * L.img_h)
      throw std::runtime_error("ObtainImageTransformed: the tables differ in size, or the output is not the level's image");
    std::vector<uint8_t> validPixel(_outputImage.size());
    check(uwt_obtain_image_transformed(ctx(), slot, _lvl, _candidatePoints.data(), _warpedPoints.data(), (int32_t)(_warpedPoints.size() / 4),
                                       _outputImage.data(), validPixel.data()), "uwt_obtain_image_transformed");
    return validPixel;
  }
  std::vector<uint8_t> ObtainImageTransformed(const ImageView& _originalImage, const std::vector<float>& _candidatePoints,
                                              const std::vector<float>& _warpedPoints, std::vector<uint8_t>& _outputImage) {
    return ObtainImageTransformed(frame_of(_originalImage), 0, _candidatePoints, _warpedPoints, _outputImage);
  }
  // include/Tracker.h:257 (src/Tracker.cpp:1694-1737): [image1 | image2] over [blend(warped, image2) | blend(image1, image2)], 2 img_w
  // x 2 img_h u8, returned instead of shown (imshow / waitKey and the window's resize loop are the caller's).  _image1 / _image2: the
  // planes of two bound frames at _lvl; _imageWarped: tight rows of that level's image.
  std::vector<uint8_t> DebugShowWarpedPerspective(Frame* _image1, Frame* _image2, const std::vector<uint8_t>& _imageWarped, int _lvl) {
    const int32_t a = bind(_image1), b = bind(_image2);
    const uwt_level L = level(_lvl);
    if (!bound(_image1) || _imageWarped.size() != (size_t)L.img_w * L.img_h)
      throw std::runtime_error("DebugShowWarpedPerspective: more frames than slots, or the warped image is not the level's image");
    std::vector<uint8_t> mosaic(4 * _imageWarped.size());
    check(uwt_warp_mosaic(ctx(), a, b, _lvl, _imageWarped.data(), mosaic.data()), "uwt_warp_mosaic");
    return mosaic;
  }
  // ObtainAllPoints -> WarpFunction -> ObtainImageTransformed for a list of (previous, current) pairs under `poses` in one call
  // (uwt_warp_image_batch): warped and valid are pairs x img_w x img_h u8, quality one record per pair.
  struct WarpedImages {
    std::vector<uint8_t> warped, valid;
    std::vector<uwt_warp_quality> quality;
  };
  WarpedImages WarpedImageBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, const std::vector<SE3>& _poses, int _lvl = 0) {
    const size_t n = _pairs.size();
    if (_poses.size() != n) throw std::runtime_error("WarpedImageBatch: one pose per pair");
    std::vector<int32_t> a(n), b(n);
    for (size_t i = 0; i < n; i++) {
      a[i] = bind(_pairs[i].first);
      b[i] = bind(_pairs[i].second);
    }
    for (size_t i = 0; i < n; i++)   // binding a later pair's frame may have taken an earlier frame's slot
      if (!bound(_pairs[i].first) || !bound(_pairs[i].second) || _pairs[i].first->slot_ != a[i] || _pairs[i].second->slot_ != b[i])
        throw std::runtime_error("WarpedImageBatch: more frames than slots (max_frames)");
    const uwt_level L = level(_lvl);
    WarpedImages r;
    r.warped.resize(n * (size_t)L.img_w * L.img_h);
    r.valid.resize(r.warped.size());
    r.quality.resize(n);
    const int st = uwt_warp_image_batch(ctx(), (int32_t)n, a.data(), b.data(), _lvl, n ? _poses[0].data() : nullptr, r.warped.data(),
                                        r.valid.data(), nullptr, r.quality.data());
    if (st != UWT_ERR_PAIR_FAILED) check(st, "uwt_warp_image_batch");   // a failed pair has its status in its record
    return r;
  }
  // Visualizer::AddPointCloudFromRGBD (src/Visualizer.cpp:421-446) for a list of frames under the accumulated poses `_traj` in one call
  // (uwt_point_cloud_batch; the contract: include/uwt.h): the records in frame order and, inside a frame, in row order; info holds
  // one record per frame, then the call's.  _params null: the reference's call (the dense level-0 table, every 100th row).
  struct PointCloud {
    std::vector<uwt_cloud_point> points;
    std::vector<uwt_cloud_info> info;
  };
  PointCloud PointCloudBatch(const std::vector<Frame*>& _frames, const std::vector<SE3>& _traj, const uwt_cloud_params* _params = nullptr) {
    const size_t n = _frames.size();
    if (_traj.size() != n || !n) throw std::runtime_error("PointCloudBatch: one pose per frame, one frame at least");
    uwt_cloud_params cp;
    if (_params) cp = *_params;
    else check(uwt_default_cloud_params(&cp), "uwt_default_cloud_params");
    if (cp.stride < 1) throw std::runtime_error("PointCloudBatch: stride < 1");
    std::vector<int32_t> slots(n);
    for (size_t i = 0; i < n; i++) {
      slots[i] = bind(_frames[i]);
      if (cp.source == 1 && !_frames[i]->obtained_gradients_)
        throw std::runtime_error("PointCloudBatch: the candidate source needs ApplyGradient (or the frame's slot was reused since)");
    }
    for (size_t i = 0; i < n; i++)   // binding a later frame may have taken an earlier frame's slot
      if (!bound(_frames[i]) || _frames[i]->slot_ != slots[i]) throw std::runtime_error("PointCloudBatch: more frames than slots (max_frames)");
    const uwt_level L = level(0);
    PointCloud r;
    r.points.resize(n * (((size_t)L.w * L.h - 1) / (size_t)cp.stride + 1));
    r.info.resize(n + 1);
    const int st = uwt_point_cloud_batch(ctx(), (int32_t)n, slots.data(), _traj[0].data(), &cp, r.points.data(), (int64_t)r.points.size(),
                                         r.info.data());
    if (st != UWT_ERR_PAIR_FAILED) check(st, "uwt_point_cloud_batch");   // a failed frame has its status in its record
    r.points.resize((size_t)r.info[n].written);
    return r;
  }
  // EXTENSION (no reference counterpart): the keyframe's depth codes from the 1..4 frames `_views` tracked against it and their poses
  // (X_view = T X_keyframe, what the tracking calls return), one job of uwt_sweep_depth_batch (the contract: include/uwt.h).  _codes: the
  // u16 hypotheses (uwt_sweep_hypotheses).  depth, cost: img_w x img_h u16 of the level, outcome: u8 (uwt_sweep_outcome), info the
  // job's record.  _params null: the defaults with n_views and n_hyp taken from the arguments.
  struct SweptDepth {
    std::vector<uint16_t> depth, cost;
    std::vector<uint8_t> outcome;
    uwt_sweep_info info;
  };
  SweptDepth SweepDepth(Frame* _keyframe, const std::vector<Frame*>& _views, const std::vector<SE3>& _poses,
                        const std::vector<uint16_t>& _codes, const uwt_sweep_params* _params = nullptr) {
    const size_t n = _views.size();
    if (_poses.size() != n || !n) throw std::runtime_error("SweepDepth: one pose per view, one view at least");
    uwt_sweep_params sp;
    if (_params) sp = *_params;
    else {
      check(uwt_default_sweep_params(&sp), "uwt_default_sweep_params");
      sp.n_views = (int32_t)n;
      sp.n_hyp = (int32_t)_codes.size();
    }
    if (sp.n_views != (int32_t)n || sp.n_hyp != (int32_t)_codes.size()) throw std::runtime_error("SweepDepth: n_views or n_hyp of the params");
    const int32_t ref = bind(_keyframe);
    if (sp.source == 1 && !_keyframe->obtained_gradients_)
      throw std::runtime_error("SweepDepth: the candidate source needs ApplyGradient on the keyframe (or its slot was reused since)");
    std::vector<int32_t> slots(n);
    for (size_t i = 0; i < n; i++) slots[i] = bind(_views[i]);
    if (!bound(_keyframe) || _keyframe->slot_ != ref) throw std::runtime_error("SweepDepth: more frames than slots (max_frames)");
    for (size_t i = 0; i < n; i++)   // binding a later frame may have taken an earlier frame's slot
      if (!bound(_views[i]) || _views[i]->slot_ != slots[i]) throw std::runtime_error("SweepDepth: more frames than slots (max_frames)");
    if (sp.lvl < 0 || sp.lvl >= params_.n_levels) throw std::runtime_error("SweepDepth: level out of range");
    const uwt_level L = level(sp.lvl);
    SweptDepth r;
    r.depth.resize((size_t)L.img_w * L.img_h);
    r.cost.resize(r.depth.size());
    r.outcome.resize(r.depth.size());
    const int st = uwt_sweep_depth_batch(ctx(), 1, &ref, slots.data(), _poses[0].data(), _codes.data(), &sp, r.depth.data(), r.cost.data(),
                                         r.outcome.data(), &r.info);
    if (st != UWT_ERR_PAIR_FAILED) check(st, "uwt_sweep_depth_batch");   // a failed job has its status in its record
    return r;
  }
  // the same on one explicit N x 4 table of any producer (uwt_point_cloud_points); _frame serves the intensities
  std::vector<uwt_cloud_point> PointCloudPoints(Frame* _frame, const std::vector<float>& _points, const SE3& _pose,
                                                const uwt_cloud_params* _params = nullptr) {
    uwt_cloud_params cp;
    if (_params) cp = *_params;
    else check(uwt_default_cloud_params(&cp), "uwt_default_cloud_params");
    if (cp.stride < 1) throw std::runtime_error("PointCloudPoints: stride < 1");
    const int32_t n = (int32_t)(_points.size() / 4);
    std::vector<uwt_cloud_point> out(n ? ((size_t)n - 1) / (size_t)cp.stride + 1 : 0);
    int64_t count = 0;
    check(uwt_point_cloud_points(ctx(), bind(_frame), _points.data(), n, _pose.data(), &cp, out.data(), (int64_t)out.size(), &count),
          "uwt_point_cloud_points");
    out.resize((size_t)count);
    return out;
  }
  // include/Tracker.h:145 — gradient_ > mean + GRADIENT_THRESHOLD (src/Options.cpp:27) on every level, x-major order
  void ObtainCandidatePoints(Frame* _frame, double gradient_threshold = 20.0) {
    const int slot = bind(_frame);
    if (!_frame->obtained_gradients_)
      throw std::runtime_error("ObtainCandidatePoints: ApplyGradient not called (or the frame's slot was reused since)");
    for (int l = 0; l < params_.n_levels && l < PYRAMID_LEVELS; l++) {
      const uwt_level L = level(l);
      std::vector<float>& t = _frame->candidatePoints_[l];
      t.resize((size_t)L.w * L.h * 4);
      int32_t n = 0;
      check(uwt_obtain_candidate_points(ctx(), slot, l, gradient_threshold, t.data(), L.w * L.h, &n), "uwt_obtain_candidate_points");
      t.resize((size_t)n * 4);
    }
    _frame->obtained_candidatePoints_ = true;
  }
  // include/Tracker.h:155 — 11x11 level-0 patches around Frame::keypoints_ (at most 200)
  void ObtainPatchesPoints(Frame* _previous_frame) {
    const int slot = bind(_previous_frame);
    std::vector<float>& t = _previous_frame->candidatePoints_[0];
    const int cap = 200 * 144;
    t.resize((size_t)cap * 4);
    int32_t n = 0;
    check(uwt_obtain_patch_points(ctx(), slot, _previous_frame->keypoints_.data(), (int)(_previous_frame->keypoints_.size() / 2),
                                  t.data(), cap, &n), "uwt_obtain_patch_points");
    t.resize((size_t)(n < cap ? n : cap) * 4);
    _previous_frame->obtained_candidatePoints_ = true;
  }
  // include/Tracker.h:128 — the reference's live variant: level 0 only, 10 iterations, gain 1, z_factor 0.002
  // (src/Tracker.cpp:634-640, 834), over previous->candidatePoints_[0]
  void EstimatePoseFeatures(Frame* _previous_frame, Frame* _current_frame) {
    const int32_t a = bind(_previous_frame), b = bind(_current_frame);
    if (!_previous_frame->obtained_gradients_)
      throw std::runtime_error("EstimatePoseFeatures: ApplyGradient(previous) not called (or its slot was reused since)");
    uwt_params saved;
    check(uwt_get_params(ctx(), &saved), "uwt_get_params");
    uwt_params f = saved;
    f.first_level = 0; f.last_level = 0; f.max_iters = 10; f.gain = 1.0f; f.z_factor = 0.002f; f.angle_factor = 1.0f;
    f.handoff_scale_t = 1; f.early_exit = 1;
    int32_t jac = UWT_JACOBIAN_REFERENCE;   // (0.002 compensates the pixel coordinate in the reference's column 2: 1 under the metric Jacobian)
    check(uwt_get_jacobian(ctx(), &jac), "uwt_get_jacobian");
    if (jac == UWT_JACOBIAN_METRIC) f.z_factor = 1.0f;
    check(uwt_update_params(ctx(), &f), "uwt_update_params");
    const float* tables[UWT_MAX_LEVELS] = {};
    int32_t counts[UWT_MAX_LEVELS] = {};
    tables[0] = _previous_frame->candidatePoints_[0].data();
    counts[0] = (int32_t)(_previous_frame->candidatePoints_[0].size() / 4);
    const int st = uwt_estimate_pose_points(ctx(), a, b, tables, counts, _previous_frame->rigid_transformation_.data(), &last_stats_);
    uwt_update_params(ctx(), &saved);
    check(st, "uwt_estimate_pose_points");
  }
  // System::Tracking's live call (src/System.cpp:214-219: ObtainPatchesPoints(previous) + EstimatePoseFeatures(previous,
  // current)) for many pairs at once: each previous frame's keypoints_ go in, its rigid_transformation_ comes out.  The patch
  // tables are built and consumed on the device (previous->candidatePoints_ is left as it is); the reference's constants are
  // the call's own, so the tracker's params are not touched.  At most max_pairs pairs, whose frames must all be bound at once
  // (2 x pairs <= max_frames for distinct frames); per-pair stats in last_batch_stats().
  // With options (uwt_table_options: robust weights and / or the bilinear sampler, the call's own): uwt_estimate_pose_features_batch_opt.
  void EstimatePoseFeaturesBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs) { features_batch(_pairs, nullptr); }
  void EstimatePoseFeaturesBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, const uwt_table_options& _options) {
    features_batch(_pairs, &_options);
  }
  // From start poses (_seeds: pairs x 7 floats, one seed per pair; handoff as EstimatePoseSeeded): uwt_estimate_pose_features_batch_seeded.
  void EstimatePoseFeaturesBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, const std::vector<float>& _seeds, int32_t handoff = 0,
                                 const uwt_table_options* _options_or_null = nullptr) {
    if (_seeds.size() != 7 * _pairs.size()) throw std::invalid_argument("EstimatePoseFeaturesBatch: 7 floats of seed per pair");
    const uwt_seed_options so = seed_options(handoff);
    features_batch(_pairs, _options_or_null, _seeds.data(), &so);
  }
 private:
  void features_batch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, const uwt_table_options* opt, const float* seeds = nullptr,
                      const uwt_seed_options* sopt = nullptr) {
    const size_t n = _pairs.size();
    if (n == 0) return;
    std::vector<int32_t> a(n), b(n), counts(n);
    std::vector<float> kp(n * 400, 0.f);
    for (size_t i = 0; i < n; i++) {
      a[i] = bind(_pairs[i].first);
      b[i] = bind(_pairs[i].second);
    }
    for (size_t i = 0; i < n; i++) {   // binding a later pair's frame may have taken an earlier frame's slot
      Frame* prev = _pairs[i].first;
      if (!bound(prev) || !bound(_pairs[i].second))
        throw std::runtime_error("EstimatePoseFeaturesBatch: more frames than slots (max_frames)");
      if (!prev->obtained_gradients_)
        throw std::runtime_error("EstimatePoseFeaturesBatch: ApplyGradient(previous) not called (or its slot was reused since)");
      const size_t m = prev->keypoints_.size() / 2;
      counts[i] = (int32_t)m;
      std::copy(prev->keypoints_.begin(), prev->keypoints_.begin() + 2 * (m < 200 ? m : 200), kp.begin() + 400 * i);
    }
    std::vector<float> poses(n * 7);
    last_batch_stats_.assign(n, uwt_stats{});
    const int st = sopt ? uwt_estimate_pose_features_batch_seeded(ctx(), (int32_t)n, a.data(), b.data(), kp.data(), counts.data(), opt,
                                                                  poses.data(), last_batch_stats_.data(), seeds, sopt)
                   : opt ? uwt_estimate_pose_features_batch_opt(ctx(), (int32_t)n, a.data(), b.data(), kp.data(), counts.data(), opt,
                                                              poses.data(), last_batch_stats_.data())
                       : uwt_estimate_pose_features_batch(ctx(), (int32_t)n, a.data(), b.data(), kp.data(), counts.data(), poses.data(),
                                                          last_batch_stats_.data());
    if (st == UWT_OK || st == UWT_ERR_PAIR_FAILED)
      for (size_t i = 0; i < n; i++) std::copy(poses.begin() + 7 * i, poses.begin() + 7 * (i + 1), _pairs[i].first->rigid_transformation_.data());
    if (st == UWT_OK) last_stats_ = last_batch_stats_.back();
    check(st, sopt ? "uwt_estimate_pose_features_batch_seeded" : opt ? "uwt_estimate_pose_features_batch_opt" : "uwt_estimate_pose_features_batch");
  }
 public:
  // Semi-dense tracking for many pairs at once: ObtainCandidatePoints(previous) (src/Tracker.cpp:1314-1362) on the levels the
  // tracker iterates, then EstimatePose(previous, current) (:362-597) over those tables, under the tracker's params.  Each
  // previous frame's rigid_transformation_ comes out.  The candidate tables are built and consumed on the device
  // (previous->candidatePoints_ is left as it is).  At most max_pairs pairs, whose frames must all be bound at once (2 x pairs <=
  // max_frames for distinct frames); per-pair stats in last_batch_stats().
  // With options (uwt_table_options: robust weights and / or the bilinear sampler, the call's own — the tracker's params keep theirs
  // and are not looked at for them): uwt_estimate_pose_candidates_batch_opt.
  void EstimatePoseCandidatesBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, double gradient_threshold = 20.0) {
    candidates_batch(_pairs, gradient_threshold, nullptr);
  }
  void EstimatePoseCandidatesBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, const uwt_table_options& _options,
                                   double gradient_threshold = 20.0) {
    candidates_batch(_pairs, gradient_threshold, &_options);
  }
  // From start poses (_seeds: pairs x 7 floats; handoff as EstimatePoseSeeded): uwt_estimate_pose_candidates_batch_seeded — the weights
  // and the sampler are then the call's (null options: identity weights and round()), as in the options overload.
  void EstimatePoseCandidatesBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, const std::vector<float>& _seeds, int32_t handoff = 0,
                                   const uwt_table_options* _options_or_null = nullptr, double gradient_threshold = 20.0) {
    if (_seeds.size() != 7 * _pairs.size()) throw std::invalid_argument("EstimatePoseCandidatesBatch: 7 floats of seed per pair");
    const uwt_seed_options so = seed_options(handoff);
    candidates_batch(_pairs, gradient_threshold, _options_or_null, _seeds.data(), &so);
  }
 private:
  void candidates_batch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, double gradient_threshold, const uwt_table_options* opt,
                        const float* seeds = nullptr, const uwt_seed_options* sopt = nullptr) {
    const size_t n = _pairs.size();
    if (n == 0) return;
    std::vector<int32_t> a(n), b(n);
    for (size_t i = 0; i < n; i++) {
      a[i] = bind(_pairs[i].first);
      b[i] = bind(_pairs[i].second);
    }
    for (size_t i = 0; i < n; i++) {   // binding a later pair's frame may have taken an earlier frame's slot
      if (!bound(_pairs[i].first) || !bound(_pairs[i].second))
        throw std::runtime_error("EstimatePoseCandidatesBatch: more frames than slots (max_frames)");
      if (!_pairs[i].first->obtained_gradients_)
        throw std::runtime_error("EstimatePoseCandidatesBatch: ApplyGradient(previous) not called (or its slot was reused since)");
    }
    std::vector<float> poses(n * 7);
    last_batch_stats_.assign(n, uwt_stats{});
    const int st = sopt ? uwt_estimate_pose_candidates_batch_seeded(ctx(), (int32_t)n, a.data(), b.data(), gradient_threshold, opt,
                                                                    poses.data(), last_batch_stats_.data(), seeds, sopt)
                   : opt ? uwt_estimate_pose_candidates_batch_opt(ctx(), (int32_t)n, a.data(), b.data(), gradient_threshold, opt,
                                                                poses.data(), last_batch_stats_.data())
                       : uwt_estimate_pose_candidates_batch(ctx(), (int32_t)n, a.data(), b.data(), gradient_threshold, poses.data(),
                                                            last_batch_stats_.data());
    if (st == UWT_OK || st == UWT_ERR_PAIR_FAILED)
      for (size_t i = 0; i < n; i++) std::copy(poses.begin() + 7 * i, poses.begin() + 7 * (i + 1), _pairs[i].first->rigid_transformation_.data());
    if (st == UWT_OK) last_stats_ = last_batch_stats_.back();
    check(st, sopt ? "uwt_estimate_pose_candidates_batch_seeded" : opt ? "uwt_estimate_pose_candidates_batch_opt" : "uwt_estimate_pose_candidates_batch");
  }
 public:
  // System::Tracking() (src/System.cpp:193-223) for a list of (previous, current) pairs through the device-resident call
  // (uwt_tracking_batch; uwt_tracking_orb_batch for RobustMatcher(tracker, 1)): the detector, the matcher, ransacTest, getGoodKeypoints
  // and the live alignment run as one chain on the device, and keypoints_, surf_keypoints_ (orb_keypoints_ with ORB), n_matches_ of
  // both frames and previous->rigid_transformation_ end up exactly as the loop
  // { ApplyGradient; DetectAndTrackFeatures(previous, current, n_matches_ >= 110); ObtainPatchesPoints; EstimatePoseFeatures } over
  // the same list leaves them.  Pairs that share no frame go into one call; a pair that names a frame an earlier pair of the list
  // has written (the next pair of a sequence) waits for that pair's results, as it does in the loop.  A pair without a good match
  // has UWT_ERR_NO_VALID_POINTS in its stats and leaves its frames' lists empty; that does not throw.  Per-pair stats in
  // last_batch_stats().  (Defined behind RobustMatcher, whose parameters it reads.)
  void TrackingBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, RobustMatcher& _robust_matcher, int32_t cap = 2048) {
    tracking_batch(_pairs, _robust_matcher, cap, nullptr);
  }
  // From start poses for the live alignment (_seeds: pairs x 7 floats; uwt_tracking_batch_seeded / uwt_tracking_orb_batch_seeded): the
  // front end is untouched, and a pair it fails keeps the identity.
  void TrackingBatch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, RobustMatcher& _robust_matcher, const std::vector<float>& _seeds,
                     int32_t cap = 2048) {
    if (_seeds.size() != 7 * _pairs.size()) throw std::invalid_argument("TrackingBatch: 7 floats of seed per pair");
    tracking_batch(_pairs, _robust_matcher, cap, _seeds.data());
  }
 private:
  void tracking_batch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, RobustMatcher& _robust_matcher, int32_t cap, const float* seeds);
 public:
  const std::vector<uwt_stats>& last_batch_stats() const { return last_batch_stats_; }
  // EstimatePose over the sparse tables a producer left in previous->candidatePoints_[lvl] (src/Tracker.cpp:401)
  void EstimatePoseOverCandidatePoints(Frame* _previous_frame, Frame* _current_frame) {
    const int32_t a = bind(_previous_frame), b = bind(_current_frame);
    const float* tables[UWT_MAX_LEVELS] = {};
    int32_t counts[UWT_MAX_LEVELS] = {};
    for (int l = 0; l < PYRAMID_LEVELS; l++) {
      tables[l] = _previous_frame->candidatePoints_[l].data();
      counts[l] = (int32_t)(_previous_frame->candidatePoints_[l].size() / 4);
    }
    check(uwt_estimate_pose_points(ctx(), a, b, tables, counts, _previous_frame->rigid_transformation_.data(), &last_stats_),
          "uwt_estimate_pose_points");
  }
  // include/Tracker.h:224 / :235 — selects the weighting of the following EstimatePose calls (the reference switches by
  // commenting src/Tracker.cpp:495-496): 0 IdentityWeights, 1 TukeyFunctionWeights, 2 Huber (extension)
  // include/Tracker.h:197 — gradients of a tightly packed u8 image (3 x Scharr, CV_16S)
  void ObtainGradientXY(const ImageView& _inputImage, std::vector<int16_t>& _gradientX, std::vector<int16_t>& _gradientY) {
    if (_inputImage.step != (size_t)_inputImage.cols) throw std::runtime_error("ObtainGradientXY: image rows must be contiguous");
    _gradientX.resize((size_t)_inputImage.rows * _inputImage.cols);
    _gradientY.resize(_gradientX.size());
    check(uwt_scharr3(ctx(), static_cast<const uint8_t*>(_inputImage.data), _inputImage.cols, _inputImage.rows, _gradientX.data(),
                      _gradientY.data()), "ObtainGradientXY");
  }

  // include/Tracker.h:206-235 — the weights helpers on an explicit residual vector
  float MedianMat(const std::vector<float>& _input) {
    float med = 0.f;
    check(uwt_robust_weights(ctx(), _input.data(), (int32_t)_input.size(), 0, nullptr, &med, nullptr), "MedianMat");
    return med;
  }
  float MedianAbsoluteDeviation(const std::vector<float>& x) {
    float mad = 0.f;
    check(uwt_robust_weights(ctx(), x.data(), (int32_t)x.size(), 0, nullptr, nullptr, &mad), "MedianAbsoluteDeviation");
    return mad;
  }
  std::vector<float> IdentityWeights(int _num_residuals) { return std::vector<float>((size_t)_num_residuals, 1.0f); }
  std::vector<float> TukeyFunctionWeights(const std::vector<float>& _residuals) {
    std::vector<float> w(_residuals.size());
    check(uwt_robust_weights(ctx(), _residuals.data(), (int32_t)_residuals.size(), 1, w.data(), nullptr, nullptr),
          "TukeyFunctionWeights");
    return w;
  }

  void SetWeights(int weights) {
    uwt_params p;
    check(uwt_get_params(ctx(), &p), "uwt_get_params");
    p.weights = weights;
    check(uwt_update_params(ctx(), &p), "uwt_update_params");
  }
  // uwt_set_jacobian: UWT_JACOBIAN_REFERENCE (the default) or UWT_JACOBIAN_METRIC — every Estimate* call from here on; metric is
  // meant to run with the seeded calls' handoff 1 (keep)
  void SetJacobian(int mode) { check(uwt_set_jacobian(ctx(), mode), "uwt_set_jacobian"); }
  const uwt_stats& last_stats() const { return last_stats_; }
  uwt_level level(int lvl) {  // w_/h_/fx_/fy_/cx_/cy_/invfx_/invfy_[lvl], include/Tracker.h:516-526
    uwt_level L;
    check(uwt_level_info(ctx(), lvl, &L), "uwt_level_info");
    return L;
  }
  uwt_ctx* ctx() {
    if (!ctx_) {
      // (throws for parameters uwt_create refuses; with depth: a depth_scale whose depths leave [UWT_DEPTH_MIN, UWT_DEPTH_MAX], uwt.h)
      check(uwt_create(&params_, &ctx_), "uwt_create");
      // the per-frame sequence (upload + pyramid in bind(), ApplyGradient, EstimatePose) waits once, in EstimatePose
      check(uwt_set_deferred(ctx_, 1), "uwt_set_deferred");
      if (!detail::ls_default_ctx()) detail::ls_default_ctx() = ctx_;   // "LS ls;" inside the tracking loop folds here
    }
    return ctx_;
  }

 private:
  void check(int st, const char* what) {
    if (st != UWT_OK)
      throw std::runtime_error(std::string(what) + ": " + uwt_status_string(st) + (ctx_ ? std::string(" — ") + uwt_last_error(ctx_) : ""));
  }
  // System::AddFrame's pyramid loop (src/System.cpp:246-251): upload level 0, build the other levels on the GPU.
  // Slots are handed out least-recently-used first; the frame that held a reused slot is told so (slot_ = -1, its
  // gradient flag cleared): it uploads again when it is next used instead of silently reading another frame's planes.
  bool bound(const Frame* f) const { return f->slot_ >= 0 && f->tracker_ == this && owner_[(size_t)f->slot_] == f; }
  int bind(Frame* f) {
    if (bound(f)) {
      last_use_[(size_t)f->slot_] = ++use_clock_;
      return f->slot_;
    }
    if (!f->images_[0].data) throw std::runtime_error("bind: Frame::images_[0] has no pixels");
    int slot = 0;
    for (int i = 0; i < max_frames_; i++) {
      if (!owner_[(size_t)i]) { slot = i; break; }
      if (last_use_[(size_t)i] < last_use_[(size_t)slot]) slot = i;
    }
    if (Frame* old = owner_[(size_t)slot]) {
      old->slot_ = -1;
      old->tracker_ = nullptr;
      old->obtained_gradients_ = false;
    }
    owner_[(size_t)slot] = f;
    last_use_[(size_t)slot] = ++use_clock_;
    f->slot_ = slot;
    f->tracker_ = this;
    f->obtained_gradients_ = false;
    check(uwt_set_frame(ctx(), slot, (const uint8_t*)f->images_[0].data, f->images_[0].step,
                        depth_available_ ? (const uint16_t*)f->depths_[0].data : nullptr, f->depths_[0].step),
          "uwt_set_frame");
    check(uwt_build_pyramids(ctx(), slot, 1), "uwt_build_pyramids");
    return slot;
  }
  // the bound frame whose level-0 pixels a view shows (by address); else the view's pixels as a frame of the tracker's own
  Frame* frame_of(const ImageView& v) {
    for (Frame* f : owner_)
      if (f && bound(f) && f->images_[0].data == v.data) return f;
    if (!v.data || v.cols != params_.width || v.rows != params_.height)
      throw std::runtime_error("ObtainImageTransformed: the view is neither a bound frame's level 0 nor an image of level 0's size");
    scratch_frame_.reset(new Frame());
    scratch_frame_->images_[0] = v;
    return scratch_frame_.get();
  }
  std::unique_ptr<Frame> scratch_frame_;
  bool depth_available_;
  int patch_size_ = 5;                 // src/Tracker.cpp:274
  int max_frames_, device_;
  std::vector<Frame*> owner_;          // slot -> frame holding it
  std::vector<uint64_t> last_use_;
  uint64_t use_clock_ = 0;
  uwt_params params_{};
  uwt_ctx* ctx_ = nullptr;
  uwt_stats last_stats_{};
  std::vector<uwt_stats> last_batch_stats_;
};

inline Frame::~Frame() {
  if (tracker_) tracker_->forget(this);
}

// include/Map.h — Map::AddPointCloudFromRGBD (src/Map.cpp:33-45): recent_cloud_points_ is the x y z columns of the frame's level-0
// candidatePoints_ (N x 3, row-major).  A frame whose points were never materialised (the dense ObtainAllPoints keeps no table) has
// none to keep: std::runtime_error.
class Map {
 public:
  std::vector<float> recent_cloud_points_;
  void AddPointCloudFromRGBD(Frame* frame) {
    const std::vector<float>& t = frame->candidatePoints_[0];
    if (t.empty()) throw std::runtime_error("Map::AddPointCloudFromRGBD: the frame has no level-0 candidatePoints_");
    const size_t num_cloud_points = t.size() / 4;
    recent_cloud_points_.resize(num_cloud_points * 3);
    for (size_t i = 0; i < num_cloud_points; i++)
      for (int k = 0; k < 3; k++) recent_cloud_points_[3 * i + k] = t[4 * i + k];
  }
};

// The map-building part of include/Visualizer.h — Visualizer::AddPointCloudFromRGBD (src/Visualizer.cpp:421-446) on the device:
// every 100th row of the frame's level-0 table (its candidatePoints_[0] when a sparse producer ran, else ObtainAllPoints' dense table of
// the bound frame), unprojected and offset by previous_pose's translation, appended to point_cloud_.  previous_pose is the
// accumulation UpdateMessages keeps (uwt_accumulate_trajectory with t_scale 40, reference_axes 0); the tags count the calls.
class Visualizer {
 public:
  explicit Visualizer(Tracker* tracker) : tracker_(tracker) {}
  std::vector<uwt_cloud_point> point_cloud_;
  SE3 previous_pose_;
  void AddPointCloudFromRGBD(Frame* frame, const SE3& previous_pose) {
    previous_pose_ = previous_pose;
    std::vector<uwt_cloud_point> rec = frame->candidatePoints_[0].empty()
                                           ? tracker_->PointCloudBatch({frame}, {previous_pose}).points
                                           : tracker_->PointCloudPoints(frame, frame->candidatePoints_[0], previous_pose);
    for (uwt_cloud_point& p : rec) p.tag = (p.tag & 255u) | ((uint32_t)n_calls_ << 8);
    n_calls_++;
    point_cloud_.insert(point_cloud_.end(), rec.begin(), rec.end());
  }

 private:
  Tracker* tracker_;
  int n_calls_ = 0;
};

// include/Tracker.h:65-88 — RobustMatcher::DetectAndTrackFeatures (src/Tracker.cpp:171-258) from the matcher on: knnMatch in both
// directions, ratioTest twice and symmetryTest on the GPU (uwt_match_descriptors_batch), ransacTest as the inlier selection of
// uwt_ransac_inliers_batch (the contract: include/uwt.h — cv::findFundamentalMat draws from OpenCV's RNG and is not pinned);
// getGoodKeypoints and the assignment of :247-254 on the host.  Detection and description with cuda::SURF_CUDA (:186-206) are
// uwt_surf_detect_describe_batch / uwt_surf_describe_batch, SURF under the contract of include/uwt.h:
// DetectAndTrackFeatures(previous, current, usekeypoints) is the reference's whole method.  RobustMatcher(tracker, 1), as
// RobustMatcher(int detector) of src/Tracker.cpp:38-46, runs cuda::ORB's branch (:210-223) in the same method:
// uwt_orb_detect_describe_batch / uwt_orb_describe_batch, ORB under the contract of include/uwt.h, matched under Hamming, the full
// records kept in Frame::orb_keypoints_.  The overloads that take the caller's descriptors stay.  A caller with a RANSAC of their
// own passes its inliers to SetKeypoints instead.
class RobustMatcher {
 public:
  explicit RobustMatcher(Tracker* tracker, int detector = 0) : detector_(detector), tracker_(tracker) {
    if (detector != 0 && detector != 1) throw std::invalid_argument("RobustMatcher: detector is 0 (SURF) or 1 (ORB)");
  }

  // symMatches of one pair (:202-236), ascending queryIdx.  float rows (n x dim, m x dim) are matched under L2 (SURF, :199), byte
  // rows under Hamming (ORB, :221).
  std::vector<uwt_match> MatchDescriptors(const float* desc_prev, int n, const float* desc_cur, int m, int dim) {
    return match(UWT_NORM_L2, desc_prev, n, desc_cur, m, dim, sizeof(float));
  }
  std::vector<uwt_match> MatchDescriptors(const uint8_t* desc_prev, int n, const uint8_t* desc_cur, int m, int dim) {
    return match(UWT_NORM_HAMMING, desc_prev, n, desc_cur, m, dim, 1);
  }
  // :260-270; keypoints as Frame::keypoints_ holds them (x0 y0 x1 y1 ...): [0] the previous frame's, [1] the current one's
  static std::array<std::vector<float>, 2> getGoodKeypoints(const std::vector<uwt_match>& goodMatches,
                                                            const std::array<std::vector<float>, 2>& keypoints) {
    std::array<std::vector<float>, 2> good;
    for (const uwt_match& mt : goodMatches) {
      const size_t q = (size_t)mt.query_idx, t = (size_t)mt.train_idx;
      if (2 * q + 1 >= keypoints[0].size() || 2 * t + 1 >= keypoints[1].size()) throw std::out_of_range("getGoodKeypoints: match index");
      good[0].insert(good[0].end(), {keypoints[0][2 * q], keypoints[0][2 * q + 1]});
      good[1].insert(good[1].end(), {keypoints[1][2 * t], keypoints[1][2 * t + 1]});
    }
    return good;
  }
  // :247-254 after ransacTest (below, or the caller's own): goodMatches (symMatches, or their inliers), getGoodKeypoints, then keypoints_
  // and n_matches_ of both frames.  Tracker::EstimatePoseFeaturesBatch can follow directly.  n_matches_ feeds the caller's
  // `n_matches_ < 110` rule (src/System.cpp:208), which stays with the caller.
  static void SetKeypoints(Frame* _previous_frame, Frame* _current_frame, const std::vector<uwt_match>& goodMatches,
                           const std::array<std::vector<float>, 2>& keypoints) {
    std::array<std::vector<float>, 2> good = getGoodKeypoints(goodMatches, keypoints);
    _previous_frame->n_matches_ = _current_frame->n_matches_ = (int)goodMatches.size();
    _previous_frame->keypoints_ = std::move(good[0]);
    _current_frame->keypoints_ = std::move(good[1]);
  }
  template <typename T>
  void MatchAndSetKeypoints(Frame* _previous_frame, Frame* _current_frame, const T* desc_prev, int n, const T* desc_cur, int m, int dim,
                            const std::array<std::vector<float>, 2>& keypoints) {
    SetKeypoints(_previous_frame, _current_frame, MatchDescriptors(desc_prev, n, desc_cur, m, dim), keypoints);
  }
  // :105-169: the matches that survive the epipolar test, in their order, into outMatches — the inlier selection of
  // uwt_ransac_inliers_batch (the contract: include/uwt.h).  The reference returns an empty Mat (the local of :124 shadows the
  // matrix it declares at :110); this returns the selection's record, whose F is the hypothesis chosen.  keypoints1 / keypoints2:
  // x0 y0 x1 y1 ... of the previous / current frame.
  uwt_ransac_info ransacTest(const std::vector<uwt_match>& matches, const std::vector<float>& keypoints1,
                             const std::vector<float>& keypoints2, std::vector<uwt_match>& outMatches) {
    const int32_t n = (int32_t)matches.size(), n1 = (int32_t)(keypoints1.size() / 2), n2 = (int32_t)(keypoints2.size() / 2);
    const int32_t cap = std::max(1, n), kp_cap = std::max(1, std::max(n1, n2));
    std::vector<uwt_match> in((size_t)cap), good((size_t)cap);
    std::copy(matches.begin(), matches.end(), in.begin());
    std::vector<float> k1((size_t)kp_cap * 2, 0.f), k2((size_t)kp_cap * 2, 0.f);
    std::copy(keypoints1.begin(), keypoints1.begin() + (size_t)n1 * 2, k1.begin());
    std::copy(keypoints2.begin(), keypoints2.begin() + (size_t)n2 * 2, k2.begin());
    std::vector<uint8_t> mask((size_t)cap);
    uwt_ransac_params rp;
    uwt_default_ransac_params(&rp);
    rp.distance = distance_;
    rp.confidence = confidence_;
    rp.max_hypotheses = max_hypotheses_;
    rp.seed = seed_;
    int32_t count = 0;
    uwt_ransac_info info;
    const int st = uwt_ransac_inliers_batch(tracker_->ctx(), 1, in.data(), &n, cap, k1.data(), &n1, k2.data(), &n2, kp_cap, &rp, mask.data(),
                                            good.data(), &count, &info);
    if (st != UWT_OK)
      throw std::runtime_error(std::string("uwt_ransac_inliers_batch: ") + uwt_status_string(st) + " (" + uwt_last_error(tracker_->ctx()) + ")");
    good.resize((size_t)count);
    outMatches = std::move(good);
    return info;
  }
  // :171-258 from the matcher on, with the caller's detector output: symmetric matches -> ransacTest -> getGoodKeypoints ->
  // keypoints_ and n_matches_ of both frames.  Returns the matches kept.
  template <typename T>
  std::vector<uwt_match> DetectAndTrackFeatures(Frame* _previous_frame, Frame* _current_frame, const T* desc_prev, int n, const T* desc_cur,
                                                int m, int dim, const std::array<std::vector<float>, 2>& keypoints) {
    std::vector<uwt_match> good;
    ransacTest(MatchDescriptors(desc_prev, n, desc_cur, m, dim), keypoints[0], keypoints[1], good);
    SetKeypoints(_previous_frame, _current_frame, good, keypoints);
    return good;
  }

  // :171-258 whole, the reference's own signature: SURF on both frames on the device — the previous frame described at the key
  // points it kept when usekeypoints is set and it has some (:192-195), the current one detected — then symmetric matches ->
  // ransacTest -> getGoodKeypoints -> keypoints_, surf_keypoints_ and n_matches_ of both frames.  Returns the matches kept.
  std::vector<uwt_match> DetectAndTrackFeatures(Frame* _previous_frame, Frame* _current_frame, bool usekeypoints) {
    const int a = tracker_->bind(_previous_frame), b = tracker_->bind(_current_frame);
    if (!tracker_->bound(_previous_frame) || _previous_frame->slot_ != a)
      throw std::runtime_error("DetectAndTrackFeatures: more frames than slots (max_frames)");
    if (detector_ == 1) {   // :210-223: ORB, its rows matched under Hamming, its records kept in orb_keypoints_
      uwt_orb_params op;
      uwt_default_orb_params(&op);
      op.n_features = n_features_;
      op.n_levels = n_levels_;
      op.edge_threshold = edge_threshold_;
      op.fast_threshold = fast_threshold_;
      op.upright = upright_ ? 1 : 0;
      if (!orb_pattern_.empty() && orb_pattern_.size() != 1024) throw std::invalid_argument("RobustMatcher: orb_pattern_ holds 1024 entries");
      if (orb_pattern_ != pattern_sent_) {   // (the context keeps a pattern until it is given another)
        status(uwt_orb_set_pattern(tracker_->ctx(), orb_pattern_.empty() ? nullptr : orb_pattern_.data()), "uwt_orb_set_pattern");
        pattern_sent_ = orb_pattern_;
      }
      return track(_previous_frame, _current_frame, a, b, usekeypoints, op, uwt_orb_detect_describe_batch, "uwt_orb_detect_describe_batch",
                   uwt_orb_describe_batch, "uwt_orb_describe_batch", 32, &Frame::orb_keypoints_);
    }
    uwt_surf_params sp;
    uwt_default_surf_params(&sp);
    sp.hessian_threshold = hessian_threshold_;
    sp.n_octaves = n_octaves_;
    sp.n_octave_layers = n_octave_layers_;
    sp.upright = upright_ ? 1 : 0;
    return track(_previous_frame, _current_frame, a, b, usekeypoints, sp, uwt_surf_detect_describe_batch, "uwt_surf_detect_describe_batch",
                 uwt_surf_describe_batch, "uwt_surf_describe_batch", 64, &Frame::surf_keypoints_);
  }

  // orb_pattern_ to the context when it is not the one sent last, for Tracker::TrackingBatch (as DetectAndTrackFeatures sends it)
  void SendOrbPattern() {
    if (!orb_pattern_.empty() && orb_pattern_.size() != 1024) throw std::invalid_argument("RobustMatcher: orb_pattern_ holds 1024 entries");
    if (orb_pattern_ != pattern_sent_) {
      status(uwt_orb_set_pattern(tracker_->ctx(), orb_pattern_.empty() ? nullptr : orb_pattern_.data()), "uwt_orb_set_pattern");
      pattern_sent_ = orb_pattern_;
    }
  }

  float ratio_ = 0.65f;      // include/Tracker.h:80
  bool refineF_ = true;      // include/Tracker.h:81 — a no-op here: the refit's result is discarded by the reference (:124, :141-166)
  double distance_ = 3.0;    // include/Tracker.h:82
  double confidence_ = 0.99; // include/Tracker.h:83
  int32_t max_hypotheses_ = 1000;   // no reference member: the budget of the selection (uwt_ransac_params)
  uint32_t seed_ = 0;
  double hessian_threshold_ = 100.0;   // cuda::SURF_CUDA's defaults (`cuda::SURF_CUDA surf;`, :188)
  int32_t n_octaves_ = 4, n_octave_layers_ = 2;
  bool upright_ = false;
  int32_t surf_cap_ = UWT_MATCH_MAX_ROWS;   // key points of a frame at most: what the matcher takes
  int detector_ = 0;                   // src/Tracker.cpp:38-46: 0 SURF, 1 ORB
  int32_t n_features_ = 500, n_levels_ = 8, edge_threshold_ = 31, fast_threshold_ = 20;   // cuda::ORB::create()'s defaults (:212)
  std::vector<int8_t> orb_pattern_;    // empty: the library's default pattern; else 256 x (x0, y0, x1, y1) (uwt_orb_set_pattern)

 private:
  // A detector's two entries, P its parameter block and D an element of its descriptor rows:
  //   uwt_surf_detect_describe_batch(ctx, n_frames, slots, &params, cap, kp_out, desc_out, counts_out), or ORB's of the same shape;
  //   uwt_surf_describe_batch(ctx, n_frames, slots, &params, keypoints_in, n_in, cap, kp_out, desc_out), or ORB's.
  template <typename P, typename D>
  using DetectFn = int (*)(uwt_ctx*, int32_t, const int32_t*, const P*, int32_t, uwt_keypoint*, D*, int32_t*);
  template <typename P, typename D>
  using DescribeFn = int (*)(uwt_ctx*, int32_t, const int32_t*, const P*, const uwt_keypoint*, const int32_t*, int32_t, uwt_keypoint*, D*);

  // :186-223 and on, either detector: the previous frame described at the records it kept (Frame::*kept) when usekeypoints is set and
  // it has some (:192-195, :216-218), else detected; the current one detected; then the matcher over rows of `row` elements,
  // ransacTest and the assignment
  template <typename P, typename D>
  std::vector<uwt_match> track(Frame* _previous_frame, Frame* _current_frame, int a, int b, bool usekeypoints, const P& params,
                               DetectFn<P, D> detect_fn, const char* detect_name, DescribeFn<P, D> describe_fn, const char* describe_name,
                               int row, std::vector<uwt_keypoint> Frame::*kept) {
    std::vector<uwt_keypoint> kp[2];
    std::vector<D> desc[2];
    const std::vector<uwt_keypoint>& had = _previous_frame->*kept;
    if (usekeypoints && !had.empty()) {
      const int32_t n = (int32_t)had.size();
      kp[0].resize((size_t)n);
      desc[0].resize((size_t)n * (size_t)row);
      status(describe_fn(tracker_->ctx(), 1, &a, &params, had.data(), &n, n, kp[0].data(), desc[0].data()), describe_name);
    } else {
      detect(a, params, detect_fn, detect_name, row, kp[0], desc[0]);
    }
    detect(b, params, detect_fn, detect_name, row, kp[1], desc[1]);
    std::array<std::vector<float>, 2> xy;
    for (int f = 0; f < 2; f++)
      for (const uwt_keypoint& k : kp[f]) xy[(size_t)f].insert(xy[(size_t)f].end(), {k.x, k.y});
    std::vector<uwt_match> good = DetectAndTrackFeatures(_previous_frame, _current_frame, desc[0].data(), (int)kp[0].size(), desc[1].data(),
                                                         (int)kp[1].size(), row, xy);
    (_previous_frame->*kept).clear();
    (_current_frame->*kept).clear();
    for (const uwt_match& mt : good) {
      (_previous_frame->*kept).push_back(kp[0][(size_t)mt.query_idx]);
      (_current_frame->*kept).push_back(kp[1][(size_t)mt.train_idx]);
    }
    return good;
  }
  template <typename P, typename D>
  void detect(int slot, const P& params, DetectFn<P, D> detect_fn, const char* detect_name, int row, std::vector<uwt_keypoint>& kp,
              std::vector<D>& desc) {
    kp.resize((size_t)surf_cap_);
    desc.resize((size_t)surf_cap_ * (size_t)row);
    int32_t count = 0;
    status(detect_fn(tracker_->ctx(), 1, &slot, &params, surf_cap_, kp.data(), desc.data(), &count), detect_name);
    kp.resize((size_t)count);
    desc.resize((size_t)count * (size_t)row);
  }
  std::vector<int8_t> pattern_sent_;
  void status(int st, const char* what) {
    if (st != UWT_OK) throw std::runtime_error(std::string(what) + ": " + uwt_status_string(st) + " (" + uwt_last_error(tracker_->ctx()) + ")");
  }
  std::vector<uwt_match> match(int norm, const void* a, int n, const void* b, int m, int dim, size_t elem) {
    if (n < 0 || m < 0 || dim < 1) throw std::invalid_argument("MatchDescriptors: negative count or dim < 1");
    const int cap = std::max(1, std::max(n, m));
    const size_t row = (size_t)dim * elem;
    std::vector<unsigned char> q((size_t)cap * row, 0), t((size_t)cap * row, 0);   // one fixed-stride block per set
    if (n) std::memcpy(q.data(), a, (size_t)n * row);
    if (m) std::memcpy(t.data(), b, (size_t)m * row);
    std::vector<uwt_match> out((size_t)cap);
    int32_t count = 0;
    const int32_t nq = n, nt = m;
    const int st = uwt_match_descriptors_batch(tracker_->ctx(), 1, norm, dim, q.data(), &nq, t.data(), &nt, cap, ratio_, out.data(), &count);
    if (st != UWT_OK)
      throw std::runtime_error(std::string("uwt_match_descriptors_batch: ") + uwt_status_string(st) + " (" + uwt_last_error(tracker_->ctx()) + ")");
    out.resize((size_t)count);
    return out;
  }
  Tracker* tracker_;
};

inline void Tracker::tracking_batch(const std::vector<std::pair<Frame*, Frame*>>& _pairs, RobustMatcher& rm, int32_t cap, const float* seeds) {
  // RobustMatcher(tracker, 1): uwt_tracking_orb_batch under the matcher's pattern, the records in orb_keypoints_
  const bool orb = rm.detector_ == 1;
  std::vector<uwt_keypoint> Frame::*kept = orb ? &Frame::orb_keypoints_ : &Frame::surf_keypoints_;
  const char* entry = orb ? (seeds ? "uwt_tracking_orb_batch_seeded" : "uwt_tracking_orb_batch") : (seeds ? "uwt_tracking_batch_seeded" : "uwt_tracking_batch");
  uwt_tracking_params tp;
  uwt_tracking_orb_params top;
  uwt_default_tracking_params(&tp);
  uwt_default_tracking_orb_params(&top);
  tp.surf.hessian_threshold = rm.hessian_threshold_;
  tp.surf.n_octaves = rm.n_octaves_;
  tp.surf.n_octave_layers = rm.n_octave_layers_;
  tp.surf.upright = top.orb.upright = rm.upright_ ? 1 : 0;
  top.orb.n_features = rm.n_features_;
  top.orb.n_levels = rm.n_levels_;
  top.orb.edge_threshold = rm.edge_threshold_;
  top.orb.fast_threshold = rm.fast_threshold_;
  tp.ransac.distance = rm.distance_;
  tp.ransac.confidence = rm.confidence_;
  tp.ransac.max_hypotheses = rm.max_hypotheses_;
  tp.ransac.seed = rm.seed_;
  top.ransac = tp.ransac;
  tp.ratio = top.ratio = rm.ratio_;
  tp.min_matches = top.min_matches = 110;   // src/System.cpp:208
  if (orb) rm.SendOrbPattern();
  if (cap < 1) throw std::invalid_argument("TrackingBatch: cap < 1");
  std::vector<uwt_stats> all;
  for (size_t i = 0; i < _pairs.size();) {
    // the run of pairs from i on that share no frame
    std::vector<std::pair<Frame*, Frame*>> run;
    std::vector<const Frame*> seen;
    auto written = [&](const Frame* f) { return std::find(seen.begin(), seen.end(), f) != seen.end(); };
    while (i < _pairs.size() && (int)run.size() < params_.max_pairs && !written(_pairs[i].first) && !written(_pairs[i].second) &&
           _pairs[i].first != _pairs[i].second) {
      run.push_back(_pairs[i]);
      seen.push_back(_pairs[i].first);
      seen.push_back(_pairs[i].second);
      i++;
    }
    if (run.empty()) throw std::invalid_argument("TrackingBatch: a pair of one frame with itself");
    const size_t n = run.size();
    for (const auto& pr : run) {
      if (!pr.first->obtained_gradients_ || !bound(pr.first)) ApplyGradient(pr.first);
      ApplyGradient(pr.second);
    }
    std::vector<int32_t> a(n), b(n), n_prev(n);
    std::vector<uwt_keypoint> prev(n * (size_t)cap);
    for (size_t k = 0; k < n; k++) {
      a[k] = bind(run[k].first);
      b[k] = bind(run[k].second);
    }
    for (size_t k = 0; k < n; k++) {   // binding a later pair's frame may have taken an earlier frame's slot
      Frame* f = run[k].first;
      if (!bound(f) || !bound(run[k].second) || !f->obtained_gradients_ || !run[k].second->obtained_gradients_)
        throw std::runtime_error("TrackingBatch: more frames than slots (max_frames)");
      const std::vector<uwt_keypoint>& had = f->*kept;
      const size_t m = had.size();
      n_prev[k] = (int32_t)m;
      std::copy(had.begin(), had.begin() + (m < (size_t)cap ? m : (size_t)cap), prev.begin() + k * (size_t)cap);
    }
    std::vector<float> poses(n * 7);
    std::vector<uwt_stats> stats(n, uwt_stats{});
    std::vector<uwt_tracking_info> info(n);
    std::vector<uwt_match> good(n * (size_t)cap);
    std::vector<uwt_keypoint> kept_prev(n * (size_t)cap), kept_cur(n * (size_t)cap);
    int st;
    if (seeds) {
      const float* run_seeds = seeds + 7 * (i - n);
      st = orb ? uwt_tracking_orb_batch_seeded(ctx(), (int32_t)n, a.data(), b.data(), &top, cap, prev.data(), n_prev.data(), poses.data(),
                                               stats.data(), info.data(), good.data(), kept_prev.data(), kept_cur.data(), run_seeds, nullptr)
               : uwt_tracking_batch_seeded(ctx(), (int32_t)n, a.data(), b.data(), &tp, cap, prev.data(), n_prev.data(), poses.data(),
                                           stats.data(), info.data(), good.data(), kept_prev.data(), kept_cur.data(), run_seeds, nullptr);
    } else {
      st = orb ? uwt_tracking_orb_batch(ctx(), (int32_t)n, a.data(), b.data(), &top, cap, prev.data(), n_prev.data(), poses.data(),
                                        stats.data(), info.data(), good.data(), kept_prev.data(), kept_cur.data())
               : uwt_tracking_batch(ctx(), (int32_t)n, a.data(), b.data(), &tp, cap, prev.data(), n_prev.data(), poses.data(),
                                    stats.data(), info.data(), good.data(), kept_prev.data(), kept_cur.data());
    }
    if (st != UWT_OK && st != UWT_ERR_PAIR_FAILED) check(st, entry);
    for (size_t k = 0; k < n; k++) {
      Frame* p = run[k].first;
      Frame* c = run[k].second;
      const size_t m = (size_t)info[k].n_matches;
      p->n_matches_ = c->n_matches_ = (int)m;
      (p->*kept).assign(kept_prev.begin() + k * (size_t)cap, kept_prev.begin() + k * (size_t)cap + m);
      (c->*kept).assign(kept_cur.begin() + k * (size_t)cap, kept_cur.begin() + k * (size_t)cap + m);
      p->keypoints_.clear();
      c->keypoints_.clear();
      for (const uwt_keypoint& q : p->*kept) p->keypoints_.insert(p->keypoints_.end(), {q.x, q.y});
      for (const uwt_keypoint& q : c->*kept) c->keypoints_.insert(c->keypoints_.end(), {q.x, q.y});
      std::copy(poses.begin() + 7 * k, poses.begin() + 7 * (k + 1), p->rigid_transformation_.data());
    }
    all.insert(all.end(), stats.begin(), stats.end());
  }
  last_batch_stats_ = all;
  if (!all.empty()) last_stats_ = all.back();
}

// Four packed floats in place of __m128 where SSE is absent (LS::updateSSE's operands, include/LeastSquares.h:42).
struct f4 {
  float v[4];
};

// include/LeastSquares.h:26-50.  update() / updateSSE() buffer rows; finish*() folds them on the GPU (uwt_ls_accumulate for
// the scalar rows, uwt_ls_accumulate_sse for the 4-wide ones — the two forms associate their products differently,
// src/LeastSquares.cpp:151-153 vs :205) and adds the two, as finishNoDivide adds the lane sums onto A, b, error
// (src/LeastSquares.cpp:39-139).  b keeps the reference's stored sign: b = -Σ w r J (:206, :117-133).
// num_constraints counts 6 per updateSSE call like the reference (:201) unless count_quirk is switched off.
class LS {
 public:
  // "LS ls;" as the reference writes it (src/Tracker.cpp:537): folds on the default context (LS::bind / the first Tracker's)
  LS() : ctx_(nullptr) { initialize(0); }
  explicit LS(uwt_ctx* ctx) : ctx_(ctx) { initialize(0); }
  static void bind(uwt_ctx* ctx) { detail::ls_default_ctx() = ctx; }
  Mat66f A;   // include/LeastSquares.h:34-35 (row-major storage; A is symmetric)
  Mat61f b;
  float error;
  int num_constraints;
  bool count_quirk = true;

  void initialize(const int /*max_num_constraints*/) {
    J_.clear(); r_.clear(); w_.clear();
    J4_.clear(); r4_.clear(); w4_.clear();
    for (int i = 0; i < 36; i++) A.data()[i] = 0.f;
    for (int i = 0; i < 6; i++) b.data()[i] = 0.f;
    error = 0.f;
    num_constraints = 0;
  }
  void update(const float J[6], const float& res, const float& weight) {
    J_.insert(J_.end(), J, J + 6);
    r_.push_back(res);
    w_.push_back(weight);
  }
  // include/LeastSquares.h:40: update(const Mat61f& J, const float& res, const float& weight)
  void update(const Mat61f& J, const float& res, const float& weight) { update(J.data(), res, weight); }
  // four points at once: J1..J6 hold Jacobian component k of the four points (include/LeastSquares.h:42-43)
  void updateSSE(const f4& J1, const f4& J2, const f4& J3, const f4& J4, const f4& J5, const f4& J6, const f4& res,
                 const f4& weight) {
    const f4* Jk[6] = {&J1, &J2, &J3, &J4, &J5, &J6};
    for (int p = 0; p < 4; p++) {
      for (int k = 0; k < 6; k++) J4_.push_back(Jk[k]->v[p]);
      r4_.push_back(res.v[p]);
      w4_.push_back(weight.v[p]);
    }
  }
#ifdef __SSE__
  void updateSSE(const __m128& J1, const __m128& J2, const __m128& J3, const __m128& J4, const __m128& J5, const __m128& J6,
                 const __m128& res, const __m128& weight) {
    f4 a[8];
    const __m128* src[8] = {&J1, &J2, &J3, &J4, &J5, &J6, &res, &weight};
    for (int i = 0; i < 8; i++) _mm_storeu_ps(a[i].v, *src[i]);
    updateSSE(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]);
  }
#endif
  void finishNoDivide() { fold(); }
  void finish() {
    fold();
    const float n = (float)num_constraints;   // src/LeastSquares.cpp:141-146
    for (int i = 0; i < 36; i++) A.data()[i] /= n;
    for (int i = 0; i < 6; i++) b.data()[i] /= n;
    error /= n;
  }

 private:
  void fold() {
    float A1[36] = {}, b1[6] = {}, e1 = 0.f, A2[36] = {}, b2[6] = {}, e2 = 0.f;
    int32_t n1 = 0, n2 = 0;
    uwt_ctx* c = context();
    if (!r_.empty()) chk(uwt_ls_accumulate(c, J_.data(), r_.data(), w_.data(), (int)r_.size(), 0, A1, b1, &e1, &n1), "uwt_ls_accumulate");
    if (!r4_.empty())
      chk(uwt_ls_accumulate_sse(c, J4_.data(), r4_.data(), w4_.data(), (int)r4_.size(), 0, count_quirk ? 1 : 0, A2, b2, &e2, &n2),
          "uwt_ls_accumulate_sse");
    for (int i = 0; i < 36; i++) A.data()[i] = A1[i] + A2[i];
    for (int i = 0; i < 6; i++) b.data()[i] = b1[i] + b2[i];
    error = e1 + e2;
    num_constraints = n1 + n2;
  }
  static void chk(int st, const char* what) {
    if (st != UWT_OK) throw std::runtime_error(std::string(what) + ": " + uwt_status_string(st));
  }
  uwt_ctx* context() { return ctx_ ? ctx_ : detail::ls_context(); }
  uwt_ctx* ctx_;
  std::vector<float> J_, r_, w_, J4_, r4_, w4_;
};

}  // namespace uw
