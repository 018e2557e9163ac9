// Drives uw::RobustMatcher (include/uw_tracker.hpp) into uw::Tracker::EstimatePoseFeaturesBatch: the matching half of
// DetectAndTrackFeatures (src/Tracker.cpp:224-254) followed by System::Tracking's live call (src/System.cpp:214-219).
//   shim_match <frames.raw> <descriptors.bin> <w> <h> <pairs> [legacy]
// frames.raw: 2 x pairs frames of w*h bytes (previous 0, current 0, previous 1, ...); descriptors.bin: per pair int32 n, m, dim,
// then n x dim and m x dim float32 descriptors (previous, current), then n and m (x, y) float32 key points.  Prints per pair:
//   MATCH <i> <n_matches> <first queryIdx> <first trainIdx>
//   PAIR <i> qx qy qz qw tx ty tz <iterations> <status> <n_valid>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "uw_tracker.hpp"

using namespace uw;

static bool read_floats(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 4, n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), n = std::atoi(argv[5]);
  if (w <= 0 || h <= 0 || n <= 0) return 2;
  std::vector<unsigned char> pix((size_t)2 * n * w * h);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(pix.data(), 1, pix.size(), f) != pix.size()) return 3;
  std::fclose(f);
  std::vector<std::unique_ptr<Frame>> frames;
  for (int i = 0; i < 2 * n; i++) {
    frames.emplace_back(new Frame());
    Frame* fr = frames.back().get();
    fr->idFrame_ = i;
    fr->images_[0] = ImageView(pix.data() + (size_t)i * w * h, h, w, (size_t)w);
    for (int l = 1; l < PYRAMID_LEVELS; l++) resize(fr->images_[l - 1], fr->images_[l], Size(), 0.5, 0.5);
  }
  FILE* k = std::fopen(argv[2], "rb");
  if (!k) return 3;
  try {
    const float fl = 525.0f * w / 640.0f;
    const float K[9] = {fl, 0, w / 2 - 0.5f, 0, fl, h / 2 - 0.5f, 0, 0, 1};
    Tracker tracker(false, /*max_frames=*/2 * n);
    tracker.InitializePyramid(w, h, K);
    if (argc > 6 && !std::strcmp(argv[6], "legacy")) tracker.params().arith = UWT_ARITH_LEGACY;   // the parity suite runs both sets
    RobustMatcher matcher(&tracker);
    std::vector<std::pair<Frame*, Frame*>> pairs;
    for (int i = 0; i < n; i++) {
      Frame* prev = frames[(size_t)2 * i].get();
      Frame* cur = frames[(size_t)2 * i + 1].get();
      int32_t hdr[3];
      if (std::fread(hdr, 4, 3, k) != 3 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 1) return 3;
      std::vector<float> da, db;
      std::array<std::vector<float>, 2> kp;
      if (!read_floats(k, da, (size_t)hdr[0] * hdr[2]) || !read_floats(k, db, (size_t)hdr[1] * hdr[2]) ||
          !read_floats(k, kp[0], (size_t)2 * hdr[0]) || !read_floats(k, kp[1], (size_t)2 * hdr[1]))
        return 3;
      // DetectAndTrackFeatures with the caller's detector output and no ransacTest
      const std::vector<uwt_match> sym = matcher.MatchDescriptors(da.data(), hdr[0], db.data(), hdr[1], hdr[2]);
      RobustMatcher::SetKeypoints(prev, cur, sym, kp);
      std::printf("MATCH %d %d %d %d\n", i, prev->n_matches_, sym.empty() ? -1 : sym[0].query_idx, sym.empty() ? -1 : sym[0].train_idx);
      if (prev->n_matches_ != cur->n_matches_ || prev->keypoints_.size() != 2 * sym.size() || cur->keypoints_.size() != 2 * sym.size()) return 4;
      tracker.ApplyGradient(prev);
      tracker.ApplyGradient(cur);
      pairs.emplace_back(prev, cur);
    }
    std::fclose(k);
    tracker.EstimatePoseFeaturesBatch(pairs);
    for (int i = 0; i < n; i++) {
      const SE3& T = pairs[(size_t)i].first->rigid_transformation_;
      const uwt_stats& s = tracker.last_batch_stats()[(size_t)i];
      std::printf("PAIR %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n", i, T.q[0], T.q[1], T.q[2], T.q[3], T.t[0], T.t[1], T.t[2],
                  s.iterations, s.status, s.n_valid);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
