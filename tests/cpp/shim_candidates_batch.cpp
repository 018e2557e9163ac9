// Drives uw::Tracker::EstimatePoseCandidatesBatch (include/uw_tracker.hpp): ObtainCandidatePoints(previous) + EstimatePose(
// previous, current) for several pairs in one call, under the tracker's default params (the reference schedule).
//   shim_candidates_batch <frames.raw> <w> <h> <pairs> [legacy]
// frames.raw: 2 x pairs frames of w*h bytes (previous 0, current 0, previous 1, ...).  Prints one line per pair:
//   PAIR <i> qx qy qz qw tx ty tz <iterations> <status> <n_valid>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "uw_tracker.hpp"

using namespace uw;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
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
  try {
    const float fl = 525.0f * w / 640.0f;
    const float K[9] = {fl, 0, w / 2 - 0.5f, 0, fl, h / 2 - 0.5f, 0, 0, 1};
    Tracker tracker(false, /*max_frames=*/2 * n);
    tracker.InitializePyramid(w, h, K);
    if (argc > 5 && !std::strcmp(argv[5], "legacy")) tracker.params().arith = UWT_ARITH_LEGACY;   // the parity suite runs both sets
    std::vector<std::pair<Frame*, Frame*>> pairs;
    for (int i = 0; i < n; i++) {
      tracker.ApplyGradient(frames[(size_t)2 * i].get());
      tracker.ApplyGradient(frames[(size_t)2 * i + 1].get());
      pairs.emplace_back(frames[(size_t)2 * i].get(), frames[(size_t)2 * i + 1].get());
    }
    tracker.EstimatePoseCandidatesBatch(pairs);
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
