// shim_tracking_orb — uw::Tracker::TrackingBatch with uw::RobustMatcher(&tracker, 1) through the header-only C++ mirror, for
// tests/test_tracking_orb_shim.py.
//   shim_tracking_orb <w> <h> <fx> <fy> <cx> <cy> <n> <frames.u8> <out.bin>
// Reads n w x h gray frames (one after the other), runs System::Tracking's loop over the pairs (k, k + 1) stage by stage
// (ApplyGradient, DetectAndTrackFeatures under ORB with the n_matches_ < 110 rule, ObtainPatchesPoints, EstimatePoseFeatures) on one tracker and
// uw::Tracker::TrackingBatch over the same list on another, and writes for the loop, then for the batch:
//   per frame: int32 n_matches_ | int32 n | n x 2 float keypoints_ | int32 m | m uwt_keypoint orb_keypoints_ | 7 float
//   rigid_transformation_;  then per pair one uwt_stats.  A frame's surf_keypoints_ must stay empty (else exit code 3).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "uw_tracker.hpp"

typedef std::vector<std::unique_ptr<uw::Frame>> Frames;

static Frames make_frames(const std::vector<unsigned char>& px, int w, int h, int n) {
  Frames fr;
  for (int i = 0; i < n; i++) {
    fr.emplace_back(new uw::Frame());
    fr.back()->idFrame_ = i;
    fr.back()->images_[0] = uw::ImageView(px.data() + (size_t)i * w * h, h, w, (size_t)w);
  }
  return fr;
}

static void dump(FILE* f, const Frames& fr, const std::vector<uwt_stats>& stats) {
  for (const auto& p : fr) {
    if (!p->surf_keypoints_.empty()) std::exit(3);
    const int32_t nm = p->n_matches_, n = (int32_t)(p->keypoints_.size() / 2), m = (int32_t)p->orb_keypoints_.size();
    std::fwrite(&nm, 4, 1, f);
    std::fwrite(&n, 4, 1, f);
    std::fwrite(p->keypoints_.data(), sizeof(float) * 2, (size_t)n, f);
    std::fwrite(&m, 4, 1, f);
    std::fwrite(p->orb_keypoints_.data(), sizeof(uwt_keypoint), (size_t)m, f);
    std::fwrite(p->rigid_transformation_.data(), sizeof(float), 7, f);
  }
  std::fwrite(stats.data(), sizeof(uwt_stats), stats.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 10) { std::fprintf(stderr, "usage: shim_tracking_orb w h fx fy cx cy n frames out\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[7]);
  const float K[9] = {(float)std::atof(argv[3]), 0.f, (float)std::atof(argv[5]), 0.f, (float)std::atof(argv[4]), (float)std::atof(argv[6]),
                      0.f, 0.f, 1.f};
  if (w < 1 || h < 1 || n < 2) return 2;
  std::vector<unsigned char> px((size_t)w * h * n);
  FILE* in = std::fopen(argv[8], "rb");
  if (!in || std::fread(px.data(), 1, px.size(), in) != px.size()) { std::fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
  std::fclose(in);
  try {
    FILE* f = std::fopen(argv[9], "wb");
    if (!f) return 2;
    {   // the loop, stage by stage
      uw::Tracker tracker(false, n + 1);
      tracker.InitializePyramid(w, h, K);
      uw::RobustMatcher rm(&tracker, 1);
      Frames fr = make_frames(px, w, h, n);
      std::vector<uwt_stats> stats;
      for (int k = 0; k + 1 < n; k++) {
        uw::Frame* prev = fr[(size_t)k].get();
        uw::Frame* cur = fr[(size_t)k + 1].get();
        if (!prev->obtained_gradients_) tracker.ApplyGradient(prev);
        tracker.ApplyGradient(cur);
        rm.DetectAndTrackFeatures(prev, cur, !(prev->n_matches_ < 110));
        tracker.ObtainPatchesPoints(prev);
        tracker.EstimatePoseFeatures(prev, cur);
        stats.push_back(tracker.last_stats());
      }
      dump(f, fr, stats);
    }
    {   // the same list in one TrackingBatch
      uw::Tracker tracker(false, n + 1);
      tracker.InitializePyramid(w, h, K);
      uw::RobustMatcher rm(&tracker, 1);
      Frames fr = make_frames(px, w, h, n);
      std::vector<std::pair<uw::Frame*, uw::Frame*>> pairs;
      for (int k = 0; k + 1 < n; k++) pairs.emplace_back(fr[(size_t)k].get(), fr[(size_t)k + 1].get());
      tracker.TrackingBatch(pairs, rm);
      dump(f, fr, tracker.last_batch_stats());
    }
    std::fclose(f);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shim_tracking_orb: %s\n", e.what());
    return 1;
  }
  return 0;
}
