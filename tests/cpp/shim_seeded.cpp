// shim_seeded — the seeded overloads of the header-only C++ mirror, for tests/test_seeded_shim.py.
//   shim_seeded <w> <h> <fx> <fy> <cx> <cy> <n> <frames.u8> <seeds.f32> <out.bin>
// Reads n w x h gray frames and 2 (n - 1) seeds (7 floats each), and over the pairs (k, k + 1) with seed k writes, each as
// (n - 1) x 7 float poses then (n - 1) uwt_stats:
//   1. EstimatePoseSeeded, handoff 0      2. EstimatePoseSeeded, handoff 1
//   3. EstimatePoseCandidatesBatch(pairs, seeds, 1)
//   4. EstimatePoseFeaturesBatch(pairs, seeds) over a fixed 6 x 5 grid of key points per frame
//   5. TrackingBatch(pairs, matcher, seeds)
// and last PredictSeeds(seeds[0 .. n-1), seeds[n-1 .. 2(n-1))): (n - 1) x 7 floats.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "uw_tracker.hpp"

typedef std::vector<std::unique_ptr<uw::Frame>> Frames;
typedef std::vector<std::pair<uw::Frame*, uw::Frame*>> Pairs;

static Frames make_frames(const std::vector<unsigned char>& px, int w, int h, int n) {
  Frames fr;
  for (int i = 0; i < n; i++) {
    fr.emplace_back(new uw::Frame());
    fr.back()->idFrame_ = i;
    fr.back()->images_[0] = uw::ImageView(px.data() + (size_t)i * w * h, h, w, (size_t)w);
    for (int y = 0; y < 5; y++)
      for (int x = 0; x < 6; x++) {
        fr.back()->keypoints_.push_back((float)(w * (x + 1)) / 7.0f);
        fr.back()->keypoints_.push_back((float)(h * (y + 1)) / 6.0f);
      }
  }
  return fr;
}

static Pairs make_pairs(const Frames& fr) {
  Pairs pairs;
  for (size_t k = 0; k + 1 < fr.size(); k++) pairs.emplace_back(fr[k].get(), fr[k + 1].get());
  return pairs;
}

static void dump(FILE* f, const Pairs& pairs, const std::vector<uwt_stats>& stats) {
  for (const auto& p : pairs) std::fwrite(p.first->rigid_transformation_.data(), sizeof(float), 7, f);
  std::fwrite(stats.data(), sizeof(uwt_stats), stats.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 11) { std::fprintf(stderr, "usage: shim_seeded w h fx fy cx cy n frames seeds out\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]), n = std::atoi(argv[7]);
  const float K[9] = {(float)std::atof(argv[3]), 0.f, (float)std::atof(argv[5]), 0.f, (float)std::atof(argv[4]), (float)std::atof(argv[6]),
                      0.f, 0.f, 1.f};
  if (w < 1 || h < 1 || n < 2) return 2;
  const size_t np = (size_t)n - 1;
  std::vector<unsigned char> px((size_t)w * h * n);
  std::vector<float> seeds(2 * np * 7);
  FILE* in = std::fopen(argv[8], "rb");
  if (!in || std::fread(px.data(), 1, px.size(), in) != px.size()) { std::fprintf(stderr, "cannot read %s\n", argv[8]); return 2; }
  std::fclose(in);
  in = std::fopen(argv[9], "rb");
  if (!in || std::fread(seeds.data(), sizeof(float), seeds.size(), in) != seeds.size()) { std::fprintf(stderr, "cannot read %s\n", argv[9]); return 2; }
  std::fclose(in);
  const std::vector<float> first(seeds.begin(), seeds.begin() + 7 * np), second(seeds.begin() + 7 * np, seeds.end());
  try {
    FILE* f = std::fopen(argv[10], "wb");
    if (!f) return 2;
    uw::Tracker tracker(false, 2 * n);
    tracker.InitializePyramid(w, h, K);
    for (int handoff = 0; handoff < 2; handoff++) {
      Frames fr = make_frames(px, w, h, n);
      const Pairs pairs = make_pairs(fr);
      std::vector<uwt_stats> stats;
      for (size_t k = 0; k < np; k++) {
        uw::SE3 seed;
        std::copy(first.begin() + 7 * k, first.begin() + 7 * (k + 1), seed.data());
        tracker.ApplyGradient(pairs[k].first);
        tracker.EstimatePoseSeeded(pairs[k].first, pairs[k].second, seed, handoff);
        stats.push_back(tracker.last_stats());
      }
      dump(f, pairs, stats);
    }
    {
      Frames fr = make_frames(px, w, h, n);
      const Pairs pairs = make_pairs(fr);
      for (const auto& p : pairs) tracker.ApplyGradient(p.first);
      tracker.EstimatePoseCandidatesBatch(pairs, first, 1);
      dump(f, pairs, tracker.last_batch_stats());
    }
    {
      Frames fr = make_frames(px, w, h, n);
      const Pairs pairs = make_pairs(fr);
      for (const auto& p : pairs) tracker.ApplyGradient(p.first);
      tracker.EstimatePoseFeaturesBatch(pairs, first);
      dump(f, pairs, tracker.last_batch_stats());
    }
    {
      Frames fr = make_frames(px, w, h, n);
      for (auto& p : fr) p->keypoints_.clear();
      const Pairs pairs = make_pairs(fr);
      uw::RobustMatcher rm(&tracker);
      tracker.TrackingBatch(pairs, rm, first);
      dump(f, pairs, tracker.last_batch_stats());
    }
    const std::vector<float> predicted = tracker.PredictSeeds(first, second);
    std::fwrite(predicted.data(), sizeof(float), predicted.size(), f);
    std::fclose(f);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shim_seeded: %s\n", e.what());
    return 1;
  }
  return 0;
}
