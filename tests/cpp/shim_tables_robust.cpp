// Drives the options overloads of uw::Tracker::EstimatePoseCandidatesBatch and ::EstimatePoseFeaturesBatch (include/uw_tracker.hpp):
// robust weights and / or the bilinear sampler as the call's own uwt_table_options, for several pairs in one call.
//   shim_tables_robust <frames.raw> <w> <h> <pairs> <weights> <sampler> [legacy]
// frames.raw: 2 x pairs frames of w*h bytes (previous 0, current 0, previous 1, ...).  The candidates call runs on levels 2..0, six
// iterations each without the early exit; the features call from 30 key points on a fixed lattice.  Prints per pair:
//   CAND <i> qx qy qz qw tx ty tz <iterations> <status> <n_valid>
//   FEAT <i> ... the same ...
// Without a device (no frames file: "shim_tables_robust --link") it only proves that the mirror compiles and links.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "uw_tracker.hpp"

using namespace uw;

static void print_pairs(const char* tag, const std::vector<std::pair<Frame*, Frame*>>& pairs, const Tracker& tracker) {
  for (size_t i = 0; i < pairs.size(); i++) {
    const SE3& T = pairs[i].first->rigid_transformation_;
    const uwt_stats& s = tracker.last_batch_stats()[i];
    std::printf("%s %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %d %d %d\n", tag, (int)i, T.q[0], T.q[1], T.q[2], T.q[3], T.t[0], T.t[1], T.t[2],
                s.iterations, s.status, s.n_valid);
  }
}

int main(int argc, char** argv) {
  uwt_table_options opt;
  if (uwt_default_table_options(&opt) != UWT_OK || opt.weights != 0 || opt.sampler != 0 || sizeof(opt) != 32) return 4;
  if (argc == 2 && !std::strcmp(argv[1], "--link")) {
    std::printf("LINK %d\n", uwt_abi_version());
    return 0;
  }
  if (argc < 7) return 2;
  const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
  opt.weights = std::atoi(argv[5]);
  opt.sampler = std::atoi(argv[6]);
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
    if (argc > 7 && !std::strcmp(argv[7], "legacy")) tracker.params().arith = UWT_ARITH_LEGACY;   // the parity suite runs both sets
    tracker.params().first_level = 2;
    tracker.params().last_level = 0;
    tracker.params().max_iters = 6;
    tracker.params().early_exit = 0;
    std::vector<std::pair<Frame*, Frame*>> pairs;
    for (int i = 0; i < n; i++) {
      Frame* prev = frames[(size_t)2 * i].get();
      tracker.ApplyGradient(prev);
      tracker.ApplyGradient(frames[(size_t)2 * i + 1].get());
      pairs.emplace_back(prev, frames[(size_t)2 * i + 1].get());
      prev->keypoints_.clear();
      for (int k = 0; k < 30; k++) {
        prev->keypoints_.push_back(10.0f + (float)(k % 10) * 14.5f);
        prev->keypoints_.push_back(10.0f + (float)(k / 10) * 30.25f);
      }
    }
    tracker.EstimatePoseCandidatesBatch(pairs, opt);
    print_pairs("CAND", pairs, tracker);
    tracker.EstimatePoseFeaturesBatch(pairs, opt);
    print_pairs("FEAT", pairs, tracker);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
