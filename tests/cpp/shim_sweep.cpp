// Drives the depth-sweep surface of uw::Tracker (include/uw_tracker.hpp): SweepDepth over the C ABI's uwt_sweep_depth_batch.
//   shim_sweep <w> <h> <ref.u8> <view0.u8> <view1.u8> <out.bin> [legacy]
// out.bin: the level-0 depth and cost planes (u16), the outcome plane (u8) and the 64-byte record of SweepDepth for the keyframe
// `ref` and the two views under the poses below, codes from uwt_sweep_hypotheses(0.5, 2.5, 0.0002, 32), the candidate source.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uw_tracker.hpp"

using namespace uw;

static bool read_file(const char* path, std::vector<unsigned char>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const bool ok = std::fread(v.data(), 1, v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  if (w <= 0 || h <= 0) return 2;
  std::vector<unsigned char> img[3];
  Frame frame[3];
  for (int i = 0; i < 3; i++) {
    img[i].resize((size_t)w * h);
    if (!read_file(argv[3 + i], img[i])) return 3;
    frame[i].images_[0] = ImageView(img[i].data(), h, w, (size_t)w);
    for (int l = 1; l < PYRAMID_LEVELS; l++) resize(frame[i].images_[l - 1], frame[i].images_[l], Size(), 0.5, 0.5);
  }
  try {
    const float fl = 525.0f * w / 640.0f;
    const float K[9] = {fl, 0, w / 2 - 0.5f, 0, fl, h / 2 - 0.5f, 0, 0, 1};
    Tracker tracker(false, /*max_frames=*/4);
    tracker.InitializePyramid(w, h, K);
    tracker.params().n_levels = 2;
    tracker.params().first_level = 1;
    tracker.params().last_level = 0;
    if (argc > 7 && !std::strcmp(argv[7], "legacy")) tracker.params().arith = UWT_ARITH_LEGACY;   // the parity suite runs both sets
    std::vector<uint16_t> codes(32);
    if (uwt_sweep_hypotheses(0.5, 2.5, 0.0002, 32, codes.data()) != UWT_OK) return 4;
    std::vector<SE3> poses(2);
    poses[0].t[0] = 0.2f; poses[0].t[1] = 0.02f;
    poses[1].t[0] = -0.15f; poses[1].t[1] = 0.05f; poses[1].t[2] = 0.01f;
    tracker.ApplyGradient(&frame[0]);
    const Tracker::SweptDepth r = tracker.SweepDepth(&frame[0], {&frame[1], &frame[2]}, poses, codes);
    if (r.info.status != UWT_OK || r.info.n_outcome[UWT_SWEEP_ESTIMATED] <= 0) return 4;
    FILE* o = std::fopen(argv[6], "wb");
    if (!o) return 3;
    std::fwrite(r.depth.data(), 2, r.depth.size(), o);
    std::fwrite(r.cost.data(), 2, r.cost.size(), o);
    std::fwrite(r.outcome.data(), 1, r.outcome.size(), o);
    std::fwrite(&r.info, sizeof(uwt_sweep_info), 1, o);
    std::fclose(o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
