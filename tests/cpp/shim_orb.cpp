// shim_orb — ORB through the C ABI and the header-only C++ mirror, for tests/test_orb_shim.py.
//   shim_orb <w> <h> <ref.u8> <tgt.u8> <out.bin>
// Reads two w x h gray frames, runs uw::RobustMatcher(&tracker, 1)::DetectAndTrackFeatures(previous, current, usekeypoints) twice
// (detection, then useProvidedKeypoints on the kept records) and uwt_orb_detect_describe_batch on the previous frame, and writes
//   int32 n_kp | n_kp uwt_keypoint | n_kp x 32 bytes | int32 n_good | n_good uwt_match | n_good x 2 float (previous keypoints_)
//   | n_good uwt_keypoint (previous orb_keypoints_) | int32 n_good2 (second call)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "uw_tracker.hpp"

static std::vector<unsigned char> read_all(const char* path, size_t n) {
  std::vector<unsigned char> b(n);
  FILE* f = std::fopen(path, "rb");
  if (!f || std::fread(b.data(), 1, n, f) != n) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
  std::fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 6) { std::fprintf(stderr, "usage: shim_orb w h ref tgt out\n"); return 2; }
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  std::vector<unsigned char> ref = read_all(argv[3], (size_t)w * h), tgt = read_all(argv[4], (size_t)w * h);
  try {
    uw::Tracker tracker(false, 2);
    const float K[9] = {(float)w * 0.82f, 0.f, (w - 1) * 0.5f, 0.f, (float)w * 0.82f, (h - 1) * 0.5f, 0.f, 0.f, 1.f};
    tracker.InitializePyramid(w, h, K);
    uw::Frame prev, cur;
    prev.images_[0] = uw::ImageView(ref.data(), h, w, (size_t)w);
    cur.images_[0] = uw::ImageView(tgt.data(), h, w, (size_t)w);
    uw::RobustMatcher rm(&tracker, 1);
    std::vector<uwt_match> good = rm.DetectAndTrackFeatures(&prev, &cur, false);
    std::vector<float> kept = prev.keypoints_;
    std::vector<uwt_keypoint> kept_records = prev.orb_keypoints_;
    if (!prev.surf_keypoints_.empty()) { std::fprintf(stderr, "surf_keypoints_ touched\n"); return 1; }
    std::vector<uwt_match> good2 = rm.DetectAndTrackFeatures(&prev, &cur, true);
    const int32_t cap = UWT_MATCH_MAX_ROWS, slot = prev.slot_;
    std::vector<uwt_keypoint> kp((size_t)cap);
    std::vector<uint8_t> desc((size_t)cap * 32);
    int32_t n = 0;
    const int st = uwt_orb_detect_describe_batch(tracker.ctx(), 1, &slot, nullptr, cap, kp.data(), desc.data(), &n);
    if (st != UWT_OK) { std::fprintf(stderr, "uwt_orb_detect_describe_batch: %s\n", uwt_status_string(st)); return 1; }
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    const int32_t ng = (int32_t)good.size(), ng2 = (int32_t)good2.size();
    std::fwrite(&n, 4, 1, f);
    std::fwrite(kp.data(), sizeof(uwt_keypoint), (size_t)n, f);
    std::fwrite(desc.data(), 32, (size_t)n, f);
    std::fwrite(&ng, 4, 1, f);
    std::fwrite(good.data(), sizeof(uwt_match), (size_t)ng, f);
    std::fwrite(kept.data(), sizeof(float) * 2, (size_t)ng, f);
    std::fwrite(kept_records.data(), sizeof(uwt_keypoint), (size_t)ng, f);
    std::fwrite(&ng2, 4, 1, f);
    std::fclose(f);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shim_orb: %s\n", e.what());
    return 1;
  }
  return 0;
}
