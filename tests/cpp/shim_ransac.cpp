// Drives uw::RobustMatcher::ransacTest and DetectAndTrackFeatures (include/uw_tracker.hpp): src/Tracker.cpp:224-254 with ransacTest.
//   shim_ransac ransac <pairs.bin> <pairs>     per pair int32 n, n1, n2, then n uwt_match, n1 and n2 (x, y) float32 key points
//   shim_ransac detect <descriptors.bin> <pairs>   per pair int32 n, m, dim, n x dim and m x dim float32 descriptors, n and m key points
// Prints per pair:
//   RANSAC <i> <count> <best_hypothesis> <hypotheses_run> <status> <nine F as hex uint64> <mask as 0/1 digits, "-" when empty>
//   DETECT <i> <n_matches> <kept queryIdx:trainIdx ...>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "uw_tracker.hpp"

using namespace uw;

static bool read_floats(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), 4, n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const bool detect = !std::strcmp(argv[1], "detect");
  const int n_pairs = std::atoi(argv[3]);
  FILE* f = std::fopen(argv[2], "rb");
  if (!f || n_pairs <= 0) return 3;
  try {
    const float K[9] = {131.25f, 0, 79.5f, 0, 131.25f, 47.5f, 0, 0, 1};
    Tracker tracker(false, /*max_frames=*/2);
    tracker.InitializePyramid(160, 96, K);
    RobustMatcher matcher(&tracker);
    for (int i = 0; i < n_pairs; i++) {
      int32_t hdr[3];
      if (std::fread(hdr, 4, 3, f) != 3 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) return 3;
      if (detect) {
        std::vector<float> da, db;
        std::array<std::vector<float>, 2> kp;
        if (hdr[2] < 1 || !read_floats(f, da, (size_t)hdr[0] * hdr[2]) || !read_floats(f, db, (size_t)hdr[1] * hdr[2]) ||
            !read_floats(f, kp[0], (size_t)2 * hdr[0]) || !read_floats(f, kp[1], (size_t)2 * hdr[1]))
          return 3;
        Frame prev, cur;
        const std::vector<uwt_match> good = matcher.DetectAndTrackFeatures(&prev, &cur, da.data(), hdr[0], db.data(), hdr[1], hdr[2], kp);
        if (prev.n_matches_ != (int)good.size() || cur.n_matches_ != (int)good.size() || prev.keypoints_.size() != 2 * good.size()) return 4;
        std::printf("DETECT %d %d", i, prev.n_matches_);
        for (const uwt_match& m : good) std::printf(" %d:%d", m.query_idx, m.train_idx);
        std::printf("\n");
        continue;
      }
      std::vector<uwt_match> matches((size_t)hdr[0]), good;
      std::vector<float> k1, k2;
      if ((hdr[0] && std::fread(matches.data(), sizeof(uwt_match), matches.size(), f) != matches.size()) ||
          !read_floats(f, k1, (size_t)2 * hdr[1]) || !read_floats(f, k2, (size_t)2 * hdr[2]))
        return 3;
      const uwt_ransac_info info = matcher.ransacTest(matches, k1, k2, good);
      std::printf("RANSAC %d %d %d %d %d", i, (int)good.size(), info.best_hypothesis, info.hypotheses_run, info.status);
      for (int k = 0; k < 9; k++) {
        uint64_t bits;
        std::memcpy(&bits, &info.F[k], 8);
        std::printf(" %016llx", (unsigned long long)bits);
      }
      std::string mask(matches.size(), '0');
      size_t g = 0;
      for (size_t j = 0; j < matches.size() && g < good.size(); j++)
        if (matches[j].query_idx == good[g].query_idx && matches[j].train_idx == good[g].train_idx) { mask[j] = '1'; g++; }
      if (g != good.size()) return 4;   // the kept matches are a subsequence of the input
      std::printf(" %s\n", mask.empty() ? "-" : mask.c_str());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fclose(f);
  return 0;
}
