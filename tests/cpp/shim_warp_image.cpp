// Drives the image-warp surface of uw::Tracker (include/uw_tracker.hpp): WarpedImageBatch, ObtainImageTransformed on the rows
// WarpFunction gives, and DebugShowWarpedPerspective.
//   shim_warp_image <w> <h> <ref.u8> <tgt.u8> <out.bin> [legacy]
// out.bin: the level-0 warped image, its mask and the 48-byte record of WarpedImageBatch under the pose below; the image and mask of
// ObtainImageTransformed over the same table as an explicit one (output pre-filled with 7); the 2w x 2h mosaic.
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
  if (argc < 6) return 2;
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  if (w <= 0 || h <= 0) return 2;
  std::vector<unsigned char> ref((size_t)w * h), tgt((size_t)w * h);
  if (!read_file(argv[3], ref) || !read_file(argv[4], tgt)) return 3;
  Frame prev, cur;
  prev.images_[0] = ImageView(ref.data(), h, w, (size_t)w);
  cur.images_[0] = ImageView(tgt.data(), h, w, (size_t)w);
  for (int l = 1; l < PYRAMID_LEVELS; l++) {
    resize(prev.images_[l - 1], prev.images_[l], Size(), 0.5, 0.5);
    resize(cur.images_[l - 1], cur.images_[l], Size(), 0.5, 0.5);
  }
  try {
    const float fl = 525.0f * w / 640.0f;
    const float K[9] = {fl, 0, w / 2 - 0.5f, 0, fl, h / 2 - 0.5f, 0, 0, 1};
    Tracker tracker(false, /*max_frames=*/4);
    tracker.InitializePyramid(w, h, K);
    tracker.params().n_levels = 3;
    tracker.params().first_level = 2;
    tracker.params().last_level = 0;
    if (argc > 6 && !std::strcmp(argv[6], "legacy")) tracker.params().arith = UWT_ARITH_LEGACY;   // the parity suite runs both sets
    SE3 pose;
    pose.t[0] = 0.02f; pose.t[1] = -0.01f; pose.t[2] = 0.3f;   // contracting: many rows share a pixel
    const Tracker::WarpedImages r = tracker.WarpedImageBatch({{&prev, &cur}}, {pose}, 0);
    if (r.quality.size() != 1 || r.quality[0].status != UWT_OK || r.quality[0].n_covered >= r.quality[0].n_landed) return 4;
    // the same as an explicit table: ObtainAllPoints without depth is (x, y, 1, 1) row by row
    std::vector<float> pts((size_t)w * h * 4);
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        float* p = &pts[4 * ((size_t)y * w + x)];
        p[0] = (float)x; p[1] = (float)y; p[2] = 1.0f; p[3] = 1.0f;
      }
    const std::vector<float> warped = tracker.WarpFunction(pts, pose, 0);
    std::vector<uint8_t> out((size_t)w * h, 7);
    const std::vector<uint8_t> valid = tracker.ObtainImageTransformed(prev.images_[0], pts, warped, out);
    const std::vector<uint8_t> mosaic = tracker.DebugShowWarpedPerspective(&prev, &cur, r.warped, 0);
    if (mosaic.size() != (size_t)4 * w * h) return 4;
    FILE* o = std::fopen(argv[5], "wb");
    if (!o) return 3;
    std::fwrite(r.warped.data(), 1, r.warped.size(), o);
    std::fwrite(r.valid.data(), 1, r.valid.size(), o);
    std::fwrite(r.quality.data(), sizeof(uwt_warp_quality), 1, o);
    std::fwrite(out.data(), 1, out.size(), o);
    std::fwrite(valid.data(), 1, valid.size(), o);
    std::fwrite(mosaic.data(), 1, mosaic.size(), o);
    std::fclose(o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
