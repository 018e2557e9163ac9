// Drives the point-cloud surface of include/uw_tracker.hpp: uw::Tracker::PointCloudBatch and PointCloudPoints, uw::Map and
// uw::Visualizer::AddPointCloudFromRGBD.
//   shim_cloud <w> <h> <a.u8> <b.u8> <a.u16> <b.u16> <out.bin> [legacy]
// out.bin: int64 counts n1 n2 n3 n4, then the records of (1) PointCloudBatch over both frames under the poses below with stride 7 and
// skip_invalid 1 in world mode, its 3 info records behind them; (2) Visualizer::AddPointCloudFromRGBD on both frames, dense (the
// reference's constants); (3) the same on frame a after ObtainCandidatePoints(a, 5.0); (4) Map::recent_cloud_points_ of that frame as
// n4 x 3 floats.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uw_tracker.hpp"

using namespace uw;

template <typename T>
static bool read_file(const char* path, std::vector<T>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const bool ok = std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
  std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
  if (w <= 0 || h <= 0) return 2;
  std::vector<unsigned char> ia((size_t)w * h), ib((size_t)w * h);
  std::vector<unsigned short> da((size_t)w * h), db((size_t)w * h);
  if (!read_file(argv[3], ia) || !read_file(argv[4], ib) || !read_file(argv[5], da) || !read_file(argv[6], db)) return 3;
  Frame a, b;
  a.images_[0] = ImageView(ia.data(), h, w, (size_t)w);
  b.images_[0] = ImageView(ib.data(), h, w, (size_t)w);
  a.depths_[0] = ImageView(da.data(), h, w, (size_t)w * 2);
  b.depths_[0] = ImageView(db.data(), h, w, (size_t)w * 2);
  a.depth_available_ = b.depth_available_ = true;
  try {
    const float fl = 525.0f * w / 640.0f;
    const float K[9] = {fl, 0, w / 2 - 0.5f, 0, fl, h / 2 - 0.5f, 0, 0, 1};
    Tracker tracker(true, /*max_frames=*/4);
    tracker.InitializePyramid(w, h, K);
    tracker.params().n_levels = 3;
    tracker.params().first_level = 2;
    tracker.params().last_level = 0;
    if (argc > 8 && !std::strcmp(argv[8], "legacy")) tracker.params().arith = UWT_ARITH_LEGACY;   // the parity suite runs both sets
    SE3 pa, pb;
    pa.t[0] = 0.5f; pa.t[1] = -0.25f; pa.t[2] = 1.5f;
    pb.q[2] = 0.0871557f; pb.q[3] = 0.9961947f;   // 10 degrees about the optical axis
    pb.t[0] = -1.0f; pb.t[1] = 0.75f; pb.t[2] = 2.0f;
    uwt_cloud_params cp;
    if (uwt_default_cloud_params(&cp) != UWT_OK) return 4;
    cp.mode = 1;
    cp.stride = 7;
    cp.skip_invalid = 1;
    const Tracker::PointCloud r = tracker.PointCloudBatch({&a, &b}, {pa, pb}, &cp);
    if (r.info.size() != 3 || r.info[0].status != UWT_OK || r.info[2].status != UWT_OK) return 4;
    Visualizer vis(&tracker);
    vis.AddPointCloudFromRGBD(&a, pa);
    vis.AddPointCloudFromRGBD(&b, pb);
    const std::vector<uwt_cloud_point> dense = vis.point_cloud_;
    tracker.ApplyGradient(&a);
    tracker.ObtainCandidatePoints(&a, 5.0);
    Visualizer vis2(&tracker);
    vis2.AddPointCloudFromRGBD(&a, pb);
    Map map;
    map.AddPointCloudFromRGBD(&a);
    FILE* o = std::fopen(argv[7], "wb");
    if (!o) return 3;
    const long long n[4] = {(long long)r.points.size(), (long long)dense.size(), (long long)vis2.point_cloud_.size(),
                            (long long)(map.recent_cloud_points_.size() / 3)};
    std::fwrite(n, sizeof(long long), 4, o);
    std::fwrite(r.points.data(), sizeof(uwt_cloud_point), r.points.size(), o);
    std::fwrite(r.info.data(), sizeof(uwt_cloud_info), r.info.size(), o);
    std::fwrite(dense.data(), sizeof(uwt_cloud_point), dense.size(), o);
    std::fwrite(vis2.point_cloud_.data(), sizeof(uwt_cloud_point), vis2.point_cloud_.size(), o);
    std::fwrite(map.recent_cloud_points_.data(), sizeof(float), map.recent_cloud_points_.size(), o);
    std::fclose(o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
