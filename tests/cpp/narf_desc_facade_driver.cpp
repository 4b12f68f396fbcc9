// narf_desc_facade_driver.cpp -- what the reference's DESC_NARF branch (src/evaluation.cpp:613-648)
// asks of PCL up to findCorrespondences, asked of include/pfx_pcl.hpp, with the body of
// Tools::getIndices (tools.h:91-102) replaced by pfx_point_indices.  The branch is reproduced as
// written, its two defects included: the cloud indices of getIndices are handed to NarfDescriptor as
// pixel indices, and the target's descriptors are taken on the SOURCE range image.
//   narf_desc_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: the NARF keypoints of each cloud as the reference's keypoint path leaves them (the
// cloud's points at the keypoints' pixel indices, keypoints.h:227-229).  Writes, for
// tests/test_narf_desc_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_idx.i32 / tgt_idx.i32 (the indices of getIndices),
//   src_rows.f32 / tgt_rows.f32 (M x 42, the Narf36 rows), src_keys.i32 / tgt_keys.i32
//   (getRowIndices), corr.i32 (pairs), checks.i32: the rows of a compute() without a range image,
//   without indices and without a support size (0 each), then of a valid one without rotation
//   invariance on the same object.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointCloud<pcl::PointXYZRGB> Cloud;
typedef pcl::PointCloud<pcl::Narf36> Rows;

static bool load_pcd(const char* path, Cloud& c) {
  std::ifstream f(path, std::ios::binary);
  std::string line;
  size_t n = 0;
  bool binary = false;
  while (f && std::getline(f, line)) {
    std::istringstream ss(line);
    std::string key, kind;
    ss >> key;
    if (key == "POINTS") ss >> n;
    if (key == "DATA") {
      ss >> kind;
      binary = kind == "binary";
      break;
    }
  }
  if (!f || !binary) return false;
  std::vector<float> raw(n * 4);
  f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)(raw.size() * sizeof(float)));
  if (!f) return false;
  c.points.resize(n);
  for (size_t i = 0; i < n; ++i) {
    c.points[i].x = raw[4 * i];
    c.points[i].y = raw[4 * i + 1];
    c.points[i].z = raw[4 * i + 2];
    c.points[i].rgb = raw[4 * i + 3];
  }
  c.width = (uint32_t)n;
  c.height = 1;
  return true;
}

template <typename T>
static void save(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return;
  std::fwrite(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
}

// Tools::convertToRangeImage: the 640 x 480 planar image of the reference's camera at the origin
static void to_range_image(const Cloud::Ptr& cloud, pcl::RangeImagePlanar& image) {
  image.createFromPointCloudWithFixedSize(*cloud, 640, 480, 320.0f, 240.0f, 525.0f, 525.0f, Eigen::Affine3f::Identity(),
                                          pcl::RangeImage::CAMERA_FRAME, 0.0f, 0.0f);
}

// the NARF keypoints as a cloud: the cloud's points at the keypoints' pixel indices
static Cloud::Ptr narf_keypoints(const Cloud::Ptr& cloud) {
  pcl::RangeImagePlanar image;
  to_range_image(cloud, image);
  pcl::RangeImageBorderExtractor border_extractor;
  pcl::NarfKeypoint detector(&border_extractor);
  detector.setRangeImage(&image);
  detector.getParameters().support_size = 0.2f;
  pcl::PointCloud<int> pixels;
  detector.compute(pixels);
  Cloud::Ptr kp(new Cloud);
  for (int p : pixels.points)
    if ((size_t)p < cloud->size()) kp->push_back(cloud->points[(size_t)p]);
  return kp;
}

// Tools::getIndices, its double loop handed to the library
static bool get_indices(const Cloud::Ptr& cloud, const Cloud::Ptr& inliers, std::vector<int>& indices) {
  const pcl::detail::SoA c = pcl::detail::soa_xyz(*cloud), k = pcl::detail::soa_xyz(*inliers);
  std::vector<int32_t> out(64 + 2 * inliers->size());
  int64_t m = 0;
  pfx_status st = pfx_point_indices(pcl::detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)c.x.size(),
                                    k.x.data(), k.y.data(), k.z.data(), (int64_t)k.x.size(), 1e-4f, out.data(),
                                    (int64_t)out.size(), &m);
  if (st == PFX_ERR_CAPACITY) {
    out.resize((size_t)m);
    st = pfx_point_indices(pcl::detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)c.x.size(), k.x.data(),
                           k.y.data(), k.z.data(), (int64_t)k.x.size(), 1e-4f, out.data(), (int64_t)out.size(), &m);
  }
  if (st != PFX_OK) return false;
  indices.insert(indices.end(), out.begin(), out.begin() + m);
  return true;
}

// nearest row of `to` for every row of `from` (k = 1)
static std::vector<int> nearest_rows(const Rows::Ptr& from, const Rows::Ptr& to) {
  pcl::KdTreeFLANN<pcl::Narf36> tree;
  tree.setInputCloud(to);
  std::vector<int> best(from->size()), idx(1);
  std::vector<float> dist(1);
  for (size_t i = 0; i < from->size(); ++i) {
    tree.nearestKSearch(*from, (int)i, 1, idx, dist);
    best[i] = idx[0];
  }
  return best;
}

// the pairs that choose each other, in source order
static std::vector<int32_t> find_correspondences(const Rows::Ptr& source, const Rows::Ptr& target) {
  std::vector<int32_t> pairs;
  if (source->empty() || target->empty()) return pairs;
  const std::vector<int> s2t = nearest_rows(source, target), t2s = nearest_rows(target, source);
  for (size_t i = 0; i < s2t.size(); ++i)
    if (t2s[(size_t)s2t[i]] == (int)i) {
      pairs.push_back((int32_t)i);
      pairs.push_back((int32_t)s2t[i]);
    }
  return pairs;
}

static void save_xyz(const std::string& path, const Cloud& kp) {
  std::vector<float> v;
  for (const pcl::PointXYZRGB& p : kp.points) {
    v.push_back(p.x);
    v.push_back(p.y);
    v.push_back(p.z);
  }
  save(path, v);
}

static std::vector<float> floats(const Rows& rows) {
  static_assert(sizeof(pcl::Narf36) == 42 * sizeof(float), "Narf36 is 42 floats");
  const float* p = reinterpret_cast<const float*>(rows.points.data());
  return std::vector<float>(p, p + rows.size() * 42);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s source.pcd target.pcd out_dir\n", argv[0]);
    return 2;
  }
  Cloud::Ptr source_cloud(new Cloud), target_cloud(new Cloud);
  if (!load_pcd(argv[1], *source_cloud) || !load_pcd(argv[2], *target_cloud)) {
    std::fprintf(stderr, "cannot read the clouds\n");
    return 2;
  }
  const std::string out = argv[3];
  const Cloud::Ptr source_keypoints = narf_keypoints(source_cloud), target_keypoints = narf_keypoints(target_cloud);
  save_xyz(out + "/src_kp_xyz.f32", *source_keypoints);
  save_xyz(out + "/tgt_kp_xyz.f32", *target_keypoints);

  {  // the DESC_NARF branch
    Rows::Ptr source_features(new Rows), target_features(new Rows);
    pcl::RangeImagePlanar source_range_image, target_range_image;
    to_range_image(source_cloud, source_range_image);
    to_range_image(target_cloud, target_range_image);
    std::vector<int> source_keypoint_indices, target_keypoint_indices;
    if (!get_indices(source_cloud, source_keypoints, source_keypoint_indices) ||
        !get_indices(target_cloud, target_keypoints, target_keypoint_indices)) {
      std::fprintf(stderr, "pfx_point_indices failed\n");
      return 1;
    }
    pcl::NarfDescriptor source_feat(&source_range_image, &source_keypoint_indices);
    pcl::NarfDescriptor target_feat(&source_range_image, &target_keypoint_indices);  // (the source image, as written)
    source_feat.getParameters().support_size = 0.2f;
    source_feat.getParameters().rotation_invariant = true;
    source_feat.compute(*source_features);
    target_feat.getParameters().support_size = 0.2f;
    target_feat.getParameters().rotation_invariant = true;
    target_feat.compute(*target_features);
    save(out + "/src_idx.i32", std::vector<int32_t>(source_keypoint_indices.begin(), source_keypoint_indices.end()));
    save(out + "/tgt_idx.i32", std::vector<int32_t>(target_keypoint_indices.begin(), target_keypoint_indices.end()));
    save(out + "/src_rows.f32", floats(*source_features));
    save(out + "/tgt_rows.f32", floats(*target_features));
    save(out + "/src_keys.i32", std::vector<int32_t>(source_feat.getRowIndices().begin(), source_feat.getRowIndices().end()));
    save(out + "/tgt_keys.i32", std::vector<int32_t>(target_feat.getRowIndices().begin(), target_feat.getRowIndices().end()));
    save(out + "/corr.i32", find_correspondences(source_features, target_features));
  }
  {  // what compute() cannot serve fails loudly; the object works afterwards
    std::vector<int32_t> checks;
    pcl::RangeImagePlanar image;
    to_range_image(source_cloud, image);
    const std::vector<int> indices = {640 * 240 + 320, 640 * 200 + 300, -1};
    Rows rows;
    pcl::NarfDescriptor d;
    d.getParameters().support_size = 0.2f;
    d.compute(rows);  // neither image nor indices
    checks.push_back((int32_t)rows.size());
    d.setRangeImage(&image);
    d.compute(rows);  // no indices
    checks.push_back((int32_t)rows.size());
    d.setRangeImage(&image, &indices);
    d.getParameters().support_size = -1.0f;
    d.compute(rows);  // no support size
    checks.push_back((int32_t)rows.size());
    d.getParameters().support_size = 0.2f;
    d.getParameters().rotation_invariant = false;
    d.compute(rows);
    checks.push_back((int32_t)rows.size());
    save(out + "/checks.i32", checks);
    save(out + "/plain_rows.f32", floats(rows));
  }
  return 0;
}
