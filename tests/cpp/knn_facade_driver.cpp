// knn_facade_driver.cpp -- the k-search half of PCL's neighbourhood contract, asked of
// include/pfx_pcl.hpp: NormalEstimationOMP with setKSearch, PCL's initCompute rule when a radius is
// set as well, a class without a k-NN path, and KdTreeFLANN<PointXYZRGB>::nearestKSearch with k > 1.
//   knn_facade_driver <cloud.pcd> <out_dir>
// The cloud is the first 4,000 points of the file.  Writes for tests/test_knn_facade.py:
//   normals.f32 (n x 4: normal_x, normal_y, normal_z, curvature of setKSearch(10)), dense.i32 (is_dense),
//   checks.i32: the sizes of compute() with k and a radius, with neither, of BoundaryEstimation with
//   setKSearch(10), then of a valid compute() on the first object after setRadiusSearch(0);
//   knn_idx.i32 / knn_d2.f32 (16 x 5) and knn_ret.i32 (16): nearestKSearch(p, 5, ...) for every 250th
//   point of the cloud, shifted by 1 mm; knn_edge.i32: the return values for k = 0, k = 257 and a NaN
//   point, and the count for k = 256.
#include <cstdio>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointXYZRGB PointRGB;
typedef pcl::PointCloud<PointRGB> Cloud;
typedef pcl::PointCloud<pcl::Normal> Normals;

static bool load_pcd(const char* path, size_t keep, Cloud& c) {
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
  if (n > keep) n = keep;
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

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s cloud.pcd out_dir\n", argv[0]);
    return 2;
  }
  Cloud::Ptr cloud(new Cloud);
  if (!load_pcd(argv[1], 4000, *cloud)) {
    std::fprintf(stderr, "cannot read the cloud\n");
    return 2;
  }
  const std::string out = argv[2];
  Normals::Ptr normals(new Normals);
  std::vector<int32_t> checks;

  pcl::NormalEstimationOMP<PointRGB, pcl::Normal> ne;
  pcl::search::KdTree<PointRGB>::Ptr tree(new pcl::search::KdTree<PointRGB>);
  ne.setSearchMethod(tree);
  ne.setInputCloud(cloud);
  ne.setKSearch(10);
  ne.compute(*normals);
  if (normals->size() != cloud->size()) {
    std::fprintf(stderr, "NormalEstimationOMP::compute with setKSearch(10) failed\n");
    return 1;
  }
  std::vector<float> flat;
  for (const pcl::Normal& p : normals->points) {
    flat.push_back(p.normal_x);
    flat.push_back(p.normal_y);
    flat.push_back(p.normal_z);
    flat.push_back(p.curvature);
  }
  save(out + "/normals.f32", flat);
  save(out + "/dense.i32", std::vector<int32_t>{(int32_t)normals->is_dense});

  {  // PCL's initCompute rule: both set is an error, neither set is one too
    Normals both;
    both.push_back(pcl::Normal());
    ne.setRadiusSearch(0.05);
    ne.compute(both);
    checks.push_back((int32_t)both.size());
    Normals neither;
    neither.push_back(pcl::Normal());
    ne.setRadiusSearch(0.0);
    ne.setKSearch(0);
    ne.compute(neither);
    checks.push_back((int32_t)neither.size());
  }
  {  // a class without a k-NN path keeps its refusal
    pcl::PointCloud<pcl::Boundary> flags;
    flags.push_back(pcl::Boundary());
    pcl::BoundaryEstimation<PointRGB, pcl::Normal, pcl::Boundary> b;
    b.setInputCloud(cloud);
    b.setInputNormals(normals);
    b.setKSearch(10);
    b.compute(flags);
    checks.push_back((int32_t)flags.size());
  }
  {  // ... and the first object works afterwards
    Normals again;
    ne.setKSearch(10);
    ne.compute(again);
    checks.push_back((int32_t)again.size());
  }
  save(out + "/checks.i32", checks);

  pcl::KdTreeFLANN<PointRGB> kd;
  kd.setInputCloud(cloud);
  std::vector<int32_t> idx, ret, edge;
  std::vector<float> d2;
  std::vector<int> k_indices;
  std::vector<float> k_sqr;
  for (size_t i = 0; i < cloud->size(); i += 250) {
    PointRGB p = cloud->points[i];
    p.x += 0.001f;
    ret.push_back(kd.nearestKSearch(p, 5, k_indices, k_sqr));
    idx.insert(idx.end(), k_indices.begin(), k_indices.end());
    d2.insert(d2.end(), k_sqr.begin(), k_sqr.end());
  }
  save(out + "/knn_idx.i32", idx);
  save(out + "/knn_d2.f32", d2);
  save(out + "/knn_ret.i32", ret);
  PointRGB p = cloud->points[0];
  edge.push_back(kd.nearestKSearch(p, 0, k_indices, k_sqr));
  edge.push_back(kd.nearestKSearch(p, PFX_KNN_MAX_K + 1, k_indices, k_sqr));
  PointRGB bad = p;
  bad.y = std::numeric_limits<float>::quiet_NaN();
  edge.push_back(kd.nearestKSearch(bad, 5, k_indices, k_sqr));
  edge.push_back(kd.nearestKSearch(p, PFX_KNN_MAX_K, k_indices, k_sqr));
  edge.push_back((int32_t)k_indices.size());
  save(out + "/knn_edge.i32", edge);
  return 0;
}
