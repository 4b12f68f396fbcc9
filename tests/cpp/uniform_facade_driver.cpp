// uniform_facade_driver.cpp -- what the reference's UNIFORM_SAMPLING branch (keypoints.h:274-290) asks
// of PCL, asked of include/pfx_pcl.hpp in its order: setRadiusSearch, setInputCloud,
// compute(PointCloud<int>&), then cloud->points[idx] for every index.
//   uniform_facade_driver <cloud.pcd> <out_dir>
// The cloud is the first 20,000 points of the file.  Prints the keypoint indices, one per line, and
// writes for tests/test_uniform_facade.py:
//   kp_xyz.f32 (K x 3: the keypoint cloud), shape.i32 (width, height, is_dense of the index cloud),
//   tree.i32 (the indices again, from an object that was also given a search tree),
//   checks.i32: the sizes of compute() without a radius, without an input cloud and with a negative
//   radius (0 each: PCL_ERROR and an empty output), then of a valid compute() on the same object.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointXYZRGB PointRGB;
typedef pcl::PointCloud<PointRGB> Cloud;

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
  if (!load_pcd(argv[1], 20000, *cloud)) {
    std::fprintf(stderr, "cannot read the cloud\n");
    return 2;
  }
  const std::string out = argv[2];
  const double normal_radius_search_ = 0.05;

  {  // the UNIFORM_SAMPLING branch
    Cloud::Ptr keypoints_cloud(new Cloud);
    pcl::PointCloud<int> keypoints;
    pcl::UniformSampling<PointRGB> uniform;
    uniform.setRadiusSearch(normal_radius_search_);
    uniform.setInputCloud(cloud);
    uniform.compute(keypoints);
    if (keypoints.empty()) {
      std::fprintf(stderr, "UniformSampling::compute failed\n");
      return 1;
    }
    std::vector<float> xyz;
    for (size_t i = 0; i < keypoints.points.size(); ++i) {
      const int idx = keypoints.points[i];
      const PointRGB& p = cloud->points[idx];
      keypoints_cloud->push_back(p);
      std::printf("%d\n", idx);
      xyz.push_back(p.x);
      xyz.push_back(p.y);
      xyz.push_back(p.z);
    }
    save(out + "/kp_xyz.f32", xyz);
    save(out + "/shape.i32", std::vector<int32_t>{(int32_t)keypoints.width, (int32_t)keypoints.height,
                                                  (int32_t)keypoints.is_dense});
  }
  {  // a search tree changes nothing: PCL builds one it never queries
    pcl::PointCloud<int> keypoints;
    pcl::UniformSampling<PointRGB> uniform;
    pcl::search::KdTree<PointRGB>::Ptr tree(new pcl::search::KdTree<PointRGB>);
    uniform.setSearchMethod(tree);
    uniform.setRadiusSearch(normal_radius_search_);
    uniform.setInputCloud(cloud);
    uniform.compute(keypoints);
    save(out + "/tree.i32", std::vector<int32_t>(keypoints.points.begin(), keypoints.points.end()));
  }
  {  // what PCL's initCompute rejects fails loudly and leaves the output empty
    std::vector<int32_t> checks;
    pcl::PointCloud<int> keypoints;
    keypoints.push_back(7);
    pcl::UniformSampling<PointRGB> uniform;
    uniform.setInputCloud(cloud);
    uniform.compute(keypoints);  // no radius
    checks.push_back((int32_t)keypoints.size());
    pcl::UniformSampling<PointRGB> no_input;
    no_input.setRadiusSearch(normal_radius_search_);
    keypoints.push_back(7);
    no_input.compute(keypoints);
    checks.push_back((int32_t)keypoints.size());
    uniform.setRadiusSearch(-1.0);
    keypoints.push_back(7);
    uniform.compute(keypoints);
    checks.push_back((int32_t)keypoints.size());
    uniform.setRadiusSearch(0.1);  // ... and the object works afterwards
    uniform.compute(keypoints);
    checks.push_back((int32_t)keypoints.size());
    save(out + "/checks.i32", checks);
  }
  return 0;
}
