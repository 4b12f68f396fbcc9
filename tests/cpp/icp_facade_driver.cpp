// icp_facade_driver.cpp -- the reference's ICP refinement (src/evaluation.cpp:863-885 and :257)
// written against include/pfx_pcl.hpp: IterativeClosestPoint<PointXYZRGB, PointXYZRGB> with the
// seven setters the reference calls, align, getFinalTransformation, getFitnessScore, hasConverged,
// then transformPointCloud of the source with the result.
//   icp_facade_driver <source.pcd> <target.pcd> <out_dir>
// Clouds: every 40th point of each file (a keypoint-sized pair).  Writes, for
// tests/test_icp_facade.py:
//   src_xyz.f32 / tgt_xyz.f32 (K x 3), tf.f32 (16, row-major), score.f64, flags.i32 (hasConverged,
//   getConvergenceState), aligned_xyz.f32 (K x 3), moved_xyz.f32 (K x 3: transformPointCloud), rgb.u32
//   (K x 3: the colour words of the source, the aligned and the moved cloud), and the same set with
//   the prefix guess_ for align(out, guess)
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

using namespace pcl;
typedef PointXYZRGB PointRGB;
typedef PointCloud<PointRGB> PointCloudRGB;
typedef IterativeClosestPoint<PointRGB, PointRGB> ItClosestPoint;

static bool read_pcd(const char* path, PointCloudRGB& c, size_t step) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::string line;
  size_t n = 0;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string key;
    ss >> key;
    if (key == "POINTS") ss >> n;
    if (key == "DATA") {
      std::string kind;
      ss >> kind;
      if (kind != "binary") return false;
      break;
    }
  }
  std::vector<float> raw(n * 4);
  f.read(reinterpret_cast<char*>(raw.data()), (std::streamsize)(raw.size() * sizeof(float)));
  if (!f) return false;
  for (size_t i = 0; i < n; i += step) {
    PointRGB p;
    p.x = raw[4 * i]; p.y = raw[4 * i + 1]; p.z = raw[4 * i + 2];
    p.rgb = raw[4 * i + 3];
    c.push_back(p);
  }
  return true;
}

template <typename T>
static void dump(const std::string& path, const T* p, size_t count) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (f) { std::fwrite(p, sizeof(T), count, f); std::fclose(f); }
}

static std::vector<float> xyz_of(const PointCloudRGB& c) {
  std::vector<float> v;
  for (const PointRGB& p : c.points) { v.push_back(p.x); v.push_back(p.y); v.push_back(p.z); }
  return v;
}

// the reference's parameters on a registration object, then the alignment and its three results
static void align_pair(const PointCloudRGB::Ptr& src, const PointCloudRGB::Ptr& tgt, const Eigen::Matrix4f* guess,
                       Eigen::Matrix4f& tf, double& score, bool& convergence, int& state, PointCloudRGB& aligned) {
  ItClosestPoint reg;
  reg.setInputSource(src);
  reg.setInputTarget(tgt);
  reg.setMaximumIterations(100);
  reg.setMaxCorrespondenceDistance(0.07);
  reg.setTransformationEpsilon(1e-6);
  reg.setEuclideanFitnessEpsilon(1e-4);
  reg.setRANSACOutlierRejectionThreshold(0.005);
  if (guess)
    reg.align(aligned, *guess);
  else
    reg.align(aligned);
  tf = reg.getFinalTransformation();
  score = reg.getFitnessScore();
  convergence = reg.hasConverged();
  state = reg.getConvergenceState();
}

static void run(const std::string& out, const std::string& prefix, const PointCloudRGB::Ptr& src,
                const PointCloudRGB::Ptr& tgt, const Eigen::Matrix4f* guess) {
  Eigen::Matrix4f tf;
  double score = 0.0;
  bool convergence = false;
  int state = -1;
  PointCloudRGB aligned;
  align_pair(src, tgt, guess, tf, score, convergence, state, aligned);
  PointCloudRGB::Ptr moved(new PointCloudRGB);
  transformPointCloud(*src, *moved, tf);
  const int32_t flags[2] = {convergence ? 1 : 0, state};
  std::vector<uint32_t> rgb;
  const PointCloudRGB* clouds[3] = {src.get(), &aligned, moved.get()};
  for (const PointCloudRGB* c : clouds)
    for (const PointRGB& p : c->points) rgb.push_back(p.rgba);
  const std::vector<float> a = xyz_of(aligned), m = xyz_of(*moved);
  dump(out + "/" + prefix + "tf.f32", tf.m, 16);
  dump(out + "/" + prefix + "score.f64", &score, 1);
  dump(out + "/" + prefix + "flags.i32", flags, 2);
  dump(out + "/" + prefix + "aligned_xyz.f32", a.data(), a.size());
  dump(out + "/" + prefix + "moved_xyz.f32", m.data(), m.size());
  dump(out + "/" + prefix + "rgb.u32", rgb.data(), rgb.size());
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <source.pcd> <target.pcd> <out_dir>\n", argv[0]);
    return 2;
  }
  PointCloudRGB::Ptr src(new PointCloudRGB), tgt(new PointCloudRGB);
  if (!read_pcd(argv[1], *src, 40) || !read_pcd(argv[2], *tgt, 40)) {
    std::fprintf(stderr, "cannot read the clouds\n");
    return 1;
  }
  const std::string out = argv[3];
  const std::vector<float> s = xyz_of(*src), t = xyz_of(*tgt);
  dump(out + "/src_xyz.f32", s.data(), s.size());
  dump(out + "/tgt_xyz.f32", t.data(), t.size());
  run(out, "", src, tgt, nullptr);
  // a guess 0.01 rad about z and a few centimetres away from the identity
  Eigen::Matrix4f guess;
  guess(0, 0) = 0.99995f; guess(0, 1) = -0.0099998f; guess(1, 0) = 0.0099998f; guess(1, 1) = 0.99995f;
  guess(0, 3) = 0.02f; guess(1, 3) = -0.01f; guess(2, 3) = 0.015f;
  dump(out + "/guess.f32", guess.m, 16);
  run(out, "guess_", src, tgt, &guess);
  return 0;
}
