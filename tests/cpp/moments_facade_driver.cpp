// moments_facade_driver.cpp -- what the reference's DESC_MOMENT_INV and DESC_PPAL_CURV branches
// (src/evaluation.cpp:554-572 and 696-715) ask of PCL, asked of include/pfx_pcl.hpp: an estimator held
// as Feature<PointXYZRGB, T>::Ptr goes through one generic wrapper (features.h:175-196) that casts
// it to FeatureFromNormals and estimates the cloud's normals only when the cast succeeds, then the
// mutual nearest neighbours of the two descriptor clouds (features.h:224-273) are taken.
//   moments_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 48)-th finite point of each cloud; the source's get one more point far away
// from the cloud (an empty neighbourhood: NaN rows).  Writes, for tests/test_moments_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_mi.f32 / tgt_mi.f32 (K x 3), src_pc.f32 / tgt_pc.f32
//   (K x 5), corr_mi.i32 / corr_pc.i32 (index_query, index_match pairs), dense.i32 (is_dense of the
//   four descriptor clouds), casts.i32 (whether the wrapper's cast found normals to compute: moment
//   invariants, curvatures), checks.i32: the rows of a curvature compute() with more keypoints than
//   normals, without normals, with normals of another size than the surface and of a moment compute()
//   without an input (0 each: PCL_ERROR and an empty output), then the rows of valid compute() calls
//   on the same two objects.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointCloud<pcl::PointXYZRGB> Cloud;

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

static Cloud::Ptr every_nth(const Cloud& cloud, size_t want, bool far_point) {
  Cloud::Ptr kp(new Cloud);
  const size_t step = cloud.size() / want ? cloud.size() / want : 1;
  for (size_t i = 0; i < cloud.size() && kp->size() < want; i += step) {
    const pcl::PointXYZRGB& p = cloud.points[i];
    if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z)) kp->push_back(p);
  }
  if (far_point) {
    pcl::PointXYZRGB p;
    p.x = p.y = p.z = 9.0e3f;
    kp->push_back(p);
  }
  return kp;
}

// The generic wrapper: the estimator arrives as its Feature base; whether it wants normals is
// found by a cast, and only then are the cloud's normals estimated (at their own radius).
template <typename DescT>
struct Wrapper {
  typedef typename pcl::Feature<pcl::PointXYZRGB, DescT>::Ptr EstimatorPtr;
  typedef typename pcl::PointCloud<DescT>::Ptr DescPtr;
  EstimatorPtr estimator;
  double radius, normal_radius;
  bool cast_found_normals = false;

  void describe(const Cloud::Ptr& cloud, const Cloud::Ptr& keypoints, DescPtr& rows) {
    typedef pcl::FeatureFromNormals<pcl::PointXYZRGB, pcl::Normal, DescT> WithNormals;
    typename WithNormals::Ptr wants_normals = boost::dynamic_pointer_cast<WithNormals>(estimator);
    cast_found_normals = (bool)wants_normals;
    if (wants_normals) {
      pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
      pcl::NormalEstimationOMP<pcl::PointXYZRGB, pcl::Normal> ne;
      pcl::search::KdTree<pcl::PointXYZRGB>::Ptr ne_tree(new pcl::search::KdTree<pcl::PointXYZRGB>);
      ne.setInputCloud(cloud);
      ne.setRadiusSearch(normal_radius);
      ne.setSearchMethod(ne_tree);
      ne.compute(*normals);
      wants_normals->setInputNormals(normals);
    }
    pcl::search::KdTree<pcl::PointXYZRGB>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZRGB>);
    estimator->setSearchSurface(cloud);
    estimator->setInputCloud(keypoints);
    estimator->setSearchMethod(tree);
    estimator->setRadiusSearch(radius);
    estimator->compute(*rows);
  }

  // nearest row of `to` for every row of `from` (k = 1)
  static std::vector<int> nearest(const DescPtr& from, const DescPtr& to) {
    pcl::KdTreeFLANN<DescT> tree;
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
  static std::vector<int32_t> mutual(const DescPtr& source, const DescPtr& target) {
    const std::vector<int> s2t = nearest(source, target), t2s = nearest(target, source);
    std::vector<int32_t> pairs;
    for (size_t i = 0; i < s2t.size(); ++i)
      if (t2s[(size_t)s2t[i]] == (int)i) {
        pairs.push_back((int32_t)i);
        pairs.push_back((int32_t)s2t[i]);
      }
    return pairs;
  }
};

static void save_xyz(const std::string& path, const Cloud& kp) {
  std::vector<float> v;
  for (const pcl::PointXYZRGB& p : kp.points) {
    v.push_back(p.x);
    v.push_back(p.y);
    v.push_back(p.z);
  }
  save(path, v);
}

static std::vector<float> floats(const pcl::PointCloud<pcl::MomentInvariants>& c) {
  std::vector<float> v;
  for (const pcl::MomentInvariants& p : c.points) {
    v.push_back(p.j1);
    v.push_back(p.j2);
    v.push_back(p.j3);
  }
  return v;
}

static std::vector<float> floats(const pcl::PointCloud<pcl::PrincipalCurvatures>& c) {
  std::vector<float> v;
  for (const pcl::PrincipalCurvatures& p : c.points) {
    v.push_back(p.principal_curvature_x);  // (the named members alias principal_curvature[3])
    v.push_back(p.principal_curvature[1]);
    v.push_back(p.principal_curvature_z);
    v.push_back(p.pc1);
    v.push_back(p.pc2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s source.pcd target.pcd out_dir\n", argv[0]);
    return 2;
  }
  Cloud::Ptr source(new Cloud), target(new Cloud);
  if (!load_pcd(argv[1], *source) || !load_pcd(argv[2], *target)) {
    std::fprintf(stderr, "cannot read the clouds\n");
    return 2;
  }
  const std::string out = argv[3];
  static_assert(sizeof(pcl::MomentInvariants) == 12, "MomentInvariants is three floats");
  static_assert(sizeof(pcl::PrincipalCurvatures) == 20, "PrincipalCurvatures is five floats");
  const Cloud::Ptr source_kp = every_nth(*source, 48, true), target_kp = every_nth(*target, 48, false);
  save_xyz(out + "/src_kp_xyz.f32", *source_kp);
  save_xyz(out + "/tgt_kp_xyz.f32", *target_kp);
  std::vector<int32_t> dense, casts, checks;

  typedef pcl::MomentInvariantsEstimation<pcl::PointXYZRGB, pcl::MomentInvariants> MomentEstimation;
  typedef pcl::PrincipalCurvaturesEstimation<pcl::PointXYZRGB, pcl::Normal, pcl::PrincipalCurvatures>
      CurvatureEstimation;

  {  // moment invariants: a plain Feature
    Wrapper<pcl::MomentInvariants> w;
    w.estimator.reset(new MomentEstimation);
    w.radius = 0.08;
    w.normal_radius = 0.05;
    pcl::PointCloud<pcl::MomentInvariants>::Ptr s(new pcl::PointCloud<pcl::MomentInvariants>),
        t(new pcl::PointCloud<pcl::MomentInvariants>);
    w.describe(source, source_kp, s);
    casts.push_back(w.cast_found_normals);
    w.describe(target, target_kp, t);
    if (s->size() != source_kp->size() || t->size() != target_kp->size()) {
      std::fprintf(stderr, "MomentInvariantsEstimation::compute failed\n");
      return 1;
    }
    save(out + "/src_mi.f32", floats(*s));
    save(out + "/tgt_mi.f32", floats(*t));
    save(out + "/corr_mi.i32", Wrapper<pcl::MomentInvariants>::mutual(s, t));
    dense.push_back(s->is_dense);
    dense.push_back(t->is_dense);
  }
  {  // principal curvatures: a FeatureFromNormals
    Wrapper<pcl::PrincipalCurvatures> w;
    w.estimator.reset(new CurvatureEstimation);
    w.radius = 0.08;
    w.normal_radius = 0.05;
    pcl::PointCloud<pcl::PrincipalCurvatures>::Ptr s(new pcl::PointCloud<pcl::PrincipalCurvatures>),
        t(new pcl::PointCloud<pcl::PrincipalCurvatures>);
    w.describe(source, source_kp, s);
    casts.push_back(w.cast_found_normals);
    w.describe(target, target_kp, t);
    if (s->size() != source_kp->size() || t->size() != target_kp->size()) {
      std::fprintf(stderr, "PrincipalCurvaturesEstimation::compute failed\n");
      return 1;
    }
    save(out + "/src_pc.f32", floats(*s));
    save(out + "/tgt_pc.f32", floats(*t));
    save(out + "/corr_pc.i32", Wrapper<pcl::PrincipalCurvatures>::mutual(s, t));
    dense.push_back(s->is_dense);
    dense.push_back(t->is_dense);
  }
  {  // what PCL 1.7 would read out of bounds is never silent
    pcl::PointCloud<pcl::PrincipalCurvatures> rows;
    pcl::PointCloud<pcl::Normal>::Ptr kp_normals(new pcl::PointCloud<pcl::Normal>);
    kp_normals->resize(source_kp->size());
    CurvatureEstimation pc;
    pc.setRadiusSearch(0.08);
    // more keypoints than normals: the cloud as the input, the keypoints as the surface
    pc.setInputNormals(kp_normals);
    pc.setSearchSurface(source_kp);
    pc.setInputCloud(source);
    pc.compute(rows);
    checks.push_back((int32_t)rows.size());
    // no normals at all
    pc.setInputNormals(pcl::PointCloud<pcl::Normal>::Ptr());
    pc.setSearchSurface(source);
    pc.setInputCloud(source_kp);
    pc.compute(rows);
    checks.push_back((int32_t)rows.size());
    // normals of another size than the surface
    pc.setInputNormals(kp_normals);
    pc.compute(rows);
    checks.push_back((int32_t)rows.size());
    // no input
    pcl::PointCloud<pcl::MomentInvariants> mrows;
    MomentEstimation mi;
    mi.setRadiusSearch(0.08);
    mi.setSearchSurface(source);
    mi.compute(mrows);
    checks.push_back((int32_t)mrows.size());
    // ... and both objects work afterwards (the keypoints are their own surface)
    pc.setSearchSurface(source_kp);
    pc.compute(rows);
    checks.push_back((int32_t)rows.size());
    mi.setInputCloud(source_kp);
    mi.compute(mrows);
    checks.push_back((int32_t)mrows.size());
  }
  save(out + "/dense.i32", dense);
  save(out + "/casts.i32", casts);
  save(out + "/checks.i32", checks);
  return 0;
}
