// boundary_facade_driver.cpp -- what the reference's DESC_BOUNDARY branch (src/evaluation.cpp:394-415)
// asks of PCL up to its compute calls, asked of include/pfx_pcl.hpp: a BoundaryEstimation held as
// Feature<PointXYZRGB, Boundary>::Ptr goes through the generic wrapper (features.h:175-196), which
// casts it to FeatureFromNormals and estimates the cloud's normals, one per point of the search
// surface, because the cast succeeds.
//   boundary_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 48)-th finite point of each cloud, so a subset of it; the source's get one
// more point far away from the cloud (no neighbour).  Writes, for tests/test_boundary_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_flags.u8 / tgt_flags.u8 (K), dense.i32 (is_dense of
//   the two flag clouds), casts.i32 (whether the wrapper's cast found normals to compute),
//   setters.f32 (getAngleThreshold of a default object, then after setAngleThreshold),
//   src_flags_wide.u8 (the source's rows at an angle threshold of 2.5), checks.i32: the rows of a
//   compute() with a k-search, without normals, with more input points than normals and with a
//   threshold below pi / 64 (0 each: PCL_ERROR and an empty output), then of a valid compute() on the
//   same object.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointCloud<pcl::PointXYZRGB> Cloud;
typedef pcl::PointCloud<pcl::Boundary> Flags;
typedef pcl::BoundaryEstimation<pcl::PointXYZRGB, pcl::Normal, pcl::Boundary> Estimator;

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

// Features<FeatureType> of the reference, as far as compute: the estimator arrives as its Feature
// base; whether it wants normals is found by a cast, and only then are the cloud's normals estimated
// (at their own radius, one per point of the cloud, not per keypoint).
template <typename DescT>
struct Features {
  typedef typename pcl::Feature<pcl::PointXYZRGB, DescT>::Ptr EstimatorPtr;
  typedef typename pcl::PointCloud<DescT>::Ptr DescPtr;
  EstimatorPtr estimator;
  double radius, normal_radius;
  bool cast_found_normals = false;

  Features(const EstimatorPtr& e, double r, double nr) : estimator(e), radius(r), normal_radius(nr) {}

  void compute(const Cloud::Ptr& cloud, const Cloud::Ptr& keypoints, DescPtr& rows) {
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

static std::vector<uint8_t> bytes(const Flags& c) {
  std::vector<uint8_t> v;
  for (const pcl::Boundary& p : c.points) v.push_back(p.boundary_point);
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
  const Cloud::Ptr source_kp = every_nth(*source, 48, true), target_kp = every_nth(*target, 48, false);
  save_xyz(out + "/src_kp_xyz.f32", *source_kp);
  save_xyz(out + "/tgt_kp_xyz.f32", *target_kp);
  std::vector<int32_t> dense, casts, checks;

  {  // the DESC_BOUNDARY branch, as far as its compute calls
    Estimator::Ptr feature_extractor_orig(new Estimator);
    pcl::Feature<pcl::PointXYZRGB, pcl::Boundary>::Ptr feature_extractor(feature_extractor_orig);
    Flags::Ptr source_features(new Flags), target_features(new Flags);
    Features<pcl::Boundary> feat(feature_extractor, 0.08, 0.05);
    feat.compute(source, source_kp, source_features);
    casts.push_back(feat.cast_found_normals);
    feat.compute(target, target_kp, target_features);
    if (source_features->size() != source_kp->size() || target_features->size() != target_kp->size()) {
      std::fprintf(stderr, "BoundaryEstimation::compute failed\n");
      return 1;
    }
    save(out + "/src_flags.u8", bytes(*source_features));
    save(out + "/tgt_flags.u8", bytes(*target_features));
    dense.push_back(source_features->is_dense);
    dense.push_back(target_features->is_dense);
  }
  {  // the setter round-trips
    std::vector<float> v;
    Estimator b;
    v.push_back(b.getAngleThreshold());
    b.setAngleThreshold(2.5f);
    v.push_back(b.getAngleThreshold());
    save(out + "/setters.f32", v);
  }
  {  // what is not on the accelerated path, or not PCL's use of the class, fails loudly
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
    pcl::NormalEstimationOMP<pcl::PointXYZRGB, pcl::Normal> ne;
    ne.setInputCloud(source);
    ne.setRadiusSearch(0.05);
    ne.compute(*normals);
    Flags rows;
    Estimator b;
    b.setSearchSurface(source);
    b.setInputCloud(source_kp);
    b.setInputNormals(normals);
    b.setRadiusSearch(0.08);
    b.setKSearch(10);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    b.setKSearch(0);
    b.setInputNormals(pcl::PointCloud<pcl::Normal>::Ptr());
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    b.setInputNormals(normals);
    b.setSearchSurface(source_kp);  // 49 surface points and normals for ...
    pcl::PointCloud<pcl::Normal>::Ptr few(new pcl::PointCloud<pcl::Normal>);
    for (size_t i = 0; i < source_kp->size(); ++i) few->push_back(normals->points[i]);
    b.setInputNormals(few);
    b.setInputCloud(source);        // ... every point of the cloud as input
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    b.setSearchSurface(source);
    b.setInputCloud(source_kp);
    b.setInputNormals(normals);
    b.setAngleThreshold(0.01f);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    // ... and the object works afterwards
    b.setAngleThreshold(2.5f);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    save(out + "/src_flags_wide.u8", bytes(rows));
  }
  save(out + "/dense.i32", dense);
  save(out + "/casts.i32", casts);
  save(out + "/checks.i32", checks);
  return 0;
}
