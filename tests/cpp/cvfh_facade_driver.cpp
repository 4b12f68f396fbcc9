// cvfh_facade_driver.cpp -- what the reference's DESC_CVFH branch (src/evaluation.cpp:649-675) asks of
// PCL, asked of include/pfx_pcl.hpp: a CVFHEstimation with setRadiusSearch(0.08) and setKSearch(0),
// held as Feature<PointXYZRGB, VFHSignature308>::Ptr, goes through the generic wrapper
// (features.h:175-196) for the source and then, the same object, for the target; the wrapper's cast to
// FeatureFromNormals succeeds, so it estimates the cloud's normals.  Then the rows are matched both
// ways with KdTreeFLANN<VFHSignature308> and the mutual pairs kept (features.h:224-273).
//   cvfh_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 1500)-th finite point of each cloud (K = 1,500: CVFH describes the first K
// points of the cloud whatever the keypoints are; only their number matters).  Writes, for
// tests/test_cvfh_facade.py:
//   src_rows.f32 / tgt_rows.f32 (rows x 308), src_about.f32 / tgt_about.f32 (rows x 6: centroid, dominant
//   normal, from the getters after each compute), counts.i32 (K of the source, K of the target, the
//   clouds' width and height), corr.i32 (index_query, index_match pairs), casts.i32, checks.i32: the rows
//   of a compute() on a fresh object with only the radius set (0: PCL_ERROR, as initCompute), after
//   setKSearch(0) (the source's rows), with more keypoints than surface points (0), and again valid.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointCloud<pcl::PointXYZRGB> Cloud;
typedef pcl::PointCloud<pcl::VFHSignature308> Rows;
typedef pcl::CVFHEstimation<pcl::PointXYZRGB, pcl::Normal, pcl::VFHSignature308> Estimator;

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

static Cloud::Ptr every_nth(const Cloud& cloud, size_t want) {
  Cloud::Ptr kp(new Cloud);
  const size_t step = cloud.size() / want ? cloud.size() / want : 1;
  for (size_t i = 0; i < cloud.size() && kp->size() < want; i += step) {
    const pcl::PointXYZRGB& p = cloud.points[i];
    if (std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z)) kp->push_back(p);
  }
  return kp;
}

// The reference's generic wrapper as far as this branch uses it: the estimator arrives as its Feature
// base; a cast tells whether it wants normals, and then the cloud's are estimated, one per point of
// the cloud; the cloud is the search surface and the keypoints the input.
struct Wrapper {
  typedef pcl::Feature<pcl::PointXYZRGB, pcl::VFHSignature308> Base;
  Base::Ptr estimator;
  double radius, normal_radius;
  bool cast_found_normals = false;

  void compute(const Cloud::Ptr& cloud, const Cloud::Ptr& keypoints, Rows::Ptr& rows) {
    typedef pcl::FeatureFromNormals<pcl::PointXYZRGB, pcl::Normal, pcl::VFHSignature308> WithNormals;
    WithNormals::Ptr wants_normals = boost::dynamic_pointer_cast<WithNormals>(estimator);
    cast_found_normals = (bool)wants_normals;
    if (wants_normals) {
      pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
      pcl::NormalEstimationOMP<pcl::PointXYZRGB, pcl::Normal> ne;
      ne.setInputCloud(cloud);
      ne.setRadiusSearch(normal_radius);
      ne.setSearchMethod(pcl::search::KdTree<pcl::PointXYZRGB>::Ptr(new pcl::search::KdTree<pcl::PointXYZRGB>));
      ne.compute(*normals);
      wants_normals->setInputNormals(normals);
    }
    estimator->setSearchSurface(cloud);
    estimator->setInputCloud(keypoints);
    estimator->setSearchMethod(pcl::search::KdTree<pcl::PointXYZRGB>::Ptr(new pcl::search::KdTree<pcl::PointXYZRGB>));
    estimator->setRadiusSearch(radius);
    estimator->compute(*rows);
  }

  // row i of `from` to its nearest row of `to`
  static std::vector<int> nearest(const Rows::Ptr& from, const Rows::Ptr& to) {
    std::vector<int> idx(1), out(from->size());
    std::vector<float> dist(1);
    pcl::KdTreeFLANN<pcl::VFHSignature308> tree;
    tree.setInputCloud(to);
    for (size_t i = 0; i < from->size(); ++i) {
      tree.nearestKSearch(*from, (int)i, 1, idx, dist);
      out[i] = idx[0];
    }
    return out;
  }
  // the pairs that choose each other
  static std::vector<int32_t> mutual(const Rows::Ptr& source, const Rows::Ptr& target) {
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

static std::vector<float> floats(const Rows& rows) {
  std::vector<float> v;
  for (const pcl::VFHSignature308& r : rows.points) v.insert(v.end(), r.histogram, r.histogram + 308);
  return v;
}

static std::vector<float> about(const Estimator& e) {
  std::vector<Eigen::Vector3f> c, n;
  e.getCentroidClusters(c);
  e.getCentroidNormalClusters(n);
  std::vector<float> v;
  for (size_t i = 0; i < c.size() && i < n.size(); ++i) {
    for (int k = 0; k < 3; ++k) v.push_back(c[i][k]);
    for (int k = 0; k < 3; ++k) v.push_back(n[i][k]);
  }
  if (c.size() != n.size()) v.clear();
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
  const Cloud::Ptr source_kp = every_nth(*source, 1500), target_kp = every_nth(*target, 1500);
  std::vector<int32_t> counts, casts, checks;

  {  // the DESC_CVFH branch
    Estimator::Ptr feature_extractor_orig(new Estimator);
    feature_extractor_orig->setRadiusSearch(0.08);
    feature_extractor_orig->setKSearch(0);
    Wrapper::Base::Ptr feature_extractor(feature_extractor_orig);
    Rows::Ptr source_features(new Rows), target_features(new Rows);
    Wrapper feat{feature_extractor, 0.08, 0.05};
    feat.compute(source, source_kp, source_features);
    casts.push_back(feat.cast_found_normals);
    save(out + "/src_about.f32", about(*feature_extractor_orig));
    feat.compute(target, target_kp, target_features);  // the same object again
    save(out + "/tgt_about.f32", about(*feature_extractor_orig));
    if (source_features->empty() || target_features->empty()) {
      std::fprintf(stderr, "CVFHEstimation::compute failed\n");
      return 1;
    }
    save(out + "/src_rows.f32", floats(*source_features));
    save(out + "/tgt_rows.f32", floats(*target_features));
    counts.push_back((int32_t)source_kp->size());
    counts.push_back((int32_t)target_kp->size());
    counts.push_back((int32_t)source_features->width);
    counts.push_back((int32_t)source_features->height);
    counts.push_back((int32_t)target_features->width);
    counts.push_back((int32_t)target_features->height);
    save(out + "/corr.i32", Wrapper::mutual(source_features, target_features));
  }
  {  // the k-search rule, and more keypoints than surface points
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
    pcl::NormalEstimationOMP<pcl::PointXYZRGB, pcl::Normal> ne;
    ne.setInputCloud(source);
    ne.setRadiusSearch(0.05);
    ne.compute(*normals);
    Rows rows;
    Estimator e;  // k = 1 from the constructor
    e.setSearchSurface(source);
    e.setInputCloud(source_kp);
    e.setInputNormals(normals);
    e.setRadiusSearch(0.08);
    e.compute(rows);
    checks.push_back((int32_t)rows.size());
    e.setKSearch(0);
    e.compute(rows);
    checks.push_back((int32_t)rows.size());
    pcl::PointCloud<pcl::Normal>::Ptr few(new pcl::PointCloud<pcl::Normal>);
    Cloud::Ptr few_points(new Cloud);
    for (size_t i = 0; i < 100; ++i) {
      few->push_back(normals->points[i]);
      few_points->push_back(source->points[i]);
    }
    e.setSearchSurface(few_points);  // 100 surface points and normals, 1,500 keypoints
    e.setInputNormals(few);
    e.compute(rows);
    checks.push_back((int32_t)rows.size());
    e.setSearchSurface(source);
    e.setInputNormals(normals);
    e.compute(rows);
    checks.push_back((int32_t)rows.size());
  }
  save(out + "/counts.i32", counts);
  save(out + "/casts.i32", casts);
  save(out + "/checks.i32", checks);
  return 0;
}
