// spin_facade_driver.cpp -- the reference's DESC_SPIN_IMAGE branch (src/evaluation.cpp:518-552)
// written against include/pfx_pcl.hpp: SpinImageEstimation<PointXYZRGB, Normal, Histogram<153>> on
// the normals of the *keypoint cloud among itself* (tools.h:22-32 at the normal radius: sparse
// keypoints, so most of these normals are NaN), then Features<T>::findCorrespondences
// (features.h:224-273) on PointCloud<Histogram<153>>.
//   spin_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 48)-th point of each cloud, four of them with four more points 1 cm around
// them (a cluster dense enough for a normal); the source's get one more point far away from the
// cloud (an empty neighbourhood: a zero row).  Writes, for tests/test_spin_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_kp_normals.f32 / tgt_kp_normals.f32 (K x 3),
//   src_spin.f32 / tgt_spin.f32 (K x 153), corr.i32 (index_query, index_match pairs), checks.i32:
//   rows of a compute() with the radial structure, the angular domain, a custom axis, normals
//   that do not match the input, a width that does not match Histogram<153> (0 each: PCL_ERROR and
//   an empty output), and whether setMinPointCountInNeighbourhood(1) threw pcl::PCLException on
//   the source (its far keypoint has no neighbour).
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

using namespace pcl;
typedef PointXYZRGB PointRGB;
typedef PointCloud<PointRGB> PointCloudRGB;
typedef Histogram<153> SpinImage;

static bool read_pcd(const char* path, PointCloudRGB& c) {
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
  c.points.resize(n);
  for (size_t i = 0; i < n; ++i) {
    c.points[i].x = raw[4 * i]; c.points[i].y = raw[4 * i + 1]; c.points[i].z = raw[4 * i + 2];
    c.points[i].rgb = raw[4 * i + 3];
  }
  c.width = (uint32_t)n;
  c.height = 1;
  return true;
}

template <typename T>
static void dump(const std::string& path, const T* p, size_t count) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (f) { std::fwrite(p, sizeof(T), count, f); std::fclose(f); }
}

// tools.h:22-32
static void estimateNormals(const PointCloudRGB::Ptr& cloud, PointCloud<Normal>::Ptr& normals, double radius) {
  NormalEstimationOMP<PointRGB, Normal> normal_estimation_omp;
  normal_estimation_omp.setInputCloud(cloud);
  normal_estimation_omp.setRadiusSearch(radius);
  search::KdTree<PointRGB>::Ptr kdtree_omp(new search::KdTree<PointRGB>);
  normal_estimation_omp.setSearchMethod(kdtree_omp);
  normal_estimation_omp.compute(*normals);
}

// features.h: the members of Features<FeatureType> the DESC_SPIN_IMAGE branch calls
template <typename FeatureType>
struct Features {
  // features.h:224-253
  void findCorrespondences(typename PointCloud<FeatureType>::Ptr source, typename PointCloud<FeatureType>::Ptr target,
                           CorrespondencesPtr& correspondences) {
    std::vector<int> source2target;
    std::vector<int> target2source;
    boost::thread thread1(&Features::getCorrespondences, this, boost::ref(source), boost::ref(target),
                          boost::ref(source2target));
    boost::thread thread2(&Features::getCorrespondences, this, boost::ref(target), boost::ref(source),
                          boost::ref(target2source));
    thread1.join();
    thread2.join();
    std::vector<std::pair<unsigned, unsigned> > c;
    for (unsigned c_idx = 0; c_idx < source2target.size(); ++c_idx)
      if (target2source[source2target[c_idx]] == (int)c_idx) c.push_back(std::make_pair(c_idx, source2target[c_idx]));
    correspondences->resize(c.size());
    for (unsigned c_idx = 0; c_idx < c.size(); ++c_idx) {
      (*correspondences)[c_idx].index_query = c[c_idx].first;
      (*correspondences)[c_idx].index_match = c[c_idx].second;
    }
  }

  // features.h:255-273
  void getCorrespondences(typename PointCloud<FeatureType>::Ptr source, typename PointCloud<FeatureType>::Ptr target,
                          std::vector<int>& source2target) {
    const int k = 1;
    std::vector<int> k_indices(k);
    std::vector<float> k_dist(k);
    source2target.clear();
    KdTreeFLANN<FeatureType> descriptor_kdtree;
    descriptor_kdtree.setInputCloud(target);
    source2target.resize(source->size());
    for (size_t i = 0; i < source->size(); ++i) {
      descriptor_kdtree.nearestKSearch(*source, i, k, k_indices, k_dist);
      source2target[i] = k_indices[0];
    }
  }
};

static PointCloudRGB::Ptr sparse_keypoints(const PointCloudRGB& cloud, bool with_far_point) {
  PointCloudRGB::Ptr kp(new PointCloudRGB);
  const size_t step = cloud.size() / 48 ? cloud.size() / 48 : 1;
  for (size_t i = 0; i < cloud.size() && kp->size() < 48; i += step)
    if (std::isfinite(cloud.points[i].x) && std::isfinite(cloud.points[i].y) && std::isfinite(cloud.points[i].z))
      kp->push_back(cloud.points[i]);
  const float off[4][3] = {{0.01f, 0.f, 0.002f}, {0.f, 0.01f, -0.002f}, {-0.01f, 0.003f, 0.f}, {0.002f, -0.01f, 0.001f}};
  const size_t base = kp->size();
  for (size_t c = 0; c < 4 && c * 11 < base; ++c)
    for (int j = 0; j < 4; ++j) {
      PointRGB p = kp->points[c * 11];
      p.x += off[j][0]; p.y += off[j][1]; p.z += off[j][2];
      kp->push_back(p);
    }
  if (with_far_point) {
    PointRGB far;
    far.x = far.y = far.z = 9.0e3f;
    kp->push_back(far);
  }
  return kp;
}

static void dump_cloud(const std::string& out, const char* tag, const PointCloudRGB& kp, const PointCloud<Normal>& nrm,
                       const PointCloud<SpinImage>& desc) {
  std::vector<float> v, n;
  for (const PointRGB& p : kp.points) {
    v.push_back(p.x);
    v.push_back(p.y);
    v.push_back(p.z);
  }
  for (const Normal& p : nrm.points) {
    n.push_back(p.normal_x);
    n.push_back(p.normal_y);
    n.push_back(p.normal_z);
  }
  dump(out + "/" + tag + "_kp_xyz.f32", v.data(), v.size());
  dump(out + "/" + tag + "_kp_normals.f32", n.data(), n.size());
  dump(out + "/" + tag + "_spin.f32", reinterpret_cast<const float*>(desc.points.data()), desc.size() * 153);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s source.pcd target.pcd out_dir\n", argv[0]);
    return 2;
  }
  PointCloudRGB::Ptr source_cloud_(new PointCloudRGB), target_cloud_(new PointCloudRGB);
  if (!read_pcd(argv[1], *source_cloud_) || !read_pcd(argv[2], *target_cloud_)) {
    std::fprintf(stderr, "cannot read the clouds\n");
    return 2;
  }
  const std::string out = argv[3];
  PointCloudRGB::Ptr source_keypoints = sparse_keypoints(*source_cloud_, true);
  PointCloudRGB::Ptr target_keypoints = sparse_keypoints(*target_cloud_, false);
  const double feat_radius_search_ = 0.08, normal_radius_search_ = 0.05;
  static_assert(sizeof(SpinImage) == 153 * sizeof(float), "Histogram<153> is 153 floats");
  if (SpinImage::descriptorSize() != 153) return 1;

  // ---- evaluation.cpp:518-552 ----
  PointCloud<SpinImage>::Ptr source_features(new PointCloud<SpinImage>);
  PointCloud<SpinImage>::Ptr target_features(new PointCloud<SpinImage>);
  PointCloud<Normal>::Ptr source_normals(new PointCloud<Normal>);
  PointCloud<Normal>::Ptr target_normals(new PointCloud<Normal>);
  estimateNormals(source_keypoints, source_normals, normal_radius_search_);
  estimateNormals(target_keypoints, target_normals, normal_radius_search_);

  SpinImageEstimation<PointXYZRGB, Normal, SpinImage> feature_extractor;

  feature_extractor.setInputNormals(source_normals);
  feature_extractor.setSearchSurface(source_cloud_);
  feature_extractor.setInputCloud(source_keypoints);
  search::KdTree<PointRGB>::Ptr kdtree(new search::KdTree<PointRGB>);
  feature_extractor.setSearchMethod(kdtree);
  feature_extractor.setRadiusSearch(feat_radius_search_);
  feature_extractor.compute(*source_features);

  feature_extractor.setInputNormals(target_normals);
  feature_extractor.setSearchSurface(target_cloud_);
  feature_extractor.setInputCloud(target_keypoints);
  feature_extractor.setSearchMethod(kdtree);
  feature_extractor.setRadiusSearch(feat_radius_search_);
  feature_extractor.compute(*target_features);

  CorrespondencesPtr correspondences(new Correspondences);
  Features<SpinImage> feat;
  feat.findCorrespondences(source_features, target_features, correspondences);

  if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size()) {
    std::fprintf(stderr, "SpinImageEstimation::compute failed\n");
    return 1;
  }
  dump_cloud(out, "src", *source_keypoints, *source_normals, *source_features);
  dump_cloud(out, "tgt", *target_keypoints, *target_normals, *target_features);
  std::vector<int32_t> pairs;
  for (const Correspondence& c : *correspondences) {
    pairs.push_back(c.index_query);
    pairs.push_back(c.index_match);
  }
  dump(out + "/corr.i32", pairs.data(), pairs.size());

  // ---- what the accelerated path refuses is never silent ----
  int32_t checks[6] = {-1, -1, -1, -1, -1, 0};
  PointCloud<SpinImage> refused;
  {
    SpinImageEstimation<PointXYZRGB, Normal, SpinImage> e;
    e.setInputNormals(source_normals);
    e.setSearchSurface(source_cloud_);
    e.setInputCloud(source_keypoints);
    e.setRadiusSearch(feat_radius_search_);
    e.setRadialStructure();
    e.compute(refused);
    checks[0] = (int32_t)refused.size();
    e.setRadialStructure(false);
    e.setAngularDomain();
    e.compute(refused);
    checks[1] = (int32_t)refused.size();
    e.setAngularDomain(false);
    e.setRotationAxis(Normal());
    e.compute(refused);
    checks[2] = (int32_t)refused.size();
    e.useNormalsAsRotationAxis();
    e.setInputNormals(target_normals);  // (another size than the source keypoints)
    e.compute(refused);
    checks[3] = target_normals->size() != source_normals->size() ? (int32_t)refused.size() : -1;
    e.setInputNormals(source_normals);
    e.setImageWidth(5);
    e.compute(refused);
    checks[4] = (int32_t)refused.size();
    e.setImageWidth(8);
    e.setMinPointCountInNeighbourhood(1);
    try {
      e.compute(refused);
    } catch (const PCLException& ex) {
      checks[5] = 1;
      std::fprintf(stderr, "(expected) %s\n", ex.what());
    }
    e.setMinPointCountInNeighbourhood(0);  // ... and the object works afterwards
    e.compute(refused);
    if (refused.size() != source_keypoints->size()) checks[5] = 0;
  }
  dump(out + "/checks.i32", checks, 6);
  std::printf("source rows %zu target rows %zu correspondences %zu\n", source_features->size(),
              target_features->size(), correspondences->size());
  return 0;
}
