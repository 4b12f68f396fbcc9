// intensity_spin_facade_driver.cpp -- the calls of the reference's DESC_INT_SPIN branch
// (src/evaluation.cpp:466-514), with their types and in their order, made against
// include/pfx_pcl.hpp, then Features<T>::findCorrespondences (features.h:224-273) on
// PointCloud<Histogram<20>>.
//   intensity_spin_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 24)-th finite point of each cloud.  Writes, for
// tests/test_intensity_spin_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_ispin.f32 / tgt_ispin.f32 (K x 20),
//   corr_ispin.i32 (index_query, index_match pairs), dense.i32 (is_dense of the two feature clouds),
//   checks.i32: the rows of a compute() with an input index beyond the surface and of one with
//   nr_distance_bins * nr_intensity_bins != 20 (0 each: PCL_ERROR and an empty output), then the rows
//   of a valid compute() on the same object, and the three defaults (4, 5, sigma == 1).
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

using namespace pcl;
typedef PointXYZRGB PointRGB;
typedef PointCloud<PointRGB> PointCloudRGB;

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
  c.is_dense = true;
  for (size_t i = 0; i < n; ++i) {
    c.points[i].x = raw[4 * i]; c.points[i].y = raw[4 * i + 1]; c.points[i].z = raw[4 * i + 2];
    c.points[i].rgb = raw[4 * i + 3];
    if (!std::isfinite(raw[4 * i]) || !std::isfinite(raw[4 * i + 1]) || !std::isfinite(raw[4 * i + 2])) c.is_dense = false;
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

// features.h: the members of Features<FeatureType> the branch calls
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

static PointCloudRGB::Ptr sparse_keypoints(const PointCloudRGB& cloud) {
  PointCloudRGB::Ptr kp(new PointCloudRGB);
  const size_t step = cloud.size() / 24 ? cloud.size() / 24 : 1;
  for (size_t i = 0; i < cloud.size() && kp->size() < 24; i += step)
    if (std::isfinite(cloud.points[i].x) && std::isfinite(cloud.points[i].y) && std::isfinite(cloud.points[i].z))
      kp->push_back(cloud.points[i]);
  return kp;
}

static void dump_xyz(const std::string& path, const PointCloudRGB& kp) {
  std::vector<float> v;
  for (const PointRGB& p : kp.points) {
    v.push_back(p.x);
    v.push_back(p.y);
    v.push_back(p.z);
  }
  dump(path, v.data(), v.size());
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
  PointCloudRGB::Ptr source_keypoints = sparse_keypoints(*source_cloud_);
  PointCloudRGB::Ptr target_keypoints = sparse_keypoints(*target_cloud_);
  const double feat_radius_search_ = 0.08;
  static_assert(sizeof(pcl::Histogram<20>) == 20 * sizeof(float), "Histogram<20> is 20 floats");
  dump_xyz(out + "/src_kp_xyz.f32", *source_keypoints);
  dump_xyz(out + "/tgt_kp_xyz.f32", *target_keypoints);

  // ---- the calls of evaluation.cpp:470-512 (DESC_INT_SPIN): the intensities of the clouds and of the
  // keypoints, one estimator and one tree object for both clouds, no normals ----
  PointCloud<PointXYZI>::Ptr source_intensities(new PointCloud<PointXYZI>);
  PointCloud<PointXYZI>::Ptr target_intensities(new PointCloud<PointXYZI>);
  PointCloud<PointXYZI>::Ptr source_keypoints_intensities(new PointCloud<PointXYZI>);
  PointCloud<PointXYZI>::Ptr target_keypoints_intensities(new PointCloud<PointXYZI>);
  PointCloud<Histogram<20> >::Ptr source_features(new PointCloud<Histogram<20> >);
  PointCloud<Histogram<20> >::Ptr target_features(new PointCloud<Histogram<20> >);
  PointCloudXYZRGBtoXYZI(*source_cloud_, *source_intensities);
  PointCloudXYZRGBtoXYZI(*target_cloud_, *target_intensities);
  PointCloudXYZRGBtoXYZI(*source_keypoints, *source_keypoints_intensities);
  PointCloudXYZRGBtoXYZI(*target_keypoints, *target_keypoints_intensities);

  IntensitySpinEstimation<PointXYZI, Histogram<20> > feature_extractor;
  const int32_t defaults[3] = {feature_extractor.getNrDistanceBins(), feature_extractor.getNrIntensityBins(),
                               feature_extractor.getSmoothingBandwidth() == 1.0f};

  feature_extractor.setSearchSurface(source_intensities);
  feature_extractor.setInputCloud(source_keypoints_intensities);
  search::KdTree<PointXYZI>::Ptr kdtree(new search::KdTree<PointXYZI>);
  feature_extractor.setSearchMethod(kdtree);
  feature_extractor.setRadiusSearch(feat_radius_search_);
  feature_extractor.compute(*source_features);

  feature_extractor.setSearchSurface(target_intensities);
  feature_extractor.setInputCloud(target_keypoints_intensities);
  feature_extractor.setSearchMethod(kdtree);
  feature_extractor.setRadiusSearch(feat_radius_search_);
  feature_extractor.compute(*target_features);

  CorrespondencesPtr correspondences(new Correspondences);
  Features<Histogram<20> > feat;
  feat.findCorrespondences(source_features, target_features, correspondences);

  if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size()) {
    std::fprintf(stderr, "IntensitySpinEstimation::compute failed\n");
    return 1;
  }
  dump(out + "/src_ispin.f32", reinterpret_cast<const float*>(source_features->points.data()), source_features->size() * 20);
  dump(out + "/tgt_ispin.f32", reinterpret_cast<const float*>(target_features->points.data()), target_features->size() * 20);
  std::vector<int32_t> pairs;
  for (const Correspondence& c : *correspondences) {
    pairs.push_back(c.index_query);
    pairs.push_back(c.index_match);
  }
  dump(out + "/corr_ispin.i32", pairs.data(), pairs.size());
  const int32_t dense[2] = {source_features->is_dense, target_features->is_dense};
  dump(out + "/dense.i32", dense, 2);
  std::printf("int_spin: source rows %zu target rows %zu correspondences %zu\n", source_features->size(),
              target_features->size(), correspondences->size());

  // ---- what PCL 1.7 would read or write out of bounds is never silent ----
  int32_t checks[6] = {-1, -1, -1, defaults[0], defaults[1], defaults[2]};
  {
    PointCloud<Histogram<20> > refused;
    IntensitySpinEstimation<PointXYZI, Histogram<20> > e;
    e.setRadiusSearch(feat_radius_search_);
    // an input index beyond the surface: the cloud as the input, the keypoints as the surface
    e.setInputCloud(source_intensities);
    e.setSearchSurface(source_keypoints_intensities);
    e.compute(refused);
    checks[0] = (int32_t)refused.size();
    // 4 x 4 bins into Histogram<20>
    e.setInputCloud(source_keypoints_intensities);
    e.setSearchSurface(source_intensities);
    e.setNrIntensityBins(4);
    e.compute(refused);
    checks[1] = (int32_t)refused.size();
    e.setNrIntensityBins(5);  // ... and the object works afterwards
    e.compute(refused);
    checks[2] = (int32_t)refused.size();
  }
  dump(out + "/checks.i32", checks, 6);
  return 0;
}
