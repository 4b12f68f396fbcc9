// shot_color_facade_driver.cpp -- the reference's DESC_SHOT_COLOR branch (src/evaluation.cpp:786-805)
// written against include/pfx_pcl.hpp: SHOTColorEstimationOMP behind Feature<...>::Ptr, driven by
// Features<T>::compute (features.h:175-196, normals through tools.h:22-32) and
// Features<T>::findCorrespondences (features.h:224-273) on PointCloud<SHOT1344>.
//   shot_color_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 64)-th point of each cloud; the source's get one more point far away from
// the cloud (an empty neighbourhood: a NaN row, is_dense = false), coloured 0x00102030.  Writes, for
// tests/test_shot_color_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_kp_rgb.u32 / tgt_kp_rgb.u32 (K), src_shot.f32 /
//   tgt_shot.f32 (K x 1353: descriptor + rf), corr.i32 (index_query, index_match pairs), dense.i32
//   (is_dense of the source and the target rows)
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

// features.h: the members of Features<FeatureType> the DESC_SHOT_COLOR branch calls
template <typename FeatureType>
struct Features {
  typename Feature<PointRGB, FeatureType>::Ptr feature_extractor_;
  double feat_radius_search_, normal_radius_search_;
  Features(typename Feature<PointRGB, FeatureType>::Ptr feature_extractor, double feat_radius_search,
           double normal_radius_search)
      : feature_extractor_(feature_extractor), feat_radius_search_(feat_radius_search),
        normal_radius_search_(normal_radius_search) {}

  // features.h:175-196
  void compute(const PointCloudRGB::Ptr cloud, const PointCloudRGB::Ptr keypoints,
               typename PointCloud<FeatureType>::Ptr& descriptors) {
    typename FeatureFromNormals<PointRGB, Normal, FeatureType>::Ptr feature_from_normals =
        boost::dynamic_pointer_cast<FeatureFromNormals<PointRGB, Normal, FeatureType> >(feature_extractor_);
    if (feature_from_normals) {
      PointCloud<Normal>::Ptr normals(new PointCloud<Normal>);
      estimateNormals(cloud, normals, normal_radius_search_);
      feature_from_normals->setInputNormals(normals);
    }
    feature_extractor_->setSearchSurface(cloud);
    feature_extractor_->setInputCloud(keypoints);
    search::KdTree<PointRGB>::Ptr kdtree(new search::KdTree<PointRGB>);
    feature_extractor_->setSearchMethod(kdtree);
    feature_extractor_->setRadiusSearch(feat_radius_search_);
    feature_extractor_->compute(*descriptors);
  }

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

static PointCloudRGB::Ptr strided_keypoints(const PointCloudRGB& cloud, bool with_far_point) {
  PointCloudRGB::Ptr kp(new PointCloudRGB);
  const size_t step = cloud.size() / 64 ? cloud.size() / 64 : 1;
  for (size_t i = 0; i < cloud.size() && kp->size() < 64; i += step)
    if (std::isfinite(cloud.points[i].x) && std::isfinite(cloud.points[i].y) && std::isfinite(cloud.points[i].z))
      kp->push_back(cloud.points[i]);
  if (with_far_point) {
    PointRGB far;
    far.x = far.y = far.z = 9.0e3f;
    far.rgba = 0x00102030u;
    kp->push_back(far);
  }
  return kp;
}

static void dump_cloud(const std::string& out, const char* tag, const PointCloudRGB& kp,
                       const PointCloud<SHOT1344>& desc) {
  static_assert(sizeof(SHOT1344) == 1353 * sizeof(float), "descriptor + rf, no padding");
  std::vector<float> v;
  std::vector<uint32_t> c;
  for (const PointRGB& p : kp.points) {
    v.push_back(p.x);
    v.push_back(p.y);
    v.push_back(p.z);
    c.push_back(p.rgba);
  }
  dump(out + "/" + tag + "_kp_xyz.f32", v.data(), v.size());
  dump(out + "/" + tag + "_kp_rgb.u32", c.data(), c.size());
  dump(out + "/" + tag + "_shot.f32", reinterpret_cast<const float*>(desc.points.data()), desc.size() * 1353);
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
  PointCloudRGB::Ptr source_keypoints = strided_keypoints(*source_cloud_, true);
  PointCloudRGB::Ptr target_keypoints = strided_keypoints(*target_cloud_, false);
  const double feat_radius_search_ = 0.08, normal_radius_search_ = 0.05;

  // ---- evaluation.cpp:786-805 ----
  Feature<PointXYZRGB, SHOT1344>::Ptr feature_extractor(new SHOTColorEstimationOMP<PointXYZRGB, Normal, SHOT1344>);
  PointCloud<SHOT1344>::Ptr source_features(new PointCloud<SHOT1344>);
  PointCloud<SHOT1344>::Ptr target_features(new PointCloud<SHOT1344>);
  Features<SHOT1344> feat(feature_extractor, feat_radius_search_, normal_radius_search_);
  feat.compute(source_cloud_, source_keypoints, source_features);
  feat.compute(target_cloud_, target_keypoints, target_features);
  CorrespondencesPtr correspondences(new Correspondences);
  feat.findCorrespondences(source_features, target_features, correspondences);

  if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size()) {
    std::fprintf(stderr, "SHOTColorEstimationOMP::compute failed\n");
    return 1;
  }
  dump_cloud(out, "src", *source_keypoints, *source_features);
  dump_cloud(out, "tgt", *target_keypoints, *target_features);
  std::vector<int32_t> pairs;
  for (const Correspondence& c : *correspondences) {
    pairs.push_back(c.index_query);
    pairs.push_back(c.index_match);
  }
  dump(out + "/corr.i32", pairs.data(), pairs.size());
  const int32_t dense[2] = {source_features->is_dense ? 1 : 0, target_features->is_dense ? 1 : 0};
  dump(out + "/dense.i32", dense, 2);
  std::printf("source rows %zu target rows %zu correspondences %zu\n", source_features->size(),
              target_features->size(), correspondences->size());
  return 0;
}
