// shape_context_facade_driver.cpp -- the calls of the reference's DESC_SHAPE_CONTEXT and DESC_USC
// branches (src/evaluation.cpp:319-345 and 346-371; the 3DSC through Features<T>::compute,
// features.h:175-196), with their types and in their order, made against include/pfx_pcl.hpp, then
// Features<T>::findCorrespondences (features.h:224-273) on PointCloud<ShapeContext1980>.
//   shape_context_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 48)-th finite point of each cloud; the source's get one more point far away
// from the cloud in the middle of the list (no neighbour: a NaN row that draws nothing).  Writes,
// for tests/test_shape_context_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3);
//   src_sc.f32 / tgt_sc.f32 (K x 1989: descriptor, then rf), ONE estimator object computing the
//   source and then the target, so the target continues the source's random stream;
//   src_usc.f32 / tgt_usc.f32 (K x 1989) with setLocalRadius(0.08); corr_sc.i32 (index_query,
//   index_match pairs); small_xyz.f32 (m x 3, every 64th source point) and small_usc.f32 (K x 1989):
//   USC with the default local radius 2.5 on that small surface; dense.i32 (is_dense of the five);
//   checks.i32: rows of a compute() with normals of another size, with the search radius below the
//   minimal radius (both estimators), and of USC at the default local radius on the whole source
//   cloud, beyond the frame search's capacity (0 each: PCL_ERROR and an empty output), then the
//   rows of a valid compute() on the same USC object.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

using namespace pcl;
typedef PointXYZRGB PointRGB;
typedef PointCloud<PointRGB> PointCloudRGB;
typedef PointCloud<ShapeContext1980> PointCloudSC;

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

// tools.h:22-32
static void estimateNormals(const PointCloudRGB::Ptr& cloud, PointCloud<Normal>::Ptr& normals, double radius) {
  NormalEstimationOMP<PointRGB, Normal> normal_estimation_omp;
  normal_estimation_omp.setInputCloud(cloud);
  normal_estimation_omp.setRadiusSearch(radius);
  search::KdTree<PointRGB>::Ptr kdtree_omp(new search::KdTree<PointRGB>);
  normal_estimation_omp.setSearchMethod(kdtree_omp);
  normal_estimation_omp.compute(*normals);
}

// features.h: the members of Features<FeatureType> the branches call
template <typename FeatureType>
struct Features {
  double feat_radius_search_ = 0.08, normal_radius_search_ = 0.05;
  typename Feature<PointRGB, FeatureType>::Ptr feature_extractor_;

  // features.h:175-196: an estimator that takes normals gets the cloud's
  void compute(const PointCloudRGB::Ptr& cloud, const PointCloudRGB::Ptr& keypoints,
               typename PointCloud<FeatureType>::Ptr& descriptors) {
    typename FeatureFromNormals<PointRGB, Normal, FeatureType>::Ptr feature_from_normals =
        std::dynamic_pointer_cast<FeatureFromNormals<PointRGB, Normal, FeatureType> >(feature_extractor_);
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

static PointCloudRGB::Ptr sparse_keypoints(const PointCloudRGB& cloud, bool with_far_point) {
  PointCloudRGB::Ptr kp(new PointCloudRGB);
  const size_t step = cloud.size() / 48 ? cloud.size() / 48 : 1;
  for (size_t i = 0; i < cloud.size() && kp->size() < 48 + (with_far_point ? 1 : 0); i += step) {
    if (with_far_point && kp->size() == 24) {
      PointRGB far;
      far.x = far.y = far.z = 9.0e3f;
      kp->push_back(far);
    }
    if (std::isfinite(cloud.points[i].x) && std::isfinite(cloud.points[i].y) && std::isfinite(cloud.points[i].z))
      kp->push_back(cloud.points[i]);
  }
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

static void dump_sc(const std::string& path, const PointCloudSC& c) {
  static_assert(sizeof(ShapeContext1980) == 1989 * sizeof(float), "ShapeContext1980 is 1980 + 9 floats");
  dump(path, reinterpret_cast<const float*>(c.points.data()), c.size() * 1989);
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
  dump_xyz(out + "/src_kp_xyz.f32", *source_keypoints);
  dump_xyz(out + "/tgt_kp_xyz.f32", *target_keypoints);
  int32_t dense[5] = {-1, -1, -1, -1, -1};
  int32_t checks[5] = {-1, -1, -1, -1, -1};

  {  // ---- DESC_SHAPE_CONTEXT: one estimator for both clouds, the radii from the feature radius ----
    PointCloudSC::Ptr source_features(new PointCloudSC), target_features(new PointCloudSC);
    Features<ShapeContext1980> feat;
    ShapeContext3DEstimation<PointRGB, Normal, ShapeContext1980>::Ptr shape_context(
        new ShapeContext3DEstimation<PointRGB, Normal, ShapeContext1980>());
    shape_context->setMinimalRadius(feat.feat_radius_search_ / 10.0);
    shape_context->setPointDensityRadius(feat.feat_radius_search_ / 5.0);
    feat.feature_extractor_ = shape_context;
    feat.compute(source_cloud_, source_keypoints, source_features);
    feat.compute(target_cloud_, target_keypoints, target_features);
    CorrespondencesPtr correspondences(new Correspondences);
    feat.findCorrespondences(source_features, target_features, correspondences);
    if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size()) {
      std::fprintf(stderr, "ShapeContext3DEstimation::compute failed\n");
      return 1;
    }
    dump_sc(out + "/src_sc.f32", *source_features);
    dump_sc(out + "/tgt_sc.f32", *target_features);
    std::vector<int32_t> pairs;
    for (const Correspondence& c : *correspondences) {
      pairs.push_back(c.index_query);
      pairs.push_back(c.index_match);
    }
    dump(out + "/corr_sc.i32", pairs.data(), pairs.size());
    dense[0] = source_features->is_dense;
    dense[1] = target_features->is_dense;
    std::printf("shape_context: source rows %zu target rows %zu correspondences %zu\n", source_features->size(),
                target_features->size(), correspondences->size());

    // normals of another size than the surface; a search radius below the minimal radius
    PointCloudSC refused;
    PointCloud<Normal>::Ptr few(new PointCloud<Normal>);
    few->resize(source_keypoints->size());
    ShapeContext3DEstimation<PointRGB, Normal, ShapeContext1980> e;
    e.setMinimalRadius(0.008);
    e.setPointDensityRadius(0.016);
    e.setInputCloud(source_keypoints);
    e.setSearchSurface(source_cloud_);
    e.setInputNormals(few);
    e.setRadiusSearch(0.08);
    e.compute(refused);
    checks[0] = (int32_t)refused.size();
    ShapeContext3DEstimation<PointRGB, Normal, ShapeContext1980> d;  // PCL's defaults: 0.1 and 0.2
    d.setInputCloud(source_keypoints);
    d.setSearchSurface(source_cloud_);
    d.setInputNormals(few);
    d.setRadiusSearch(0.08);
    d.compute(refused);
    checks[1] = (int32_t)refused.size() + (d.getMinimalRadius() == 0.1 && d.getPointDensityRadius() == 0.2 ? 0 : 100);
  }

  {  // ---- DESC_USC: no normals; the frames are the estimator's own ----
    PointCloudSC::Ptr source_features(new PointCloudSC), target_features(new PointCloudSC);
    Features<ShapeContext1980> feat;
    UniqueShapeContext<PointRGB, ShapeContext1980>::Ptr usc(new UniqueShapeContext<PointRGB, ShapeContext1980>());
    usc->setMinimalRadius(feat.feat_radius_search_ / 10.0);
    usc->setPointDensityRadius(feat.feat_radius_search_ / 5.0);
    feat.feature_extractor_ = usc;
    // the default local radius (2.5) on the whole cloud: beyond the frame search's capacity
    PointCloudSC::Ptr refused(new PointCloudSC);
    feat.compute(source_cloud_, source_keypoints, refused);
    checks[2] = (int32_t)refused->size() + (usc->getLocalRadius() == 2.5 ? 0 : 100);
    usc->setMinimalRadius(1.0);  // above the search radius
    feat.compute(source_cloud_, source_keypoints, refused);
    checks[3] = (int32_t)refused->size();
    usc->setMinimalRadius(feat.feat_radius_search_ / 10.0);
    // ... and the object works afterwards, with a local radius the capacity holds
    usc->setLocalRadius(feat.feat_radius_search_);
    feat.compute(source_cloud_, source_keypoints, source_features);
    feat.compute(target_cloud_, target_keypoints, target_features);
    checks[4] = (int32_t)source_features->size();
    if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size()) {
      std::fprintf(stderr, "UniqueShapeContext::compute failed\n");
      return 1;
    }
    dump_sc(out + "/src_usc.f32", *source_features);
    dump_sc(out + "/tgt_usc.f32", *target_features);
    dense[2] = source_features->is_dense;
    dense[3] = target_features->is_dense;

    // the default local radius on a small surface: every 64th point of the source
    PointCloudRGB::Ptr small(new PointCloudRGB);
    for (size_t i = 0; i < source_cloud_->size(); i += 64) small->push_back(source_cloud_->points[i]);
    dump_xyz(out + "/small_xyz.f32", *small);
    PointCloudSC::Ptr small_features(new PointCloudSC);
    Features<ShapeContext1980> feat_small;
    UniqueShapeContext<PointRGB, ShapeContext1980>::Ptr usc_default(new UniqueShapeContext<PointRGB, ShapeContext1980>());
    usc_default->setMinimalRadius(feat.feat_radius_search_ / 10.0);
    usc_default->setPointDensityRadius(feat.feat_radius_search_ / 5.0);
    feat_small.feature_extractor_ = usc_default;
    feat_small.compute(small, source_keypoints, small_features);
    if (small_features->size() != source_keypoints->size()) {
      std::fprintf(stderr, "UniqueShapeContext::compute at the default local radius failed\n");
      return 1;
    }
    dump_sc(out + "/small_usc.f32", *small_features);
    dense[4] = small_features->is_dense;
    std::printf("usc: source rows %zu target rows %zu small rows %zu\n", source_features->size(),
                target_features->size(), small_features->size());
  }
  dump(out + "/dense.i32", dense, 5);
  dump(out + "/checks.i32", checks, 5);
  return 0;
}
