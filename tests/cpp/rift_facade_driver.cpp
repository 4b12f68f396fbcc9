// rift_facade_driver.cpp -- the calls of the reference's DESC_INT_GRAD and DESC_RIFT branches
// (src/evaluation.cpp:419-462 and 720-762, with Tools::computeGradient, tools.h:40-54), with their
// types and in their order, made against include/pfx_pcl.hpp, then Features<T>::findCorrespondences
// (features.h:224-273) on PointCloud<IntensityGradient> and PointCloud<Histogram<32>>.
//   rift_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 48)-th finite point of each cloud; the source's get one more point far
// away from the cloud (an empty neighbourhood: a NaN gradient row).  Writes, for
// tests/test_rift_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_igrad.f32 / tgt_igrad.f32 (K x 3),
//   src_cloud_grad.f32 / tgt_cloud_grad.f32 (n x 3, Tools::computeGradient's output),
//   src_rift.f32 / tgt_rift.f32 (K x 32), corr_igrad.i32 / corr_rift.i32 (index_query, index_match
//   pairs), dense.i32 (is_dense of the four feature clouds and the two gradient clouds), checks.i32:
//   rows of a compute() with an input index beyond the surface (gradient, RIFT), a gradient cloud
//   of another size than the surface, and nr_distance_bins * nr_gradient_bins != 32 (0 each:
//   PCL_ERROR and an empty output), then the rows of a valid compute() on the same object.
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

// tools.h:22-32
static void estimateNormals(const PointCloudRGB::Ptr& cloud, PointCloud<Normal>::Ptr& normals, double radius) {
  NormalEstimationOMP<PointRGB, Normal> normal_estimation_omp;
  normal_estimation_omp.setInputCloud(cloud);
  normal_estimation_omp.setRadiusSearch(radius);
  search::KdTree<PointRGB>::Ptr kdtree_omp(new search::KdTree<PointRGB>);
  normal_estimation_omp.setSearchMethod(kdtree_omp);
  normal_estimation_omp.compute(*normals);
}

typedef IntensityGradientEstimation<PointXYZI, Normal, IntensityGradient, common::IntensityFieldAccessor<PointXYZI> >
    GradientEstimation;
typedef RIFTEstimation<PointXYZI, IntensityGradient, pcl::Histogram<32> > Rift;

// the calls of tools.h:40-54 (Tools::computeGradient): the whole cloud, no search surface, no tree
static void computeGradient(const PointCloud<PointXYZI>::Ptr& cloud, const PointCloud<Normal>::Ptr& normals,
                            PointCloud<IntensityGradient>::Ptr& gradients, double radius) {
  GradientEstimation estimation;
  estimation.setInputCloud(cloud);
  estimation.setInputNormals(normals);
  estimation.setRadiusSearch(radius);
  estimation.compute(*gradients);
}

// what both branches prepare for one cloud: its intensities, its keypoints' and its normals
struct Prepared {
  PointCloud<PointXYZI>::Ptr cloud{new PointCloud<PointXYZI>}, keypoints{new PointCloud<PointXYZI>};
  PointCloud<Normal>::Ptr normals{new PointCloud<Normal>};
};
static Prepared prepare(const PointCloudRGB::Ptr& cloud, const PointCloudRGB::Ptr& keypoints, double normal_radius) {
  Prepared p;
  PointCloudXYZRGBtoXYZI(*cloud, *p.cloud);
  PointCloudXYZRGBtoXYZI(*keypoints, *p.keypoints);
  estimateNormals(cloud, p.normals, normal_radius);
  return p;
}

// features.h: the members of Features<FeatureType> the two branches call
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
  if (with_far_point) {
    PointRGB far;
    far.x = far.y = far.z = 9.0e3f;
    kp->push_back(far);
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

static void dump_gradients(const std::string& path, const PointCloud<IntensityGradient>& g) {
  std::vector<float> v;
  for (const IntensityGradient& p : g.points) {
    v.push_back(p.gradient_x);  // (the named members alias gradient[3])
    v.push_back(p.gradient[1]);
    v.push_back(p.gradient_z);
  }
  dump(path, v.data(), v.size());
}

static void dump_pairs(const std::string& path, const Correspondences& corr) {
  std::vector<int32_t> pairs;
  for (const Correspondence& c : corr) {
    pairs.push_back(c.index_query);
    pairs.push_back(c.index_match);
  }
  dump(path, pairs.data(), pairs.size());
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
  static_assert(sizeof(IntensityGradient) == 16, "IntensityGradient is 16 bytes");
  static_assert(sizeof(pcl::Histogram<32>) == 32 * sizeof(float), "Histogram<32> is 32 floats");
  int32_t dense[6] = {-1, -1, -1, -1, -1, -1};
  dump_xyz(out + "/src_kp_xyz.f32", *source_keypoints);
  dump_xyz(out + "/tgt_kp_xyz.f32", *target_keypoints);

  const Prepared src = prepare(source_cloud_, source_keypoints, normal_radius_search_);
  const Prepared tgt = prepare(target_cloud_, target_keypoints, normal_radius_search_);

  {  // ---- the calls of evaluation.cpp:419-462 (DESC_INT_GRAD), per cloud: the normals are the
     // cloud's, the surface the cloud, the input the keypoints, one tree object for both clouds ----
    PointCloud<IntensityGradient>::Ptr source_features(new PointCloud<IntensityGradient>);
    PointCloud<IntensityGradient>::Ptr target_features(new PointCloud<IntensityGradient>);
    GradientEstimation feature_extractor;
    search::KdTree<PointXYZI>::Ptr kdtree(new search::KdTree<PointXYZI>);
    const Prepared* both[2] = {&src, &tgt};
    PointCloud<IntensityGradient>::Ptr features[2] = {source_features, target_features};
    for (int c = 0; c < 2; ++c) {
      feature_extractor.setInputNormals(both[c]->normals);
      feature_extractor.setSearchSurface(both[c]->cloud);
      feature_extractor.setInputCloud(both[c]->keypoints);
      feature_extractor.setSearchMethod(kdtree);
      feature_extractor.setRadiusSearch(feat_radius_search_);
      feature_extractor.compute(*features[c]);
    }
    CorrespondencesPtr correspondences(new Correspondences);
    Features<IntensityGradient> feat;
    feat.findCorrespondences(source_features, target_features, correspondences);

    if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size()) {
      std::fprintf(stderr, "IntensityGradientEstimation::compute failed\n");
      return 1;
    }
    dump_gradients(out + "/src_igrad.f32", *source_features);
    dump_gradients(out + "/tgt_igrad.f32", *target_features);
    dump_pairs(out + "/corr_igrad.i32", *correspondences);
    dense[0] = source_features->is_dense;
    dense[1] = target_features->is_dense;
    std::printf("int_grad: source rows %zu target rows %zu correspondences %zu\n", source_features->size(),
                target_features->size(), correspondences->size());
  }

  int32_t checks[5] = {-1, -1, -1, -1, -1};
  {  // ---- the calls of evaluation.cpp:720-762 (DESC_RIFT): the whole-cloud gradients at the normal
     // radius, then one estimator with 4 x 8 bins and no search method set, per cloud ----
    PointCloud<pcl::Histogram<32> >::Ptr source_features(new PointCloud<pcl::Histogram<32> >);
    PointCloud<pcl::Histogram<32> >::Ptr target_features(new PointCloud<pcl::Histogram<32> >);
    PointCloud<IntensityGradient>::Ptr source_gradients(new PointCloud<IntensityGradient>);
    PointCloud<IntensityGradient>::Ptr target_gradients(new PointCloud<IntensityGradient>);
    computeGradient(src.cloud, src.normals, source_gradients, normal_radius_search_);
    computeGradient(tgt.cloud, tgt.normals, target_gradients, normal_radius_search_);

    Rift rift;
    rift.setRadiusSearch(feat_radius_search_);
    rift.setNrDistanceBins(4);
    rift.setNrGradientBins(8);
    const Prepared* both[2] = {&src, &tgt};
    PointCloud<IntensityGradient>::Ptr gradients[2] = {source_gradients, target_gradients};
    PointCloud<pcl::Histogram<32> >::Ptr features[2] = {source_features, target_features};
    for (int c = 0; c < 2; ++c) {
      rift.setInputCloud(both[c]->keypoints);
      rift.setSearchSurface(both[c]->cloud);
      rift.setInputGradient(gradients[c]);
      rift.compute(*features[c]);
    }
    CorrespondencesPtr correspondences(new Correspondences);
    Features<pcl::Histogram<32> > feat;
    feat.findCorrespondences(source_features, target_features, correspondences);

    if (source_features->size() != source_keypoints->size() || target_features->size() != target_keypoints->size() ||
        source_gradients->size() != source_cloud_->size() || target_gradients->size() != target_cloud_->size()) {
      std::fprintf(stderr, "RIFTEstimation::compute or the whole-cloud gradient failed\n");
      return 1;
    }
    dump_gradients(out + "/src_cloud_grad.f32", *source_gradients);
    dump_gradients(out + "/tgt_cloud_grad.f32", *target_gradients);
    dump(out + "/src_rift.f32", reinterpret_cast<const float*>(source_features->points.data()), source_features->size() * 32);
    dump(out + "/tgt_rift.f32", reinterpret_cast<const float*>(target_features->points.data()), target_features->size() * 32);
    dump_pairs(out + "/corr_rift.i32", *correspondences);
    dense[2] = source_features->is_dense;
    dense[3] = target_features->is_dense;
    dense[4] = source_gradients->is_dense;
    dense[5] = target_gradients->is_dense;
    std::printf("rift: source rows %zu target rows %zu correspondences %zu\n", source_features->size(),
                target_features->size(), correspondences->size());
    const PointCloud<PointXYZI>::Ptr source_intensities = src.cloud, source_keypoint_intensities = src.keypoints;

    // ---- what PCL 1.7 would read or write out of bounds is never silent ----
    {
      // an input index beyond the surface: the cloud as the input, the keypoints as the surface
      PointCloud<Normal>::Ptr kp_normals(new PointCloud<Normal>);
      kp_normals->resize(source_keypoints->size());
      PointCloud<IntensityGradient> refused_g;
      GradientEstimation ge;
      ge.setInputNormals(kp_normals);
      ge.setSearchSurface(source_keypoint_intensities);
      ge.setInputCloud(source_intensities);
      ge.setRadiusSearch(feat_radius_search_);
      ge.compute(refused_g);
      checks[0] = (int32_t)refused_g.size();

      PointCloud<pcl::Histogram<32> > refused;
      PointCloud<IntensityGradient>::Ptr kp_gradients(new PointCloud<IntensityGradient>);
      kp_gradients->resize(source_keypoints->size());
      Rift e;
      e.setRadiusSearch(feat_radius_search_);
      e.setNrDistanceBins(4);
      e.setNrGradientBins(8);
      e.setInputCloud(source_intensities);
      e.setSearchSurface(source_keypoint_intensities);
      e.setInputGradient(kp_gradients);
      e.compute(refused);
      checks[1] = (int32_t)refused.size();
      // a gradient cloud of another size than the surface
      e.setInputCloud(source_keypoint_intensities);
      e.setSearchSurface(source_intensities);
      e.compute(refused);
      checks[2] = (int32_t)refused.size();
      // 4 x 4 bins (PCL's defaults) into Histogram<32>: PCL writes past histogram[N] when D G > N
      e.setInputGradient(source_gradients);
      e.setNrGradientBins(4);
      e.compute(refused);
      checks[3] = (int32_t)refused.size();
      e.setNrGradientBins(8);  // ... and the object works afterwards
      e.compute(refused);
      checks[4] = (int32_t)refused.size();
    }
  }
  dump(out + "/dense.i32", dense, 6);
  dump(out + "/checks.i32", checks, 5);
  return 0;
}
