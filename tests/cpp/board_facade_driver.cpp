// board_facade_driver.cpp -- what the reference's DESC_BOARD branch (src/evaluation.cpp:372-393) asks
// of PCL, asked of include/pfx_pcl.hpp: a BOARDLocalReferenceFrameEstimation held as
// Feature<PointXYZRGB, ReferenceFrame>::Ptr goes through the generic wrapper (features.h:175-196),
// which casts it to FeatureFromNormals and estimates the cloud's normals because the cast succeeds;
// then the mutual nearest neighbours of the two frame clouds (features.h:224-273) are taken.
//   board_facade_driver <source.pcd> <target.pcd> <out_dir>
// Keypoints: every (n / 48)-th finite point of each cloud; the source's get one more point far away
// from the cloud (an empty neighbourhood: a NaN row).  Writes, for tests/test_board_facade.py:
//   src_kp_xyz.f32 / tgt_kp_xyz.f32 (K x 3), src_rf.f32 / tgt_rf.f32 (K x 9), corr.i32 (index_query,
//   index_match pairs), dense.i32 (is_dense of the two frame clouds), casts.i32 (whether the wrapper's
//   cast found normals to compute), setters.f32 (the six getters of a default object, then after
//   each setter was called), checks.i32: the rows of a compute() with setFindHoles(true), with a
//   k-search, without normals (0 each: PCL_ERROR and an empty output), then of a valid compute() on
//   the same object, and of one with a tangent radius set.
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#define PFX_PCL_BOOST_SHIM
#include "pfx_pcl.hpp"

typedef pcl::PointCloud<pcl::PointXYZRGB> Cloud;
typedef pcl::PointCloud<pcl::ReferenceFrame> Frames;
typedef pcl::BOARDLocalReferenceFrameEstimation<pcl::PointXYZRGB, pcl::Normal, pcl::ReferenceFrame> Board;

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

// Features<FeatureType> of the reference: the estimator arrives as its Feature base; whether it
// wants normals is found by a cast, and only then are the cloud's normals estimated (at their own
// radius).
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

  // nearest row of `to` for every row of `from` (k = 1)
  static std::vector<int> getCorrespondences(const DescPtr& from, const DescPtr& to) {
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
  static std::vector<int32_t> findCorrespondences(const DescPtr& source, const DescPtr& target) {
    const std::vector<int> s2t = getCorrespondences(source, target), t2s = getCorrespondences(target, source);
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

static std::vector<float> floats(const Frames& c) {
  std::vector<float> v;
  for (const pcl::ReferenceFrame& p : c.points) {
    v.insert(v.end(), p.x_axis, p.x_axis + 3);
    v.insert(v.end(), p.y_axis, p.y_axis + 3);
    v.insert(v.end(), p.z_axis, p.z_axis + 3);
  }
  return v;
}

static void getters(const Board& b, std::vector<float>& v) {
  v.push_back(b.getTangentRadius());
  v.push_back(b.getFindHoles() ? 1.0f : 0.0f);
  v.push_back(b.getMarginThresh());
  v.push_back((float)b.getCheckMarginArraySize());
  v.push_back(b.getHoleSizeProbThresh());
  v.push_back(b.getSteepThresh());
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
  static_assert(sizeof(pcl::ReferenceFrame) == 36, "ReferenceFrame is nine floats");
  const Cloud::Ptr source_kp = every_nth(*source, 48, true), target_kp = every_nth(*target, 48, false);
  save_xyz(out + "/src_kp_xyz.f32", *source_kp);
  save_xyz(out + "/tgt_kp_xyz.f32", *target_kp);
  std::vector<int32_t> dense, casts, checks;

  {  // the DESC_BOARD branch
    Board::Ptr feature_extractor_orig(new Board);
    pcl::Feature<pcl::PointXYZRGB, pcl::ReferenceFrame>::Ptr feature_extractor(feature_extractor_orig);
    Frames::Ptr source_features(new Frames), target_features(new Frames);
    Features<pcl::ReferenceFrame> feat(feature_extractor, 0.08, 0.05);
    feat.compute(source, source_kp, source_features);
    casts.push_back(feat.cast_found_normals);
    feat.compute(target, target_kp, target_features);
    if (source_features->size() != source_kp->size() || target_features->size() != target_kp->size()) {
      std::fprintf(stderr, "BOARDLocalReferenceFrameEstimation::compute failed\n");
      return 1;
    }
    save(out + "/src_rf.f32", floats(*source_features));
    save(out + "/tgt_rf.f32", floats(*target_features));
    save(out + "/corr.i32", Features<pcl::ReferenceFrame>::findCorrespondences(source_features, target_features));
    dense.push_back(source_features->is_dense);
    dense.push_back(target_features->is_dense);
  }
  {  // the setters round-trip
    std::vector<float> v;
    Board b;
    getters(b, v);
    b.setTangentRadius(0.03f);
    b.setFindHoles(true);
    b.setMarginThresh(0.5f);
    b.setCheckMarginArraySize(36);
    b.setHoleSizeProbThresh(0.3f);
    b.setSteepThresh(0.25f);
    getters(b, v);
    save(out + "/setters.f32", v);
  }
  {  // what is not on the accelerated path, or not PCL's use of the class, fails loudly
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
    pcl::NormalEstimationOMP<pcl::PointXYZRGB, pcl::Normal> ne;
    ne.setInputCloud(source);
    ne.setRadiusSearch(0.05);
    ne.compute(*normals);
    Frames rows;
    Board b;
    b.setSearchSurface(source);
    b.setInputCloud(source_kp);
    b.setInputNormals(normals);
    b.setRadiusSearch(0.08);
    b.setFindHoles(true);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    b.setFindHoles(false);
    b.setKSearch(10);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    b.setKSearch(0);
    b.setInputNormals(pcl::PointCloud<pcl::Normal>::Ptr());
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    // ... and the object works afterwards
    b.setInputNormals(normals);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    b.setTangentRadius(0.05f);
    b.compute(rows);
    checks.push_back((int32_t)rows.size());
    save(out + "/src_rf_tangent.f32", floats(rows));
  }
  save(out + "/dense.i32", dense);
  save(out + "/casts.i32", casts);
  save(out + "/checks.i32", checks);
  return 0;
}
