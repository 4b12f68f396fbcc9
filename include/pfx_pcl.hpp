// pfx_pcl.hpp -- PCL 1.7-compatible C++ facade over the libpfx C-ABI (include/pfx.h).
//
// The reference's wrapper headers call PCL's class API on the hot path and nothing else:
//   include/pcl_feature_extraction/keypoints.h:199-231  RangeImagePlanar, RangeImageBorderExtractor,
//                                                       NarfKeypoint, PointCloud<int>
//   include/pcl_feature_extraction/features.h:175-196   Feature / FeatureFromNormals (polymorphic,
//                                                       probed with dynamic_pointer_cast),
//                                                       search::KdTree, setRadiusSearch, compute
//   include/pcl_feature_extraction/tools.h:22-32        NormalEstimationOMP
//   src/evaluation.cpp:593-612, :676-695, :766-785      FPFHEstimation, PFHEstimation, SHOTEstimationOMP
//   src/evaluation.cpp:786-805                           SHOTColorEstimationOMP
//   src/evaluation.cpp:514-553                           SpinImageEstimation, Histogram<153>
//   src/evaluation.cpp:863-885, :257                     IterativeClosestPoint, transformPointCloud
//   include/pcl_feature_extraction/features.h:224-273   KdTreeFLANN<FeatureT>::nearestKSearch,
//                                                       Correspondence(s), boost::thread / ref
// This header provides those names in namespace pcl (plus the minimal Eigen subset the calls
// touch), implemented on the GPU through libpfx, so the wrapper headers compile unchanged when
// this header stands in for the PCL includes.  Point types keep PCL's 16-byte-aligned layouts.
//
// Behaviour mirrors PCL 1.7: compute() never throws on algorithmic failure -- a failed
// initCompute / device error prints PCL_ERROR and leaves an empty output cloud; per-point failure
// is NaN in the row, is_dense = false.  Objects are not re-entrant; one libpfx context per
// process (device from $PFX_DEVICE, default 0), calls are synchronous on the caller's thread.
//
// Define PFX_PCL_BOOST_SHIM before including to get boost::shared_ptr / dynamic_pointer_cast
// aliases for code written against PCL 1.7's boost pointers (features.h:181-182).
#ifndef PFX_PCL_HPP_
#define PFX_PCL_HPP_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <limits>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "pfx.h"

#ifndef PCL_ERROR
#define PCL_ERROR(...) std::fprintf(stderr, __VA_ARGS__)
#endif

#ifdef PFX_PCL_BOOST_SHIM
namespace boost {
using std::dynamic_pointer_cast;
using std::ref;
using std::shared_ptr;
using std::thread;  // features.h:234-239 runs the two getCorrespondences on boost::thread
}  // namespace boost
#endif

// ---- the Eigen subset used by keypoints.h:207-210 ------------------------------------------
namespace Eigen {

struct Vector3f {
  float v[3] = {0, 0, 0};
  Vector3f() = default;
  Vector3f(float x, float y, float z) : v{x, y, z} {}
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
};

struct Vector4f {
  float v[4] = {0, 0, 0, 0};
  Vector4f() = default;
  Vector4f(float x, float y, float z, float w) : v{x, y, z, w} {}
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
  static Vector4f Zero() { return Vector4f(); }
};

struct Quaternionf {
  float qw = 1, qx = 0, qy = 0, qz = 0;
  Quaternionf() = default;
  Quaternionf(float w, float x, float y, float z) : qw(w), qx(x), qy(y), qz(z) {}
  static Quaternionf Identity() { return Quaternionf(); }
  float w() const { return qw; }
  float x() const { return qx; }
  float y() const { return qy; }
  float z() const { return qz; }
};

struct Translation3f {
  float t[3];
  Translation3f(float x, float y, float z) : t{x, y, z} {}
};

// 4x4 affine transform, row-major storage
struct Affine3f {
  float m[16];
  Affine3f() { setIdentity(); }
  explicit Affine3f(const Translation3f& tr) {
    setIdentity();
    m[3] = tr.t[0]; m[7] = tr.t[1]; m[11] = tr.t[2];
  }
  // Eigen's Quaternion::toRotationMatrix (unit quaternion)
  explicit Affine3f(const Quaternionf& q) {
    setIdentity();
    const float tx = 2.f * q.qx, ty = 2.f * q.qy, tz = 2.f * q.qz;
    const float twx = tx * q.qw, twy = ty * q.qw, twz = tz * q.qw;
    const float txx = tx * q.qx, txy = ty * q.qx, txz = tz * q.qx;
    const float tyy = ty * q.qy, tyz = tz * q.qy, tzz = tz * q.qz;
    m[0] = 1.f - (tyy + tzz); m[1] = txy - twz;         m[2] = txz + twy;
    m[4] = txy + twz;         m[5] = 1.f - (txx + tzz); m[6] = tyz - twx;
    m[8] = txz - twy;         m[9] = tyz + twx;         m[10] = 1.f - (txx + tyy);
  }
  static Affine3f Identity() { return Affine3f(); }
  void setIdentity() {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
  }
  float& operator()(int r, int c) { return m[4 * r + c]; }
  float operator()(int r, int c) const { return m[4 * r + c]; }
  Affine3f operator*(const Affine3f& o) const {
    Affine3f r;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        float s = 0.f;
        for (int k = 0; k < 4; ++k) s += m[4 * i + k] * o.m[4 * k + j];
        r.m[4 * i + j] = s;
      }
    return r;
  }
};

// 4x4 float matrix (registration's getBestTransformation), row-major storage
struct Matrix4f {
  float m[16];
  Matrix4f() { setIdentity(); }
  static Matrix4f Identity() { return Matrix4f(); }
  void setIdentity() {
    for (int i = 0; i < 16; ++i) m[i] = (i % 5 == 0) ? 1.f : 0.f;
  }
  float& operator()(int r, int c) { return m[4 * r + c]; }
  float operator()(int r, int c) const { return m[4 * r + c]; }
};

}  // namespace Eigen

namespace pcl {

namespace detail {
// one libpfx context per process (thread-affine use, as PCL objects are not re-entrant)
inline pfx_ctx* context() {
  static pfx_ctx* ctx = [] {
    pfx_ctx* c = nullptr;
    const char* dev = std::getenv("PFX_DEVICE");
    if (pfx_ctx_create(dev ? std::atoi(dev) : 0, &c) != PFX_OK) {
      PCL_ERROR("[pfx_pcl] no HIP device: %s\n", c ? pfx_last_error(c) : "pfx_ctx_create failed");
      return static_cast<pfx_ctx*>(nullptr);
    }
    return c;
  }();
  return ctx;
}
inline float nanf() { return std::numeric_limits<float>::quiet_NaN(); }
// serialises calls that may come from several threads at once (features.h:234-239 queries two
// descriptor trees on two threads; a libpfx context is not re-entrant)
inline std::mutex& context_mutex() {
  static std::mutex m;
  return m;
}
}  // namespace detail

// ---- point types (PCL 1.7 layouts, 16-byte aligned) ----------------------------------------
struct alignas(16) PointXYZRGB {
  float x = 0, y = 0, z = 0, data_pad = 1.f;
  union { float rgb; uint32_t rgba = 0; };
  float pad_[3] = {0, 0, 0};
};
struct alignas(16) Normal {
  float normal_x = 0, normal_y = 0, normal_z = 0, data_pad = 0.f;
  float curvature = 0;
  float pad_[3] = {0, 0, 0};
};
struct alignas(16) PointWithRange {
  float x = 0, y = 0, z = 0, data_pad = 1.f;
  float range = 0;
  float pad_[3] = {0, 0, 0};
};
struct alignas(16) PointXYZI {
  float x = 0, y = 0, z = 0, data_pad = 1.f;
  float intensity = 0;
  float pad_[3] = {0, 0, 0};
};
// pcl::IntensityGradient: 16 bytes, the gradient as an array and by name
struct alignas(16) IntensityGradient {
  union {
    float gradient[3];
    struct { float gradient_x, gradient_y, gradient_z; };
  };
  float pad_ = 0;
  IntensityGradient() : gradient{0, 0, 0} {}
};
static_assert(sizeof(IntensityGradient) == 16, "pcl::IntensityGradient is 16 bytes");
// pcl::MomentInvariants: j1 j2 j3, 12 bytes
struct MomentInvariants { float j1 = 0, j2 = 0, j3 = 0; };
static_assert(sizeof(MomentInvariants) == 12, "pcl::MomentInvariants is 12 bytes");
// pcl::PrincipalCurvatures: 20 bytes, the direction of the largest curvature as an array and by
// name, then the largest and the smallest curvature
struct PrincipalCurvatures {
  union {
    float principal_curvature[3];
    struct { float principal_curvature_x, principal_curvature_y, principal_curvature_z; };
  };
  float pc1 = 0, pc2 = 0;
  PrincipalCurvatures() : principal_curvature{0, 0, 0} {}
};
static_assert(sizeof(PrincipalCurvatures) == 20, "pcl::PrincipalCurvatures is 20 bytes");
struct FPFHSignature33 { float histogram[33]; };
struct PFHSignature125 { float histogram[125]; };
// pcl::Histogram<N> (spin images, RIFT, intensity spin images): N floats, nothing else
template <int N>
struct Histogram {
  float histogram[N];
  static int descriptorSize() { return N; }
};
struct SHOT352 { float descriptor[352]; float rf[9]; };
struct SHOT1344 { float descriptor[1344]; float rf[9]; };
struct ShapeContext1980 { float descriptor[1980]; float rf[9]; };
struct ReferenceFrame { float x_axis[3], y_axis[3], z_axis[3]; };
// pcl::Boundary: one byte
struct Boundary { uint8_t boundary_point = 0; };
static_assert(sizeof(Boundary) == 1, "pcl::Boundary is one byte");
// (PCL's Narf36: the patch's position and orientation in the world, then the descriptor)
// pcl::VFHSignature308: CVFH's row (45 bins each of f1, f2, f3, f4, then 128 of the viewpoint component)
struct VFHSignature308 { float histogram[308]; };
struct Narf36 { float x = 0, y = 0, z = 0, roll = 0, pitch = 0, yaw = 0; float descriptor[36] = {}; };
static_assert(sizeof(Narf36) == 42 * sizeof(float), "pcl::Narf36 is 42 floats");

// pcl::PCLException, as far as the facade throws it (SpinImageEstimation where PCL's throws)
class PCLException : public std::runtime_error {
 public:
  explicit PCLException(const std::string& what) : std::runtime_error(what) {}
};

template <typename T>
class PointCloud {
 public:
  typedef std::shared_ptr<PointCloud<T> > Ptr;
  typedef std::shared_ptr<const PointCloud<T> > ConstPtr;
  std::vector<T> points;
  uint32_t width = 0, height = 1;
  bool is_dense = true;
  Eigen::Vector4f sensor_origin_ = Eigen::Vector4f(0, 0, 0, 0);
  Eigen::Quaternionf sensor_orientation_ = Eigen::Quaternionf::Identity();
  size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  void push_back(const T& p) { points.push_back(p); width = (uint32_t)points.size(); height = 1; }
  void resize(size_t n) { points.resize(n); width = (uint32_t)n; height = 1; }
  void clear() { points.clear(); width = 0; height = 1; }
  T& operator[](size_t i) { return points[i]; }
  const T& operator[](size_t i) const { return points[i]; }
};

namespace detail {
struct SoA {
  std::vector<float> x, y, z;
  size_t size() const { return x.size(); }
  int64_t n() const { return (int64_t)x.size(); }  // the count as the C-ABI takes it
};
template <typename P>
inline SoA soa_xyz(const PointCloud<P>& c) {
  SoA s;
  const size_t n = c.size();
  s.x.resize(n); s.y.resize(n); s.z.resize(n);
  for (size_t i = 0; i < n; ++i) { s.x[i] = c.points[i].x; s.y[i] = c.points[i].y; s.z[i] = c.points[i].z; }
  return s;
}
inline SoA soa_normals(const PointCloud<Normal>& c) {
  SoA s;
  const size_t n = c.size();
  s.x.resize(n); s.y.resize(n); s.z.resize(n);
  for (size_t i = 0; i < n; ++i) {
    s.x[i] = c.points[i].normal_x; s.y[i] = c.points[i].normal_y; s.z[i] = c.points[i].normal_z;
  }
  return s;
}
inline bool ok(pfx_status st, const char* who) {
  if (st == PFX_OK) return true;
  PCL_ERROR("[pcl::%s::compute] %s\n", who, context() ? pfx_last_error(context()) : "no device");
  return false;
}
// Which NaN of a row clears is_dense.  The C-ABI fills a row it could not compute with NaN, so its
// first float tells; kAnyFloat is for the classes whose computed rows can hold a NaN as well (stricter
// than PCL, which clears is_dense only for a row without neighbours).
enum class NanRule { kFirstFloat, kAnyFloat };
// The descriptor classes' one way from the C-ABI's rows to the output cloud: nq points, point i
// taking WA floats of `a` and then WB floats of `b` (a descriptor and its rf) as its first floats.
template <int WA, int WB = 0, typename PointOutT>
inline void write_rows(PointCloud<PointOutT>& out, size_t nq, NanRule rule, const std::vector<float>& a,
                       const std::vector<float>& b = std::vector<float>()) {
  static_assert(sizeof(PointOutT) >= sizeof(float) * (WA + WB), "the output point holds the floats of a row");
  out.resize(nq);
  out.is_dense = true;
  for (size_t i = 0; i < nq; ++i) {
    float* row = reinterpret_cast<float*>(&out.points[i]);
    std::copy(a.begin() + i * WA, a.begin() + (i + 1) * WA, row);
    if (WB) std::copy(b.begin() + i * WB, b.begin() + (i + 1) * WB, row + WA);
    const int tested = rule == NanRule::kAnyFloat ? WA + WB : 1;
    for (int c = 0; c < tested; ++c)
      if (std::isnan(row[c])) out.is_dense = false;
  }
}
}  // namespace detail

namespace search {
// The GPU path builds its own uniform-grid index; the tree object only carries the type.
template <typename PointT>
class KdTree {
 public:
  typedef std::shared_ptr<KdTree<PointT> > Ptr;
  explicit KdTree(bool sorted = true) : sorted_(sorted) {}
  virtual ~KdTree() = default;
 private:
  bool sorted_;
};
}  // namespace search

// ---- Feature hierarchy (features.h:175-196 probes FeatureFromNormals by dynamic cast) -------
template <typename PointInT, typename PointOutT>
class Feature {
 public:
  typedef PointCloud<PointInT> PointCloudIn;
  typedef typename PointCloudIn::ConstPtr PointCloudInConstPtr;
  typedef PointCloud<PointOutT> PointCloudOut;
  typedef std::shared_ptr<Feature<PointInT, PointOutT> > Ptr;
  typedef typename search::KdTree<PointInT>::Ptr KdTreePtr;
  virtual ~Feature() = default;
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setSearchSurface(const PointCloudInConstPtr& cloud) { surface_ = cloud; }
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  void setRadiusSearch(double r) { search_radius_ = r; }
  void setKSearch(int k) { k_ = k; }
  double getRadiusSearch() const { return search_radius_; }
  // Feature::compute: initCompute -> computeFeature -> deinitCompute
  void compute(PointCloudOut& output) {
    output.clear();
    if (k_ != 0 && !k_search_error_.empty()) {
      PCL_ERROR("%s\n", k_search_error_.c_str());
      return;
    }
    if (accepts_k_search_ && k_ != 0 && input_ && !input_->empty()) {
      // PCL's initCompute rule for the class that opted in: one of the two, never both
      if (search_radius_ != 0.0) {
        PCL_ERROR("[pcl::%s::compute] Both radius (%f) and K (%d) defined! Set one of them to zero first and then "
                  "re-run compute ().\n", name_.c_str(), search_radius_, k_);
        return;
      }
      if (!detail::context()) return;
      computeFeature(output);
      return;
    }
    if (!input_ || input_->empty() || k_ != 0 || !(search_radius_ > 0.0)) {
      PCL_ERROR("[pcl::%s::compute] initCompute failed (needs an input cloud and a radius; "
                "k-NN search is not on the accelerated path)\n", name_.c_str());
      return;
    }
    if (!detail::context()) return;
    computeFeature(output);
  }

 protected:
  virtual void computeFeature(PointCloudOut& output) = 0;
  const PointCloudIn& surface() const { return surface_ ? *surface_ : *input_; }
  bool input_is_surface() const { return !surface_ || surface_.get() == input_.get(); }
  // for the classes whose row i reads element i of something the surface has one of per point (a
  // normal, a gradient, the point itself): more input points than surface points is an error
  bool input_within_surface() const {
    const size_t ns = surface().size();
    if (input_->size() <= ns) return true;
    PCL_ERROR("[pcl::%s::compute] input index %zu is beyond the search surface (%zu points)\n", name_.c_str(), ns, ns);
    return false;
  }
  std::string name_ = "Feature";
  std::string k_search_error_;  // a class whose PCL original refuses a k-search in its own words sets them
  bool accepts_k_search_ = false;  // a class with a k-NN path sets it: k_ != 0 and radius 0 reach computeFeature
  PointCloudInConstPtr input_, surface_;
  KdTreePtr tree_;
  double search_radius_ = 0.0;
  int k_ = 0;
};

template <typename PointInT, typename PointNT, typename PointOutT>
class FeatureFromNormals : public Feature<PointInT, PointOutT> {
 public:
  typedef typename PointCloud<PointNT>::ConstPtr PointCloudNConstPtr;
  typedef std::shared_ptr<FeatureFromNormals<PointInT, PointNT, PointOutT> > Ptr;
  void setInputNormals(const PointCloudNConstPtr& normals) { normals_ = normals; }

 protected:
  // one normal per surface point, or PCL_ERROR with the class's own words for it
  bool normals_match(const std::string& what) const {
    if (normals_ && normals_->size() == this->surface().size()) return true;
    PCL_ERROR("[pcl::%s::compute] %s\n", this->name_.c_str(), what.c_str());
    return false;
  }
  PointCloudNConstPtr normals_;
};

// NormalEstimationOMP<In, Normal> (tools.h:22-32): viewpoint (0,0,0) unless set.  setRadiusSearch(r) runs
// pfx_normals, setKSearch(k) with radius 0 pfx_normals_knn (1 <= k <= PFX_KNN_MAX_K); both set is PCL's error.
template <typename PointInT, typename PointOutT>
class NormalEstimationOMP : public Feature<PointInT, PointOutT> {
 public:
  explicit NormalEstimationOMP(unsigned int /*nr_threads*/ = 0) {
    this->name_ = "NormalEstimationOMP";
    this->accepts_k_search_ = true;
  }
  void setViewPoint(float vx, float vy, float vz) { vp_[0] = vx; vp_[1] = vy; vp_[2] = vz; }
  void setNumberOfThreads(unsigned int) {}

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const PointCloud<PointInT>& in = *this->input_;
    if (!this->input_is_surface()) {
      PCL_ERROR("[pcl::NormalEstimationOMP::compute] a search surface other than the input is not on "
                "the accelerated path\n");
      return;
    }
    const detail::SoA s = detail::soa_xyz(in);
    const size_t n = in.size();
    std::vector<float> nx(n), ny(n), nz(n), cv(n);
    const pfx_status st =
        this->k_ != 0 ? pfx_normals_knn(detail::context(), s.x.data(), s.y.data(), s.z.data(), (int64_t)n, this->k_, vp_,
                                        nx.data(), ny.data(), nz.data(), cv.data())
                      : pfx_normals(detail::context(), s.x.data(), s.y.data(), s.z.data(), (int64_t)n,
                                    this->search_radius_, vp_, nx.data(), ny.data(), nz.data(), cv.data());
    if (!detail::ok(st, "NormalEstimationOMP")) return;
    out.resize(n);
    out.is_dense = true;
    for (size_t i = 0; i < n; ++i) {
      out.points[i].normal_x = nx[i]; out.points[i].normal_y = ny[i];
      out.points[i].normal_z = nz[i]; out.points[i].curvature = cv[i];
      if (std::isnan(nx[i])) out.is_dense = false;
    }
  }
  float vp_[3] = {0.f, 0.f, 0.f};
};

// FPFHEstimation<In, Normal, FPFHSignature33> (evaluation.cpp:597)
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33>
class FPFHEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<FPFHEstimation<PointInT, PointNT, PointOutT> > Ptr;
  FPFHEstimation() { this->name_ = "FPFHEstimation"; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    if (!this->normals_match("normals missing or not matching the surface")) return;
    const detail::SoA s = detail::soa_xyz(this->surface()), nrm = detail::soa_normals(*this->normals_);
    const detail::SoA q = detail::soa_xyz(*this->input_);
    std::vector<float> h(q.size() * 33);
    if (!detail::ok(pfx_fpfh(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(), nrm.y.data(),
                             nrm.z.data(), s.n(), q.x.data(), q.y.data(), q.z.data(), q.n(),
                             this->input_is_surface() ? 1 : 0, this->search_radius_, h.data()),
                    "FPFHEstimation"))
      return;
    detail::write_rows<33>(out, q.size(), detail::NanRule::kFirstFloat, h);
  }
};

// PFHEstimation<In, Normal, PFHSignature125> (evaluation.cpp:680); the feature cache
// (setUseInternalCache) is not on the accelerated path -- the reference never enables it
template <typename PointInT, typename PointNT, typename PointOutT = PFHSignature125>
class PFHEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<PFHEstimation<PointInT, PointNT, PointOutT> > Ptr;
  PFHEstimation() { this->name_ = "PFHEstimation"; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    if (!this->normals_match("normals missing or not matching the surface")) return;
    const detail::SoA s = detail::soa_xyz(this->surface()), nrm = detail::soa_normals(*this->normals_);
    const detail::SoA q = detail::soa_xyz(*this->input_);
    std::vector<float> h(q.size() * 125);
    if (!detail::ok(pfx_pfh(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(), nrm.y.data(),
                            nrm.z.data(), s.n(), q.x.data(), q.y.data(), q.z.data(), q.n(), this->search_radius_,
                            h.data()),
                    "PFHEstimation"))
      return;
    detail::write_rows<125>(out, q.size(), detail::NanRule::kFirstFloat, h);
  }
};

// SHOTEstimationOMP<In, Normal, SHOT352> + SHOTLocalReferenceFrameEstimation (evaluation.cpp:770)
template <typename PointInT, typename PointNT, typename PointOutT = SHOT352,
          typename PointRFT = ReferenceFrame>
class SHOTEstimationOMP : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<SHOTEstimationOMP<PointInT, PointNT, PointOutT, PointRFT> > Ptr;
  explicit SHOTEstimationOMP(unsigned int /*nr_threads*/ = 0) { this->name_ = "SHOTEstimationOMP"; }
  void setNumberOfThreads(unsigned int) {}

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    if (!this->normals_match("normals missing or not matching the surface")) return;
    const detail::SoA s = detail::soa_xyz(this->surface()), nrm = detail::soa_normals(*this->normals_);
    const detail::SoA q = detail::soa_xyz(*this->input_);
    std::vector<float> d(q.size() * 352), rf(q.size() * 9);
    if (!detail::ok(pfx_shot(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(), nrm.y.data(),
                             nrm.z.data(), s.n(), q.x.data(), q.y.data(), q.z.data(), q.n(), this->search_radius_,
                             d.data(), rf.data()),
                    "SHOTEstimationOMP"))
      return;
    detail::write_rows<352, 9>(out, q.size(), detail::NanRule::kFirstFloat, d, rf);
  }
};

// SHOTColorEstimationOMP<In, Normal, SHOT1344> (evaluation.cpp:790): shape and colour, PCL's
// defaults.  The colours are the low 24 bits of rgba, the surface's for the neighbours and the
// input cloud's for the reference colour of each query.
template <typename PointInT, typename PointNT, typename PointOutT = SHOT1344,
          typename PointRFT = ReferenceFrame>
class SHOTColorEstimationOMP : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<SHOTColorEstimationOMP<PointInT, PointNT, PointOutT, PointRFT> > Ptr;
  explicit SHOTColorEstimationOMP(unsigned int /*nr_threads*/ = 0) { this->name_ = "SHOTColorEstimationOMP"; }
  void setNumberOfThreads(unsigned int) {}

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const PointCloud<PointInT>& surf = this->surface();
    if (!this->normals_match("normals missing or not matching the surface")) return;
    const detail::SoA s = detail::soa_xyz(surf), nrm = detail::soa_normals(*this->normals_);
    const detail::SoA q = detail::soa_xyz(*this->input_);
    const size_t ns = surf.size(), nq = this->input_->size();
    std::vector<uint32_t> srgb(ns + 1), qrgb(nq + 1);
    for (size_t i = 0; i < ns; ++i) srgb[i] = surf.points[i].rgba & 0x00ffffffu;
    for (size_t i = 0; i < nq; ++i) qrgb[i] = this->input_->points[i].rgba & 0x00ffffffu;
    std::vector<float> d(nq * 1344), rf(nq * 9);
    if (!detail::ok(pfx_shot_color(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(),
                                   nrm.y.data(), nrm.z.data(), srgb.data(), s.n(), q.x.data(), q.y.data(), q.z.data(),
                                   qrgb.data(), q.n(), this->search_radius_, d.data(), rf.data()),
                    "SHOTColorEstimationOMP"))
      return;
    detail::write_rows<1344, 9>(out, nq, detail::NanRule::kFirstFloat, d, rf);
  }
};

// SpinImageEstimation<In, Normal, Histogram<153>> (evaluation.cpp:525).  As in PCL 1.7 it is not a
// FeatureFromNormals: it keeps its own input normals, one per point of the *input* cloud, and the
// normal of a point is the rotation axis of its image.  Custom rotation axes, the radial structure
// and the angular domain are not on the accelerated path: compute() then fails with PCL_ERROR and
// an empty output.  Where PCL's computeFeature throws (fewer neighbours than
// setMinPointCountInNeighbourhood, a cosine out of range because an axis or normal is not of unit
// length), compute() throws pcl::PCLException.
template <typename PointInT, typename PointNT, typename PointOutT>
class SpinImageEstimation : public Feature<PointInT, PointOutT> {
 public:
  typedef PointCloud<PointNT> PointCloudN;
  typedef typename PointCloudN::Ptr PointCloudNPtr;
  typedef typename PointCloudN::ConstPtr PointCloudNConstPtr;
  typedef std::shared_ptr<SpinImageEstimation<PointInT, PointNT, PointOutT> > Ptr;
  explicit SpinImageEstimation(unsigned int image_width = 8, double support_angle_cos = 0.0,
                               unsigned int min_pts_neighb = 0)
      : image_width_(image_width), support_angle_cos_(support_angle_cos), min_pts_neighb_(min_pts_neighb) {
    this->name_ = "SpinImageEstimation";
  }
  void setInputNormals(const PointCloudNConstPtr& normals) { input_normals_ = normals; }
  void setImageWidth(unsigned int bin_count) { image_width_ = bin_count; }
  void setSupportAngle(double support_angle_cos) { support_angle_cos_ = support_angle_cos; }
  void setMinPointCountInNeighbourhood(unsigned int min_pts_neighb) { min_pts_neighb_ = min_pts_neighb; }
  void setRadialStructure(bool is_radial = true) { is_radial_ = is_radial; }
  void setAngularDomain(bool is_angular = true) { is_angular_ = is_angular; }
  void setRotationAxis(const PointNT& /*axis*/) { custom_axis_ = true; }
  void setInputRotationAxes(const PointCloudNConstPtr& /*axes*/) { custom_axis_ = true; }
  void useNormalsAsRotationAxis() { custom_axis_ = false; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const size_t nq = this->input_->size();
    const int64_t S = ((int64_t)image_width_ + 1) * (2 * (int64_t)image_width_ + 1);
    if (custom_axis_ || is_radial_ || is_angular_) {
      PCL_ERROR("[pcl::SpinImageEstimation::compute] custom rotation axes, the radial structure and the "
                "angular domain are not on the accelerated path\n");
      return;
    }
    if (!input_normals_ || input_normals_->size() != nq) {
      PCL_ERROR("[pcl::SpinImageEstimation::compute] the input normals are missing or do not match the input "
                "cloud\n");
      return;
    }
    if (image_width_ < 1 || image_width_ > 16 || S != (int64_t)(sizeof(PointOutT) / sizeof(float))) {
      PCL_ERROR("[pcl::SpinImageEstimation::compute] (image_width + 1) * (2 * image_width + 1) = %lld does not "
                "match the output histogram (image_width in [1, 16])\n", (long long)S);
      return;
    }
    if (!(support_angle_cos_ >= 0.0 && support_angle_cos_ <= 1.0)) {
      PCL_ERROR("[pcl::SpinImageEstimation::compute] the support angle cosine must be in [0, 1]\n");
      return;
    }
    // PCL reads the normal of a *surface* neighbour from the input normals: meaningful only when
    // the input cloud is the surface
    const bool support = support_angle_cos_ > 0.0;
    if (support && !this->input_is_surface()) {
      PCL_ERROR("[pcl::SpinImageEstimation::compute] a support angle needs the input cloud to be the search "
                "surface\n");
      return;
    }
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    const detail::SoA ax = detail::soa_normals(*input_normals_);
    pfx_spin_params prm;
    pfx_spin_params_default(&prm);
    prm.image_width = (int32_t)image_width_;
    prm.support_angle_cos = support_angle_cos_;
    prm.min_pts_neighb = (int32_t)min_pts_neighb_;
    std::vector<float> h(nq * (size_t)S);
    const pfx_status st = pfx_spin_image(
        detail::context(), s.x.data(), s.y.data(), s.z.data(), support ? ax.x.data() : nullptr,
        support ? ax.y.data() : nullptr, support ? ax.z.data() : nullptr, s.n(), q.x.data(), q.y.data(), q.z.data(),
        ax.x.data(), ax.y.data(), ax.z.data(), q.n(), this->search_radius_, &prm, h.data(), nullptr, nullptr);
    // (every argument was checked above: PFX_ERR_INVALID is one of the two rules PCL throws on)
    if (st == PFX_ERR_INVALID)
      throw PCLException(std::string("[pcl::SpinImageEstimation::compute] ") + pfx_last_error(detail::context()));
    if (!detail::ok(st, "SpinImageEstimation")) return;
    // (S floats a row: the output histogram's own size, as checked above)
    detail::write_rows<sizeof(PointOutT) / sizeof(float)>(out, nq, detail::NanRule::kFirstFloat, h);
  }
  PointCloudNConstPtr input_normals_;
  unsigned int image_width_;
  double support_angle_cos_;
  unsigned int min_pts_neighb_;
  bool is_radial_ = false, is_angular_ = false, custom_axis_ = false;
};

// ---- intensity gradients and RIFT (evaluation.cpp:416-465, 716-765; tools.h:40-54) ------------
namespace common {
// common::IntensityFieldAccessor<PointXYZI> (common/intensity.h): the float accessor
template <typename PointT> struct IntensityFieldAccessor;
template <>
struct IntensityFieldAccessor<PointXYZI> {
  float operator()(const PointXYZI& p) const { return p.intensity; }
  void get(const PointXYZI& p, float& intensity) const { intensity = p.intensity; }
  void set(PointXYZI& p, float intensity) const { p.intensity = intensity; }
  void demean(PointXYZI& p, float value) const { p.intensity -= value; }
  void add(PointXYZI& p, float value) const { p.intensity += value; }
};
}  // namespace common

// pcl::PointCloudXYZRGBtoXYZI (point_types_conversion.h): I = (0.299f r + 0.587f g) + 0.114f b
inline void PointXYZRGBtoXYZI(const PointXYZRGB& in, PointXYZI& out) {
  out.x = in.x; out.y = in.y; out.z = in.z;
  const float r = (float)((in.rgba >> 16) & 255u), g = (float)((in.rgba >> 8) & 255u), b = (float)(in.rgba & 255u);
  out.intensity = 0.299f * r + 0.587f * g + 0.114f * b;
}
inline void PointCloudXYZRGBtoXYZI(const PointCloud<PointXYZRGB>& in, PointCloud<PointXYZI>& out) {
  out.points.resize(in.size());
  out.width = in.width;
  out.height = in.height;
  out.is_dense = in.is_dense;
  for (size_t i = 0; i < in.size(); ++i) PointXYZRGBtoXYZI(in.points[i], out.points[i]);
}

// IntensityGradientEstimation<PointXYZI, Normal, IntensityGradient, IntensityFieldAccessor<PointXYZI>>
// with PCL 1.7's indexing: row i takes the neighbours of input point i in the surface, and the
// normal normals_[i] -- the *surface's* i-th normal (the normals must match the surface, as PCL's
// initCompute demands), so with keypoints as the input (evaluation.cpp:439-445) not the
// keypoint's own.  Without a search surface (tools.h:50-53) the whole-cloud path runs.
template <typename PointInT, typename PointNT, typename PointOutT,
          typename IntensitySelectorT = common::IntensityFieldAccessor<PointInT> >
class IntensityGradientEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<IntensityGradientEstimation<PointInT, PointNT, PointOutT, IntensitySelectorT> > Ptr;
  IntensityGradientEstimation() { this->name_ = "IntensityGradientEstimation"; }
  void setNumberOfThreads(unsigned int) {}

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const PointCloud<PointInT>& surf = this->surface();
    const size_t nq = this->input_->size(), ns = surf.size();
    if (!this->normals_match("the input normals are missing or do not match the search surface")) return;
    if (!this->input_within_surface()) return;  // row i reads normals_[i]
    const bool same = this->input_is_surface();
    const detail::SoA s = detail::soa_xyz(surf), q = same ? detail::SoA() : detail::soa_xyz(*this->input_);
    detail::SoA nrm = detail::soa_normals(*this->normals_);
    nrm.x.resize(nq); nrm.y.resize(nq); nrm.z.resize(nq);
    std::vector<float> si(ns), g(nq * 3);
    IntensitySelectorT intensity;
    for (size_t i = 0; i < ns; ++i) si[i] = intensity(surf.points[i]);
    const detail::SoA& qq = same ? s : q;
    if (!detail::ok(pfx_intensity_gradient(detail::context(), s.x.data(), s.y.data(), s.z.data(), si.data(),
                                           s.n(), qq.x.data(), qq.y.data(), qq.z.data(), nrm.x.data(), nrm.y.data(),
                                           nrm.z.data(), (int64_t)nq, same ? 1 : 0, this->search_radius_, g.data()),
                    "IntensityGradientEstimation"))
      return;
    detail::write_rows<3>(out, nq, detail::NanRule::kFirstFloat, g);
  }
};

// MomentInvariantsEstimation<PointXYZRGB, MomentInvariants> (evaluation.cpp:554-572): a plain Feature,
// so Features<T>::compute's cast (features.h:175-196) computes no normals for it.  Row i is j1 j2 j3
// of the radius neighbours of input point i in the surface; a row without neighbours is NaN.
template <typename PointInT, typename PointOutT>
class MomentInvariantsEstimation : public Feature<PointInT, PointOutT> {
 public:
  typedef std::shared_ptr<MomentInvariantsEstimation<PointInT, PointOutT> > Ptr;
  MomentInvariantsEstimation() { this->name_ = "MomentInvariantsEstimation"; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    std::vector<float> j(q.size() * 3);
    if (!detail::ok(pfx_moment_invariants(detail::context(), s.x.data(), s.y.data(), s.z.data(), s.n(), q.x.data(),
                                          q.y.data(), q.z.data(), q.n(), this->search_radius_, j.data()),
                    "MomentInvariantsEstimation"))
      return;
    detail::write_rows<3>(out, q.size(), detail::NanRule::kAnyFloat, j);
  }
};

// PrincipalCurvaturesEstimation<PointXYZRGB, Normal, PrincipalCurvatures> (evaluation.cpp:696-715): a
// FeatureFromNormals, so Features<T>::compute's cast computes the surface normals for it.  With PCL
// 1.7's indexing: computeFeature passes (*indices_)[i], an index into the *input*, to normals_, the
// *surface's* normals.  So the query normal of row i is the normal of cloud point i, not the
// keypoint's own: the facade passes normals[0 .. nq).  More input points than normals, which PCL
// would read out of bounds, is an error here.
template <typename PointInT, typename PointNT, typename PointOutT>
class PrincipalCurvaturesEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<PrincipalCurvaturesEstimation<PointInT, PointNT, PointOutT> > Ptr;
  PrincipalCurvaturesEstimation() { this->name_ = "PrincipalCurvaturesEstimation"; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    if (!this->normals_match("the input normals are missing or do not match the search surface")) return;
    if (!this->input_within_surface()) return;  // row i reads normals_[i]
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    const detail::SoA nrm = detail::soa_normals(*this->normals_);
    std::vector<float> pc(q.size() * 5);
    // (the query normals are the first nq surface normals: the arrays' own prefixes)
    if (!detail::ok(pfx_principal_curvatures(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(),
                                             nrm.y.data(), nrm.z.data(), s.n(), q.x.data(), q.y.data(), q.z.data(),
                                             nrm.x.data(), nrm.y.data(), nrm.z.data(), q.n(), this->search_radius_,
                                             pc.data()),
                    "PrincipalCurvaturesEstimation"))
      return;
    detail::write_rows<5>(out, q.size(), detail::NanRule::kAnyFloat, pc);
  }
};

// RIFTEstimation<PointXYZI, IntensityGradient, Histogram<32>> with PCL 1.7's indexing:
// `tree_->radiusSearch ((*indices_)[i], ...)` and `cloud.points[p_idx]` both index the search
// *surface*, so row i describes surface_[i], not input point i (the input cloud only sets the number
// of rows): those surface points are the centres passed to pfx_rift.  A caller who wants the
// descriptor at the keypoints calls pfx_rift with them.  A row without neighbours is NaN (PCL
// leaves the previous row's values).
template <typename PointInT, typename GradientT, typename PointOutT>
class RIFTEstimation : public Feature<PointInT, PointOutT> {
 public:
  typedef PointCloud<GradientT> PointCloudGradient;
  typedef typename PointCloudGradient::Ptr PointCloudGradientPtr;
  typedef typename PointCloudGradient::ConstPtr PointCloudGradientConstPtr;
  typedef std::shared_ptr<RIFTEstimation<PointInT, GradientT, PointOutT> > Ptr;
  RIFTEstimation() { this->name_ = "RIFTEstimation"; }
  void setInputGradient(const PointCloudGradientConstPtr& gradient) { gradient_ = gradient; }
  PointCloudGradientConstPtr getInputGradient() const { return gradient_; }
  void setNrDistanceBins(int nr_distance_bins) { nr_distance_bins_ = nr_distance_bins; }
  int getNrDistanceBins() const { return nr_distance_bins_; }
  void setNrGradientBins(int nr_gradient_bins) { nr_gradient_bins_ = nr_gradient_bins; }
  int getNrGradientBins() const { return nr_gradient_bins_; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const PointCloud<PointInT>& surf = this->surface();
    const size_t nq = this->input_->size(), ns = surf.size();
    const int D = nr_distance_bins_, G = nr_gradient_bins_;
    if (!gradient_ || gradient_->size() != ns) {
      PCL_ERROR("[pcl::RIFTEstimation::compute] the input gradient is missing or its size differs from the search "
                "surface's\n");
      return;
    }
    if (!this->input_within_surface()) return;  // row i reads surface_[i]
    if (D < 1 || D > 16 || G < 1 || G > 16 || (size_t)(D * G) != sizeof(PointOutT) / sizeof(float)) {
      PCL_ERROR("[pcl::RIFTEstimation::compute] nr_distance_bins * nr_gradient_bins = %d does not match the "
                "output histogram (each in [1, 16])\n", D * G);
      return;
    }
    const detail::SoA s = detail::soa_xyz(surf);
    std::vector<float> gx(ns), gy(ns), gz(ns), h(nq * (size_t)(D * G));
    for (size_t i = 0; i < ns; ++i) {
      gx[i] = gradient_->points[i].gradient[0];
      gy[i] = gradient_->points[i].gradient[1];
      gz[i] = gradient_->points[i].gradient[2];
    }
    // (the centres are the first nq surface points: the arrays' own prefixes)
    if (!detail::ok(pfx_rift(detail::context(), s.x.data(), s.y.data(), s.z.data(), gx.data(), gy.data(), gz.data(),
                             s.n(), s.x.data(), s.y.data(), s.z.data(), (int64_t)nq, this->search_radius_, D, G,
                             h.data()),
                    "RIFTEstimation"))
      return;
    // (D * G floats a row: the output histogram's own size, as checked above)
    detail::write_rows<sizeof(PointOutT) / sizeof(float)>(out, nq, detail::NanRule::kFirstFloat, h);
  }
  PointCloudGradientConstPtr gradient_;
  int nr_distance_bins_ = 4, nr_gradient_bins_ = 4;
};

// ---- intensity spin images (evaluation.cpp:466-514) --------------------------------------------
// IntensitySpinEstimation<PointXYZI, Histogram<20>> with PCL 1.7's indexing, which is RIFT's:
// `tree_->radiusSearch ((*indices_)[idx], ...)` searches at surface_[idx], so row i describes
// surface_[i], not input point i (the input cloud only sets the number of rows): those surface
// points are the centres passed to pfx_intensity_spin.  A caller who wants the descriptor at the
// keypoints calls pfx_intensity_spin with them.  No normals are read.  A row without neighbours is
// NaN, as PCL's.  sigma == 0 drops the neighbours PCL would write out of bounds (pfx.h).
template <typename PointInT, typename PointOutT>
class IntensitySpinEstimation : public Feature<PointInT, PointOutT> {
 public:
  typedef std::shared_ptr<IntensitySpinEstimation<PointInT, PointOutT> > Ptr;
  IntensitySpinEstimation() { this->name_ = "IntensitySpinEstimation"; }
  void setNrDistanceBins(size_t nr_distance_bins) { nr_distance_bins_ = (int)nr_distance_bins; }
  int getNrDistanceBins() { return nr_distance_bins_; }
  void setNrIntensityBins(size_t nr_intensity_bins) { nr_intensity_bins_ = (int)nr_intensity_bins; }
  int getNrIntensityBins() { return nr_intensity_bins_; }
  void setSmoothingBandwidth(float sigma) { sigma_ = sigma; }
  float getSmoothingBandwidth() { return sigma_; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const PointCloud<PointInT>& surf = this->surface();
    const size_t nq = this->input_->size(), ns = surf.size();
    const int D = nr_distance_bins_, I = nr_intensity_bins_;
    if (!this->input_within_surface()) return;  // row i reads surface_[i]
    if (D < 1 || D > 16 || I < 1 || I > 16 || (size_t)(D * I) != sizeof(PointOutT) / sizeof(float)) {
      PCL_ERROR("[pcl::IntensitySpinEstimation::compute] nr_distance_bins * nr_intensity_bins = %d does not match "
                "the output histogram (each in [1, 16])\n", D * I);
      return;
    }
    const detail::SoA s = detail::soa_xyz(surf);
    const size_t S = (size_t)(D * I);
    std::vector<float> si(ns), h(nq * S);
    for (size_t i = 0; i < ns; ++i) si[i] = surf.points[i].intensity;
    // (the centres are the first nq surface points: the arrays' own prefixes)
    if (!detail::ok(pfx_intensity_spin(detail::context(), s.x.data(), s.y.data(), s.z.data(), si.data(), s.n(),
                                       s.x.data(), s.y.data(), s.z.data(), (int64_t)nq, this->search_radius_, D, I,
                                       sigma_, h.data()),
                    "IntensitySpinEstimation"))
      return;
    // (S floats a row: the output histogram's own size, as checked above)
    detail::write_rows<sizeof(PointOutT) / sizeof(float)>(out, nq, detail::NanRule::kAnyFloat, h);
  }
  int nr_distance_bins_ = 4, nr_intensity_bins_ = 5;
  float sigma_ = 1.0f;
};

// ---- 3D shape contexts (evaluation.cpp:319-371) ------------------------------------------------
namespace detail {
// PCL's initCompute rule of both shape contexts
inline bool sc_radii_ok(const char* who, double radius, double min_radius, double density_radius) {
  if (radius < min_radius || !(min_radius > 0.0) || !(density_radius > 0.0)) {
    PCL_ERROR("[pcl::%s::compute] the search radius (%g) must not be below the minimal radius (%g), and the minimal "
              "and point density (%g) radii must be positive\n", who, radius, min_radius, density_radius);
    return false;
  }
  return true;
}
}  // namespace detail

// ShapeContext3DEstimation<In, Normal, ShapeContext1980>: PCL 1.7's fixed 12 x 11 x 15 bins.  The
// estimator owns its random stream (boost::mt19937 seeded 12345, or from the clock with
// random = true) and never reseeds it: a second compute() continues where the first one stopped,
// three floats per row that has a neighbour.
template <typename PointInT, typename PointNT, typename PointOutT = ShapeContext1980>
class ShapeContext3DEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<ShapeContext3DEstimation<PointInT, PointNT, PointOutT> > Ptr;
  explicit ShapeContext3DEstimation(bool random = false)
      : seed_(random ? static_cast<uint32_t>(std::time(nullptr)) : 12345u) {
    this->name_ = "ShapeContext3DEstimation";
  }
  void setMinimalRadius(double radius) { min_radius_ = radius; }
  double getMinimalRadius() const { return min_radius_; }
  void setPointDensityRadius(double radius) { point_density_radius_ = radius; }
  double getPointDensityRadius() const { return point_density_radius_; }
  size_t getAzimuthBins() const { return 12; }
  size_t getElevationBins() const { return 11; }
  size_t getRadiusBins() const { return 15; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const PointCloud<PointInT>& surf = this->surface();
    if (!detail::sc_radii_ok("ShapeContext3DEstimation", this->search_radius_, min_radius_, point_density_radius_))
      return;
    if (!this->normals_match("the normals are missing or their number (" +
                             std::to_string(this->normals_ ? this->normals_->size() : (size_t)0) +
                             ") differs from the search surface's points (" + std::to_string(surf.size()) +
                             "): a row's frame is the normal at its nearest surface point"))
      return;
    const detail::SoA s = detail::soa_xyz(surf), nrm = detail::soa_normals(*this->normals_);
    const detail::SoA q = detail::soa_xyz(*this->input_);
    const size_t nq = q.size();
    std::vector<float> d(nq * 1980), rf(nq * 9), rnd(nq * 3);
    // drawn ahead: three floats for every row; the rows that draw take them in order
    pfx_rng_uniform01(seed_, stream_pos_, (int64_t)rnd.size(), rnd.data());
    if (!detail::ok(pfx_shape_context(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(),
                                      nrm.y.data(), nrm.z.data(), s.n(), q.x.data(), q.y.data(), q.z.data(), q.n(),
                                      this->search_radius_, min_radius_, point_density_radius_, rnd.data(), d.data(),
                                      rf.data()),
                    "ShapeContext3DEstimation"))
      return;
    int64_t draws = 0;
    if (!detail::ok(pfx_ctx_last_stats(detail::context(), "sc_draws", &draws), "ShapeContext3DEstimation")) return;
    stream_pos_ += 3 * draws;
    detail::write_rows<1980, 9>(out, nq, detail::NanRule::kFirstFloat, d, rf);
  }
  double min_radius_ = 0.1, point_density_radius_ = 0.2;
  uint32_t seed_;
  int64_t stream_pos_ = 0;  // floats of the stream already used
};

// SHOTLocalReferenceFrameEstimation<In, ReferenceFrame>: SHOT's frames alone (a NaN frame where
// fewer than five neighbours define it)
template <typename PointInT, typename PointOutT = ReferenceFrame>
class SHOTLocalReferenceFrameEstimation : public Feature<PointInT, PointOutT> {
 public:
  typedef std::shared_ptr<SHOTLocalReferenceFrameEstimation<PointInT, PointOutT> > Ptr;
  typedef std::shared_ptr<const SHOTLocalReferenceFrameEstimation<PointInT, PointOutT> > ConstPtr;
  SHOTLocalReferenceFrameEstimation() { this->name_ = "SHOTLocalReferenceFrameEstimation"; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    std::vector<float> rf(q.size() * 9);
    if (!detail::ok(pfx_shot_lrf(detail::context(), s.x.data(), s.y.data(), s.z.data(), s.n(), q.x.data(), q.y.data(),
                                 q.z.data(), q.n(), this->search_radius_, rf.data()),
                    "SHOTLocalReferenceFrameEstimation"))
      return;
    // (a ReferenceFrame is its x, y and z axes in a row, as the C-ABI's nine floats are)
    detail::write_rows<9>(out, q.size(), detail::NanRule::kFirstFloat, rf);
  }
};

// BOARDLocalReferenceFrameEstimation<In, Normal, ReferenceFrame> (evaluation.cpp:372-393): the frames
// of pfx_board_lrf, a NaN frame where fewer than six neighbours define it or no normal qualifies.
// Hole analysis (setFindHoles(true)) is not on the accelerated path: PCL seeds it from rand(), and
// compute() fails; its three parameters are kept for the getters.
template <typename PointInT, typename PointNT, typename PointOutT = ReferenceFrame>
class BOARDLocalReferenceFrameEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<BOARDLocalReferenceFrameEstimation<PointInT, PointNT, PointOutT> > Ptr;
  typedef std::shared_ptr<const BOARDLocalReferenceFrameEstimation<PointInT, PointNT, PointOutT> > ConstPtr;
  BOARDLocalReferenceFrameEstimation() {
    this->name_ = "BOARDLocalReferenceFrameEstimation";
    // (PCL's computeFeature refuses a k-search itself, with these words)
    this->k_search_error_ = "[pcl::BOARDLocalReferenceFrameEstimation::computeFeature] Error! Search method set to "
                            "k-neighborhood. Call setKSearch(0) and setRadiusSearch( radius ) to use this class.";
    pfx_board_params_default(&prm_);
  }
  void setTangentRadius(float radius) { prm_.tangent_radius = radius; }
  float getTangentRadius() const { return prm_.tangent_radius; }
  void setFindHoles(bool find_holes) { prm_.find_holes = find_holes ? 1 : 0; }
  bool getFindHoles() const { return prm_.find_holes != 0; }
  void setMarginThresh(float margin_thresh) { prm_.margin_thresh = margin_thresh; }
  float getMarginThresh() const { return prm_.margin_thresh; }
  void setCheckMarginArraySize(int size) { prm_.check_margin_array_size = size; }
  int getCheckMarginArraySize() const { return prm_.check_margin_array_size; }
  void setHoleSizeProbThresh(float prob_thresh) { prm_.hole_size_prob_thresh = prob_thresh; }
  float getHoleSizeProbThresh() const { return prm_.hole_size_prob_thresh; }
  void setSteepThresh(float steep_thresh) { prm_.steep_thresh = steep_thresh; }
  float getSteepThresh() const { return prm_.steep_thresh; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    if (!this->normals_match("the input normals are missing or do not match the search surface")) return;
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    const detail::SoA nrm = detail::soa_normals(*this->normals_);
    std::vector<float> rf(q.size() * 9);
    if (!detail::ok(pfx_board_lrf(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(), nrm.y.data(),
                                  nrm.z.data(), s.n(), q.x.data(), q.y.data(), q.z.data(), q.n(),
                                  this->search_radius_, &prm_, rf.data()),
                    "BOARDLocalReferenceFrameEstimation"))
      return;
    // (a ReferenceFrame is its x, y and z axes in a row, as the C-ABI's nine floats are; a computed
    // row can have NaN x and y axes beside a finite z)
    detail::write_rows<9>(out, q.size(), detail::NanRule::kAnyFloat, rf);
  }
  pfx_board_params prm_;
};

// BoundaryEstimation<In, Normal, Boundary> (evaluation.cpp:394-415): the flags of pfx_boundary.
// PCL 1.7's indexing: the normal of input point i is `normals_->points[(*indices_)[i]]`, that is
// normals_[i], while the reference hands in one normal per point of the search *surface*; a
// keypoint that is not surface point i gets surface point i's normal all the same.  Reproduced: the
// facade passes normals[0 .. nq) as the queries' normals.  More input points than normals, which
// PCL would read out of bounds, is an error here.
// A row without a neighbour (PFX_BOUNDARY_NO_NEIGHBORS) is boundary_point = 0 and is_dense = false:
// PCL assigns quiet_NaN() of uint8_t, which is 0.  There is no KdTreeFLANN<Boundary>: matching on the
// flags is not on this path.
template <typename PointInT, typename PointNT, typename PointOutT = Boundary>
class BoundaryEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<BoundaryEstimation<PointInT, PointNT, PointOutT> > Ptr;
  typedef std::shared_ptr<const BoundaryEstimation<PointInT, PointNT, PointOutT> > ConstPtr;
  BoundaryEstimation() { this->name_ = "BoundaryEstimation"; }
  void setAngleThreshold(float angle) { angle_threshold_ = angle; }
  float getAngleThreshold() const { return angle_threshold_; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    if (!this->normals_match("the input normals are missing or do not match the search surface")) return;
    if (!this->input_within_surface()) return;  // row i reads normals_[i]
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    const detail::SoA nrm = detail::soa_normals(*this->normals_);
    std::vector<uint8_t> flags(q.size());
    // (the query normals are the first nq surface normals: the arrays' own prefixes)
    if (!detail::ok(pfx_boundary(detail::context(), s.x.data(), s.y.data(), s.z.data(), s.n(), q.x.data(), q.y.data(),
                                 q.z.data(), nrm.x.data(), nrm.y.data(), nrm.z.data(), q.n(), this->search_radius_,
                                 angle_threshold_, flags.data()),
                    "BoundaryEstimation"))
      return;
    out.resize(q.size());
    out.is_dense = true;
    for (size_t i = 0; i < q.size(); ++i) {
      const bool none = flags[i] == PFX_BOUNDARY_NO_NEIGHBORS;
      out.points[i].boundary_point = none ? 0 : flags[i];
      if (none) out.is_dense = false;
    }
  }
  float angle_threshold_ = static_cast<float>(M_PI) / 2.0f;
};

// CVFHEstimation<In, Normal, VFHSignature308> (evaluation.cpp:649-675): the rows of pfx_cvfh, one per
// smooth cluster, or one row without a cluster.  A FeatureFromNormals, so the generic wrapper
// (features.h:181-187) estimates the cloud's normals, curvature included.  Two things PCL 1.7 does on
// this path are reproduced:
//   the wrapper calls compute on the Feature base, so Feature::compute runs and CVFH's own compute,
//   which hides it, does not; computeFeature sizes the output to the number of rows;
//   the wrapper sets the cloud as the search surface and the keypoints as the input, so the indices
//   are 0 .. K - 1 and CVFH reads the surface's points and normals at them: it describes the FIRST K
//   POINTS OF THE CLOUD, not the keypoints.  More keypoints than surface points, which PCL would read
//   out of bounds, is PFX_ERR_INVALID.
// The constructor sets k = 1 and no radius, as PCL's: with a radius set, compute() fails as PCL's
// initCompute does until setKSearch(0).  The lists getCentroidClusters / getCentroidNormalClusters
// return are cleared by every compute (PCL 1.7 clears only the first).
template <typename PointInT, typename PointNT, typename PointOutT = VFHSignature308>
class CVFHEstimation : public FeatureFromNormals<PointInT, PointNT, PointOutT> {
 public:
  typedef std::shared_ptr<CVFHEstimation<PointInT, PointNT, PointOutT> > Ptr;
  typedef std::shared_ptr<const CVFHEstimation<PointInT, PointNT, PointOutT> > ConstPtr;
  CVFHEstimation() {
    this->name_ = "CVFHEstimation";
    this->k_ = 1;
    this->search_radius_ = 0.0;
    this->k_search_error_ = "[pcl::CVFHEstimation::initCompute] Both radius and K defined! Set one of them to zero "
                            "first and then re-run compute ().";
    pfx_cvfh_params_default(&prm_);
  }
  void setViewPoint(float vpx, float vpy, float vpz) { prm_.viewpoint[0] = vpx; prm_.viewpoint[1] = vpy; prm_.viewpoint[2] = vpz; }
  void getViewPoint(float& vpx, float& vpy, float& vpz) const { vpx = prm_.viewpoint[0]; vpy = prm_.viewpoint[1]; vpz = prm_.viewpoint[2]; }
  void setRadiusNormals(float radius_normals) { prm_.radius_normals = radius_normals; }
  void setClusterTolerance(float d) { prm_.cluster_tolerance = d; }
  void setEPSAngleThreshold(float d) { prm_.eps_angle_threshold = d; }
  void setCurvatureThreshold(float d) { prm_.curvature_threshold = d; }
  void setMinPoints(size_t min) { prm_.min_points = (int32_t)min; }
  void setNormalizeBins(bool normalize) { prm_.normalize_bins = normalize ? 1 : 0; }
  void getCentroidClusters(std::vector<Eigen::Vector3f>& centroids) const {
    for (const Eigen::Vector3f& c : centroids_) centroids.push_back(c);
  }
  void getCentroidNormalClusters(std::vector<Eigen::Vector3f>& centroids) const {
    for (const Eigen::Vector3f& c : dominant_normals_) centroids.push_back(c);
  }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    centroids_.clear();
    dominant_normals_.clear();
    if (!this->normals_match("the input normals are missing or do not match the search surface")) return;
    const detail::SoA s = detail::soa_xyz(this->surface()), nrm = detail::soa_normals(*this->normals_);
    std::vector<float> curv(s.size());
    for (size_t i = 0; i < curv.size(); ++i) curv[i] = this->normals_->points[i].curvature;
    std::vector<int32_t> indices(this->input_->size());  // Feature::initCompute's: 0 .. K - 1
    for (size_t i = 0; i < indices.size(); ++i) indices[i] = (int32_t)i;
    const int64_t cap = std::max<int64_t>(1, (int64_t)indices.size() / std::max<int32_t>(1, prm_.min_points));
    std::vector<float> rows((size_t)cap * PFX_CVFH_DIM), cen((size_t)cap * 3), dn((size_t)cap * 3);
    int64_t n_rows = 0;
    if (!detail::ok(pfx_cvfh(detail::context(), s.x.data(), s.y.data(), s.z.data(), nrm.x.data(), nrm.y.data(),
                             nrm.z.data(), curv.data(), s.n(), indices.data(), (int64_t)indices.size(), &prm_,
                             rows.data(), cap, &n_rows, cen.data(), dn.data(), nullptr),
                    "CVFHEstimation"))
      return;
    detail::write_rows<PFX_CVFH_DIM>(out, (size_t)n_rows, detail::NanRule::kFirstFloat, rows);
    for (int64_t r = 0; r < n_rows; ++r) {
      centroids_.push_back(Eigen::Vector3f(cen[r * 3], cen[r * 3 + 1], cen[r * 3 + 2]));
      dominant_normals_.push_back(Eigen::Vector3f(dn[r * 3], dn[r * 3 + 1], dn[r * 3 + 2]));
    }
  }
  pfx_cvfh_params prm_;
  std::vector<Eigen::Vector3f> centroids_, dominant_normals_;
};

// UniqueShapeContext<In, ShapeContext1980, ReferenceFrame>.  Without input frames it computes them
// with SHOTLocalReferenceFrameEstimation at the local radius (PCL's default: 2.5) over the search
// surface.  That frame search has SHOT's capacity, 16,384 neighbours: on a cloud where the local
// radius reaches more, compute() fails with that message (set a smaller local radius or frames).
template <typename PointInT, typename PointOutT = ShapeContext1980, typename PointRFT = ReferenceFrame>
class UniqueShapeContext : public Feature<PointInT, PointOutT> {
 public:
  typedef PointCloud<PointRFT> PointCloudLRF;
  typedef typename PointCloudLRF::ConstPtr PointCloudLRFConstPtr;
  typedef std::shared_ptr<UniqueShapeContext<PointInT, PointOutT, PointRFT> > Ptr;
  UniqueShapeContext() { this->name_ = "UniqueShapeContext"; }
  void setMinimalRadius(double radius) { min_radius_ = radius; }
  double getMinimalRadius() const { return min_radius_; }
  void setPointDensityRadius(double radius) { point_density_radius_ = radius; }
  double getPointDensityRadius() const { return point_density_radius_; }
  void setLocalRadius(double radius) { local_radius_ = radius; }
  double getLocalRadius() const { return local_radius_; }
  void setInputReferenceFrames(const PointCloudLRFConstPtr& frames) { frames_ = frames; }
  PointCloudLRFConstPtr getInputReferenceFrames() const { return frames_; }

 protected:
  void computeFeature(PointCloud<PointOutT>& out) override {
    const size_t nq = this->input_->size();
    if (!detail::sc_radii_ok("UniqueShapeContext", this->search_radius_, min_radius_, point_density_radius_)) return;
    if (frames_ && frames_->size() != nq) {
      PCL_ERROR("[pcl::UniqueShapeContext::compute] the number of input reference frames (%zu) differs from the "
                "input cloud's points (%zu)\n", frames_->size(), nq);
      return;
    }
    const detail::SoA s = detail::soa_xyz(this->surface()), q = detail::soa_xyz(*this->input_);
    std::vector<float> fr(nq * 9), d(nq * 1980), rf(nq * 9);
    if (frames_) {
      for (size_t i = 0; i < nq; ++i)
        for (int b = 0; b < 3; ++b) {
          fr[i * 9 + b] = frames_->points[i].x_axis[b];
          fr[i * 9 + 3 + b] = frames_->points[i].y_axis[b];
          fr[i * 9 + 6 + b] = frames_->points[i].z_axis[b];
        }
    } else {
      if (!(local_radius_ > 0.0)) {
        PCL_ERROR("[pcl::UniqueShapeContext::compute] the local radius must be positive\n");
        return;
      }
      const pfx_status st = pfx_shot_lrf(detail::context(), s.x.data(), s.y.data(), s.z.data(), s.n(), q.x.data(),
                                         q.y.data(), q.z.data(), q.n(), local_radius_, fr.data());
      if (st == PFX_ERR_CAPACITY) {
        PCL_ERROR("[pcl::UniqueShapeContext::compute] the reference frames at the local radius %g exceed the frame "
                  "search's capacity of 16384 neighbours (%s): set a smaller local radius with setLocalRadius or "
                  "give frames with setInputReferenceFrames\n", local_radius_, pfx_last_error(detail::context()));
        return;
      }
      if (!detail::ok(st, "UniqueShapeContext")) return;
    }
    if (!detail::ok(pfx_usc(detail::context(), s.x.data(), s.y.data(), s.z.data(), s.n(), q.x.data(), q.y.data(),
                            q.z.data(), fr.data(), q.n(), this->search_radius_, min_radius_, point_density_radius_,
                            d.data(), rf.data()),
                    "UniqueShapeContext"))
      return;
    detail::write_rows<1980, 9>(out, nq, detail::NanRule::kFirstFloat, d, rf);
  }
  double min_radius_ = 0.1, point_density_radius_ = 0.2, local_radius_ = 2.5;
  PointCloudLRFConstPtr frames_;
};

// ---- range image + NARF (keypoints.h:203-224) ---------------------------------------------
class RangeImage : public PointCloud<PointWithRange> {
 public:
  enum CoordinateFrame { CAMERA_FRAME = 0, LASER_FRAME = 1 };
  virtual ~RangeImage() = default;
};

class RangeImagePlanar : public RangeImage {
 public:
  // Keeps the SoA cloud and the camera for the accelerated NARF pass and materialises the
  // range image itself (PointWithRange per pixel, like PCL) through pfx_range_image_planar.
  template <typename PointCloudType>
  void createFromPointCloudWithFixedSize(const PointCloudType& cloud, int di_width, int di_height,
                                         float di_center_x, float di_center_y, float di_focal_length_x,
                                         float di_focal_length_y, const Eigen::Affine3f& sensor_pose,
                                         CoordinateFrame coordinate_frame = CAMERA_FRAME,
                                         float noise_level = 0.0f, float min_range = 0.0f) {
    cloud_ = detail::soa_xyz(cloud);
    pfx_camera_default(&cam_);
    cam_.width = di_width; cam_.height = di_height;
    cam_.center_x = di_center_x; cam_.center_y = di_center_y;
    cam_.focal_length_x = di_focal_length_x; cam_.focal_length_y = di_focal_length_y;
    for (int i = 0; i < 16; ++i) cam_.sensor_pose[i] = sensor_pose.m[i];
    cam_.coordinate_frame = (int32_t)coordinate_frame;
    cam_.noise_level = noise_level;
    cam_.min_range = min_range;
    width = (uint32_t)di_width;
    height = (uint32_t)di_height;
    points.clear();
    if (!detail::context()) return;
    std::vector<float> pr((size_t)di_width * di_height * 4);
    if (!detail::ok(pfx_range_image_planar(detail::context(), cloud_.x.data(), cloud_.y.data(), cloud_.z.data(),
                                           (int64_t)cloud_.x.size(), &cam_, pr.data()),
                    "RangeImagePlanar"))
      return;
    points.resize((size_t)di_width * di_height);
    for (size_t i = 0; i < points.size(); ++i) {
      points[i].x = pr[4 * i]; points[i].y = pr[4 * i + 1]; points[i].z = pr[4 * i + 2];
      points[i].range = pr[4 * i + 3];
    }
    is_dense = false;
  }
  const detail::SoA& source_cloud() const { return cloud_; }
  const pfx_camera& camera() const { return cam_; }

 private:
  detail::SoA cloud_;
  pfx_camera cam_;
};

class RangeImageBorderExtractor {
 public:
  struct Parameters {
    int pixel_radius_borders = 3;
    int pixel_radius_plane_extraction = 2;
    int pixel_radius_border_direction = 2;
    float minimum_border_probability = 0.8f;
    int pixel_radius_principal_curvature = 2;
  };
  explicit RangeImageBorderExtractor(const RangeImage* = nullptr) {}
  Parameters& getParameters() { return parameters_; }

 private:
  Parameters parameters_;
};

class NarfKeypoint {
 public:
  struct Parameters {
    float support_size = -1.0f;
    int max_no_of_interest_points = -1;
    float min_distance_between_interest_points = 0.25f;
    float optimal_distance_to_high_surface_change = 0.25f;
    float min_interest_value = 0.45f;
    float min_surface_change_score = 0.2f;
    int optimal_range_image_patch_size = 10;
    float distance_for_additional_points = 0.0f;
    bool add_points_on_straight_edges = false;
    bool do_non_maximum_suppression = true;
    int no_of_polynomial_approximations_per_point = 0;
    int max_no_of_threads = 1;
    bool use_recursive_scale_reduction = false;
    // PCL's default (true).  Both values compute the COMPLETE interest formula here (true only
    // prunes pixels that cannot reach min_interest_value: same keypoints); PCL 1.7's sparse
    // heuristics are not reproduced -- unpinned, measured sensitivity 1-2 keypoints per reference
    // cloud (pfx.h)
    bool calculate_sparse_interest_image = true;
  };
  explicit NarfKeypoint(RangeImageBorderExtractor* border_extractor = nullptr, float support_size = -1.0f)
      : border_extractor_(border_extractor) {
    parameters_.support_size = support_size;
  }
  void setRangeImage(const RangeImage* range_image) {
    range_image_ = dynamic_cast<const RangeImagePlanar*>(range_image);
  }
  Parameters& getParameters() { return parameters_; }
  // NarfKeypoint::compute: ascending pixel indices of the keypoints
  void compute(PointCloud<int>& out) {
    out.clear();
    if (!range_image_ || !(parameters_.support_size > 0.0f)) {
      PCL_ERROR("[pcl::NarfKeypoint::compute] needs a RangeImagePlanar and support_size > 0\n");
      return;
    }
    if (!detail::context()) return;
    pfx_narf_params p;
    pfx_narf_params_default(&p);
    p.support_size = parameters_.support_size;
    p.max_no_of_interest_points = parameters_.max_no_of_interest_points;
    p.min_distance_between_interest_points = parameters_.min_distance_between_interest_points;
    p.optimal_distance_to_high_surface_change = parameters_.optimal_distance_to_high_surface_change;
    p.min_interest_value = parameters_.min_interest_value;
    p.min_surface_change_score = parameters_.min_surface_change_score;
    p.do_non_maximum_suppression = parameters_.do_non_maximum_suppression ? 1 : 0;
    p.calculate_sparse_interest_image = parameters_.calculate_sparse_interest_image ? 1 : 0;
    p.no_of_polynomial_approximations_per_point = parameters_.no_of_polynomial_approximations_per_point ? 1 : 0;
    p.add_points_on_straight_edges = parameters_.add_points_on_straight_edges ? 1 : 0;
    if (border_extractor_) {
      const RangeImageBorderExtractor::Parameters& b = border_extractor_->getParameters();
      p.pixel_radius_borders = b.pixel_radius_borders;
      p.pixel_radius_plane_extraction = b.pixel_radius_plane_extraction;
      p.pixel_radius_border_direction = b.pixel_radius_border_direction;
      p.minimum_border_probability = b.minimum_border_probability;
      p.pixel_radius_principal_curvature = b.pixel_radius_principal_curvature;
    }
    const detail::SoA& c = range_image_->source_cloud();
    const pfx_camera cam = range_image_->camera();
    std::vector<int32_t> idx((size_t)cam.width * cam.height);
    int64_t k = 0;
    if (!detail::ok(pfx_narf_keypoints(detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)c.x.size(),
                                       &cam, &p, idx.data(), (int64_t)idx.size(), &k),
                    "NarfKeypoint"))
      return;
    out.points.assign(idx.begin(), idx.begin() + k);
    out.width = (uint32_t)k;
    out.height = 1;
  }

 private:
  RangeImageBorderExtractor* border_extractor_;
  const RangeImagePlanar* range_image_ = nullptr;
  Parameters parameters_;
};

// ---- NARF descriptors (evaluation.cpp:613-648) ------------------------------------------------
// NarfDescriptor (range image, indices): compute() -> one Narf36 per rotation of every index
// (pfx_narf_descriptors on the cloud and camera the RangeImagePlanar keeps; the indices are PIXEL
// indices y * width + x, whatever the caller took them from).  With rotation_invariant an index
// gives 0 to 5 rows, so the rows are not one per index: getRowIndices() says which entry of the
// index vector each row came from.  A row's x, y, z and roll, pitch, yaw are those of the inverse of
// its pose (Narf::copyToNarf36: the patch's frame in the world).  A missing range image or index
// vector, support_size <= 0: PCL_ERROR and an empty output.
class NarfDescriptor {
 public:
  struct Parameters {
    float support_size = -1.0f;
    bool rotation_invariant = true;
  };
  explicit NarfDescriptor(const RangeImage* range_image = nullptr, const std::vector<int>* indices = nullptr) {
    setRangeImage(range_image, indices);
  }
  void setRangeImage(const RangeImage* range_image, const std::vector<int>* indices = nullptr) {
    range_image_ = dynamic_cast<const RangeImagePlanar*>(range_image);
    indices_ = indices;
  }
  Parameters& getParameters() { return parameters_; }
  const std::vector<int>& getRowIndices() const { return row_keys_; }
  void compute(PointCloud<Narf36>& out) {
    out.clear();
    row_keys_.clear();
    if (!range_image_ || !indices_ || !(parameters_.support_size > 0.0f)) {
      PCL_ERROR("[pcl::NarfDescriptor::compute] needs a RangeImagePlanar, an index vector and support_size > 0\n");
      return;
    }
    if (!detail::context()) return;
    pfx_narf_desc_params p;
    pfx_narf_desc_params_default(&p);
    p.support_size = parameters_.support_size;
    p.rotation_invariant = parameters_.rotation_invariant ? 1 : 0;
    const detail::SoA& c = range_image_->source_cloud();
    const pfx_camera cam = range_image_->camera();
    const std::vector<int32_t> pix(indices_->begin(), indices_->end());
    const int64_t cap = 5 * (int64_t)pix.size();
    std::vector<float> desc((size_t)cap * 36), pose((size_t)cap * 12);
    std::vector<int32_t> key((size_t)cap);
    int64_t m = 0;
    if (!detail::ok(pfx_narf_descriptors(detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)c.x.size(), &cam,
                                         pix.data(), (int64_t)pix.size(), &p, desc.data(), pose.data(), key.data(), cap,
                                         &m),
                    "NarfDescriptor"))
      return;
    out.points.resize((size_t)m);
    for (int64_t r = 0; r < m; ++r) {
      const float* a = &pose[(size_t)r * 12];  // [R | t]; its inverse: R^T, -(R^T t)
      Narf36& o = out.points[(size_t)r];
      o.x = -((a[0] * a[3] + a[4] * a[7]) + a[8] * a[11]);
      o.y = -((a[1] * a[3] + a[5] * a[7]) + a[9] * a[11]);
      o.z = -((a[2] * a[3] + a[6] * a[7]) + a[10] * a[11]);
      // getEulerAngles of the inverse's rotation m = R^T: atan2 (m21, m22), asin (-m20), atan2 (m10, m00)
      o.roll = std::atan2(a[6], a[10]);
      o.pitch = std::asin(-a[2]);
      o.yaw = std::atan2(a[1], a[0]);
      for (int k = 0; k < 36; ++k) o.descriptor[k] = desc[(size_t)r * 36 + k];
    }
    row_keys_.assign(key.begin(), key.begin() + m);
    out.width = (uint32_t)m;
    out.height = 1;
  }

 private:
  const RangeImagePlanar* range_image_ = nullptr;
  const std::vector<int>* indices_ = nullptr;
  Parameters parameters_;
  std::vector<int> row_keys_;
};

// ---- ISS keypoints (keypoints.h:177-189) ------------------------------------------------------
// ISSKeypoint3D<In, Out, NormalT>: the reference's setters, compute() -> the keypoints' xyz in
// index order (pfx_iss_keypoints; PCL pushes them from an OpenMP loop).  A
// parameter initCompute rejects (radius, threshold or min neighbours <= 0) -> PCL_ERROR and an
// empty output.  Border radius / normals are not on the accelerated path (the reference sets
// neither).
template <typename PointInT, typename PointOutT, typename NormalT = Normal>
class ISSKeypoint3D {
 public:
  typedef typename PointCloud<PointInT>::ConstPtr PointCloudInConstPtr;
  typedef typename search::KdTree<PointInT>::Ptr KdTreePtr;
  explicit ISSKeypoint3D(double salient_radius = 0.0001) : salient_radius_(salient_radius) {}
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  void setSalientRadius(double r) { salient_radius_ = r; }
  void setNonMaxRadius(double r) { non_max_radius_ = r; }
  void setMinNeighbors(int k) { min_neighbors_ = k; }
  void setThreshold21(double t) { gamma_21_ = t; }
  void setThreshold32(double t) { gamma_32_ = t; }
  const std::vector<int>& getKeypointsIndices() const { return indices_; }
  void compute(PointCloud<PointOutT>& output) {
    output.clear();
    indices_.clear();
    if (!input_) {
      PCL_ERROR("[pcl::ISSKeypoint3D::compute] no input cloud\n");
      return;
    }
    if (!detail::context()) return;
    const detail::SoA c = detail::soa_xyz(*input_);
    std::vector<int32_t> idx(c.x.size() + 1);
    int64_t k = 0;
    if (!detail::ok(pfx_iss_keypoints(detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)c.x.size(),
                                      salient_radius_, non_max_radius_, min_neighbors_, gamma_21_, gamma_32_,
                                      idx.data(), (int64_t)idx.size(), &k, nullptr),
                    "ISSKeypoint3D"))
      return;
    for (int64_t j = 0; j < k; ++j) {
      PointOutT p;
      p.x = input_->points[idx[j]].x;
      p.y = input_->points[idx[j]].y;
      p.z = input_->points[idx[j]].z;
      output.push_back(p);
      indices_.push_back(idx[j]);
    }
  }

 private:
  PointCloudInConstPtr input_;
  KdTreePtr tree_;
  double salient_radius_, non_max_radius_ = 0.0, gamma_21_ = 0.975, gamma_32_ = 0.975;
  int min_neighbors_ = 5;
  std::vector<int> indices_;
};

// ---- UniformSampling (keypoints.h:274-290) -----------------------------------------------------
// UniformSampling<In>: setRadiusSearch, setInputCloud, compute(PointCloud<int>&) -> the cloud
// indices of one keypoint per occupied voxel (pfx_uniform_sampling), in ascending leaf index where
// PCL emits them in the iteration order of a boost::unordered_map (the same set; DESIGN.md "Uniform
// sampling: the contract").  setSearchMethod is accepted and unused: PCL builds a tree it never
// queries.  No radius set, no input, or a status other than success (a radius PCL's leaf size
// cannot take, more cells than an int indexes) -> PCL_ERROR and an empty output.
template <typename PointInT>
class UniformSampling {
 public:
  typedef typename PointCloud<PointInT>::ConstPtr PointCloudInConstPtr;
  typedef typename search::KdTree<PointInT>::Ptr KdTreePtr;
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setSearchMethod(const KdTreePtr& tree) { tree_ = tree; }
  void setRadiusSearch(double radius) { search_radius_ = radius; }
  double getRadiusSearch() const { return search_radius_; }
  void compute(PointCloud<int>& output) {
    output.clear();
    output.is_dense = true;
    if (!input_) {
      PCL_ERROR("[pcl::UniformSampling::compute] no input cloud\n");
      return;
    }
    if (search_radius_ == 0.0) {
      PCL_ERROR("[pcl::UniformSampling::compute] no radius set (setRadiusSearch)\n");
      return;
    }
    if (!detail::context()) return;
    const detail::SoA c = detail::soa_xyz(*input_);
    std::vector<int32_t> idx(c.size() + 1);
    int64_t k = 0;
    if (!detail::ok(pfx_uniform_sampling(detail::context(), c.x.data(), c.y.data(), c.z.data(), c.n(), search_radius_,
                                         idx.data(), (int64_t)idx.size(), &k, nullptr),
                    "UniformSampling"))
      return;
    output.points.assign(idx.begin(), idx.begin() + k);
    output.width = (uint32_t)k;
    output.height = 1;
  }

 private:
  PointCloudInConstPtr input_;
  KdTreePtr tree_;
  double search_radius_ = 0.0;
};

// Keypoints::computeCloudResolution (keypoints.h:401-428) is the reference's own helper; its
// body becomes this call (same value: see DESIGN.md, F3)
template <typename PointT>
inline double cloudResolution(const typename PointCloud<PointT>::ConstPtr& cloud) {
  if (!cloud || !detail::context()) return 0.0;
  const detail::SoA c = detail::soa_xyz(*cloud);
  double res = 0.0;
  if (!detail::ok(pfx_cloud_resolution(detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)c.x.size(),
                                       &res),
                  "computeCloudResolution"))
    return 0.0;
  return res;
}

// ---- HarrisKeypoint3D / HarrisKeypoint6D (keypoints.h:150-176) --------------------------------
// compute(): the corners as PCL outputs them -- refined position, intensity = the response of
// the corner's own point -- in corner (index) order (PCL: omp critical order).
// Only the reference's configuration is accelerated: method HARRIS (3D) with non-maximum
// suppression; anything else -> PCL_ERROR + empty output.  The radius defaults to PCL's 0.01.
namespace detail {
template <typename PointOutT, typename PointInT>
inline void harris_output(const PointCloud<PointInT>& in, const std::vector<float>& resp,
                          const std::vector<float>& corners, const std::vector<int32_t>& cidx, int64_t nc,
                          PointCloud<PointOutT>& out) {
  for (int64_t c = 0; c < nc; ++c) {
    PointOutT p;
    p.x = corners[3 * c];
    p.y = corners[3 * c + 1];
    p.z = corners[3 * c + 2];
    p.intensity = resp[(size_t)cidx[c]];
    out.push_back(p);
  }
  (void)in;
  out.is_dense = true;
}
}  // namespace detail

template <typename PointInT, typename PointOutT, typename NormalT = Normal>
class HarrisKeypoint3D {
 public:
  typedef typename PointCloud<PointInT>::ConstPtr PointCloudInConstPtr;
  enum ResponseMethod { HARRIS = 1, NOBLE, LOWE, TOMASI, CURVATURE };
  explicit HarrisKeypoint3D(ResponseMethod method = HARRIS, float radius = 0.01f, float threshold = 0.0f)
      : method_(method), radius_(radius), threshold_(threshold) {}
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setMethod(ResponseMethod m) { method_ = m; }
  void setRadius(float r) { radius_ = r; }
  void setRadiusSearch(double r) { radius_ = (float)r; }
  void setThreshold(float t) { threshold_ = t; }
  void setNonMaxSupression(bool b) { nonmax_ = b; }
  void setRefine(bool b) { refine_ = b; }
  void compute(PointCloud<PointOutT>& output) {
    output.clear();
    if (!input_) {
      PCL_ERROR("[pcl::HarrisKeypoint3D::compute] no input cloud\n");
      return;
    }
    if (method_ != HARRIS || !nonmax_) {
      PCL_ERROR("[pcl::HarrisKeypoint3D::compute] only method HARRIS with non-maximum suppression is accelerated\n");
      return;
    }
    if (!detail::context()) return;
    const detail::SoA c = detail::soa_xyz(*input_);
    const size_t n = c.x.size();
    std::vector<int32_t> idx(n + 1), cidx(n + 1);
    std::vector<float> resp(n + 1), corners(3 * (n + 1));
    int64_t k = 0, nc = 0;
    if (!detail::ok(pfx_harris3d_keypoints(detail::context(), c.x.data(), c.y.data(), c.z.data(), (int64_t)n, radius_,
                                           threshold_, 1, refine_ ? 1 : 0, idx.data(), (int64_t)n + 1, &k, resp.data(),
                                           corners.data(), &nc, cidx.data()),
                    "HarrisKeypoint3D"))
      return;
    detail::harris_output(*input_, resp, corners, cidx, nc, output);
  }

 private:
  PointCloudInConstPtr input_;
  ResponseMethod method_;
  float radius_, threshold_;
  bool nonmax_ = false, refine_ = true;
};

// HarrisKeypoint6D<PointXYZRGB, ...>: the colour intensity comes from the points' rgb field
template <typename PointInT, typename PointOutT, typename NormalT = Normal>
class HarrisKeypoint6D {
 public:
  typedef typename PointCloud<PointInT>::ConstPtr PointCloudInConstPtr;
  explicit HarrisKeypoint6D(float radius = 0.01f, float threshold = 0.0f) : radius_(radius), threshold_(threshold) {}
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setRadius(float r) { radius_ = r; }
  void setRadiusSearch(double r) { radius_ = (float)r; }
  void setThreshold(float t) { threshold_ = t; }
  void setNonMaxSupression(bool b) { nonmax_ = b; }
  void setRefine(bool b) { refine_ = b; }
  void compute(PointCloud<PointOutT>& output) {
    output.clear();
    if (!input_) {
      PCL_ERROR("[pcl::HarrisKeypoint6D::compute] no input cloud\n");
      return;
    }
    if (!nonmax_) {
      PCL_ERROR("[pcl::HarrisKeypoint6D::compute] only non-maximum suppression is accelerated\n");
      return;
    }
    if (!detail::context()) return;
    const detail::SoA c = detail::soa_xyz(*input_);
    const size_t n = c.x.size();
    std::vector<uint32_t> rgb(n + 1);
    for (size_t i = 0; i < n; ++i) rgb[i] = input_->points[i].rgba & 0x00ffffffu;
    std::vector<int32_t> idx(n + 1), cidx(n + 1);
    std::vector<float> resp(n + 1), corners(3 * (n + 1));
    int64_t k = 0, nc = 0;
    if (!detail::ok(pfx_harris6d_keypoints(detail::context(), c.x.data(), c.y.data(), c.z.data(), rgb.data(),
                                           (int64_t)n, radius_, threshold_, 1, refine_ ? 1 : 0, idx.data(),
                                           (int64_t)n + 1, &k, resp.data(), corners.data(), &nc, nullptr, cidx.data()),
                    "HarrisKeypoint6D"))
      return;
    detail::harris_output(*input_, resp, corners, cidx, nc, output);
  }

 private:
  PointCloudInConstPtr input_;
  float radius_, threshold_;
  bool nonmax_ = false, refine_ = true;
};

// ---- descriptor matching (features.h:224-273) ------------------------------------------------
struct Correspondence {
  int index_query = 0;
  int index_match = -1;
  float distance = std::numeric_limits<float>::max();
  Correspondence() = default;
  Correspondence(int q, int m, float d) : index_query(q), index_match(m), distance(d) {}
};
typedef std::vector<Correspondence> Correspondences;
typedef std::shared_ptr<Correspondences> CorrespondencesPtr;
typedef std::shared_ptr<const Correspondences> CorrespondencesConstPtr;

namespace detail {
// DefaultFeatureRepresentation: the compared floats of a descriptor and the point stride
template <typename T> struct DescriptorLayout;
template <> struct DescriptorLayout<FPFHSignature33> { static constexpr int dim = 33, stride = 33; };
template <> struct DescriptorLayout<SHOT352> { static constexpr int dim = 352, stride = 361; };
template <> struct DescriptorLayout<SHOT1344> { static constexpr int dim = 1344, stride = 1353; };
template <> struct DescriptorLayout<ShapeContext1980> { static constexpr int dim = 1980, stride = 1989; };
template <> struct DescriptorLayout<PFHSignature125> { static constexpr int dim = 125, stride = 125; };
template <> struct DescriptorLayout<VFHSignature308> { static constexpr int dim = 308, stride = 308; };
template <int N> struct DescriptorLayout<Histogram<N> > { static constexpr int dim = N, stride = N; };
// (DefaultPointRepresentation<IntensityGradient>: the three gradient floats of a 16-byte point)
template <> struct DescriptorLayout<IntensityGradient> { static constexpr int dim = 3, stride = 4; };
template <> struct DescriptorLayout<MomentInvariants> { static constexpr int dim = 3, stride = 3; };
// (DefaultPointRepresentation caps a point type it does not know at its first three floats: the
// principal direction alone is compared)
template <> struct DescriptorLayout<PrincipalCurvatures> { static constexpr int dim = 3, stride = 5; };
// (the same rule for the nine floats of a ReferenceFrame: the x axis alone is compared)
template <> struct DescriptorLayout<ReferenceFrame> { static constexpr int dim = 3, stride = 9; };
// (Narf36's representation: the 36 descriptor floats behind x, y, z, roll, pitch, yaw)
template <> struct DescriptorLayout<Narf36> { static constexpr int dim = 36, stride = 42, offset = 6; };
// the float of a point the descriptor starts at: a layout's `offset`, 0 for a layout without one
template <typename L, typename = void> struct LayoutOffset { static constexpr int value = 0; };
template <typename L> struct LayoutOffset<L, decltype((void)L::offset)> { static constexpr int value = L::offset; };
}  // namespace detail

// KdTreeFLANN<FeatureT> with nearestKSearch(k = 1), as the reference uses it (features.h:258-272):
// exact 1-NN under FLANN's L2_Simple on the GPU (pfx_nearest_descriptors).  The reference asks
// one source row at a time; the first query of a source cloud answers all its rows in one GPU
// pass and the following calls read that batch (the cloud must not change in between, as with
// the reference's loop).  A row without a match (non-finite values: undefined in FLANN) returns
// 0 neighbours with k_indices = {0}, which the mutual check of findCorrespondences rejects
// (target rows never match a non-finite source row).
template <typename PointT>
class KdTreeFLANN {
 public:
  typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;
  typedef std::shared_ptr<KdTreeFLANN<PointT> > Ptr;
  explicit KdTreeFLANN(bool sorted = true) : sorted_(sorted) {}
  void setInputCloud(const PointCloudConstPtr& cloud) {
    target_ = cloud;
    batch_src_ = nullptr;
  }
  int nearestKSearch(const PointCloud<PointT>& cloud, int index, int k, std::vector<int>& k_indices,
                     std::vector<float>& k_sqr_distances) const {
    if (k != 1 || !target_ || index < 0 || (size_t)index >= cloud.size()) {
      PCL_ERROR("[pcl::KdTreeFLANN::nearestKSearch] only k = 1 over a set input cloud is accelerated\n");
      return 0;
    }
    if (batch_src_ != &cloud || batch_n_ != cloud.size()) {
      idx_.assign(cloud.size(), -1);
      dist_.assign(cloud.size(), detail::nanf());
      std::lock_guard<std::mutex> lock(detail::context_mutex());
      typedef detail::DescriptorLayout<PointT> L;
      constexpr int offset = detail::LayoutOffset<L>::value;
      if (!detail::context() ||
          !detail::ok(pfx_nearest_descriptors(detail::context(),
                                              reinterpret_cast<const float*>(cloud.points.data()) + offset,
                                              (int64_t)cloud.size(), L::stride,
                                              reinterpret_cast<const float*>(target_->points.data()) + offset,
                                              (int64_t)target_->size(), L::stride, L::dim, idx_.data(), dist_.data()),
                      "KdTreeFLANN"))
        idx_.assign(cloud.size(), -1);
      batch_src_ = &cloud;
      batch_n_ = cloud.size();
    }
    k_indices.assign(1, idx_[index] < 0 ? 0 : idx_[index]);
    k_sqr_distances.assign(1, dist_[index]);
    return idx_[index] < 0 ? 0 : 1;
  }
  int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
    PointCloud<PointT> one;
    one.push_back(point);
    KdTreeFLANN<PointT> tmp;
    tmp.setInputCloud(target_);
    return tmp.nearestKSearch(one, 0, k, k_indices, k_sqr_distances);
  }

 private:
  bool sorted_;
  PointCloudConstPtr target_;
  mutable const PointCloud<PointT>* batch_src_ = nullptr;
  mutable size_t batch_n_ = 0;
  mutable std::vector<int32_t> idx_;
  mutable std::vector<float> dist_;
};

// KdTreeFLANN over a point cloud (Keypoints::getKeypointsCloud, keypoints.h:374-392): exact
// nearestKSearch(k = 1) as radius searches on the GPU (pfx_radius_search) over a growing ball --
// the first non-empty ball holds the nearest point, the first entry of FLANN's (d2, index) order.
// 2 <= k <= PFX_KNN_MAX_K: pfx_knn_search, the min(k, finite points) smallest (d2, index) in that
// order (exact d2 ties by index, DESIGN.md "k-NN: the contract"); returns their number.
template <>
class KdTreeFLANN<PointXYZRGB> {
 public:
  typedef PointCloud<PointXYZRGB>::ConstPtr PointCloudConstPtr;
  explicit KdTreeFLANN(bool sorted = true) : sorted_(sorted) {}
  void setInputCloud(const PointCloudConstPtr& cloud) {
    target_ = cloud;
    soa_ = cloud ? detail::soa_xyz(*cloud) : detail::SoA();
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < soa_.x.size(); ++i) {
      const float p[3] = {soa_.x[i], soa_.y[i], soa_.z[i]};
      if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
      for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], p[d]); hi[d] = std::max(hi[d], p[d]); }
    }
    extent_ = 0.0;
    for (int d = 0; d < 3; ++d) extent_ = std::max(extent_, (double)hi[d] - (double)lo[d]);
  }
  int nearestKSearch(const PointXYZRGB& point, int k, std::vector<int>& k_indices,
                     std::vector<float>& k_sqr_distances) const {
    k_indices.clear();
    k_sqr_distances.clear();
    if (k < 1 || k > PFX_KNN_MAX_K || !target_ || soa_.x.empty()) {
      if (k < 1 || k > PFX_KNN_MAX_K)
        PCL_ERROR("[pcl::KdTreeFLANN::nearestKSearch] k must be in [1, %d]\n", PFX_KNN_MAX_K);
      return 0;
    }
    if (!(std::isfinite(point.x) && std::isfinite(point.y) && std::isfinite(point.z)) || !detail::context())
      return 0;
    std::lock_guard<std::mutex> lock(detail::context_mutex());
    const float qx = point.x, qy = point.y, qz = point.z;
    if (k > 1) {
      int64_t cnt = 0;
      std::vector<int32_t> idx(k);
      std::vector<float> d2(k);
      if (!detail::ok(pfx_knn_search(detail::context(), soa_.x.data(), soa_.y.data(), soa_.z.data(),
                                     (int64_t)soa_.x.size(), &qx, &qy, &qz, 1, k, &cnt, idx.data(), d2.data()),
                      "KdTreeFLANN"))
        return 0;
      k_indices.assign(idx.begin(), idx.begin() + cnt);
      k_sqr_distances.assign(d2.begin(), d2.begin() + cnt);
      return (int)cnt;
    }
    // the ball must reach the farthest point of the cloud's box: its diagonal from any point in it
    const double limit = 4.0 * (extent_ + std::fabs((double)qx) + std::fabs((double)qy) + std::fabs((double)qz)) + 1.0;
    for (double r = 0.01; r <= limit; r *= 4.0) {
      int64_t cnt = 0;
      int32_t idx = -1;
      float d2 = 0.f;
      if (!detail::ok(pfx_radius_search(detail::context(), soa_.x.data(), soa_.y.data(), soa_.z.data(),
                                        (int64_t)soa_.x.size(), &qx, &qy, &qz, 1, r, &cnt, &idx, &d2, 1),
                      "KdTreeFLANN"))
        return 0;
      if (cnt > 0) {
        k_indices.assign(1, idx);
        k_sqr_distances.assign(1, d2);
        return 1;
      }
    }
    return 0;
  }

 private:
  bool sorted_;
  PointCloudConstPtr target_;
  detail::SoA soa_;
  double extent_ = 0.0;
};

// ---- RANSAC correspondence rejection (features.h:282-297) -------------------------------------
namespace registration {
// CorrespondenceRejectorSampleConsensus<PointT>: PCL's fixed-seed sample sequence and adaptive
// stop, every hypothesis scored on the GPU (pfx_ransac_rejector)
template <typename PointT>
class CorrespondenceRejectorSampleConsensus {
 public:
  typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;
  void setInputSource(const PointCloudConstPtr& c) { source_ = c; }
  void setInputTarget(const PointCloudConstPtr& c) { target_ = c; }
  void setInputCorrespondences(const CorrespondencesConstPtr& c) { input_ = c; }
  void setInlierThreshold(double t) { threshold_ = t; }
  void setMaximumIterations(int n) { max_iterations_ = n; }
  double getInlierThreshold() const { return threshold_; }
  int getMaximumIterations() const { return max_iterations_; }
  Eigen::Matrix4f getBestTransformation() const { return best_; }
  // CorrespondenceRejector::getCorrespondences -> applyRejection(correspondences)
  void getCorrespondences(Correspondences& out) {
    out.clear();
    best_.setIdentity();
    if (!input_ || !source_ || !target_) {
      PCL_ERROR("[pcl::registration::CorrespondenceRejectorSampleConsensus::getCorrespondences] no input\n");
      return;
    }
    getRemainingCorrespondences(*input_, out);
  }
  void getRemainingCorrespondences(const Correspondences& original, Correspondences& remaining) {
    remaining.clear();
    best_.setIdentity();
    if (!source_ || !target_ || !detail::context()) return;
    const detail::SoA s = detail::soa_xyz(*source_), t = detail::soa_xyz(*target_);
    const size_t n = original.size();
    std::vector<int32_t> q(n + 1), m(n + 1), keep(n + 1);
    for (size_t i = 0; i < n; ++i) {
      q[i] = original[i].index_query;
      m[i] = original[i].index_match;
    }
    int64_t nk = 0;
    float T[16];
    std::lock_guard<std::mutex> lock(detail::context_mutex());
    if (!detail::ok(pfx_ransac_rejector(detail::context(), s.x.data(), s.y.data(), s.z.data(), (int64_t)s.x.size(),
                                        t.x.data(), t.y.data(), t.z.data(), (int64_t)t.x.size(), q.data(), m.data(),
                                        (int64_t)n, threshold_, max_iterations_, keep.data(), &nk, T),
                    "CorrespondenceRejectorSampleConsensus"))
      return;
    for (int64_t j = 0; j < nk; ++j) remaining.push_back(original[(size_t)keep[j]]);
    for (int i = 0; i < 16; ++i) best_.m[i] = T[i];
  }

 private:
  PointCloudConstPtr source_, target_;
  CorrespondencesConstPtr input_;
  double threshold_ = 0.05;
  int max_iterations_ = 1000;
  Eigen::Matrix4f best_;
};
}  // namespace registration

// ---- ICP alignment (evaluation.cpp:863-885, 257) ------------------------------------------------
// transformPointCloud(in, out, Matrix4f): every finite point under the affine part of the matrix,
// ((R_i0 x + R_i1 y) + R_i2 z) + t_i in float (on a target with fused multiply-add, build with
// -ffp-contract=off to keep this order); the other fields are copied
template <typename PointT>
inline void transformPointCloud(const PointCloud<PointT>& in, PointCloud<PointT>& out, const Eigen::Matrix4f& T) {
  if (&in != &out) out = in;
  for (auto& p : out.points) {
    if (!(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) continue;
    const float x = p.x, y = p.y, z = p.z;
    p.x = ((T(0, 0) * x + T(0, 1) * y) + T(0, 2) * z) + T(0, 3);
    p.y = ((T(1, 0) * x + T(1, 1) * y) + T(1, 2) * z) + T(1, 3);
    p.z = ((T(2, 0) * x + T(2, 1) * y) + T(2, 2) * z) + T(2, 3);
  }
}

// IterativeClosestPoint<PointSource, PointTarget>: PCL 1.7.2's defaults (no reciprocal
// correspondences, no rejectors, Umeyama's fit, DefaultConvergenceCriteria), the whole loop on the
// GPU (pfx_icp).  The RANSAC outlier threshold is stored and unused, as in PCL's align().
template <typename PointSource, typename PointTarget, typename Scalar = float>
class IterativeClosestPoint {
 public:
  typedef PointCloud<PointSource> PointCloudSource;
  typedef PointCloud<PointTarget> PointCloudTarget;
  typedef typename PointCloudSource::ConstPtr PointCloudSourceConstPtr;
  typedef typename PointCloudTarget::ConstPtr PointCloudTargetConstPtr;
  IterativeClosestPoint() { pfx_icp_params_default(&params_); }
  void setInputSource(const PointCloudSourceConstPtr& c) { source_ = c; }
  void setInputTarget(const PointCloudTargetConstPtr& c) { target_ = c; }
  void setMaxCorrespondenceDistance(double d) { params_.max_correspondence_distance = d; }
  void setRANSACOutlierRejectionThreshold(double t) { ransac_threshold_ = t; }
  void setTransformationEpsilon(double e) { params_.transformation_epsilon = e; }
  void setEuclideanFitnessEpsilon(double e) { params_.euclidean_fitness_epsilon = e; }
  void setMaximumIterations(int n) { params_.max_iterations = n; }
  double getMaxCorrespondenceDistance() const { return params_.max_correspondence_distance; }
  double getRANSACOutlierRejectionThreshold() const { return ransac_threshold_; }
  double getTransformationEpsilon() const { return params_.transformation_epsilon; }
  double getEuclideanFitnessEpsilon() const { return params_.euclidean_fitness_epsilon; }
  int getMaximumIterations() const { return params_.max_iterations; }
  void align(PointCloudSource& output) { align(output, Eigen::Matrix4f::Identity()); }
  void align(PointCloudSource& output, const Eigen::Matrix4f& guess) {
    final_.setIdentity();
    converged_ = false;
    fitness_ = std::numeric_limits<double>::max();
    state_ = PFX_ICP_NOT_CONVERGED;
    if (!source_ || !target_) {
      PCL_ERROR("[pcl::IterativeClosestPoint::align] no input source or target\n");
      return;
    }
    output = *source_;
    if (!detail::context()) return;
    const detail::SoA s = detail::soa_xyz(*source_), t = detail::soa_xyz(*target_);
    const size_t n = s.x.size();
    std::vector<float> ax(n + 1), ay(n + 1), az(n + 1);
    float T[16];
    int32_t conv = 0, it = 0, state = 0;
    std::lock_guard<std::mutex> lock(detail::context_mutex());
    if (!detail::ok(pfx_icp(detail::context(), s.x.data(), s.y.data(), s.z.data(), (int64_t)n, t.x.data(), t.y.data(),
                            t.z.data(), (int64_t)t.x.size(), &params_, guess.m, T, &fitness_, &conv, &it, &state,
                            ax.data(), ay.data(), az.data()),
                    "IterativeClosestPoint"))
      return;
    for (size_t i = 0; i < n; ++i) {
      output.points[i].x = ax[i];
      output.points[i].y = ay[i];
      output.points[i].z = az[i];
    }
    for (int i = 0; i < 16; ++i) final_.m[i] = T[i];
    converged_ = conv != 0;
    state_ = state;
  }
  Eigen::Matrix4f getFinalTransformation() const { return final_; }
  // the mean squared distance of the aligned source to the target, without a distance cap
  double getFitnessScore() const { return fitness_; }
  bool hasConverged() const { return converged_; }
  // DefaultConvergenceCriteria::getConvergenceState() of the last align (PFX_ICP_*)
  int getConvergenceState() const { return state_; }

 private:
  PointCloudSourceConstPtr source_;
  PointCloudTargetConstPtr target_;
  pfx_icp_params params_;
  double ransac_threshold_ = 0.05;
  Eigen::Matrix4f final_;
  double fitness_ = std::numeric_limits<double>::max();
  bool converged_ = false;
  int state_ = PFX_ICP_NOT_CONVERGED;
};

}  // namespace pcl

#endif  // PFX_PCL_HPP_
