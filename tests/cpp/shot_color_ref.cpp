// shot_color_ref.cpp -- TEST INFRASTRUCTURE ONLY: a CPU restatement of PCL 1.7
// SHOTColorEstimation (features/impl/shot.hpp: computePointSHOT with describe_shape and
// describe_color, RGB2CIELAB, interpolateDoubleChannel, normalizeHistogram) as DESIGN.md
// "SHOT-1344: the contract" states it, on the oracle's helpers (oracle/or_common.h:
// NeighborGrid, dot4).  The local reference frames are an input (the tests pass the oracle's
// SHOT-352 frames), so only the Lab conversion, the double-channel histogram and the
// normalisation are restated here.  Built by tests/shot_color_ref.py into a shared object; never
// linked into libpfx.  Single-threaded, plain sequential `+=` in FLANN neighbour order.
#include "or_common.h"

using namespace orc;

namespace {

const double PST_RAD_45 = 0.78539816339744830961566084581988;
const double PST_RAD_90 = 1.5707963267948966192313216916398;
const double PST_RAD_135 = 2.3561944901923449288469825374596;
const double PST_RAD_PI_7_8 = 2.7488935718910690836548129603691;

const int kShape = 352, kLen = 1344, kXyz = 4000;

float sRGB_LUT[256];
float sXYZ_LUT[kXyz];

void fillTables() {
  static bool done = false;
  if (done) return;
  for (int i = 0; i < 256; i++) {
    float f = static_cast<float>(i) / 255.0f;
    if (f > 0.04045)
      sRGB_LUT[i] = powf((f + 0.055f) / 1.055f, 2.4f);
    else
      sRGB_LUT[i] = f / 12.92f;
  }
  for (int i = 0; i < kXyz; i++) {
    float f = static_cast<float>(i) / 4000.0f;
    if (f > 0.008856)
      sXYZ_LUT[i] = static_cast<float>(powf(f, 0.3333f));
    else
      sXYZ_LUT[i] = static_cast<float>((7.787 * f) + (16.0 / 116.0));
  }
  done = true;
}

// sXYZ_LUT[int(v * 4000)]; PCL reads past the table for v == 1.0f: clamped to the last entry
float xyzEntry(float v, bool& clamped) {
  int i = int(v * 4000);
  if (i >= kXyz) {
    i = kXyz - 1;
    clamped = true;
  }
  return sXYZ_LUT[i];
}

// RGB2CIELAB; returns whether a table index was clamped
bool RGB2CIELAB(unsigned char R, unsigned char G, unsigned char B, float& L, float& A, float& B2) {
  fillTables();
  float fr = sRGB_LUT[R];
  float fg = sRGB_LUT[G];
  float fb = sRGB_LUT[B];
  const float x = fr * 0.412453f + fg * 0.357580f + fb * 0.180423f;
  const float y = fr * 0.212671f + fg * 0.715160f + fb * 0.072169f;
  const float z = fr * 0.019334f + fg * 0.119193f + fb * 0.950227f;
  float vx = x / 0.95047f;
  float vy = y;
  float vz = z / 1.08883f;
  bool clamped = false;
  vx = xyzEntry(vx, clamped);
  vy = xyzEntry(vy, clamped);
  vz = xyzEntry(vz, clamped);
  L = 116.0f * vy - 16.0f;
  if (L > 100) L = 100.0f;
  A = 500.0f * (vx - vy);
  if (A > 120) A = 120.0f;
  else if (A < -120) A = -120.0f;
  B2 = 200.0f * (vy - vz);
  if (B2 > 120) B2 = 120.0f;
  else if (B2 < -120) B2 = -120.0f;
  return clamped;
}

struct Lab { float L, a, b; };

// the colour as computePointSHOT uses it: L / 100, a / 120, b / 120
Lab labOf(uint32_t rgb, bool* clamped = 0) {
  Lab c;
  const bool cl = RGB2CIELAB((unsigned char)((rgb >> 16) & 0xff), (unsigned char)((rgb >> 8) & 0xff),
                             (unsigned char)(rgb & 0xff), c.L, c.a, c.b);
  if (clamped) *clamped = cl;
  c.L /= 100.0f;
  c.a /= 120.0f;
  c.b /= 120.0f;
  return c;
}

// computePointSHOT (shape + colour) up to, not including, normalizeHistogram
void histogram(const float* sx, const float* sy, const float* sz, const float* nx, const float* ny,
               const float* nz, const uint32_t* srgb, float cx, float cy, float cz, uint32_t qrgb,
               const float rf[9], const std::vector<int>& nb, const std::vector<float>& d2, double radius,
               float shot[1344]) {
  const int nr_bins_shape = 10, nr_bins_color = 30, maxAngularSectors = 32;
  const int shapeToColorStride = maxAngularSectors * (nr_bins_shape + 1);
  const double radius3_4 = (radius * 3) / 4, radius1_4 = radius / 4, radius1_2 = radius / 2;
  const V3 fx = v3(rf[0], rf[1], rf[2]), fy = v3(rf[3], rf[4], rf[5]), fz = v3(rf[6], rf[7], rf[8]);
  // createBinDistanceShape
  std::vector<double> binDistanceShape(nb.size()), binDistanceColor(nb.size());
  for (size_t i = 0; i < nb.size(); ++i) {
    const int p = nb[i];
    if (!std::isfinite(nx[p]) || !std::isfinite(ny[p]) || !std::isfinite(nz[p])) {
      binDistanceShape[i] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    double cosineDesc = dot4(v3(nx[p], ny[p], nz[p]), fz);
    if (cosineDesc > 1.0) cosineDesc = 1.0;
    if (cosineDesc < -1.0) cosineDesc = -1.0;
    binDistanceShape[i] = ((1.0 + cosineDesc) * nr_bins_shape) / 2;
  }
  // the colour bin distances: the reference colour is the query's own
  const Lab ref = labOf(qrgb);
  for (size_t i = 0; i < nb.size(); ++i) {
    const Lab c = labOf(srgb[nb[i]]);
    // float differences; PCL's unqualified fabs is the C double function
    double colorDistance = (std::fabs((double)(ref.L - c.L)) +
                            ((std::fabs((double)(ref.a - c.a)) + std::fabs((double)(ref.b - c.b))) / 2)) / 3;
    if (colorDistance > 1.0) colorDistance = 1.0;
    if (colorDistance < 0.0) colorDistance = 0.0;
    binDistanceColor[i] = colorDistance * nr_bins_color;
  }
  for (int k = 0; k < kLen; ++k) shot[k] = 0.0f;
  // interpolateDoubleChannel
  for (size_t i = 0; i < nb.size(); ++i) {
    if (!std::isfinite(binDistanceShape[i])) continue;
    const int p = nb[i];
    const V3 delta = v3(sx[p] - cx, sy[p] - cy, sz[p] - cz);
    const double distance = std::sqrt((double)d2[i]);
    if (std::fabs(distance - 0.0) < 1E-15) continue;
    double xInFeatRef = dot4(delta, fx);
    double yInFeatRef = dot4(delta, fy);
    double zInFeatRef = dot4(delta, fz);
    if (std::fabs(yInFeatRef) < 1E-30) yInFeatRef = 0;
    if (std::fabs(xInFeatRef) < 1E-30) xInFeatRef = 0;
    if (std::fabs(zInFeatRef) < 1E-30) zInFeatRef = 0;
    unsigned char bit4 = ((yInFeatRef > 0) || ((yInFeatRef == 0.0) && (xInFeatRef < 0))) ? 1 : 0;
    unsigned char bit3 = (unsigned char)(((xInFeatRef > 0) || ((xInFeatRef == 0.0) && (yInFeatRef > 0))) ? !bit4 : bit4);
    int desc_index = (bit4 << 3) + (bit3 << 2);
    desc_index = desc_index << 1;
    if ((xInFeatRef * yInFeatRef > 0) || (xInFeatRef == 0.0))
      desc_index += (std::fabs(xInFeatRef) >= std::fabs(yInFeatRef)) ? 0 : 4;
    else
      desc_index += (std::fabs(xInFeatRef) > std::fabs(yInFeatRef)) ? 4 : 0;
    desc_index += zInFeatRef > 0 ? 1 : 0;
    desc_index += (distance > radius1_2) ? 2 : 0;
    const int step_index_shape = (int)std::floor(binDistanceShape[i] + 0.5);
    const int step_index_color = (int)std::floor(binDistanceColor[i] + 0.5);
    const int volume_index_shape = desc_index * (nr_bins_shape + 1);
    const int volume_index_color = shapeToColorStride + desc_index * (nr_bins_color + 1);
    binDistanceShape[i] -= step_index_shape;
    binDistanceColor[i] -= step_index_color;
    double intWeightShape = (1 - std::fabs(binDistanceShape[i]));
    double intWeightColor = (1 - std::fabs(binDistanceColor[i]));
    if (binDistanceShape[i] > 0)
      shot[volume_index_shape + ((step_index_shape + 1) % nr_bins_shape)] += (float)binDistanceShape[i];
    else
      shot[volume_index_shape + ((step_index_shape - 1 + nr_bins_shape) % nr_bins_shape)] -= (float)binDistanceShape[i];
    if (binDistanceColor[i] > 0)
      shot[volume_index_color + ((step_index_color + 1) % nr_bins_color)] += (float)binDistanceColor[i];
    else
      shot[volume_index_color + ((step_index_color - 1 + nr_bins_color) % nr_bins_color)] -= (float)binDistanceColor[i];
    if (distance > radius1_2) {
      const double radiusDistance = (distance - radius3_4) / radius1_2;
      if (distance > radius3_4) {
        intWeightShape += 1 - radiusDistance;
        intWeightColor += 1 - radiusDistance;
      } else {
        intWeightShape += 1 + radiusDistance;
        intWeightColor += 1 + radiusDistance;
        shot[(desc_index - 2) * (nr_bins_shape + 1) + step_index_shape] -= (float)radiusDistance;
        shot[shapeToColorStride + (desc_index - 2) * (nr_bins_color + 1) + step_index_color] -= (float)radiusDistance;
      }
    } else {
      const double radiusDistance = (distance - radius1_4) / radius1_2;
      if (distance < radius1_4) {
        intWeightShape += 1 + radiusDistance;
        intWeightColor += 1 + radiusDistance;
      } else {
        intWeightShape += 1 - radiusDistance;
        intWeightColor += 1 - radiusDistance;
        shot[(desc_index + 2) * (nr_bins_shape + 1) + step_index_shape] += (float)radiusDistance;
        shot[shapeToColorStride + (desc_index + 2) * (nr_bins_color + 1) + step_index_color] += (float)radiusDistance;
      }
    }
    double inclinationCos = zInFeatRef / distance;
    if (inclinationCos < -1.0) inclinationCos = -1.0;
    if (inclinationCos > 1.0) inclinationCos = 1.0;
    const double inclination = std::acos(inclinationCos);
    if (inclination > PST_RAD_90 || (std::fabs(inclination - PST_RAD_90) < 1e-30 && zInFeatRef <= 0)) {
      const double inclinationDistance = (inclination - PST_RAD_135) / PST_RAD_90;
      if (inclination > PST_RAD_135) {
        intWeightShape += 1 - inclinationDistance;
        intWeightColor += 1 - inclinationDistance;
      } else {
        intWeightShape += 1 + inclinationDistance;
        intWeightColor += 1 + inclinationDistance;
        shot[(desc_index + 1) * (nr_bins_shape + 1) + step_index_shape] -= (float)inclinationDistance;
        shot[shapeToColorStride + (desc_index + 1) * (nr_bins_color + 1) + step_index_color] -= (float)inclinationDistance;
      }
    } else {
      const double inclinationDistance = (inclination - PST_RAD_45) / PST_RAD_90;
      if (inclination < PST_RAD_45) {
        intWeightShape += 1 + inclinationDistance;
        intWeightColor += 1 + inclinationDistance;
      } else {
        intWeightShape += 1 - inclinationDistance;
        intWeightColor += 1 - inclinationDistance;
        shot[(desc_index - 1) * (nr_bins_shape + 1) + step_index_shape] += (float)inclinationDistance;
        shot[shapeToColorStride + (desc_index - 1) * (nr_bins_color + 1) + step_index_color] += (float)inclinationDistance;
      }
    }
    if (yInFeatRef != 0.0 || xInFeatRef != 0.0) {
      const double azimuth = std::atan2(yInFeatRef, xInFeatRef);
      const int sel = desc_index >> 2;
      const double angularSectorSpan = PST_RAD_45;
      const double angularSectorStart = -PST_RAD_PI_7_8;
      double azimuthDistance = (azimuth - (angularSectorStart + angularSectorSpan * sel)) / angularSectorSpan;
      azimuthDistance = std::max(-0.5, std::min(azimuthDistance, 0.5));
      if (azimuthDistance > 0) {
        intWeightShape += 1 - azimuthDistance;
        intWeightColor += 1 - azimuthDistance;
        const int interp_index = (desc_index + 4) % maxAngularSectors;
        shot[interp_index * (nr_bins_shape + 1) + step_index_shape] += (float)azimuthDistance;
        shot[shapeToColorStride + interp_index * (nr_bins_color + 1) + step_index_color] += (float)azimuthDistance;
      } else {
        const int interp_index = (desc_index - 4 + maxAngularSectors) % maxAngularSectors;
        intWeightShape += 1 + azimuthDistance;
        intWeightColor += 1 + azimuthDistance;
        shot[interp_index * (nr_bins_shape + 1) + step_index_shape] -= (float)azimuthDistance;
        shot[shapeToColorStride + interp_index * (nr_bins_color + 1) + step_index_color] -= (float)azimuthDistance;
      }
    }
    shot[volume_index_shape + step_index_shape] += (float)intWeightShape;
    shot[volume_index_color + step_index_color] += (float)intWeightColor;
  }
  (void)kShape;
}

}  // namespace

extern "C" {

// out[0..2] = RGB2CIELAB's L, a, b; out[3..5] = L / 100, a / 120, b / 120; returns 1 when a
// table index was clamped.  rgb: 0x00RRGGBB (the high byte is ignored).
int shot_color_ref_lab(uint32_t rgb, float out[6]) {
  float L, A, B;
  const bool cl = RGB2CIELAB((unsigned char)((rgb >> 16) & 0xff), (unsigned char)((rgb >> 8) & 0xff),
                             (unsigned char)(rgb & 0xff), L, A, B);
  out[0] = L; out[1] = A; out[2] = B;
  const Lab c = labOf(rgb);
  out[3] = c.L; out[4] = c.a; out[5] = c.b;
  return cl ? 1 : 0;
}

// sXYZ_LUT[i], 0 <= i < 4000
float shot_color_ref_xyz_entry(int i) {
  fillTables();
  return sXYZ_LUT[i];
}

// rf_in: nq x 9 frames (a NaN frame -> NaN row).  desc: nq x 1344 normalised rows; raw
// (nullable): the same before normalizeHistogram; neighbours (nullable): the sum of |N(q)| over
// the finite queries; clamped (nullable): surface points + queries whose table index was clamped.
int shot_color_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
                   const float* snz, const uint32_t* srgb, i64 ns, const float* qx, const float* qy,
                   const float* qz, const uint32_t* qrgb, i64 nq, double radius, const float* rf_in, float* desc,
                   float* raw, i64* neighbours, i64* clamped) {
  NeighborGrid g;
  g.build(sx, sy, sz, ns, radius);
  std::vector<int> nb;
  std::vector<float> dd;
  i64 nsum = 0, ncl = 0;
  for (i64 i = 0; i < ns; ++i) {
    bool cl;
    labOf(srgb[i], &cl);
    ncl += cl ? 1 : 0;
  }
  for (i64 q = 0; q < nq; ++q) {
    bool cl;
    labOf(qrgb[q], &cl);
    ncl += cl ? 1 : 0;
    float* d = desc + q * kLen;
    float* u = raw ? raw + q * kLen : 0;
    const float* rf = rf_in + q * 9;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    bool ok = std::isfinite(cx) && std::isfinite(cy) && std::isfinite(cz);
    if (ok) {
      g.radius(cx, cy, cz, radius, nb, dd);
      nsum += (i64)nb.size();
      for (int k = 0; k < 9; ++k) ok = ok && std::isfinite(rf[k]);
      ok = ok && nb.size() >= 5;
    }
    if (!ok) {
      for (int k = 0; k < kLen; ++k) d[k] = kNaN;
      if (u) for (int k = 0; k < kLen; ++k) u[k] = kNaN;
      continue;
    }
    histogram(sx, sy, sz, snx, sny, snz, srgb, cx, cy, cz, qrgb[q], rf, nb, dd, radius, d);
    if (u) for (int k = 0; k < kLen; ++k) u[k] = d[k];
    // normalizeHistogram
    double acc_norm = 0;
    for (int j = 0; j < kLen; ++j) acc_norm += d[j] * d[j];
    acc_norm = std::sqrt(acc_norm);
    for (int j = 0; j < kLen; ++j) d[j] /= (float)acc_norm;
  }
  if (neighbours) *neighbours = nsum;
  if (clamped) *clamped = ncl;
  return 0;
}

}  // extern "C"
