// The per-pair arithmetic of LocalMapping::CreateNewMapPoints and
// CreateNewMapLines (LocalMapping.cc:346-665, 668-916), LocalMapping::ComputeF12
// (:1106-1127) and the geometric tests of ORBmatcher::SearchForTriangulation
// (ORBmatcher.cc:884-1095, CheckDistEpipolarLine :205-232) as pinned in
// the
// reference's float / double mix operation by operation. Host and device run
// the same text (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "lsd_math.h"
#include "orbpl_math.h"

#if defined(__HIPCC__)
#define LM_HD __host__ __device__ __forceinline__
#else
#define LM_HD static inline
#endif

namespace orbpl {
namespace lm {

constexpr int kMaxKp = 2048;     // keypoints per keyframe
constexpr int kNeighbours = 10;  // GetBestCovisibilityKeyFrames(nn = 10), non-monocular
constexpr int kMaxLevels = 16;
constexpr int kThLow = 50;       // ORBmatcher::TH_LOW
constexpr int kJacobiSweeps = 30;                        // pnp_core.h's svd_jacobi
constexpr double kJacobiTol = 1.4210854715202004e-14;    // 2^-46

struct Consts {
  float fx, fy, cx, cy, invfx, invfy;
  float bf, mb;
  float ratio_factor;   // 1.5f * mfScaleFactor
  int nlevels;
  float scale[kMaxLevels];    // mvScaleFactors
  float sigma2[kMaxLevels];   // mvLevelSigma2
};

// what a keyframe pose gives: Tcw row-major 4x4, the camera centre Ow = -Rwc tcw
struct Pose {
  float T[16];
  float Ow[3];
};

LM_HD void make_pose(const float* Tcw, Pose* p) {
  for (int i = 0; i < 16; i++) p->T[i] = Tcw[i];
  for (int r = 0; r < 3; r++) {
    double s = (double)Tcw[0 * 4 + r] * Tcw[3];
    s += (double)Tcw[1 * 4 + r] * Tcw[7];
    s += (double)Tcw[2 * 4 + r] * Tcw[11];
    p->Ow[r] = (float)(s * -1.0);
  }
}

// P6: float 3x3 product, double accumulation, one rounding
LM_HD void mul33(const float* A, const float* B, float* C) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double s = (double)A[r * 3] * B[c];
      s += (double)A[r * 3 + 1] * B[3 + c];
      s += (double)A[r * 3 + 2] * B[6 + c];
      C[r * 3 + c] = (float)s;
    }
}

// P34: cv::Mat::inv() of a float 3x3 as OpenCV 3.4's closed form: determinant
// and cofactors in double, one rounding per entry. A singular matrix gives 0.
LM_HD void inv33(const float* m, float* o) {
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5],
               m20 = m[6], m21 = m[7], m22 = m[8];
  double d = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) +
             m02 * (m10 * m21 - m11 * m20);
  if (d == 0.0) {
    for (int i = 0; i < 9; i++) o[i] = 0.0f;
    return;
  }
  d = 1.0 / d;
  o[0] = (float)((m11 * m22 - m12 * m21) * d);
  o[1] = (float)((m02 * m21 - m01 * m22) * d);
  o[2] = (float)((m01 * m12 - m02 * m11) * d);
  o[3] = (float)((m12 * m20 - m10 * m22) * d);
  o[4] = (float)((m00 * m22 - m02 * m20) * d);
  o[5] = (float)((m02 * m10 - m00 * m12) * d);
  o[6] = (float)((m10 * m21 - m11 * m20) * d);
  o[7] = (float)((m01 * m20 - m00 * m21) * d);
  o[8] = (float)((m00 * m11 - m01 * m10) * d);
}

// LocalMapping::ComputeF12: K1^-T [t12]x R12 K2^-1, both keyframes share K
LM_HD void compute_f12(const Consts& c, const float* T1, const float* T2, float* F) {
  float R12[9], t12[3];
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 3; q++) {
      double s = (double)T1[r * 4] * T2[q * 4];
      s += (double)T1[r * 4 + 1] * T2[q * 4 + 1];
      s += (double)T1[r * 4 + 2] * T2[q * 4 + 2];
      R12[r * 3 + q] = (float)s;
    }
  // (-R1w * R2w.t()) is a matrix of its own (= -R12), then * t2w + t1w in one gemm
  for (int r = 0; r < 3; r++) {
    double s = (double)(-R12[r * 3]) * T2[3];
    s += (double)(-R12[r * 3 + 1]) * T2[7];
    s += (double)(-R12[r * 3 + 2]) * T2[11];
    t12[r] = (float)(s + (double)T1[r * 4 + 3]);
  }
  const float tx[9] = {0.0f, -t12[2], t12[1], t12[2], 0.0f, -t12[0], -t12[1], t12[0], 0.0f};
  const float K[9] = {c.fx, 0.0f, c.cx, 0.0f, c.fy, c.cy, 0.0f, 0.0f, 1.0f};
  const float Kt[9] = {c.fx, 0.0f, 0.0f, 0.0f, c.fy, 0.0f, c.cx, c.cy, 1.0f};
  float Kti[9], Ki[9], A[9], B[9];
  inv33(Kt, Kti);
  inv33(K, Ki);
  mul33(Kti, tx, A);
  mul33(A, R12, B);
  mul33(B, Ki, F);
}

// the epipole of KF1's centre in KF2 (ORBmatcher.cc:893-902)
LM_HD void epipole(const Consts& c, const float* Ow1, const float* T2, float* ex, float* ey) {
  float C2[3];
  for (int r = 0; r < 3; r++) {
    double s = (double)T2[r * 4] * Ow1[0];
    s += (double)T2[r * 4 + 1] * Ow1[1];
    s += (double)T2[r * 4 + 2] * Ow1[2];
    C2[r] = (float)(s + (double)T2[r * 4 + 3]);
  }
  const float invz = 1.0f / C2[2];
  *ex = c.fx * C2[0] * invz + c.cx;
  *ey = c.fy * C2[1] * invz + c.cy;
}

// The tests of one (KF1 feature, KF2 feature) candidate that do not depend on
// the search's state: the epipole distance (only when neither has a right
// coordinate) and CheckDistEpipolarLine.
LM_HD bool pair_geometry(const Consts& c, const float* F, float ex, float ey, float x1, float y1,
                         bool stereo1, float x2, float y2, int oct2, bool stereo2) {
  if (!stereo1 && !stereo2) {
    const float dx = ex - x2, dy = ey - y2;
    if (dx * dx + dy * dy < 100.0f * c.scale[oct2]) return false;
  }
  const float a = x1 * F[0] + y1 * F[3] + F[6];
  const float b = x1 * F[1] + y1 * F[4] + F[7];
  const float cc = x1 * F[2] + y1 * F[5] + F[8];
  const float num = a * x2 + b * y2 + cc;
  const float den = a * a + b * b;
  if (den == 0.0f) return false;
  const float dsqr = num * num / den;
  return (double)dsqr < 3.84 * (double)c.sigma2[oct2];
}

// P16: cv::norm of a float 3-vector; Mat::dot in double
LM_HD double norm3d(const float* v) {
  return sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
}
LM_HD double dot3d(const float* a, const float* b) {
  double s = (double)a[0] * b[0];
  s += (double)a[1] * b[1];
  s += (double)a[2] * b[2];
  return s;
}

// P35: the right singular vector of the smallest singular value of the float
// 4x4 A, by pnp_core.h's one-sided Jacobi in double (the same operations in
// the same order, the 4x4 case unrolled so that it stays in registers),
// rounded to float.
LM_HD void svd4_last(const float* Af, float* x) {
  double A[16], V[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    A[i] = (double)Af[i];
    V[i] = (i % 5 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
    int rotations = 0;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const double ap = A[i * 4 + p], aq = A[i * 4 + q];
          alpha = alpha + ap * ap;
          beta = beta + aq * aq;
          gamma = gamma + ap * aq;
        }
        if (fabs(gamma) > kJacobiTol * sqrt(alpha * beta)) {
          const double zeta = (beta - alpha) / (2.0 * gamma);
          double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          if (zeta < 0.0) t = -t;
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const double ap = A[i * 4 + p], aq = A[i * 4 + q];
            A[i * 4 + p] = cs * ap - sn * aq;
            A[i * 4 + q] = sn * ap + cs * aq;
            const double vp = V[i * 4 + p], vq = V[i * 4 + q];
            V[i * 4 + p] = cs * vp - sn * vq;
            V[i * 4 + q] = sn * vp + cs * vq;
          }
          rotations++;
        }
      }
    if (!rotations) break;
  }
  double s[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) ss = ss + A[i * 4 + k] * A[i * 4 + k];
    s[k] = sqrt(ss);
  }
  // svd_jacobi's selection sort (descending, first maximum first): the column
  // left in the last place
  double v0[4], v1[4], v2[4], v3[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    v0[i] = V[i * 4];
    v1[i] = V[i * 4 + 1];
    v2[i] = V[i * 4 + 2];
    v3[i] = V[i * 4 + 3];
  }
#define LM_SWAP(sa, va, sb, vb)            \
  {                                        \
    const double ts = sa;                  \
    sa = sb;                               \
    sb = ts;                               \
    _Pragma("unroll") for (int i = 0; i < 4; i++) { \
      const double tv = va[i];             \
      va[i] = vb[i];                       \
      vb[i] = tv;                          \
    }                                      \
  }
  {  // k = 0: best among 0..3
    int best = 0;
    if (s[1] > s[best]) best = 1;
    if (s[2] > s[best]) best = 2;
    if (s[3] > s[best]) best = 3;
    if (best == 1) LM_SWAP(s[0], v0, s[1], v1)
    else if (best == 2) LM_SWAP(s[0], v0, s[2], v2)
    else if (best == 3) LM_SWAP(s[0], v0, s[3], v3)
  }
  {  // k = 1: best among 1..3
    int best = 1;
    if (s[2] > s[best]) best = 2;
    if (s[3] > s[best]) best = 3;
    if (best == 2) LM_SWAP(s[1], v1, s[2], v2)
    else if (best == 3) LM_SWAP(s[1], v1, s[3], v3)
  }
  if (s[3] > s[2]) LM_SWAP(s[2], v2, s[3], v3)
#undef LM_SWAP
#pragma unroll
  for (int i = 0; i < 4; i++) x[i] = (float)v3[i];
}

struct PointOut {
  float xyz[3], normal[3], min_dist, max_dist;
};

// One matched pair of CreateNewMapPoints (LocalMapping.cc:449-663): true when
// a map point is created. (x, y, octave) are mvKeysUn's, (rx, ry) mvKeys' pt
// (UnprojectStereo reads the raw keypoint), ur = mvuRight, z = mvDepth.
// kf1_first: KF1's id is the lower one (observation order, P24).
LM_HD bool triangulate_pair(const Consts& c, const Pose& P1, const Pose& P2, float x1, float y1,
                            int oct1, float rx1, float ry1, float ur1, float z1d, float x2,
                            float y2, int oct2, float rx2, float ry2, float ur2, float z2d,
                            bool kf1_first, PointOut* out) {
  const bool stereo1 = ur1 >= 0.0f, stereo2 = ur2 >= 0.0f;
  const float xn1[3] = {(x1 - c.cx) * c.invfx, (y1 - c.cy) * c.invfy, 1.0f};
  const float xn2[3] = {(x2 - c.cx) * c.invfx, (y2 - c.cy) * c.invfy, 1.0f};
  float ray1[3], ray2[3];
  for (int r = 0; r < 3; r++) {
    double s = (double)P1.T[0 * 4 + r] * xn1[0];
    s += (double)P1.T[1 * 4 + r] * xn1[1];
    s += (double)P1.T[2 * 4 + r] * xn1[2];
    ray1[r] = (float)s;
    double u = (double)P2.T[0 * 4 + r] * xn2[0];
    u += (double)P2.T[1 * 4 + r] * xn2[1];
    u += (double)P2.T[2 * 4 + r] * xn2[2];
    ray2[r] = (float)u;
  }
  const float cosRays = (float)(dot3d(ray1, ray2) / (norm3d(ray1) * norm3d(ray2)));
  float cosStereo1 = cosRays + 1.0f, cosStereo2 = cosStereo1;
  if (stereo1 || stereo2) {
    // cos(2 * atan2(mb / 2, depth)), float overloads (P12, P2)
    const float dep = stereo1 ? z1d : z2d;
    const float at = (float)lsdm::atan2_((double)(c.mb / 2.0f), (double)dep);
    float cs, sn;
    cr_cos_sin(2.0f * at, &cs, &sn);
    if (stereo1) cosStereo1 = cs;
    else cosStereo2 = cs;
  }
  const float cosStereo = cosStereo1 < cosStereo2 ? cosStereo1 : cosStereo2;   // std::min
  float X[3];
  if (cosRays < cosStereo && cosRays > 0.0f &&
      (stereo1 || stereo2 || (double)cosRays < 0.9998)) {
    float A[16];
    for (int k = 0; k < 4; k++) {
      // s * row(2) - row(0): addWeighted, double with one rounding (P36)
      A[k] = (float)((double)xn1[0] * (double)P1.T[8 + k] - (double)P1.T[k]);
      A[4 + k] = (float)((double)xn1[1] * (double)P1.T[8 + k] - (double)P1.T[4 + k]);
      A[8 + k] = (float)((double)xn2[0] * (double)P2.T[8 + k] - (double)P2.T[k]);
      A[12 + k] = (float)((double)xn2[1] * (double)P2.T[8 + k] - (double)P2.T[4 + k]);
    }
    float h[4];
    svd4_last(A, h);
    if (h[3] == 0.0f) return false;
    const float inv = (float)(1.0 / (double)h[3]);   // Mat / scalar: scale by float(1 / w)
    X[0] = h[0] * inv;
    X[1] = h[1] * inv;
    X[2] = h[2] * inv;
  } else if (stereo1 && cosStereo1 < cosStereo2) {
    if (!(z1d > 0.0f)) return false;   // UnprojectStereo returns an empty Mat: no point
    const float x3[3] = {(rx1 - c.cx) * z1d * c.invfx, (ry1 - c.cy) * z1d * c.invfy, z1d};
    for (int r = 0; r < 3; r++) {
      double s = (double)P1.T[0 * 4 + r] * x3[0];
      s += (double)P1.T[1 * 4 + r] * x3[1];
      s += (double)P1.T[2 * 4 + r] * x3[2];
      X[r] = (float)(s + (double)P1.Ow[r]);
    }
  } else if (stereo2 && cosStereo2 < cosStereo1) {
    if (!(z2d > 0.0f)) return false;
    const float x3[3] = {(rx2 - c.cx) * z2d * c.invfx, (ry2 - c.cy) * z2d * c.invfy, z2d};
    for (int r = 0; r < 3; r++) {
      double s = (double)P2.T[0 * 4 + r] * x3[0];
      s += (double)P2.T[1 * 4 + r] * x3[1];
      s += (double)P2.T[2 * 4 + r] * x3[2];
      X[r] = (float)(s + (double)P2.Ow[r]);
    }
  } else {
    return false;
  }
  const float z1 = (float)(dot3d(P1.T + 8, X) + (double)P1.T[11]);
  if (z1 <= 0.0f) return false;
  const float z2 = (float)(dot3d(P2.T + 8, X) + (double)P2.T[11]);
  if (z2 <= 0.0f) return false;
  {
    const float sig = c.sigma2[oct1];
    const float px = (float)(dot3d(P1.T, X) + (double)P1.T[3]);
    const float py = (float)(dot3d(P1.T + 4, X) + (double)P1.T[7]);
    const float invz = (float)(1.0 / (double)z1);
    const float u = c.fx * px * invz + c.cx, v = c.fy * py * invz + c.cy;
    const float eX = u - x1, eY = v - y1;
    if (!stereo1) {
      if ((double)(eX * eX + eY * eY) > 5.991 * (double)sig) return false;
    } else {
      const float ur = u - c.bf * invz;
      const float eR = ur - ur1;
      if ((double)(eX * eX + eY * eY + eR * eR) > 7.8 * (double)sig) return false;
    }
  }
  {
    const float sig = c.sigma2[oct2];
    const float px = (float)(dot3d(P2.T, X) + (double)P2.T[3]);
    const float py = (float)(dot3d(P2.T + 4, X) + (double)P2.T[7]);
    const float invz = (float)(1.0 / (double)z2);
    const float u = c.fx * px * invz + c.cx, v = c.fy * py * invz + c.cy;
    const float eX = u - x2, eY = v - y2;
    if (!stereo2) {
      if ((double)(eX * eX + eY * eY) > 5.991 * (double)sig) return false;
    } else {
      const float ur = u - c.bf * invz;   // KF1's mbf, as written (one camera here)
      const float eR = ur - ur2;
      if ((double)(eX * eX + eY * eY + eR * eR) > 7.8 * (double)sig) return false;
    }
  }
  const float n1[3] = {X[0] - P1.Ow[0], X[1] - P1.Ow[1], X[2] - P1.Ow[2]};
  const float n2[3] = {X[0] - P2.Ow[0], X[1] - P2.Ow[1], X[2] - P2.Ow[2]};
  const float dist1 = (float)norm3d(n1), dist2 = (float)norm3d(n2);
  if (dist1 == 0.0f || dist2 == 0.0f) return false;
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = c.scale[oct1] / c.scale[oct2];
  if (ratioDist * c.ratio_factor < ratioOctave || ratioDist > ratioOctave * c.ratio_factor)
    return false;
  // the new MapPoint: UpdateNormalAndDepth with its two observations in
  // keyframe-id order (P24, P25), reference keyframe KF1
  const float i1 = (float)(1.0 / norm3d(n1)), i2 = (float)(1.0 / norm3d(n2));
  for (int q = 0; q < 3; q++) {
    float nq = 0.0f;
    if (kf1_first) {
      nq = nq + n1[q] * i1;
      nq = nq + n2[q] * i2;
    } else {
      nq = nq + n2[q] * i2;
      nq = nq + n1[q] * i1;
    }
    out->normal[q] = nq / 2.0f;
    out->xyz[q] = X[q];
  }
  out->max_dist = dist1 * c.scale[oct1];
  out->min_dist = out->max_dist / c.scale[c.nlevels - 1];
  return true;
}

// ---- CreateNewMapLines (LocalMapping.cc:668-916) ----
constexpr int kMaxLines = 256;   // key lines per keyframe

// M = K * Tcw (3x4), P6
LM_HD void projection_matrix(const Consts& c, const float* T, float* M) {
  const float K[9] = {c.fx, 0.0f, c.cx, 0.0f, c.fy, c.cy, 0.0f, 0.0f, 1.0f};
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 4; k++) {
      double s = (double)K[r * 3] * T[k];
      s += (double)K[r * 3 + 1] * T[4 + k];
      s += (double)K[r * 3 + 2] * T[8 + k];
      M[r * 4 + k] = (float)s;
    }
}

// LineMatcher::SearchForTriangulation's threshold from the two medians
// (KeyFrame::lineDescriptorMAD, KeyFrame.cc:773-797): 1.4826 * mad * 0.1
LM_HD double line_nn12_threshold(int mad) { return 1.4826 * (double)(float)mad * 0.1; }

// One matched line pair (LocalMapping.cc:764-913): the two end points of KF1's
// raw key line (sx, sy)-(ex, ey) on the planes of both lines; coef = the
// Vector3d line coefficients, cast to float as the reference does; median =
// pKF2->ComputeSceneMedianDepth(2). True when a map line is created.
LM_HD bool triangulate_line(const Consts& c, const Pose& P1, const Pose& P2, const float* M1,
                            const float* M2, const double* coef1, const double* coef2, float sx,
                            float sy, float ex, float ey, float median, float* xyz6) {
  const float l1[3] = {(float)coef1[0], (float)coef1[1], (float)coef1[2]};
  const float l2[3] = {(float)coef2[0], (float)coef2[1], (float)coef2[2]};
  float A[16];
  for (int k = 0; k < 4; k++) {
    double s = (double)l1[0] * M1[k];
    s += (double)l1[1] * M1[4 + k];
    s += (double)l1[2] * M1[8 + k];
    A[k] = (float)s;
    double u = (double)l2[0] * M2[k];
    u += (double)l2[1] * M2[4 + k];
    u += (double)l2[2] * M2[8 + k];
    A[4 + k] = (float)u;
  }
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const float xn = ((e ? ex : sx) - c.cx) * c.invfx, yn = ((e ? ey : sy) - c.cy) * c.invfy;
    for (int k = 0; k < 4; k++) {
      A[8 + k] = (float)((double)xn * (double)P1.T[8 + k] - (double)P1.T[k]);
      A[12 + k] = (float)((double)yn * (double)P1.T[8 + k] - (double)P1.T[4 + k]);
    }
    float h[4];
    svd4_last(A, h);
    if (h[3] == 0.0f) return false;
    const float inv = (float)(1.0 / (double)h[3]);
    xyz6[3 * e] = h[0] * inv;
    xyz6[3 * e + 1] = h[1] * inv;
    xyz6[3 * e + 2] = h[2] * inv;
  }
  const float* s3 = xyz6;
  const float* e3 = xyz6 + 3;
  const float v1[3] = {s3[0] - P1.Ow[0], s3[1] - P1.Ow[1], s3[2] - P1.Ow[2]};
  if ((double)((float)norm3d(v1) / median) < 0.3) return false;
  const float v2[3] = {s3[0] - P2.Ow[0], s3[1] - P2.Ow[1], s3[2] - P2.Ow[2]};
  if ((double)((float)norm3d(v2) / median) < 0.3) return false;
  const float v3[3] = {e3[0] - s3[0], e3[1] - s3[1], e3[2] - s3[2]};
  if ((float)norm3d(v3) / median > 1.0f) return false;
  if ((float)(dot3d(P1.T + 8, s3) + (double)P1.T[11]) <= 0.0f) return false;
  if ((float)(dot3d(P2.T + 8, s3) + (double)P2.T[11]) <= 0.0f) return false;
  if ((float)(dot3d(P1.T + 8, e3) + (double)P1.T[11]) <= 0.0f) return false;
  if ((float)(dot3d(P2.T + 8, e3) + (double)P2.T[11]) <= 0.0f) return false;
  return true;
}

// the depth of a world point in a keyframe (ComputeSceneMedianDepth)
LM_HD float scene_depth(const float* T, const float* X) {
  return (float)(dot3d(T + 8, X) + (double)T[11]);
}

}  // namespace lm
}  // namespace orbpl
