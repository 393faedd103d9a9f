// Sim3Solver's arithmetic (Sim3Solver.cc:37-112, 226-403) as pinned in
// Horn's closed form on three correspondences in float
// where the reference holds CV_32F, the OpenCV calls replaced by the pinned
// steps below, with only + - * /, sqrt and P10's sin / cos / atan2. The code is
// shared by the kernels of sim3.hip and the host form of orbsim3_setup.
#pragma once
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "lsd_math.h"
#include "pnp_core.h"

#if defined(__HIPCC__)
#define SIM3_HD __host__ __device__
#else
#define SIM3_HD
#endif

namespace orbpl {
namespace sim3 {

constexpr int kMaxSweeps = 30;                         // Jacobi sweeps, upper bound
constexpr double kJacobiTol = 2.220446049250313e-16;   // 2^-52 of the Frobenius norm
constexpr double kDblEps = 2.220446049250313e-16;      // DBL_EPSILON of cv::Rodrigues

// P6 / P55: a sum of three products accumulates in double in ascending index
// order; the caller rounds it once to float at the store
SIM3_HD inline double dot3d(float a0, float a1, float a2, float b0, float b1, float b2) {
  return ((double)a0 * (double)b0 + (double)a1 * (double)b1) + (double)a2 * (double)b2;
}

// The three indices hypothesis draws d[0..2] pick from mvAllIndices = 0..N-1
// (:163-177): PnPsolver's swap-with-back removal with a minimal set of 3, N >= 3.
SIM3_HD inline void sample3(const int* d, int N, double rand_max_p1, int* idx) {
  pnp::sample_k<3>(d, N, rand_max_p1, idx);
}

// P54, cv::eigen of the symmetric 4 x 4 matrix a: cyclic two-sided Jacobi in
// double, pairs (p, q), p < q, row by row; a pair is rotated when |a_pq| >
// kJacobiTol * |a|_F of the input (a comparison with a NaN is false, so a NaN
// matrix rotates nothing, and the zero matrix has nothing above 0); sweeps stop
// after one without a rotation or after kMaxSweeps. On return the diagonal of a
// holds the eigenvalues and the columns of v the eigenvectors, with whatever
// sign the rotations give. Returns the column of the largest eigenvalue, the
// first one among equals.
SIM3_HD inline int eig_jacobi4(double a[4][4], double v[4][4]) {
  double ss = 0.0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      ss = ss + a[i][j] * a[i][j];
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  const double thr = kJacobiTol * sqrt(ss);
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    int rotations = 0;
#pragma unroll
    for (int p = 0; p < 3; p++) {
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        const double apq = a[p][q];
        if (fabs(apq) > thr) {
          const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
          double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
          if (theta < 0.0) t = -t;
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          a[p][p] = a[p][p] - t * apq;
          a[q][q] = a[q][q] + t * apq;
          a[p][q] = 0.0;
          a[q][p] = 0.0;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            if (r == p || r == q) continue;
            const double arp = a[r][p], arq = a[r][q];
            a[r][p] = c * arp - s * arq;
            a[p][r] = a[r][p];
            a[r][q] = s * arp + c * arq;
            a[q][r] = a[r][q];
          }
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const double vrp = v[r][p], vrq = v[r][q];
            v[r][p] = c * vrp - s * vrq;
            v[r][q] = s * vrp + c * vrq;
          }
          rotations++;
        }
      }
    }
    if (!rotations) break;
  }
  int k = 0;
#pragma unroll
  for (int j = 1; j < 4; j++)
    if (a[j][j] > a[k][k]) k = j;
  return k;
}

// mR12i, mt12i, ms12i of one hypothesis
struct Hyp {
  float R[9];
  float t[3];
  float s;
};

// Sim3Solver::ComputeSim3 (:226-337). P1[r][c], P2[r][c]: coordinate r of the
// sampled point c in camera 1 and camera 2.
SIM3_HD inline void compute_sim3(const float P1[3][3], const float P2[3][3], bool fix_scale,
                                 Hyp& h) {
  // step 1: centroids (sum, then / 3) and relative coordinates, float
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
  for (int r = 0; r < 3; r++) {
    O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
    O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
    for (int c = 0; c < 3; c++) {
      Pr1[r][c] = P1[r][c] - O1[r];
      Pr2[r][c] = P2[r][c] - O2[r];
    }
  }
  // step 2: M = Pr2 * Pr1^T (P55)
  float M[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      M[i][j] = (float)dot3d(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
  // step 3: N, float expressions as the reference writes them
  const float N11 = M[0][0] + M[1][1] + M[2][2];
  const float N12 = M[1][2] - M[2][1];
  const float N13 = M[2][0] - M[0][2];
  const float N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2];
  const float N23 = M[0][1] + M[1][0];
  const float N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2];
  const float N34 = M[1][2] + M[2][1];
  const float N44 = -M[0][0] - M[1][1] + M[2][2];
  double a[4][4] = {{N11, N12, N13, N14}, {N12, N22, N23, N24}, {N13, N23, N33, N34},
                    {N14, N24, N34, N44}};
  // step 4: the eigenvector of the largest eigenvalue (P54), stored as float
  double v[4][4];
  const int k = eig_jacobi4(a, v);
  float q[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    // (a selection, not an indexed read: the matrices stay in registers)
    double e = v[i][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
      if (k == j) e = v[i][j];
    q[i] = (float)e;
  }
  // P55: cv::norm in double, atan2 of P10 rounded to float, the scalar in double
  const double nv = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) +
                         (double)q[3] * (double)q[3]);
  const float ang = (float)lsdm::atan2_(nv, (double)q[0]);
  const double kk = (2.0 * (double)ang) / nv;  // 0 / 0 when the imaginary part is zero
  float rv[3];
  for (int i = 0; i < 3; i++) rv[i] = (float)(kk * (double)q[1 + i]);
  // P56: cv::Rodrigues in double
  {
    double rx = rv[0], ry = rv[1], rz = rv[2];
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < kDblEps) {
      for (int i = 0; i < 9; i++) h.R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    } else {
      const double c = (double)(float)lsdm::cos_(theta), s = (double)(float)lsdm::sin_(theta);
      const double c1 = 1.0 - c, it = 1.0 / theta;
      rx = rx * it;
      ry = ry * it;
      rz = rz * it;
      const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz,
                             rx * rz, ry * rz, rz * rz};
      const double rxm[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
      for (int i = 0; i < 9; i++)
        h.R[i] = (float)((c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * rxm[i]);
    }
  }
  // step 5: P3 = R * Pr2 (P55)
  float P3[3][3];
  for (int i = 0; i < 3; i++)
    for (int c = 0; c < 3; c++)
      P3[i][c] = (float)dot3d(h.R[3 * i], h.R[3 * i + 1], h.R[3 * i + 2], Pr2[0][c], Pr2[1][c],
                              Pr2[2][c]);
  // step 6: scale; Mat::dot and the den loop run over the elements row by row
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    for (int i = 0; i < 3; i++)
      for (int c = 0; c < 3; c++) {
        nom = nom + (double)Pr1[i][c] * (double)P3[i][c];
        den = den + (double)(P3[i][c] * P3[i][c]);
      }
    h.s = (float)(nom / den);
  } else {
    h.s = 1.0f;
  }
  // step 7: t = O1 - (s R) O2 (P57)
  for (int i = 0; i < 3; i++) {
    const float sRO2 = (float)dot3d(h.s * h.R[3 * i], h.s * h.R[3 * i + 1], h.s * h.R[3 * i + 2],
                                    O2[0], O2[1], O2[2]);
    h.t[i] = O1[i] - sRO2;
  }
}

// step 8 (P57): the 3 x 4 parts of mT12i = [s R | t] and mT21i = [sRinv | tinv]
struct Xf {
  float sR[9], t[3], sRi[9], ti[3];
};
SIM3_HD inline void expand(const Hyp& h, Xf& x) {
  const double inv = 1.0 / (double)h.s;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      x.sR[3 * i + j] = h.s * h.R[3 * i + j];
      x.sRi[3 * i + j] = (float)(inv * (double)h.R[3 * j + i]);
    }
    x.t[i] = h.t[i];
  }
  for (int i = 0; i < 3; i++)
    x.ti[i] = -(float)dot3d(x.sRi[3 * i], x.sRi[3 * i + 1], x.sRi[3 * i + 2], h.t[0], h.t[1],
                            h.t[2]);
}
SIM3_HD inline void to_T12(const Hyp& h, float* T) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = h.s * h.R[3 * i + j];
    T[4 * i + 3] = h.t[i];
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

// R * X + t as one gemm (P6): the three products and t are added in double
// and rounded once
SIM3_HD inline void transform(const float* R, const float* t, const float* X, float* Y) {
  for (int i = 0; i < 3; i++)
    Y[i] = (float)(dot3d(R[3 * i], R[3 * i + 1], R[3 * i + 2], X[0], X[1], X[2]) + (double)t[i]);
}
// FromCameraToImage / the tail of Project (:382-423): float, no sign test
SIM3_HD inline void to_image(const float* Xc, const float* cam, float* uv) {
  const float invz = 1.0f / Xc[2];
  const float x = Xc[0] * invz, y = Xc[1] * invz;
  uv[0] = cam[0] * x + cam[2];
  uv[1] = cam[1] * y + cam[3];
}
// dist.dot(dist): Mat::dot accumulates in double, the result is stored as float
SIM3_HD inline float err2(float dx, float dy) {
  return (float)((double)dx * (double)dx + (double)dy * (double)dy);
}

// CheckInliers (:340-364) for one correspondence; e[0..1] = err1, err2
SIM3_HD inline bool is_inlier(const Xf& x, const float* cam, const float* X1, const float* X2,
                              const float* im1, const float* im2, int max1, int max2, float* e) {
  float Y[3], uv[2];
  transform(x.sR, x.t, X2, Y);  // camera 2's point in image 1
  to_image(Y, cam, uv);
  e[0] = err2(im1[0] - uv[0], im1[1] - uv[1]);
  transform(x.sRi, x.ti, X1, Y);  // camera 1's point in image 2
  to_image(Y, cam, uv);
  e[1] = err2(uv[0] - im2[0], uv[1] - im2[1]);
  // mvnMaxError1/2 are vector<size_t>: the float is compared to the integer
  return e[0] < (float)max1 && e[1] < (float)max2;
}

// mvnMaxError's entry: 9.210 * sigma2 in double, truncated toward zero
SIM3_HD inline int max_error(float sigma2) {
  const double v = 9.210 * (double)sigma2;
  if (!(v >= 0.0)) return 0;
  if (v >= 2147483647.0) return INT_MAX;
  return (int)v;
}

// the constructor's test of feature i1 (:64-79); m = matched12[i1]
SIM3_HD inline bool accepts(int m, bool valid1, int n2, const uint8_t* valid2) {
  if (m < 0 || m >= n2) return false;  // no match, or a point keyframe 2 does not observe
  return valid1 && valid2[m];
}

}  // namespace sim3
}  // namespace orbpl
