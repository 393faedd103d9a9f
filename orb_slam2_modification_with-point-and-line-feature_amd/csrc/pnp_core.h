// PnPsolver's arithmetic (PnPsolver.cc:308-950) as pinned in DESIGN.md P28:
// EPnP in double with only + - * / sqrt, the OpenCV SVD calls replaced by one
// one-sided Jacobi routine, and every reduction over the correspondences
// summed as kParts strided partials that are then added in ascending order.
// The code is shared by the one-thread-per-hypothesis path (SeqReduce) and the
// workgroup-parallel Refine() path (a reducer in pnp.hip): the reducer is the
// only difference, so both follow the same operation order.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PNP_HD __host__ __device__
#else
#define PNP_HD
#endif

namespace orbpl {
namespace pnp {

constexpr int kParts = 256;                            // strided partial sums per reduction
constexpr int kMaxSweeps = 30;                         // Jacobi sweeps, upper bound
constexpr double kJacobiTol = 1.4210854715202004e-14;  // 2^-46: columns count as orthogonal
constexpr double kEps = 2.220446049250313e-16;         // 2^-52, rank threshold unit

// One-sided (Hestenes) Jacobi SVD of the row-major m x n matrix A, n <= 12.
// Pairs (p, q), p < q, row-cyclic; a pair is rotated when |a_p . a_q| >
// kJacobiTol * sqrt(|a_p|^2 |a_q|^2); sweeps stop after one without a rotation
// or after kMaxSweeps. On return A holds U (column k = A v_k / s_k, zero where
// s_k == 0), s the singular values descending (first maximum first) and V the
// right singular vectors as columns.
PNP_HD inline void svd_jacobi(double* A, int m, int n, double* s, double* V) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    int rotations = 0;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < m; i++) {
          const double ap = A[i * n + p], aq = A[i * n + q];
          alpha = alpha + ap * ap;
          beta = beta + aq * aq;
          gamma = gamma + ap * aq;
        }
        if (!(fabs(gamma) > kJacobiTol * sqrt(alpha * beta))) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        double t = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        if (zeta < 0.0) t = -t;
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int i = 0; i < m; i++) {
          const double ap = A[i * n + p], aq = A[i * n + q];
          A[i * n + p] = c * ap - sn * aq;
          A[i * n + q] = sn * ap + c * aq;
        }
        for (int i = 0; i < n; i++) {
          const double vp = V[i * n + p], vq = V[i * n + q];
          V[i * n + p] = c * vp - sn * vq;
          V[i * n + q] = sn * vp + c * vq;
        }
        rotations++;
      }
    if (!rotations) break;
  }
  for (int k = 0; k < n; k++) {
    double ss = 0.0;
    for (int i = 0; i < m; i++) ss = ss + A[i * n + k] * A[i * n + k];
    s[k] = sqrt(ss);
  }
  for (int k = 0; k < n - 1; k++) {
    int best = k;
    for (int j = k + 1; j < n; j++)
      if (s[j] > s[best]) best = j;
    if (best == k) continue;
    double tmp = s[k];
    s[k] = s[best];
    s[best] = tmp;
    for (int i = 0; i < m; i++) {
      tmp = A[i * n + k];
      A[i * n + k] = A[i * n + best];
      A[i * n + best] = tmp;
    }
    for (int i = 0; i < n; i++) {
      tmp = V[i * n + k];
      V[i * n + k] = V[i * n + best];
      V[i * n + best] = tmp;
    }
  }
  for (int k = 0; k < n; k++)
    for (int i = 0; i < m; i++) A[i * n + k] = s[k] > 0.0 ? A[i * n + k] / s[k] : 0.0;
}

// singular value k takes part in a pseudo-inverse / least-squares solve
PNP_HD inline bool svd_in_rank(const double* s, int k, int m, int n) {
  return s[k] > s[0] * ((double)(m > n ? m : n) * kEps);
}

// cvSolve(A, b, x, CV_SVD): x = V diag(1 / s) U^T b over the singular values in
// rank. A (m x n, n <= 5) is destroyed.
PNP_HD inline void svd_solve(double* A, int m, int n, const double* b, double* x) {
  double s[5], V[25], y[5];
  svd_jacobi(A, m, n, s, V);
  for (int k = 0; k < n; k++) {
    y[k] = 0.0;
    if (!svd_in_rank(s, k, m, n)) continue;
    for (int i = 0; i < m; i++) y[k] = y[k] + A[i * n + k] * b[i];
    y[k] = y[k] / s[k];
  }
  for (int j = 0; j < n; j++) {
    x[j] = 0.0;
    for (int k = 0; k < n; k++) x[j] = x[j] + V[j * n + k] * y[k];
  }
}

PNP_HD inline double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
PNP_HD inline double dist2(const double* a, const double* b) {
  return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) +
         (a[2] - b[2]) * (a[2] - b[2]);
}

// PnPsolver::qr_solve (:860-950) for the 6 x 4 system, as written: the pivot
// scan stops one row early, and a zero pivot returns with x untouched.
PNP_HD inline void qr_solve_6x4(double* A, double* b, double* x) {
  const int nr = 6, nc = 4;
  double A1[4], A2[4];
  for (int k = 0; k < nc; k++) {
    double eta = fabs(A[k * nc + k]);
    for (int i = k + 1; i < nr; i++) {
      const double elt = fabs(A[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) return;
    const double inv_eta = 1. / eta;
    double sum = 0.0;
    for (int i = k; i < nr; i++) {
      A[i * nc + k] *= inv_eta;
      sum = sum + A[i * nc + k] * A[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (A[k * nc + k] < 0) sigma = -sigma;
    A[k * nc + k] += sigma;
    A1[k] = sigma * A[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double sm = 0;
      for (int i = k; i < nr; i++) sm = sm + A[i * nc + k] * A[i * nc + j];
      const double tau = sm / A1[k];
      for (int i = k; i < nr; i++) A[i * nc + j] -= tau * A[i * nc + k];
    }
  }
  for (int j = 0; j < nc; j++) {
    double tau = 0;
    for (int i = j; i < nr; i++) tau = tau + A[i * nc + j] * b[i];
    tau /= A1[j];
    for (int i = j; i < nr; i++) b[i] -= tau * A[i * nc + j];
  }
  x[nc - 1] = b[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < nc; j++) sum = sum + A[i * nc + j] * x[j];
    x[i] = (b[i] - sum) / A2[i];
  }
}

PNP_HD inline void gauss_newton(const double* L, const double* rho, double* betas) {
  double x[4] = {0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < 5; it++) {
    double a[24], b[6];
    for (int i = 0; i < 6; i++) {
      const double* r = L + i * 10;
      double* ra = a + i * 4;
      ra[0] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3];
      ra[1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3];
      ra[2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3];
      ra[3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3];
      b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] +
                       r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                       r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] +
                       r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                       r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3]);
    }
    qr_solve_6x4(a, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

// find_betas_approx_1 / _2 / _3 (:667-758); which = 1, 2, 3
PNP_HD inline void find_betas_approx(int which, const double* L, const double* rho,
                                     double* betas) {
  double l[30], b[5];
  if (which == 1) {
    const int col[4] = {0, 1, 3, 6};
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 4; j++) l[i * 4 + j] = L[i * 10 + col[j]];
    svd_solve(l, 6, 4, rho, b);
    if (b[0] < 0) {
      betas[0] = sqrt(-b[0]);
      betas[1] = -b[1] / betas[0];
      betas[2] = -b[2] / betas[0];
      betas[3] = -b[3] / betas[0];
    } else {
      betas[0] = sqrt(b[0]);
      betas[1] = b[1] / betas[0];
      betas[2] = b[2] / betas[0];
      betas[3] = b[3] / betas[0];
    }
    return;
  }
  const int nc = which == 2 ? 3 : 5;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < nc; j++) l[i * nc + j] = L[i * 10 + j];
  svd_solve(l, 6, nc, rho, b);
  if (b[0] < 0) {
    betas[0] = sqrt(-b[0]);
    betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
  } else {
    betas[0] = sqrt(b[0]);
    betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
  }
  if (b[1] < 0) betas[0] = -betas[0];
  betas[2] = which == 2 ? 0.0 : b[3] / betas[0];
  betas[3] = 0.0;
}

// Every small matrix of one compute_pose() call. In the workgroup path it
// lives in LDS and is written by the leader thread only.
struct Work {
  double cam[4];  // fu fv uc vc
  double sum[9];  // result of the running reduction
  double cws[4][3], ci[9];
  double A[144], V[144], s[12];  // MtM -> U, V (ut row r = column r of V)
  double L[60], rho[6], betas[4];
  double ccs[4][3], pc0[3];
  double Rs[3][9], ts[3][3], err[3];
  double R[9], t[3];  // compute_pose's result
};

PNP_HD inline void alphas_of(const Work& w, const double* pw, double* a) {
  for (int j = 0; j < 3; j++)
    a[1 + j] = w.ci[3 * j] * (pw[0] - w.cws[0][0]) + w.ci[3 * j + 1] * (pw[1] - w.cws[0][1]) +
               w.ci[3 * j + 2] * (pw[2] - w.cws[0][2]);
  a[0] = 1.0 - a[1] - a[2] - a[3];
}
PNP_HD inline void pc_of(const Work& w, const double* a, double* pc) {
  for (int j = 0; j < 3; j++)
    pc[j] = a[0] * w.ccs[0][j] + a[1] * w.ccs[1][j] + a[2] * w.ccs[2][j] + a[3] * w.ccs[3][j];
}

// The reduction order of P28 on one thread.
struct SeqReduce {
  PNP_HD bool leader() const { return true; }
  template <int C, class F>
  PNP_HD void run(int n, F f, double* out) {
    for (int c = 0; c < C; c++) out[c] = 0.0;
    for (int j = 0; j < kParts && j < n; j++) {
      double part[C];
      for (int c = 0; c < C; c++) part[c] = 0.0;
      for (int i = j; i < n; i += kParts) f(i, part);
      for (int c = 0; c < C; c++) out[c] = out[c] + part[c];
    }
  }
};

// PnPsolver::compute_pose (:477-525) over the n correspondences P.get(i, pw,
// uv) hands out. w.cam is set by the caller; the result is w.R / w.t. Every
// thread of the reducer's group calls this; red.run() returns its sums in
// w.sum to all of them, the leader alone does the small-matrix steps.
template <class Pts, class Red>
PNP_HD inline void compute_pose(const Pts& P, int n, Red& red, Work& w) {
  const double dn = (double)n;
  // choose_control_points
  red.template run<3>(n, [&](int i, double* a) {
    double pw[3], uv[2];
    P.get(i, pw, uv);
    for (int j = 0; j < 3; j++) a[j] = a[j] + pw[j];
  }, w.sum);
  if (red.leader())
    for (int j = 0; j < 3; j++) w.cws[0][j] = w.sum[j] / dn;
  red.template run<9>(n, [&](int i, double* a) {
    double pw[3], uv[2], d[3];
    P.get(i, pw, uv);
    for (int j = 0; j < 3; j++) d[j] = pw[j] - w.cws[0][j];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) a[3 * r + c] = a[3 * r + c] + d[r] * d[c];
  }, w.sum);
  if (red.leader()) {
    double G[9], s3[3], V3[9], cc[9];
    for (int j = 0; j < 9; j++) G[j] = w.sum[j];
    svd_jacobi(G, 3, 3, s3, V3);
    for (int i = 1; i < 4; i++) {
      const double k = sqrt(s3[i - 1] / dn);
      for (int j = 0; j < 3; j++) w.cws[i][j] = w.cws[0][j] + k * V3[j * 3 + (i - 1)];
    }
    // compute_barycentric_coordinates: cvInvert(CC, CV_SVD)
    for (int i = 0; i < 3; i++)
      for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = w.cws[j][i] - w.cws[0][i];
    svd_jacobi(cc, 3, 3, s3, V3);
    for (int j = 0; j < 3; j++)
      for (int i = 0; i < 3; i++) {
        double v = 0.0;
        for (int k = 0; k < 3; k++)
          if (svd_in_rank(s3, k, 3, 3)) v = v + V3[j * 3 + k] * (cc[i * 3 + k] / s3[k]);
        w.ci[3 * j + i] = v;
      }
  }
  // MtM (fill_M + cvMulTransposed), half a row per reduction
  for (int h = 0; h < 24; h++) {
    const int ra = h >> 1, b0 = (h & 1) * 6;
    red.template run<6>(n, [&](int i, double* acc) {
      double pw[3], uv[2], a[4], M1[12], M2[12];
      P.get(i, pw, uv);
      alphas_of(w, pw, a);
      for (int j = 0; j < 4; j++) {
        M1[3 * j] = a[j] * w.cam[0];
        M1[3 * j + 1] = 0.0;
        M1[3 * j + 2] = a[j] * (w.cam[2] - uv[0]);
        M2[3 * j] = 0.0;
        M2[3 * j + 1] = a[j] * w.cam[1];
        M2[3 * j + 2] = a[j] * (w.cam[3] - uv[1]);
      }
      for (int b = 0; b < 6; b++) {
        acc[b] = acc[b] + M1[ra] * M1[b0 + b];
        acc[b] = acc[b] + M2[ra] * M2[b0 + b];
      }
    }, w.sum);
    if (red.leader())
      for (int b = 0; b < 6; b++) w.A[12 * ra + b0 + b] = w.sum[b];
  }
  if (red.leader()) {
    svd_jacobi(w.A, 12, 12, w.s, w.V);
    // compute_L_6x10: v[i] = ut row 11 - i = column 11 - i of V
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
      int a = 0, b = 1;
      for (int j = 0; j < 6; j++) {
        for (int k = 0; k < 3; k++)
          dv[i][j][k] = w.V[(3 * a + k) * 12 + (11 - i)] - w.V[(3 * b + k) * 12 + (11 - i)];
        b++;
        if (b > 3) {
          a++;
          b = a + 1;
        }
      }
    }
    for (int i = 0; i < 6; i++) {
      double* row = w.L + 10 * i;
      row[0] = dot3(dv[0][i], dv[0][i]);
      row[1] = 2.0 * dot3(dv[0][i], dv[1][i]);
      row[2] = dot3(dv[1][i], dv[1][i]);
      row[3] = 2.0 * dot3(dv[0][i], dv[2][i]);
      row[4] = 2.0 * dot3(dv[1][i], dv[2][i]);
      row[5] = dot3(dv[2][i], dv[2][i]);
      row[6] = 2.0 * dot3(dv[0][i], dv[3][i]);
      row[7] = 2.0 * dot3(dv[1][i], dv[3][i]);
      row[8] = 2.0 * dot3(dv[2][i], dv[3][i]);
      row[9] = dot3(dv[3][i], dv[3][i]);
    }
    w.rho[0] = dist2(w.cws[0], w.cws[1]);
    w.rho[1] = dist2(w.cws[0], w.cws[2]);
    w.rho[2] = dist2(w.cws[0], w.cws[3]);
    w.rho[3] = dist2(w.cws[1], w.cws[2]);
    w.rho[4] = dist2(w.cws[1], w.cws[3]);
    w.rho[5] = dist2(w.cws[2], w.cws[3]);
  }
  for (int sol = 0; sol < 3; sol++) {
    if (red.leader()) {
      find_betas_approx(sol + 1, w.L, w.rho, w.betas);
      gauss_newton(w.L, w.rho, w.betas);
      // compute_ccs, then solve_for_sign on the first point's depth
      for (int i = 0; i < 4; i++) w.ccs[i][0] = w.ccs[i][1] = w.ccs[i][2] = 0.0;
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
          for (int k = 0; k < 3; k++)
            w.ccs[j][k] = w.ccs[j][k] + w.betas[i] * w.V[(3 * j + k) * 12 + (11 - i)];
      double pw[3], uv[2], a[4], pc[3];
      P.get(0, pw, uv);
      alphas_of(w, pw, a);
      pc_of(w, a, pc);
      if (pc[2] < 0.0)
        for (int i = 0; i < 4; i++)
          for (int j = 0; j < 3; j++) w.ccs[i][j] = -w.ccs[i][j];
    }
    // estimate_R_and_t: pw0 is the centroid cws[0] (the same sum in the same order)
    red.template run<3>(n, [&](int i, double* acc) {
      double pw[3], uv[2], a[4], pc[3];
      P.get(i, pw, uv);
      alphas_of(w, pw, a);
      pc_of(w, a, pc);
      for (int j = 0; j < 3; j++) acc[j] = acc[j] + pc[j];
    }, w.sum);
    if (red.leader())
      for (int j = 0; j < 3; j++) w.pc0[j] = w.sum[j] / dn;
    red.template run<9>(n, [&](int i, double* acc) {
      double pw[3], uv[2], a[4], pc[3];
      P.get(i, pw, uv);
      alphas_of(w, pw, a);
      pc_of(w, a, pc);
      for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++)
          acc[3 * j + k] = acc[3 * j + k] + (pc[j] - w.pc0[j]) * (pw[k] - w.cws[0][k]);
    }, w.sum);
    if (red.leader()) {
      double U[9], s3[3], V3[9];
      for (int j = 0; j < 9; j++) U[j] = w.sum[j];
      svd_jacobi(U, 3, 3, s3, V3);
      if (!svd_in_rank(s3, 2, 3, 3)) {  // rank 2: the third left vector is u0 x u1
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
      }
      double* R = w.Rs[sol];
      double* t = w.ts[sol];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = dot3(U + 3 * i, V3 + 3 * j);
      const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] -
                         R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
      if (det < 0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
      }
      t[0] = w.pc0[0] - dot3(R, w.cws[0]);
      t[1] = w.pc0[1] - dot3(R + 3, w.cws[0]);
      t[2] = w.pc0[2] - dot3(R + 6, w.cws[0]);
    }
    red.template run<1>(n, [&](int i, double* acc) {
      double pw[3], uv[2];
      P.get(i, pw, uv);
      const double* R = w.Rs[sol];
      const double* t = w.ts[sol];
      const double Xc = dot3(R, pw) + t[0];
      const double Yc = dot3(R + 3, pw) + t[1];
      const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
      const double ue = w.cam[2] + w.cam[0] * Xc * inv_Zc;
      const double ve = w.cam[3] + w.cam[1] * Yc * inv_Zc;
      acc[0] = acc[0] + sqrt((uv[0] - ue) * (uv[0] - ue) + (uv[1] - ve) * (uv[1] - ve));
    }, w.sum);
    if (red.leader()) w.err[sol] = w.sum[0] / dn;
  }
  if (red.leader()) {
    int best = 0;
    if (w.err[1] < w.err[0]) best = 1;
    if (w.err[2] < w.err[best]) best = 2;
    for (int j = 0; j < 9; j++) w.R[j] = w.Rs[best][j];
    for (int j = 0; j < 3; j++) w.t[j] = w.ts[best][j];
  }
}

// PnPsolver::CheckInliers (:308-339) for one correspondence
PNP_HD inline bool is_inlier(const double* R, const double* t, const double* cam,
                             const float* p3, const float* p2, float max_error) {
  const float Xc = (float)(R[0] * p3[0] + R[1] * p3[1] + R[2] * p3[2] + t[0]);
  const float Yc = (float)(R[3] * p3[0] + R[4] * p3[1] + R[5] * p3[2] + t[1]);
  const float invZc = (float)(1 / (R[6] * p3[0] + R[7] * p3[1] + R[8] * p3[2] + t[2]));
  const double ue = cam[2] + cam[0] * Xc * invZc;
  const double ve = cam[3] + cam[1] * Yc * invZc;
  const float distX = (float)(p2[0] - ue);
  const float distY = (float)(p2[1] - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < max_error;
}

// DUtils::Random::RandomInt(0, size - 1) on a raw rand() value (P29);
// rand_max_p1 = (double)RAND_MAX + 1.0
PNP_HD inline int random_int(int raw, int size, double rand_max_p1) {
  return (int)(((double)raw / rand_max_p1) * size);
}

// The K indices hypothesis draws d[0..K-1] pick from mvAllIndices = 0..N-1
// with the swap-with-back removal (:188-201; Sim3Solver.cc:163-177 with K = 3),
// N >= K.
template <int K>
PNP_HD inline void sample_k(const int* d, int N, double rand_max_p1, int* idx) {
  int pos[K], val[K], nov = 0;
  for (int i = 0; i < K; i++) {
    const int size = N - i;
    int r = random_int(d[i], size, rand_max_p1);
    r = r < 0 ? 0 : (r > size - 1 ? size - 1 : r);  // raw values outside [0, RAND_MAX]
    int v = r, back = size - 1;
    for (int k = 0; k < nov; k++) {  // later overrides win
      if (pos[k] == r) v = val[k];
      if (pos[k] == size - 1) back = val[k];
    }
    idx[i] = v;
    pos[nov] = r;
    val[nov] = back;
    nov++;
  }
}
PNP_HD inline void sample4(const int* d, int N, double rand_max_p1, int* idx) {
  sample_k<4>(d, N, rand_max_p1, idx);
}

}  // namespace pnp
}  // namespace orbpl
