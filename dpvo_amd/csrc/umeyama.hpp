// umeyama.hpp -- Umeyama's Sim(3) fit from the moments of two point sets, fp64,
// one thread.  Shared by the loop-closure RANSAC (ransac.hip) and the
// trajectory evaluation (evaluate.hip): one copy, so both round identically.
//
// The covariance of three points has rank <= 2, so the SVD cannot deliver the
// third singular vectors.  One-sided Jacobi gives A V = U diag(d); with the
// columns ordered by d, R = [u0 u1 u0 x u1] [v0 v1 v0 x v1]^T is the proper
// rotation U S V^T of Umeyama's eq. 40 for any rank >= 2: the two cross
// products have determinant +1 each, which is where the Kabsch sign S ends up.
// The sign itself (det U det V of the Jacobi factors) is only needed for the
// scale, c = (d0 + d1 +- d2) / sigma_x.
#pragma once

#include "common.hpp"

namespace dpvo {
namespace umeyama {

constexpr double kRankEps = 2.220446049250313e-16;  // np.finfo(float64).eps, absolute
constexpr int kMaxSweeps = 12;

struct Model {
  double R[9], t[3], c;
  bool ok;
};

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double dot3(const double* a, const double* b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// Umeyama (1991) eq. 40-42 from the means, sigma_x and the covariance
// cov[r][c] = mean((y - mean_y)[r] (x - mean_x)[c]).
__device__ inline Model umeyama_from_moments(const double* mx, const double* my, double sigma_x,
                                             const double* cov) {
  // columns of G = cov V, V starts as the identity
  double g[3][3], v[3][3];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      g[k][r] = cov[r * 3 + k];
      v[k][r] = r == k ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int pq = 0; pq < 3; pq++) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double al = dot3(g[p], g[p]), be = dot3(g[q], g[q]), ga = dot3(g[p], g[q]);
      if (ga == 0.0 || fabs(ga) <= 1e-16 * sqrt(al * be)) continue;
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double gp = g[p][r], gq = g[q][r], vp = v[p][r], vq = v[q][r];
        g[p][r] = cs * gp - sn * gq;
        g[q][r] = sn * gp + cs * gq;
        v[p][r] = cs * vp - sn * vq;
        v[q][r] = sn * vp + cs * vq;
      }
    }
    if (!rotated) break;
  }
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; k++) d[k] = sqrt(dot3(g[k], g[k]));
  // order the columns by singular value, largest first
  auto swap_cols = [&](int a, int b) {
    if (d[a] < d[b]) {
      const double td = d[a];
      d[a] = d[b];
      d[b] = td;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double tg = g[a][r], tv = v[a][r];
        g[a][r] = g[b][r];
        g[b][r] = tg;
        v[a][r] = v[b][r];
        v[b][r] = tv;
      }
    }
  };
  swap_cols(0, 1);
  swap_cols(0, 2);
  swap_cols(1, 2);
  Model m;
  // the reference: fewer than m - 1 = 2 singular values above eps -> no model
  m.ok = d[1] > kRankEps && sigma_x > 0.0;
  if (!m.ok) return m;
  double u0[3], u1[3], u2[3], v2[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    u0[r] = g[0][r] / d[0];
    u1[r] = g[1][r] / d[1];
  }
  cross3(u0, u1, u2);
  cross3(v[0], v[1], v2);
  // det U det V of the Jacobi factors: the sign of d2 in tr(D S)
  const double sgn = dot3(g[2], u2) * dot3(v[2], v2) < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int k = 0; k < 3; k++)
      m.R[r * 3 + k] = u0[r] * v[0][k] + u1[r] * v[1][k] + u2[r] * v2[k];
  m.c = (d[0] + d[1] + sgn * d[2]) / sigma_x;
#pragma unroll
  for (int r = 0; r < 3; r++)
    m.t[r] = my[r] - m.c * (m.R[r * 3] * mx[0] + m.R[r * 3 + 1] * mx[1] + m.R[r * 3 + 2] * mx[2]);
  return m;
}

}  // namespace umeyama
}  // namespace dpvo
