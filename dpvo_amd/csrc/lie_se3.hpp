// lie_se3.hpp -- SO3 / SE3 device functions of lietorch on gfx950 (L-SE3),
// shared by lie.hip (the lietorch operators) and frontend.hip (motion model,
// trajectory read-out).
//
// Reference semantics: dpvo/lietorch/include/so3.h, se3.h.  Restated without
// Eigen: plain fixed-size register math, templated on float/double, quaternion
// (x, y, z, w) normalised on load (so3.h:95-97), tangent ordering (tau, phi).
#pragma once

#include "common.hpp"
#include "sim3.hpp"

namespace dpvo {
namespace lie {

template <typename S>
struct Q4 { S x, y, z, w; };

template <typename S>
__device__ __forceinline__ Q4<S> qnorm(S x, S y, S z, S w) {
  const S n = sqrt(x * x + y * y + z * z + w * w);
  return {x / n, y / n, z / n, w / n};
}
template <typename S>
__device__ __forceinline__ Q4<S> qmul(const Q4<S>& p, const Q4<S>& q) {  // then normalise
  return qnorm<S>(p.w * q.x + p.x * q.w + p.y * q.z - p.z * q.y,
                  p.w * q.y + p.y * q.w + p.z * q.x - p.x * q.z,
                  p.w * q.z + p.z * q.w + p.x * q.y - p.y * q.x,
                  p.w * q.w - p.x * q.x - p.y * q.y - p.z * q.z);
}
template <typename S>
__device__ __forceinline__ void cross(const S* a, const S* b, S* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename S>
__device__ __forceinline__ void qact(const Q4<S>& q, const S* p, S* o) {  // so3.h:115-120
  const S v[3] = {q.x, q.y, q.z};
  S uv[3], uv2[3];
  cross(v, p, uv);
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  cross(v, uv, uv2);
  for (int i = 0; i < 3; i++) o[i] = p[i] + q.w * uv[i] + uv2[i];
}
template <typename S>
__device__ __forceinline__ void qmat(const Q4<S>& q, S* R) {  // Eigen toRotationMatrix
  const S tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const S twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const S txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const S tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
template <typename S>
__device__ __forceinline__ void hat(const S* p, S* H) {  // so3.h:161-169
  H[0] = 0; H[1] = -p[2]; H[2] = p[1];
  H[3] = p[2]; H[4] = 0; H[5] = -p[0];
  H[6] = -p[1]; H[7] = p[0]; H[8] = 0;
}
template <typename S>
__device__ __forceinline__ void mm3(const S* A, const S* B, S* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
// ---- coefficient functions ----
// Every scalar coefficient of Exp, Log, J_l, J_l^-1 and Q is a function of
// t2 = theta^2 alone.  The textbook closed forms (so3.h:175-268, se3.h:133-162)
// cancel for small theta -- (1 - cos t) / t^2 loses 1 / t^2 of the precision,
// Q's (2t - 3 sin t + t cos t) / (2 t^5) loses 1 / t^4 -- and lietorch's switch
// to a two-term series only below theta = 1e-6 leaves the whole band up to
// ~1e-2 wrong: 1e-9 in fp64, 1e-2 in fp32.  Here they are evaluated in fp64
// for both tensor types (a handful of scalar operations per element; the
// matrix algebra around them stays in S), by five terms of the series in t2
// below sim3::kTheta2 (next term < 1e-17 of the leading one) and above it by
// forms whose cancellation costs at most 1 / t2 = 400 roundoffs of fp64.
struct JlCoef {
  double b, c;  // (1 - cos t) / t^2, (t - sin t) / t^3
};
__device__ __forceinline__ JlCoef jl_coef(double t2) {
  JlCoef k;
  if (t2 < sim3::kTheta2) {
    k.b = 0.5 - t2 * (1.0 / 24 - t2 * (1.0 / 720 - t2 * (1.0 / 40320 - t2 * (1.0 / 3628800))));
    k.c = 1.0 / 6 - t2 * (1.0 / 120 - t2 * (1.0 / 5040 - t2 * (1.0 / 362880 - t2 * (1.0 / 39916800))));
  } else {
    const double t = sqrt(t2), sh = sin(0.5 * t);
    k.b = 2 * sh * sh / t2;  // 1 - cos t = 2 sin^2(t / 2)
    k.c = (t - sin(t)) / (t2 * t);
  }
  return k;
}
// (t^2 + 2 cos t - 2) / (2 t^4) and (2t - 3 sin t + t cos t) / (2 t^5) of se3_Q
__device__ __forceinline__ void q_coef(double t2, const JlCoef& k, double& c2, double& c3) {
  if (t2 < sim3::kTheta2) {
    c2 = 1.0 / 24 - t2 * (1.0 / 720 - t2 * (1.0 / 40320 - t2 * (1.0 / 3628800 - t2 * (1.0 / 479001600))));
    c3 = 1.0 / 120 - t2 * (2.0 / 5040 - t2 * (3.0 / 362880 - t2 * (4.0 / 39916800 - t2 * (5.0 / 6227020800))));
  } else {  // the same numerators through b and c
    c2 = (0.5 - k.b) / t2;
    c3 = (3 * k.c - k.b) / (2 * t2);
  }
}
// (1 - (t / 2) cot(t / 2)) / t^2 of J_l^-1
__device__ __forceinline__ double jl_inv_coef(double t2) {
  if (t2 < sim3::kTheta2)
    return 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600 + t2 * (1.0 / 47900160))));
  const double ht = 0.5 * sqrt(t2);
  return (1 - ht * cos(ht) / sin(ht)) / t2;
}

template <typename S>
__device__ __forceinline__ void so3_log(const Q4<S>& q, S* o) {  // so3.h:175-211
  const double sq = (double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z;
  const double w = q.w;
  double f;  // 2 atan(n / w) / n, n = |v|
  if (sq < sim3::kLogR2 * w * w) {
    const double r = sq / (w * w);
    f = 2 / w * (1 - r * (1.0 / 3 - r * (1.0 / 5 - r * (1.0 / 7 - r * (1.0 / 9 - r * (1.0 / 11))))));
  } else {  // atan2 is exact through w = 0 (theta = pi), where lietorch puts +-pi / n
    const double n = sqrt(sq);
    f = (w < 0 ? -2 : 2) * atan2(n, fabs(w)) / n;
  }
  o[0] = (S)(f * q.x); o[1] = (S)(f * q.y); o[2] = (S)(f * q.z);
}
template <typename S>
__device__ __forceinline__ Q4<S> so3_exp(const S* phi) {  // so3.h:213-230
  const double t2 = (double)(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
  double im, re;
  if (t2 < sim3::kTheta2) {
    const double h = 0.25 * t2;  // (theta / 2)^2
    im = 0.5 * (1 - h * (1.0 / 6 - h * (1.0 / 120 - h * (1.0 / 5040 - h * (1.0 / 362880)))));
    re = 1 - h * (0.5 - h * (1.0 / 24 - h * (1.0 / 720 - h * (1.0 / 40320))));
  } else {
    const double t = sqrt(t2);
    im = sin(0.5 * t) / t;
    re = cos(0.5 * t);
  }
  return qnorm<S>((S)im * phi[0], (S)im * phi[1], (S)im * phi[2], (S)re);
}
template <typename S>
__device__ __forceinline__ void so3_jl(const S* phi, S* J) {  // so3.h:232-250
  S Ph[9], Ph2[9];
  hat(phi, Ph);
  mm3(Ph, Ph, Ph2);
  const JlCoef k = jl_coef((double)(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]));
  const S c1 = (S)k.b, c2 = (S)k.c;
  for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0 ? S(1) : S(0)) + c1 * Ph[i] + c2 * Ph2[i];
}
template <typename S>
__device__ __forceinline__ void so3_jl_inv(const S* phi, S* J) {  // so3.h:252-268
  S Ph[9], Ph2[9];
  hat(phi, Ph);
  mm3(Ph, Ph, Ph2);
  const S c2 = (S)jl_inv_coef((double)(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]));
  for (int i = 0; i < 9; i++) J[i] = (i % 4 == 0 ? S(1) : S(0)) + S(-0.5) * Ph[i] + c2 * Ph2[i];
}
template <typename S>
__device__ __forceinline__ void se3_Q(const S* xi, S* Qm) {  // se3.h:133-162
  S Ta[9], Ph[9];
  hat(xi, Ta);
  hat(xi + 3, Ph);
  const double t2 = (double)(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
  const JlCoef k = jl_coef(t2);
  double d2, d3;
  q_coef(t2, k, d2, d3);
  const S c1 = (S)k.c, c2 = (S)d2, c3 = (S)d3;
  S PT[9], TP[9], PTP[9], PPT[9], TPP[9], PTPP[9], PPTP[9];
  mm3(Ph, Ta, PT); mm3(Ta, Ph, TP); mm3(PT, Ph, PTP);
  mm3(Ph, PT, PPT); mm3(TP, Ph, TPP); mm3(PTP, Ph, PTPP); mm3(Ph, PTP, PPTP);
  for (int i = 0; i < 9; i++)
    Qm[i] = S(0.5) * Ta[i] + c1 * (PT[i] + TP[i] + PTP[i]) + c2 * (PPT[i] + TPP[i] - 3 * PTP[i]) +
            c3 * (PTPP[i] + PPTP[i]);
}

// 6x6 row-major helpers
template <typename S>
__device__ __forceinline__ void blocks6(const S* A, const S* B, const S* D, S* M) {
  // M = [[A, B], [0, D]]
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      M[i * 6 + j] = A[i * 3 + j];
      M[i * 6 + 3 + j] = B[i * 3 + j];
      M[(3 + i) * 6 + j] = 0;
      M[(3 + i) * 6 + 3 + j] = D[i * 3 + j];
    }
}
template <typename S>
__device__ __forceinline__ void rowvec_mat(const S* v, const S* M, int n, int m, S* o) {
  for (int j = 0; j < m; j++) {
    S s = 0;
    for (int i = 0; i < n; i++) s += v[i] * M[i * m + j];
    o[j] = s;
  }
}
template <typename S>
__device__ __forceinline__ void mat_vec(const S* M, const S* v, int n, int m, S* o) {
  for (int i = 0; i < n; i++) {
    S s = 0;
    for (int j = 0; j < m; j++) s += M[i * m + j] * v[j];
    o[i] = s;
  }
}

template <typename S>
struct SE3g {
  S t[3];
  Q4<S> q;
};
template <typename S>
__device__ __forceinline__ SE3g<S> se3_load(const S* d) {
  SE3g<S> g;
  g.t[0] = d[0]; g.t[1] = d[1]; g.t[2] = d[2];
  g.q = qnorm<S>(d[3], d[4], d[5], d[6]);
  return g;
}
template <typename S>
__device__ __forceinline__ void se3_store(const SE3g<S>& g, S* d) {
  d[0] = g.t[0]; d[1] = g.t[1]; d[2] = g.t[2];
  d[3] = g.q.x; d[4] = g.q.y; d[5] = g.q.z; d[6] = g.q.w;
}
template <typename S>
__device__ __forceinline__ SE3g<S> se3_inv(const SE3g<S>& g) {  // se3.h:325-327
  SE3g<S> o;
  o.q = qnorm<S>(-g.q.x, -g.q.y, -g.q.z, g.q.w);
  S t[3];
  qact(o.q, g.t, t);
  o.t[0] = -t[0]; o.t[1] = -t[1]; o.t[2] = -t[2];
  return o;
}
template <typename S>
__device__ __forceinline__ SE3g<S> se3_mul(const SE3g<S>& a, const SE3g<S>& b) {  // :334-336
  SE3g<S> o;
  o.q = qmul(a.q, b.q);
  S t[3];
  qact(a.q, b.t, t);
  for (int i = 0; i < 3; i++) o.t[i] = a.t[i] + t[i];
  return o;
}
template <typename S>
__device__ __forceinline__ void se3_Adj(const SE3g<S>& g, S* A) {  // se3.h:347-356
  S R[9], tx[9], tR[9];
  qmat(g.q, R);
  hat(g.t, tx);
  mm3(tx, R, tR);
  blocks6(R, tR, R, A);
}
template <typename S>
__device__ __forceinline__ void se3_adj_small(const S* xi, S* A) {  // se3.h:389-401
  S Ta[9], Ph[9];
  hat(xi, Ta);
  hat(xi + 3, Ph);
  blocks6(Ph, Ta, Ph, A);
}
template <typename S>
__device__ __forceinline__ SE3g<S> se3_exp(const S* xi) {  // se3.h:423-431
  SE3g<S> g;
  g.q = so3_exp(xi + 3);
  S J[9];
  so3_jl(xi + 3, J);
  for (int i = 0; i < 3; i++) g.t[i] = J[i * 3] * xi[0] + J[i * 3 + 1] * xi[1] + J[i * 3 + 2] * xi[2];
  return g;
}
template <typename S>
__device__ __forceinline__ void se3_log(const SE3g<S>& g, S* xi) {  // se3.h:413-421
  so3_log(g.q, xi + 3);
  S Vi[9];
  so3_jl_inv(xi + 3, Vi);
  for (int i = 0; i < 3; i++) xi[i] = Vi[i * 3] * g.t[0] + Vi[i * 3 + 1] * g.t[1] + Vi[i * 3 + 2] * g.t[2];
}
template <typename S>
__device__ __forceinline__ void se3_jl(const S* xi, S* J) {  // se3.h:464-475
  S Jr[9], Qm[9];
  so3_jl(xi + 3, Jr);
  se3_Q(xi, Qm);
  blocks6(Jr, Qm, Jr, J);
}
template <typename S>
__device__ __forceinline__ void se3_jl_inv(const S* xi, S* J) {  // se3.h:477-490
  S Ji[9], Qm[9], T1[9], T2[9];
  so3_jl_inv(xi + 3, Ji);
  se3_Q(xi, Qm);
  mm3(Ji, Qm, T1);
  mm3(T1, Ji, T2);
  for (int i = 0; i < 9; i++) T2[i] = -T2[i];
  blocks6(Ji, T2, Ji, J);
}

}  // namespace lie
}  // namespace dpvo
