// sim3.hpp -- Sim3 (lietorch group 4) register math, shared by lie.hip (the
// group ops) and pgo.hip (the pose-graph residual kernel).
//
// Conventions are lietorch's (dpvo/lietorch/include/sim3.h, rxso3.h): data
// (tx, ty, tz, qx, qy, qz, qw, s), tangent (tau, phi, sigma), X = [[sR, t], [0, 1]].
// Everything is templated on the scalar T = double or Dual (one forward-mode
// direction), so every derivative this build needs -- the left Jacobian of
// Exp, its inverse, the pose-graph Jacobians -- is the derivative of the very
// code that computes the value.  Arithmetic is fp64 for f32 tensors too.
//
// Small arguments.  W(phi, sigma) = C I + A Phi + B Phi^2 is the integral of
// exp(u (Phi + sigma I)) over u in [0, 1]:
//   C = I_0,  A = sum_k (-theta^2)^k I_{2k+1} / (2k+1)!,
//   B = sum_k (-theta^2)^k I_{2k+2} / (2k+2)!,   I_m(sigma) = int_0^1 u^m e^{u sigma} du.
// theta^2 < kTheta2 uses four terms of these series (next term < 1e-16), with
// I_m from its power series for |sigma| < kSigma and from the recurrence
// I_m = (e^sigma - m I_{m-1}) / sigma beyond (its error growth m!/sigma^m is
// cancelled by the 1/m! of the series).  theta^2 >= kTheta2 uses the closed
// form of (e^z - 1)/z, z = sigma + i theta, which is regular at sigma = 0.
// No branch is a constant, so value and derivative are both right at 0.
#pragma once

#include "common.hpp"

// plain IEEE operations: the value part of a Dual evaluation then equals the
// double evaluation bit for bit (residual with and without Jacobians)
#pragma clang fp contract(off)

// host and device: the same code is unit-tested on the CPU
// (tests/test_sim3_host.py, every op over every theta / sigma regime)
#define DPVO_HD __host__ __device__ inline

namespace dpvo {
namespace sim3 {

constexpr double kTheta2 = 2.5e-3;  // theta < 0.05: series in theta^2
constexpr double kSigma = 0.5;      // |sigma| < 0.5: series in sigma
constexpr double kLogR2 = 1.0e-4;   // |v|^2 / w^2 below this: atan series in Log

struct Dual {
  double v, d;
  Dual() = default;
  DPVO_HD Dual(double v_) : v(v_), d(0.0) {}
  DPVO_HD Dual(double v_, double d_) : v(v_), d(d_) {}
};
DPVO_HD Dual operator+(const Dual& a, const Dual& b) { return {a.v + b.v, a.d + b.d}; }
DPVO_HD Dual operator-(const Dual& a, const Dual& b) { return {a.v - b.v, a.d - b.d}; }
DPVO_HD Dual operator-(const Dual& a) { return {-a.v, -a.d}; }
DPVO_HD Dual operator*(const Dual& a, const Dual& b) {
  return {a.v * b.v, a.d * b.v + a.v * b.d};
}
DPVO_HD Dual operator/(const Dual& a, const Dual& b) {
  const double q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
DPVO_HD double val(double x) { return x; }
DPVO_HD double val(const Dual& x) { return x.v; }

DPVO_HD double f_sqrt(double x) { return ::sqrt(x); }
DPVO_HD double f_sin(double x) { return ::sin(x); }
DPVO_HD double f_cos(double x) { return ::cos(x); }
DPVO_HD double f_exp(double x) { return ::exp(x); }
DPVO_HD double f_log(double x) { return ::log(x); }
DPVO_HD Dual f_sqrt(const Dual& x) {
  const double r = ::sqrt(x.v);
  return {r, x.d / (2.0 * r)};
}
DPVO_HD Dual f_sin(const Dual& x) { return {::sin(x.v), ::cos(x.v) * x.d}; }
DPVO_HD Dual f_cos(const Dual& x) { return {::cos(x.v), -(::sin(x.v) * x.d)}; }
DPVO_HD Dual f_exp(const Dual& x) {
  const double e = ::exp(x.v);
  return {e, e * x.d};
}
DPVO_HD Dual f_log(const Dual& x) { return {::log(x.v), x.d / x.v}; }
DPVO_HD double f_atan2(double y, double x) { return ::atan2(y, x); }
DPVO_HD Dual f_atan2(const Dual& y, const Dual& x) {
  return {::atan2(y.v, x.v), (x.v * y.d - y.v * x.d) / (x.v * x.v + y.v * y.v)};
}

template <typename T>
struct Elem {  // X = [[s R(q), t], [0, 1]], q = (x, y, z, w) of unit norm
  T t[3];
  T q[4];
  T s;
};

template <typename T>
DPVO_HD void cross(const T* a, const T* b, T* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename T>
DPVO_HD void qnormalise(T* q) {
  const T n = f_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] = q[i] / n;
}
template <typename T>
DPVO_HD void qmul(const T* p, const T* q, T* o) {  // normalised, like SO3
  o[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
  o[1] = p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2];
  o[2] = p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0];
  o[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
  qnormalise(o);
}
template <typename T>
DPVO_HD void qact(const T* q, const T* p, T* o) {  // so3.h:115-120
  T uv[3], uv2[3];
  cross(q, p, uv);
  for (int i = 0; i < 3; i++) uv[i] = uv[i] + uv[i];
  cross(q, uv, uv2);
  for (int i = 0; i < 3; i++) o[i] = p[i] + q[3] * uv[i] + uv2[i];
}
template <typename T>
DPVO_HD void qmat(const T* q, T* R) {  // Eigen toRotationMatrix
  const T tx = q[0] + q[0], ty = q[1] + q[1], tz = q[2] + q[2];
  const T twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const T txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const T tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0] = T(1.0) - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = T(1.0) - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = T(1.0) - (txx + tyy);
}

template <typename T>
DPVO_HD Elem<T> load(const T* d) {
  Elem<T> g;
  for (int i = 0; i < 3; i++) g.t[i] = d[i];
  for (int i = 0; i < 4; i++) g.q[i] = d[3 + i];
  qnormalise(g.q);
  g.s = d[7];
  return g;
}
template <typename T>
DPVO_HD void store(const Elem<T>& g, T* d) {
  for (int i = 0; i < 3; i++) d[i] = g.t[i];
  for (int i = 0; i < 4; i++) d[3 + i] = g.q[i];
  d[7] = g.s;
}
template <typename T>
DPVO_HD Elem<T> inv(const Elem<T>& g) {  // sim3.h:43-45
  Elem<T> o;
  o.q[0] = -g.q[0]; o.q[1] = -g.q[1]; o.q[2] = -g.q[2]; o.q[3] = g.q[3];
  o.s = T(1.0) / g.s;
  T t[3];
  qact(o.q, g.t, t);
  for (int i = 0; i < 3; i++) o.t[i] = -(o.s * t[i]);
  return o;
}
template <typename T>
DPVO_HD Elem<T> mul(const Elem<T>& a, const Elem<T>& b) {  // sim3.h:52-54
  Elem<T> o;
  qmul(a.q, b.q, o.q);
  o.s = a.s * b.s;
  T t[3];
  qact(a.q, b.t, t);
  for (int i = 0; i < 3; i++) o.t[i] = a.t[i] + a.s * t[i];
  return o;
}

// A, B, C of W = C I + A Phi + B Phi^2 (header comment); t2 = |phi|^2
template <typename T>
DPVO_HD void w_coeffs(const T& t2, const T& sg, T& A, T& B, T& C) {
  const bool small_s = fabs(val(sg)) < kSigma;
  const T es = f_exp(sg);
  if (val(t2) < kTheta2 || small_s) {
    constexpr int M = 8;  // I_m(sigma), m = 0 .. 8
    T I[9];
    if (small_s) {
      for (int m = 0; m <= M; m++) I[m] = T(0.0);
      T p = T(1.0);  // sigma^j / j!
      for (int j = 0; j < 16; j++) {
        for (int m = 0; m <= M; m++) I[m] = I[m] + p * T(1.0 / (double)(m + j + 1));
        p = p * sg * T(1.0 / (double)(j + 1));
      }
    } else {
      I[0] = (es - T(1.0)) / sg;
      for (int m = 1; m <= M; m++) I[m] = (es - T((double)m) * I[m - 1]) / sg;
    }
    C = I[0];
    if (val(t2) < kTheta2) {
      A = I[1] - t2 * (I[3] * T(1.0 / 6.0) - t2 * (I[5] * T(1.0 / 120.0) - t2 * I[7] * T(1.0 / 5040.0)));
      B = I[2] * T(0.5) -
          t2 * (I[4] * T(1.0 / 24.0) - t2 * (I[6] * T(1.0 / 720.0) - t2 * I[8] * T(1.0 / 40320.0)));
      return;
    }
  } else {
    C = (es - T(1.0)) / sg;
  }
  const T th = f_sqrt(t2);
  const T a = es * f_sin(th), b = es * f_cos(th), c = t2 + sg * sg;
  A = (a * sg + (T(1.0) - b) * th) / (th * c);
  B = (C - ((b - T(1.0)) * sg + a * th) / c) / t2;
}

// o = W(phi, sigma) v
template <typename T>
DPVO_HD void w_apply(const T& A, const T& B, const T& C, const T* phi, const T* v,
                                        T* o) {
  T pv[3], ppv[3];
  cross(phi, v, pv);
  cross(phi, pv, ppv);
  for (int i = 0; i < 3; i++) o[i] = C * v[i] + A * pv[i] + B * ppv[i];
}

template <typename T>
DPVO_HD Elem<T> expm(const T* x) {  // sim3.h:156-165, rxso3.h:168-188
  const T* phi = x + 3;
  const T t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  T A, B, C;
  w_coeffs(t2, x[6], A, B, C);
  Elem<T> g;
  w_apply(A, B, C, phi, x, g.t);
  T im, re;
  if (val(t2) < kTheta2) {
    const T h = t2 * T(0.25);  // (theta / 2)^2
    im = T(0.5) * (T(1.0) - h * (T(1.0 / 6.0) - h * (T(1.0 / 120.0) - h * (T(1.0 / 5040.0) - h * T(1.0 / 362880.0)))));
    re = T(1.0) - h * (T(0.5) - h * (T(1.0 / 24.0) - h * (T(1.0 / 720.0) - h * T(1.0 / 40320.0))));
  } else {
    const T th = f_sqrt(t2);
    im = f_sin(T(0.5) * th) / th;
    re = f_cos(T(0.5) * th);
  }
  g.q[0] = im * phi[0]; g.q[1] = im * phi[1]; g.q[2] = im * phi[2]; g.q[3] = re;
  qnormalise(g.q);
  g.s = f_exp(x[6]);
  return g;
}

template <typename T>
DPVO_HD void logm(const Elem<T>& g, T* x) {  // sim3.h:145-154, rxso3.h:131-166
  const T sq = g.q[0] * g.q[0] + g.q[1] * g.q[1] + g.q[2] * g.q[2];
  const T w = g.q[3];
  T f;
  if (val(sq) < kLogR2 * val(w) * val(w)) {
    const T r = sq / (w * w);  // 2 atan(n / w) / n = (2 / w) sum_k (-r)^k / (2k + 1)
    f = T(2.0) / w *
        (T(1.0) - r * (T(1.0 / 3.0) - r * (T(1.0 / 5.0) - r * (T(1.0 / 7.0) - r * (T(1.0 / 9.0) - r * T(1.0 / 11.0))))));
  } else {
    // 2 atan(n / w) / n by atan2: value and derivative stay right through
    // w = 0 (theta = pi), where lietorch switches to the constant +-pi / n
    const T n = f_sqrt(sq);
    f = val(w) < 0.0 ? -(T(2.0) * f_atan2(n, -w) / n) : T(2.0) * f_atan2(n, w) / n;
  }
  T* phi = x + 3;
  phi[0] = f * g.q[0]; phi[1] = f * g.q[1]; phi[2] = f * g.q[2];
  x[6] = f_log(g.s);
  const T t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  T A, B, C;
  w_coeffs(t2, x[6], A, B, C);
  // tau = W^-1 t by the adjugate of the 3x3 W (its eigenvalues (e^z - 1)/z,
  // z = sigma, sigma +- i theta, do not vanish for theta < 2 pi)
  T W[9];
  for (int j = 0; j < 3; j++) {
    T e[3] = {T(j == 0 ? 1.0 : 0.0), T(j == 1 ? 1.0 : 0.0), T(j == 2 ? 1.0 : 0.0)}, c[3];
    w_apply(A, B, C, phi, e, c);
    W[j] = c[0]; W[3 + j] = c[1]; W[6 + j] = c[2];
  }
  const T c00 = W[4] * W[8] - W[5] * W[7], c01 = W[5] * W[6] - W[3] * W[8],
          c02 = W[3] * W[7] - W[4] * W[6];
  const T det = W[0] * c00 + W[1] * c01 + W[2] * c02;
  const T c10 = W[2] * W[7] - W[1] * W[8], c11 = W[0] * W[8] - W[2] * W[6],
          c12 = W[1] * W[6] - W[0] * W[7];
  const T c20 = W[1] * W[5] - W[2] * W[4], c21 = W[2] * W[3] - W[0] * W[5],
          c22 = W[0] * W[4] - W[1] * W[3];
  x[0] = (c00 * g.t[0] + c10 * g.t[1] + c20 * g.t[2]) / det;
  x[1] = (c01 * g.t[0] + c11 * g.t[1] + c21 * g.t[2]) / det;
  x[2] = (c02 * g.t[0] + c12 * g.t[1] + c22 * g.t[2]) / det;
}

// Exp(eps a) X to first order in eps: the left perturbation of X along the
// tangent a, carried in the dual parts
DPVO_HD Elem<Dual> perturb(const Elem<double>& X, const double* a) {
  Elem<Dual> o;
  double pt[3], pq[3];
  cross(a + 3, X.t, pt);
  cross(a + 3, X.q, pq);
  for (int i = 0; i < 3; i++) {
    o.t[i] = Dual(X.t[i], a[i] + pt[i] + a[6] * X.t[i]);
    o.q[i] = Dual(X.q[i], 0.5 * (X.q[3] * a[3 + i] + pq[i]));
  }
  o.q[3] = Dual(X.q[3], -0.5 * (a[3] * X.q[0] + a[4] * X.q[1] + a[5] * X.q[2]));
  o.s = Dual(X.s, X.s * a[6]);
  return o;
}
// the tangent a with dX = hat(a) X, read off the dual parts of X
DPVO_HD void left_tangent(const Elem<Dual>& X, double* a) {
  double dv[3] = {X.q[0].d, X.q[1].d, X.q[2].d}, qv[3] = {X.q[0].v, X.q[1].v, X.q[2].v}, c[3];
  cross(dv, qv, c);
  for (int i = 0; i < 3; i++) a[3 + i] = 2.0 * (X.q[3].v * dv[i] - X.q[3].d * qv[i] - c[i]);
  a[6] = X.s.d / X.s.v;
  double t[3] = {X.t[0].v, X.t[1].v, X.t[2].v}, pt[3];
  cross(a + 3, t, pt);
  for (int i = 0; i < 3; i++) a[i] = X.t[i].d - pt[i] - a[6] * t[i];
}

// 7x7 row-major Adjoint (sim3.h:89-101) and adjoint of the algebra (126-142)
DPVO_HD void Adj(const Elem<double>& g, double* A) {
  double R[9];
  qmat(g.q, R);
  for (int i = 0; i < 49; i++) A[i] = 0.0;
  for (int j = 0; j < 3; j++) {
    double Rj[3] = {R[j], R[3 + j], R[6 + j]}, tR[3];
    cross(g.t, Rj, tR);  // column j of [t]x R
    for (int i = 0; i < 3; i++) {
      A[i * 7 + j] = g.s * R[i * 3 + j];
      A[i * 7 + 3 + j] = tR[i];
      A[(3 + i) * 7 + 3 + j] = R[i * 3 + j];
    }
  }
  for (int i = 0; i < 3; i++) A[i * 7 + 6] = -g.t[i];
  A[48] = 1.0;
}
DPVO_HD void adj_small(const double* x, double* A) {
  for (int i = 0; i < 49; i++) A[i] = 0.0;
  const double Ta[9] = {0, -x[2], x[1], x[2], 0, -x[0], -x[1], x[0], 0};
  const double Ph[9] = {0, -x[5], x[4], x[5], 0, -x[3], -x[4], x[3], 0};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) {
      A[i * 7 + j] = Ph[i * 3 + j] + (i == j ? x[6] : 0.0);
      A[i * 7 + 3 + j] = Ta[i * 3 + j];
      A[(3 + i) * 7 + 3 + j] = Ph[i * 3 + j];
    }
    A[i * 7 + 6] = -x[i];
  }
}

DPVO_HD void rowvec_mat7(const double* v, const double* M, double* o) {  // o = v^T M
  for (int j = 0; j < 7; j++) {
    double s = 0.0;
    for (int i = 0; i < 7; i++) s += v[i] * M[i * 7 + j];
    o[j] = s;
  }
}
DPVO_HD void mat_vec7(const double* M, const double* v, double* o) {
  for (int i = 0; i < 7; i++) {
    double s = 0.0;
    for (int j = 0; j < 7; j++) s += M[i * 7 + j] * v[j];
    o[i] = s;
  }
}

// the op numbers of lie.hip / ext_lietorch.cpp
enum { EXP = 0, LOG, INV, MUL, ADJ, ADJT, ACT, ACT4, MATRIX, PROJ, JINV };

// ---- forward, one element (lietorch_gpu.cu:20-294 with Sim3) ----
DPVO_HD void fwd(int op, const double* X, const double* Y, double* out) {
  switch (op) {
    case EXP: store(expm(X), out); break;
    case LOG: logm(load(X), out); break;
    case INV: store(inv(load(X)), out); break;
    case MUL: store(mul(load(X), load(Y)), out); break;
    case ADJ: { double A[49]; Adj(load(X), A); mat_vec7(A, Y, out); } break;
    case ADJT: { double A[49]; Adj(load(X), A); rowvec_mat7(Y, A, out); } break;
    case ACT:
    case ACT4: {
      const Elem<double> g = load(X);
      double p[3];
      qact(g.q, Y, p);
      const double h = op == ACT4 ? Y[3] : 1.0;
      for (int i = 0; i < 3; i++) out[i] = g.s * p[i] + g.t[i] * h;
      if (op == ACT4) out[3] = Y[3];
    } break;
    case MATRIX: {
      const Elem<double> g = load(X);
      double R[9];
      qmat(g.q, R);
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[i * 4 + j] = g.s * R[i * 3 + j];
        out[i * 4 + 3] = g.t[i];
        out[12 + i] = 0.0;
      }
      out[15] = 1.0;
    } break;
    case PROJ: {  // sim3.h:79-87, rxso3.h:87-102
      const Elem<double> g = load(X);
      for (int i = 0; i < 64; i++) out[i] = 0.0;
      const double Ht[9] = {0, g.t[2], -g.t[1], -g.t[2], 0, g.t[0], g.t[1], -g.t[0], 0};     // hat(-t)
      const double Hq[9] = {0, g.q[2], -g.q[1], -g.q[2], 0, g.q[0], g.q[1], -g.q[0], 0};     // hat(-v)
      for (int i = 0; i < 3; i++) {
        out[i * 8 + i] = 1.0;
        for (int j = 0; j < 3; j++) {
          out[i * 8 + 3 + j] = Ht[i * 3 + j];
          out[(3 + i) * 8 + 3 + j] = 0.5 * ((i == j ? g.q[3] : 0.0) + Hq[i * 3 + j]);
        }
        out[i * 8 + 6] = g.t[i];
        out[6 * 8 + 3 + i] = -0.5 * g.q[i];
      }
      out[7 * 8 + 6] = g.s;
    } break;
    case JINV: {  // J_l^-1(Log X) a = d/de Log(Exp(e a) X)
      Dual x[7];
      logm(perturb(load(X), Y), x);
      for (int i = 0; i < 7; i++) out[i] = x[i].d;
    } break;
  }
}

// ---- backward, one element: g is the gradient of the output, o0 / o1 those
// of X / Y (left-perturbation tangents for group elements) ----
DPVO_HD void bwd(int op, const double* g, const double* X, const double* Y, double* o0,
                 double* o1) {
  double A[49], T[7], b[7];
  switch (op) {
    case EXP:  // row k of J_l(x): the left tangent of d Exp(x) / d x_k
      for (int k = 0; k < 7; k++) {
        Dual x[7];
        for (int i = 0; i < 7; i++) x[i] = Dual(X[i], i == k ? 1.0 : 0.0);
        left_tangent(expm(x), T);
        double s = 0.0;
        for (int i = 0; i < 7; i++) s += g[i] * T[i];
        o0[k] = s;
      }
      break;
    case LOG: {  // column k of J_l^-1: d Log(Exp(e e_k) X) / de
      const Elem<double> G = load(X);
      for (int k = 0; k < 7; k++) {
        for (int i = 0; i < 7; i++) b[i] = i == k ? 1.0 : 0.0;
        Dual x[7];
        logm(perturb(G, b), x);
        double s = 0.0;
        for (int i = 0; i < 7; i++) s += g[i] * x[i].d;
        o0[k] = s;
      }
    } break;
    case INV:
      Adj(inv(load(X)), A);
      rowvec_mat7(g, A, T);
      for (int i = 0; i < 7; i++) o0[i] = -T[i];
      break;
    case MUL:
      for (int i = 0; i < 7; i++) o0[i] = g[i];
      Adj(load(X), A);
      rowvec_mat7(g, A, o1);
      break;
    case ADJ:
      Adj(load(X), A);
      mat_vec7(A, Y, b);
      rowvec_mat7(g, A, o1);
      adj_small(b, A);
      rowvec_mat7(g, A, T);
      for (int i = 0; i < 7; i++) o0[i] = -T[i];
      break;
    case ADJT:
      Adj(load(X), A);
      mat_vec7(A, g, b);
      for (int i = 0; i < 7; i++) o1[i] = b[i];
      adj_small(b, A);
      rowvec_mat7(Y, A, T);
      for (int i = 0; i < 7; i++) o0[i] = -T[i];
      break;
    case ACT:
    case ACT4: {  // sim3.h:193-209
      const Elem<double> G = load(X);
      const double h = op == ACT4 ? Y[3] : 1.0;
      double R[9], q[3], gq[3];
      qmat(G.q, R);
      qact(G.q, Y, q);
      for (int i = 0; i < 3; i++) q[i] = G.s * q[i] + G.t[i] * h;  // X p
      for (int j = 0; j < 3; j++)
        o1[j] = G.s * (g[0] * R[j] + g[1] * R[3 + j] + g[2] * R[6 + j]);
      if (op == ACT4) o1[3] = g[0] * G.t[0] + g[1] * G.t[1] + g[2] * G.t[2] + g[3];
      cross(q, g, gq);  // g^T hat(-q) = q x g
      for (int i = 0; i < 3; i++) {
        o0[i] = h * g[i];
        o0[3 + i] = gq[i];
      }
      o0[6] = g[0] * q[0] + g[1] * q[1] + g[2] * q[2];
    } break;
  }
}

// ---- pose-graph edge: r = Log(C Exp(gi) Exp(gj)^-1) (optim_utils.py:158-161) ----
template <typename T>
DPVO_HD void pgo_edge(const Elem<T>& C, const T* gi, const T* gj, T* r) {
  logm(mul(mul(C, expm(gi)), inv(expm(gj))), r);
}

}  // namespace sim3
}  // namespace dpvo

#undef DPVO_HD

#pragma clang fp contract(fast)
