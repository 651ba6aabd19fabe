// train.hip -- the three small launch-bound pieces of a training step that
// are not compositions of the other kernels ("Training step"):
//
//   transform   projective_ops.transform (projective_ops.py:53-113, SE3, the
//               whole P x P patch) forward and backward,
//   flow loss   train.py:87-88, forward and backward,
//   pose loss   train.py:90-113 (kabsch_umeyama scale included) for n <= 32
//               poses in one workgroup, forward and backward.
//
// fp32 in and out, fp64 arithmetic inside (the SE3 device functions of
// lie_se3.hpp at S = double).  Every sum over edges, points or pairs runs in
// an order fixed by the sizes alone; no floating-point atomics: two calls
// give identical bits.  Plain launches on the caller's stream, no allocation,
// no host synchronisation.  Gradients of group elements are left-tangent
// rows (tau, phi), lietorch's convention.
#include <math.h>

#include "common.hpp"
#include "sim3.hpp"
// No FMA contraction in this file, the SE3 functions of lie_se3.hpp included
// (sim3.hpp, which it includes, switches contraction back on at its end, so it
// comes first): a w - a w must be exactly 0, so that two identical poses have
// the relative pose (0, 0, 0; 0, 0, 0, 1) and the error Log(I) = 0 to the bit,
// and the pose loss's gradient of that pair is zero, not a rounding residue's
// direction.
#pragma clang fp contract(off)
#include "lie_se3.hpp"

namespace dpvo {
namespace {

constexpr int kT = 256;
constexpr int kMaxPoses = 32;  // pose loss: one workgroup, 32 x 32 ordered pairs
typedef lie::SE3g<double> G64;

__device__ __forceinline__ G64 load_pose(const float* __restrict__ d) {
  G64 g;
  g.t[0] = d[0]; g.t[1] = d[1]; g.t[2] = d[2];
  g.q = lie::qnorm<double>(d[3], d[4], d[5], d[6]);  // normalised on load (so3.h:95-97)
  return g;
}

// Adj(G)^T g for G = (R, t):  (R^T g_tau, R^T (g_phi - t x g_tau))
__device__ __forceinline__ void adjT_apply(const double* R, const double* t, const double* g,
                                           double* o) {
  double c[3], u[3];
  lie::cross(t, g, c);
  for (int a = 0; a < 3; a++) u[a] = g[3 + a] - c[a];
  for (int a = 0; a < 3; a++) {
    o[a] = R[a] * g[0] + R[3 + a] * g[1] + R[6 + a] * g[2];
    o[3 + a] = R[a] * u[0] + R[3 + a] * u[1] + R[6 + a] * u[2];
  }
}

// sum of a double over the workgroup (kT threads): xor butterflies inside a
// wave, the four wave totals in a fixed order
template <int N>
__device__ __forceinline__ void block_sum(double* acc, double* red) {  // red [4][N]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
#pragma unroll
  for (int x = 0; x < N; x++) acc[x] = wave_sum(acc[x]);
  if (lane == 0)
    for (int x = 0; x < N; x++) red[wid * N + x] = acc[x];
  __syncthreads();
  for (int x = 0; x < N; x++) acc[x] = (red[x] + red[N + x]) + (red[2 * N + x] + red[3 * N + x]);
}

// ------------------------------------------------------------------ transform

struct Edge {
  double R[9], t[3];            // Gij = Gj Gi^-1
  double fi[4], fj[4];          // intrinsics of the source and of the target frame
  const float* patch;           // patches + kk * 3 * P * P
};

__device__ __forceinline__ bool edge_load(const float* __restrict__ poses,
                                          const float* __restrict__ patches,
                                          const float* __restrict__ intr,
                                          const int64_t* __restrict__ ii,
                                          const int64_t* __restrict__ jj,
                                          const int64_t* __restrict__ kk, int e, int N, int M,
                                          int PP, Edge& g) {
  const int64_t i = ii[e], j = jj[e], k = kk[e];
  if (i < 0 || i >= N || j < 0 || j >= N || k < 0 || k >= M) return false;  // nothing is read
  const G64 Gi = load_pose(poses + 7 * i), Gj = load_pose(poses + 7 * j);
  const G64 Gij = lie::se3_mul(Gj, lie::se3_inv(Gi));
  lie::qmat(Gij.q, g.R);
  for (int a = 0; a < 3; a++) g.t[a] = Gij.t[a];
  for (int a = 0; a < 4; a++) {
    g.fi[a] = intr[4 * i + a];
    g.fj[a] = intr[4 * j + a];
  }
  g.patch = patches + (size_t)k * 3 * PP;
  return true;
}

// X1 = Gij (u, v, 1, d) of patch point pt; returns d
__device__ __forceinline__ double point_lift(const Edge& g, int pt, int PP, double* X) {
  const double u = ((double)g.patch[pt] - g.fi[2]) / g.fi[0];
  const double v = ((double)g.patch[PP + pt] - g.fi[3]) / g.fi[1];
  const double d = g.patch[2 * PP + pt];
  for (int a = 0; a < 3; a++) X[a] = g.R[3 * a] * u + g.R[3 * a + 1] * v + g.R[3 * a + 2] + g.t[a] * d;
  return d;
}

template <int P>
__global__ void __launch_bounds__(kT) tf_forward(const float* __restrict__ poses,
                                                 const float* __restrict__ patches,
                                                 const float* __restrict__ intr,
                                                 const int64_t* __restrict__ ii,
                                                 const int64_t* __restrict__ jj,
                                                 const int64_t* __restrict__ kk, int E, int N, int M,
                                                 float* __restrict__ coords,
                                                 float* __restrict__ valid,
                                                 float* __restrict__ coords1) {
  constexpr int PP = P * P;
  const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (idx >= (int64_t)E * PP) return;
  const int e = (int)(idx / PP), pt = (int)(idx % PP);
  float x = __builtin_nanf(""), y = __builtin_nanf(""), v = 0.0f;
  Edge g;
  if (edge_load(poses, patches, intr, ii, jj, kk, e, N, M, PP, g)) {
    double X[3];
    point_lift(g, pt, PP, X);
    const double dinv = 1.0 / fmax(X[2], 0.1);
    x = (float)(g.fj[0] * (dinv * X[0]) + g.fj[2]);
    y = (float)(g.fj[1] * (dinv * X[1]) + g.fj[3]);
    v = X[2] > 0.2 ? 1.0f : 0.0f;
  }
  coords[2 * idx] = x;
  coords[2 * idx + 1] = y;
  valid[idx] = v;
  if (coords1) {  // the [E, 2, P, P] copy A-CORR takes
    coords1[((size_t)e * 2) * PP + pt] = x;
    coords1[((size_t)e * 2 + 1) * PP + pt] = y;
  }
}

// per-edge record of the backward: g_Gi [6], g_Gj [6], g_patch [3][P*P]
__host__ __device__ constexpr int tf_rec(int PP) { return 12 + 3 * PP; }

// one thread per edge: the cotangent of the edge's P*P points -> its record
template <int P>
__global__ void __launch_bounds__(kT) tf_edge_grad(const float* __restrict__ poses,
                                                   const float* __restrict__ patches,
                                                   const float* __restrict__ intr,
                                                   const int64_t* __restrict__ ii,
                                                   const int64_t* __restrict__ jj,
                                                   const int64_t* __restrict__ kk, int E, int N,
                                                   int M, const float* __restrict__ gc,
                                                   double* __restrict__ rec, int want_pose,
                                                   int want_patch) {
  constexpr int PP = P * P, kRec = tf_rec(PP);
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= E) return;
  double* r = rec + (size_t)e * kRec;
  Edge g;
  if (!edge_load(poses, patches, intr, ii, jj, kk, e, N, M, PP, g)) {
    for (int a = 0; a < kRec; a++) r[a] = 0.0;  // the edge contributes no gradient
    return;
  }
  double gG[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int pt = 0; pt < PP; pt++) {
    double X[3];
    const double d = point_lift(g, pt, PP, X);
    const double dinv = 1.0 / fmax(X[2], 0.1);
    const double gx = gc[((size_t)e * PP + pt) * 2], gy = gc[((size_t)e * PP + pt) * 2 + 1];
    double gv[3];
    gv[0] = g.fj[0] * dinv * gx;
    gv[1] = g.fj[1] * dinv * gy;
    const double gd = g.fj[0] * X[0] * gx + g.fj[1] * X[1] * gy;
    gv[2] = X[2] >= 0.1 ? -dinv * dinv * gd : 0.0;  // clamp(min=0.1): nothing through d' below it
    if (want_pose) {  // d X1 / d xi = [d I, -[X1]x]
      double c[3];
      lie::cross(X, gv, c);
      for (int a = 0; a < 3; a++) {
        gG[a] += d * gv[a];
        gG[3 + a] += c[a];
      }
    }
    if (want_patch) {
      const double ru = g.R[0] * gv[0] + g.R[3] * gv[1] + g.R[6] * gv[2];
      const double rv = g.R[1] * gv[0] + g.R[4] * gv[1] + g.R[7] * gv[2];
      r[12 + pt] = ru / g.fi[0];
      r[12 + PP + pt] = rv / g.fi[1];
      r[12 + 2 * PP + pt] = g.t[0] * gv[0] + g.t[1] * gv[1] + g.t[2] * gv[2];
    }
  }
  if (want_pose) {  // Gij = Gj Gi^-1:  g_Gj = g,  g_Gi = -Adj(Gij)^T g
    double gi[6];
    adjT_apply(g.R, g.t, gG, gi);
    for (int a = 0; a < 6; a++) {
      r[a] = -gi[a];
      r[6 + a] = gG[a];
    }
  }
}

// one workgroup per pose: thread t adds edges t, t + kT, .. in ascending order
// (source role before target role), then the fixed tree of block_sum
__global__ void __launch_bounds__(kT) tf_gpose(const double* __restrict__ rec, int kRec,
                                               const int64_t* __restrict__ ii,
                                               const int64_t* __restrict__ jj, int E,
                                               float* __restrict__ gP) {
  __shared__ double red[4 * 6];
  const int a = blockIdx.x, tid = threadIdx.x;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int e = tid; e < E; e += kT) {
    const bool si = ii[e] == a, sj = jj[e] == a;
    if (!si && !sj) continue;
    const double* r = rec + (size_t)e * kRec;  // zeros for an out-of-range edge
    if (si)
      for (int d = 0; d < 6; d++) acc[d] += r[d];
    if (sj)
      for (int d = 0; d < 6; d++) acc[d] += r[6 + d];
  }
  block_sum<6>(acc, red);
  if (tid < 6) gP[6 * (size_t)a + tid] = (float)acc[tid];
}

// one wave per patch: lane l adds edges l, l + 64, .. in ascending order, then
// the xor butterfly
template <int P>
__global__ void __launch_bounds__(kWave) tf_gpatch(const double* __restrict__ rec,
                                                   const int64_t* __restrict__ kk, int E,
                                                   float* __restrict__ gK) {
  constexpr int PP = P * P, kRec = tf_rec(PP), C = 3 * PP;
  const int m = blockIdx.x, lane = threadIdx.x;
  double acc[C];
#pragma unroll
  for (int x = 0; x < C; x++) acc[x] = 0.0;
  for (int e = lane; e < E; e += kWave) {
    if (kk[e] != m) continue;
    const double* r = rec + (size_t)e * kRec + 12;
#pragma unroll
    for (int x = 0; x < C; x++) acc[x] += r[x];
  }
#pragma unroll
  for (int x = 0; x < C; x++) {
    const double s = wave_sum(acc[x]);
    if (lane == x) gK[(size_t)m * C + x] = (float)s;
  }
}

// ------------------------------------------------------------------ flow loss

constexpr int kFlowT = 1024;

// one workgroup: thread t takes edges t, t + 1024, ..
template <int P>
__global__ void __launch_bounds__(kFlowT) flow_forward(const float* __restrict__ x,
                                                       const float* __restrict__ y,
                                                       const float* __restrict__ valid, int E,
                                                       float* __restrict__ loss,
                                                       int32_t* __restrict__ count,
                                                       float* __restrict__ emin,
                                                       int32_t* __restrict__ amin) {
  constexpr int PP = P * P;
  __shared__ double rs[kFlowT / kWave];
  __shared__ int rc[kFlowT / kWave];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  double s = 0.0;
  int c = 0;
  for (int e = tid; e < E; e += kFlowT) {
    double best = 0.0;
    int arg = 0;
#pragma unroll
    for (int pt = 0; pt < PP; pt++) {
      const size_t o = ((size_t)e * PP + pt) * 2;
      const double dx = (double)x[o] - (double)y[o], dy = (double)x[o + 1] - (double)y[o + 1];
      const double n = sqrt(dx * dx + dy * dy);
      if (pt == 0 || n < best) {  // ties keep the lowest point index
        best = n;
        arg = pt;
      }
    }
    emin[e] = (float)best;
    amin[e] = arg;
    if (valid[e] > 0.5f) {
      s += best;
      c += 1;
    }
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if (lane == 0) {
    rs[wid] = s;
    rc[wid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0;
    int tc = 0;
    for (int w = 0; w < kFlowT / kWave; w++) {
      ts += rs[w];
      tc += rc[w];
    }
    loss[0] = tc > 0 ? (float)(ts / tc) : 0.0f;  // no valid edge: 0, not the NaN of an empty mean
    count[0] = tc;
  }
}

template <int P>
__global__ void __launch_bounds__(kT) flow_backward(const float* __restrict__ x,
                                                    const float* __restrict__ y,
                                                    const float* __restrict__ valid,
                                                    const int32_t* __restrict__ count,
                                                    const int32_t* __restrict__ amin,
                                                    const float* __restrict__ g, int E,
                                                    float* __restrict__ gx) {
  constexpr int PP = P * P;
  const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (idx >= (int64_t)E * PP) return;
  const int e = (int)(idx / PP), pt = (int)(idx % PP);
  float o0 = 0.0f, o1 = 0.0f;
  if (valid[e] > 0.5f && amin[e] == pt) {
    const double dx = (double)x[2 * idx] - (double)y[2 * idx];
    const double dy = (double)x[2 * idx + 1] - (double)y[2 * idx + 1];
    const double n = sqrt(dx * dx + dy * dy);
    if (n > 0.0) {  // an exactly-zero difference: zero gradient
      const double k = (double)g[0] / n / (double)count[0];
      o0 = (float)(k * dx);
      o1 = (float)(k * dy);
    }
  }
  gx[2 * idx] = o0;
  gx[2 * idx + 1] = o1;
}

// ------------------------------------------------------------------ pose loss

// sum of the singular values of a 3x3 matrix: one-sided Jacobi on its columns
// (as ransac.hip), the singular values are the column norms at convergence
__device__ inline double sv_sum3(double* H) {
  for (int sweep = 0; sweep < 40; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 3; r++) {
          al += H[3 * r + p] * H[3 * r + p];
          be += H[3 * r + q] * H[3 * r + q];
          ga += H[3 * r + p] * H[3 * r + q];
        }
        if (ga == 0.0 || fabs(ga) <= 1e-16 * sqrt(al * be)) continue;
        rotated = true;
        const double ze = (be - al) / (2 * ga);
        const double t = (ze < 0 ? -1.0 : 1.0) / (fabs(ze) + sqrt(1 + ze * ze));
        const double c = 1 / sqrt(1 + t * t), s = c * t;
        for (int r = 0; r < 3; r++) {
          const double hp = H[3 * r + p], hq = H[3 * r + q];
          H[3 * r + p] = c * hp - s * hq;
          H[3 * r + q] = s * hp + c * hq;
        }
      }
    if (!rotated) break;
  }
  double tr = 0;
  for (int c = 0; c < 3; c++)
    tr += sqrt(H[c] * H[c] + H[3 + c] * H[3 + c] + H[6 + c] * H[6 + c]);
  return tr;
}

struct PoseLds {
  G64 A[kMaxPoses], B[kMaxPoses];  // inv(G_i) (translation scaled after pose_setup), inv(Ps_i)
  double tu[kMaxPoses][3];         // the unscaled translation of inv(G_i)
  double s;
};

// A, B and the scale s = clamp(VarA / trace(D), max=10) of kabsch_umeyama(t_gt,
// t_est) (train.py:31-41, 102-105).  Called by every thread of the workgroup.
__device__ inline void pose_setup(const float* __restrict__ G, const float* __restrict__ Ps, int n,
                                  PoseLds& L) {
  const int tid = threadIdx.x;
  if (tid < n) {
    L.A[tid] = lie::se3_inv(load_pose(G + 7 * tid));
    L.B[tid] = lie::se3_inv(load_pose(Ps + 7 * tid));
  }
  __syncthreads();
  if (tid == 0) {
    double ea[3] = {0, 0, 0}, eb[3] = {0, 0, 0};
    for (int i = 0; i < n; i++)
      for (int a = 0; a < 3; a++) {
        ea[a] += L.B[i].t[a];  // "A" of kabsch_umeyama: the ground-truth translations
        eb[a] += L.A[i].t[a];
      }
    for (int a = 0; a < 3; a++) {
      ea[a] /= n;
      eb[a] /= n;
    }
    double var = 0, H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
      double da[3], db[3];
      for (int a = 0; a < 3; a++) {
        da[a] = L.B[i].t[a] - ea[a];
        db[a] = L.A[i].t[a] - eb[a];
      }
      var += da[0] * da[0] + da[1] * da[1] + da[2] * da[2];
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) H[3 * a + b] += da[a] * db[b];
    }
    var /= n;
    for (int a = 0; a < 9; a++) H[a] /= n;
    const double q = var / sv_sum3(H);  // IEEE: x / 0 = inf clamps to 10, 0 / 0 stays NaN
    L.s = q > 10.0 ? 10.0 : q;
  }
  __syncthreads();
  if (tid < n)
    for (int a = 0; a < 3; a++) {
      L.tu[tid][a] = L.A[tid].t[a];
      L.A[tid].t[a] *= L.s;
    }
  __syncthreads();
}

// e_ij = Log((A_i^-1 A_j) (B_i^-1 B_j)^-1); Ainv = A_i^-1
__device__ __forceinline__ void pair_error(const PoseLds& L, int i, int j, double* e, G64& Ainv) {
  Ainv = lie::se3_inv(L.A[i]);
  const G64 dP = lie::se3_mul(Ainv, L.A[j]);
  const G64 dG = lie::se3_mul(lie::se3_inv(L.B[i]), L.B[j]);
  lie::se3_log(lie::se3_mul(dP, lie::se3_inv(dG)), e);
}

__device__ __forceinline__ double norm3(const double* v) {
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}

// out: {mean tr, mean ro, s}; tr / ro: the n (n - 1) pairs in meshgrid 'ij'
// order with the diagonal removed
__global__ void __launch_bounds__(kT) pose_forward(const float* __restrict__ G,
                                                   const float* __restrict__ Ps, int n,
                                                   float* __restrict__ out, float* __restrict__ tr,
                                                   float* __restrict__ ro) {
  __shared__ PoseLds L;
  __shared__ double red[4 * 2];
  pose_setup(G, Ps, n, L);
  const int tid = threadIdx.x;
  double acc[2] = {0, 0};
  for (int p = tid; p < n * n; p += kT) {  // ascending pairs per thread
    const int i = p / n, j = p % n;
    if (i == j) continue;
    double e[6];
    G64 Ainv;
    pair_error(L, i, j, e, Ainv);
    const double t = norm3(e), r = norm3(e + 3);
    const int o = i * (n - 1) + (j < i ? j : j - 1);
    tr[o] = (float)t;
    ro[o] = (float)r;
    acc[0] += t;
    acc[1] += r;
  }
  block_sum<2>(acc, red);
  if (tid == 0) {
    const double np = (double)n * (n - 1);
    out[0] = (float)(acc[0] / np);
    out[1] = (float)(acc[1] / np);
    out[2] = (float)L.s;
  }
}

// g: {cotangent of mean tr, cotangent of mean ro}; gG [n, 6]
__global__ void __launch_bounds__(kT) pose_backward(const float* __restrict__ G,
                                                    const float* __restrict__ Ps, int n,
                                                    const float* __restrict__ g,
                                                    float* __restrict__ gG) {
  __shared__ PoseLds L;
  __shared__ double V[kMaxPoses * kMaxPoses * 6];  // per pair: Adj(A_i^-1)^T g_E
  __shared__ double gA[kMaxPoses * 6];
  pose_setup(G, Ps, n, L);
  const int tid = threadIdx.x;
  const double np = (double)n * (n - 1);
  const double gt = (double)g[0] / np, gr = (double)g[1] / np;
  for (int p = tid; p < n * n; p += kT) {
    const int i = p / n, j = p % n;
    double* v = V + 6 * (i * kMaxPoses + j);
    if (i == j) {
      for (int a = 0; a < 6; a++) v[a] = 0.0;
      continue;
    }
    double e[6], ge[6], J[36], gE[6], R[9];
    G64 Ainv;
    pair_error(L, i, j, e, Ainv);
    const double t = norm3(e), r = norm3(e + 3);
    for (int a = 0; a < 3; a++) {  // a zero error (identical poses) has a zero gradient
      ge[a] = t > 0.0 ? gt * e[a] / t : 0.0;
      ge[3 + a] = r > 0.0 ? gr * e[3 + a] / r : 0.0;
    }
    lie::se3_jl_inv(e, J);  // Log(Exp(d) E) = e + J_l^-1(e) d
    lie::rowvec_mat(ge, J, 6, 6, gE);
    // E = dP dG^-1, dP = A_i^-1 A_j:  g_Aj = Adj(A_i^-1)^T g_E,  g_Ai = -g_Aj
    lie::qmat(Ainv.q, R);
    adjT_apply(R, Ainv.t, gE, v);
  }
  __syncthreads();
  if (tid < 6 * n) {
    const int i = tid / 6, c = tid % 6;
    double acc = 0.0;
    for (int j = 0; j < n; j++) acc -= V[6 * (i * kMaxPoses + j) + c];
    for (int j = 0; j < n; j++) acc += V[6 * (j * kMaxPoses + i) + c];
    gA[tid] = c < 3 ? L.s * acc : acc;  // the scaled translation maps tau by s, phi unchanged
  }
  __syncthreads();
  if (tid < n) {  // A = G^-1:  g_G = -Adj(A)^T g_A, A with the unscaled translation
    double R[9], o[6];
    lie::qmat(L.A[tid].q, R);
    adjT_apply(R, L.tu[tid], gA + 6 * tid, o);
    for (int a = 0; a < 6; a++) gG[6 * tid + a] = (float)(-o[a]);
  }
}

inline int blocks(size_t n) { return (int)((n + kT - 1) / kT); }

}  // namespace
}  // namespace dpvo

using namespace dpvo;

// Status order of every entry: unsupported shape, nothing to do, null
// pointer, workspace size -- all before any launch.

DPVO_EXPORT size_t dpvo_transform_workspace_bytes(int E, int P) {
  if (E <= 0 || (P != 1 && P != 3)) return 0;
  return (size_t)E * tf_rec(P * P) * sizeof(double);
}

DPVO_EXPORT int dpvo_transform_forward(const float* poses, const float* patches,
                                       const float* intrinsics, const int64_t* ii,
                                       const int64_t* jj, const int64_t* kk, int E, int P, int N,
                                       int M, float* coords, float* valid, float* coords_corr,
                                       void* stream) {
  if (P != 1 && P != 3) return DPVO_ERR_UNSUPPORTED;
  if ((int64_t)E * P * P >= ((int64_t)1 << 30)) return DPVO_ERR_UNSUPPORTED;
  if (E <= 0) return DPVO_OK;
  if (!poses || !patches || !intrinsics || !ii || !jj || !kk || !coords || !valid)
    return DPVO_ERR_INVALID;
  if (N < 1 || M < 1) return DPVO_ERR_INVALID;
  const hipStream_t st = as_stream(stream);
  const dim3 grid(blocks((size_t)E * P * P));
  if (P == 3)
    hipLaunchKernelGGL(tf_forward<3>, grid, dim3(kT), 0, st, poses, patches, intrinsics, ii, jj, kk,
                       E, N, M, coords, valid, coords_corr);
  else
    hipLaunchKernelGGL(tf_forward<1>, grid, dim3(kT), 0, st, poses, patches, intrinsics, ii, jj, kk,
                       E, N, M, coords, valid, coords_corr);
  return launch_status();
}

DPVO_EXPORT int dpvo_transform_backward(const float* poses, const float* patches,
                                        const float* intrinsics, const int64_t* ii,
                                        const int64_t* jj, const int64_t* kk, int E, int P, int N,
                                        int M, const float* g_coords, float* g_poses,
                                        float* g_patches, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  if (P != 1 && P != 3) return DPVO_ERR_UNSUPPORTED;
  if ((int64_t)E * P * P >= ((int64_t)1 << 30)) return DPVO_ERR_UNSUPPORTED;
  if (E <= 0 || (!g_poses && !g_patches)) return DPVO_OK;
  if (!poses || !patches || !intrinsics || !ii || !jj || !kk || !g_coords || !workspace)
    return DPVO_ERR_INVALID;
  if (N < 1 || M < 1) return DPVO_ERR_INVALID;
  if (workspace_bytes < dpvo_transform_workspace_bytes(E, P)) return DPVO_ERR_WORKSPACE;
  const hipStream_t st = as_stream(stream);
  double* rec = (double*)workspace;
  const int wp = g_poses ? 1 : 0, wk = g_patches ? 1 : 0;
  if (P == 3)
    hipLaunchKernelGGL(tf_edge_grad<3>, dim3(blocks(E)), dim3(kT), 0, st, poses, patches,
                       intrinsics, ii, jj, kk, E, N, M, g_coords, rec, wp, wk);
  else
    hipLaunchKernelGGL(tf_edge_grad<1>, dim3(blocks(E)), dim3(kT), 0, st, poses, patches,
                       intrinsics, ii, jj, kk, E, N, M, g_coords, rec, wp, wk);
  if (g_poses)
    hipLaunchKernelGGL(tf_gpose, dim3(N), dim3(kT), 0, st, rec, tf_rec(P * P), ii, jj, E, g_poses);
  if (g_patches) {
    if (P == 3)
      hipLaunchKernelGGL(tf_gpatch<3>, dim3(M), dim3(kWave), 0, st, rec, kk, E, g_patches);
    else
      hipLaunchKernelGGL(tf_gpatch<1>, dim3(M), dim3(kWave), 0, st, rec, kk, E, g_patches);
  }
  return launch_status();
}

DPVO_EXPORT int dpvo_flow_loss_forward(const float* coords, const float* coords_gt,
                                       const float* valid, int E, int P, float* loss,
                                       int32_t* count, float* emin, int32_t* argmin,
                                       void* stream) {
  if (P != 1 && P != 3) return DPVO_ERR_UNSUPPORTED;
  if ((int64_t)E * P * P >= ((int64_t)1 << 30)) return DPVO_ERR_UNSUPPORTED;
  if (E <= 0) return DPVO_OK;
  if (!coords || !coords_gt || !valid || !loss || !count || !emin || !argmin)
    return DPVO_ERR_INVALID;
  const hipStream_t st = as_stream(stream);
  if (P == 3)
    hipLaunchKernelGGL(flow_forward<3>, dim3(1), dim3(kFlowT), 0, st, coords, coords_gt, valid, E,
                       loss, count, emin, argmin);
  else
    hipLaunchKernelGGL(flow_forward<1>, dim3(1), dim3(kFlowT), 0, st, coords, coords_gt, valid, E,
                       loss, count, emin, argmin);
  return launch_status();
}

DPVO_EXPORT int dpvo_flow_loss_backward(const float* coords, const float* coords_gt,
                                        const float* valid, const int32_t* count,
                                        const int32_t* argmin, const float* g_loss, int E, int P,
                                        float* g_coords, void* stream) {
  if (P != 1 && P != 3) return DPVO_ERR_UNSUPPORTED;
  if ((int64_t)E * P * P >= ((int64_t)1 << 30)) return DPVO_ERR_UNSUPPORTED;
  if (E <= 0) return DPVO_OK;
  if (!coords || !coords_gt || !valid || !count || !argmin || !g_loss || !g_coords)
    return DPVO_ERR_INVALID;
  const hipStream_t st = as_stream(stream);
  const dim3 grid(blocks((size_t)E * P * P));
  if (P == 3)
    hipLaunchKernelGGL(flow_backward<3>, grid, dim3(kT), 0, st, coords, coords_gt, valid, count,
                       argmin, g_loss, E, g_coords);
  else
    hipLaunchKernelGGL(flow_backward<1>, grid, dim3(kT), 0, st, coords, coords_gt, valid, count,
                       argmin, g_loss, E, g_coords);
  return launch_status();
}

DPVO_EXPORT int dpvo_pose_loss_forward(const float* G, const float* Ps, int n, float* out,
                                       float* tr, float* ro, void* stream) {
  if (n > kMaxPoses) return DPVO_ERR_UNSUPPORTED;
  if (n < 2) return DPVO_OK;
  if (!G || !Ps || !out || !tr || !ro) return DPVO_ERR_INVALID;
  hipLaunchKernelGGL(pose_forward, dim3(1), dim3(kT), 0, as_stream(stream), G, Ps, n, out, tr, ro);
  return launch_status();
}

DPVO_EXPORT int dpvo_pose_loss_backward(const float* G, const float* Ps, int n,
                                        const float* g_out, float* g_G, void* stream) {
  if (n > kMaxPoses) return DPVO_ERR_UNSUPPORTED;
  if (n < 2) return DPVO_OK;
  if (!G || !Ps || !g_out || !g_G) return DPVO_ERR_INVALID;
  hipLaunchKernelGGL(pose_backward, dim3(1), dim3(kT), 0, as_stream(stream), G, Ps, n, g_out, g_G);
  return launch_status();
}
