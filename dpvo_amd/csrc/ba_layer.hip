// ba_layer.hip -- the differentiable bundle-adjustment layer of dpvo/ba.py
// (BA, 88-297: one Gauss-Newton step, B = 1) as fused forward and backward
// kernels on gfx950.  Semantics differ from the inference kernels (ba.hip):
// |r| < 250, depth clamp [1e-3, 10] (in Python), ep an argument, fixedp,
// structure_only, and a backward.
//
// Forward (8 launches, independent of E, M, N):
//   memset      status words and the per-patch edge counts
//   bal_lin     one thread per edge: gates, residual, Ji / Jj / Jz in fp64,
//               stored once (32 doubles); counts open edges per patch; an
//               edge with an index outside [0, n) / [0, M) is closed, touches
//               no memory and is counted in status[0]
//   bal_scan    exclusive scan of the counts (one workgroup)
//   bal_place   edge ids into their patch's segment (integer atomics)
//   bal_patch   one thread per patch: sorts its segment by edge id (so every
//               sum below has a fixed order whatever the atomics gave), C_k,
//               u_k, Q_k and the compact list of the patch's E_k blocks
//               (<= 2 per edge: E is never stored as 6 n_free x M)
//   bal_schur   one workgroup per 6x6 block (a >= b) of S = B - E Q E^T and
//               per 6-row of y = v - E Q u, damping on the diagonal
//   dpvo_spd_solve   A = L L^T, dX = A^-1 y, info on the device (dX = 0 on failure)
//   bal_dz      dZ = Q (u - E^T dX), outputs in the caller's dtype
// Backward (7 launches): the adjoint of the dense part
//   bal_rhs     gX - E qz           (qz = Q gZ)
//   dpvo_spd_solve (stored factor)  mu = A^-1 (.)   (mu = 0 where info != 0)
//   bal_pbar    per patch: E^T mu, E^T dX, ubar, Cbar
//   bal_ebar    per edge: wbar, rbar (the target / weight gradients) and the
//               cotangents (abar, zbar, proj-bar) of its linearisation; Ebar_k
//               is formed on the fly from its rank structure
//   bal_egrad   per (edge, direction): the edge's linearisation again on
//               forward-mode duals seeded along one of the 15 directions
//               (left tangents of pose i and pose j, x, y, d), contracted with
//               the cotangents: includes the derivative of the Jacobians
//   bal_gpose / bal_gpatch   fixed-order sums over the edges of a pose / patch
// All sums are fp64 in a fixed order: two calls are bit-identical.
#include "common.hpp"

namespace dpvo {
namespace {

constexpr int kT = 256;
constexpr int kRec = 32;  // per edge: w[2] r[2] z[2] Ji[2][6] Jj[2][6] (+2 pad)
constexpr int kBar = 28;  // per edge: pbar[2] zbar[2] abarI[2][6] abarJ[2][6]
constexpr int kDir = 16;  // per edge: 15 directional gradients (+1 pad)
constexpr int kPb = 8;    // per patch: qz, Qu, Q, EdX, Emu, ubar, Cbar
constexpr int kStatus = 8;

// ---- forward-mode dual (value, one tangent) --------------------------------
struct Du {
  double v, d;
  __device__ Du() : v(0), d(0) {}
  __device__ Du(double a) : v(a), d(0) {}
  __device__ Du(double a, double b) : v(a), d(b) {}
};
__device__ __forceinline__ Du operator+(Du a, Du b) { return Du(a.v + b.v, a.d + b.d); }
__device__ __forceinline__ Du operator-(Du a, Du b) { return Du(a.v - b.v, a.d - b.d); }
__device__ __forceinline__ Du operator-(Du a) { return Du(-a.v, -a.d); }
__device__ __forceinline__ Du operator*(Du a, Du b) { return Du(a.v * b.v, a.d * b.v + a.v * b.d); }
__device__ __forceinline__ Du operator/(Du a, Du b) {
  const double q = a.v / b.v;
  return Du(q, (a.d - q * b.d) / b.v);
}

template <typename S>
struct Lin {
  S proj[2], Z, Jz[2], Ji[2][6], Jj[2][6];
};

template <typename S>
__device__ __forceinline__ void rotq(const S* q, const S* v, S* o) {  // o = R(q) v
  const S u0 = S(2.0) * (q[1] * v[2] - q[2] * v[1]);
  const S u1 = S(2.0) * (q[2] * v[0] - q[0] * v[2]);
  const S u2 = S(2.0) * (q[0] * v[1] - q[1] * v[0]);
  o[0] = v[0] + q[3] * u0 + (q[1] * u2 - q[2] * u1);
  o[1] = v[1] + q[3] * u1 + (q[2] * u0 - q[0] * u2);
  o[2] = v[2] + q[3] * u2 + (q[0] * u1 - q[1] * u0);
}

// The edge's projection and Jacobians at the patch centre, as
// projective_ops.transform(jacobian=True) for Z > 0.2 (the only edges that
// stay open): G_ij = T_j T_i^-1, X1 = G_ij X0, Jj = Jp Ja, Ji = -Ad(G_ij)^T Jj,
// Jz = Jp [t_ij; 1].  Ki / Kj: intrinsics of frames i and j.
template <typename S>
__device__ void linearise(const S* ti, const S* qi, const S* tj, const S* qj, S x, S y, S d,
                          const double* Ki, const double* Kj, Lin<S>& o) {
  const S qc[4] = {-qi[0], -qi[1], -qi[2], qi[3]};
  S q[4];  // q_ij = q_j conj(q_i)
  q[0] = qj[3] * qc[0] + qj[0] * qc[3] + qj[1] * qc[2] - qj[2] * qc[1];
  q[1] = qj[3] * qc[1] + qj[1] * qc[3] + qj[2] * qc[0] - qj[0] * qc[2];
  q[2] = qj[3] * qc[2] + qj[2] * qc[3] + qj[0] * qc[1] - qj[1] * qc[0];
  q[3] = qj[3] * qc[3] - qj[0] * qc[0] - qj[1] * qc[1] - qj[2] * qc[2];
  // t_ij of T_j * (T_i^-1) as lietorch composes it: two rotations of t_i (one
  // rotation by q_ij differs when the stored quaternions are not exactly unit)
  S ri[3], rt[3], t[3];
  rotq(qc, ti, ri);
  rotq(qj, ri, rt);
  for (int a = 0; a < 3; a++) t[a] = tj[a] - rt[a];
  const S X0[3] = {(x - S(Ki[2])) / S(Ki[0]), (y - S(Ki[3])) / S(Ki[1]), S(1.0)};
  S X1[3];
  rotq(q, X0, X1);
  for (int a = 0; a < 3; a++) X1[a] = X1[a] + t[a] * d;
  const S X = X1[0], Y = X1[1], Z = X1[2], H = d;
  o.Z = Z;
  const S dinv = S(1.0) / Z;
  o.proj[0] = S(Kj[0]) * (X * dinv) + S(Kj[2]);
  o.proj[1] = S(Kj[1]) * (Y * dinv) + S(Kj[3]);
  const S a0 = S(Kj[0]) * dinv, c0 = -(S(Kj[0]) * X * dinv * dinv);
  const S b1 = S(Kj[1]) * dinv, c1 = -(S(Kj[1]) * Y * dinv * dinv);
  o.Jj[0][0] = a0 * H;
  o.Jj[0][1] = S(0.0);
  o.Jj[0][2] = c0 * H;
  o.Jj[0][3] = c0 * Y;
  o.Jj[0][4] = a0 * Z - c0 * X;
  o.Jj[0][5] = -(a0 * Y);
  o.Jj[1][0] = S(0.0);
  o.Jj[1][1] = b1 * H;
  o.Jj[1][2] = c1 * H;
  o.Jj[1][3] = c1 * Y - b1 * Z;
  o.Jj[1][4] = -(c1 * X);
  o.Jj[1][5] = b1 * X;
  const S qi_[4] = {-q[0], -q[1], -q[2], q[3]};  // R^T
  for (int c = 0; c < 2; c++) {
    const S* a = o.Jj[c];
    S u[3], r0[3], r1[3];
    u[0] = a[1] * t[2] - a[2] * t[1] + a[3];  // a_t x t + a_phi
    u[1] = a[2] * t[0] - a[0] * t[2] + a[4];
    u[2] = a[0] * t[1] - a[1] * t[0] + a[5];
    rotq(qi_, a, r0);
    rotq(qi_, u, r1);
    for (int k = 0; k < 3; k++) {
      o.Ji[c][k] = -r0[k];
      o.Ji[c][3 + k] = -r1[k];
    }
  }
  o.Jz[0] = a0 * t[0] + c0 * t[2];
  o.Jz[1] = b1 * t[1] + c1 * t[2];
}

struct Ws {  // workspace layout (device pointers into one buffer)
  int *status, *cnt, *start, *cursor, *order, *ccnt, *cpose, *eopen, *ek;
  int2* epose;  // (ii, jj) of an open edge, (-1, -1) of a closed one: one load per edge in the scans
  double *rec, *Q, *u, *cvec, *S, *y, *L, *dX, *rhs, *mu, *pb, *bar, *ge;
  size_t bytes;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

Ws layout(void* base, int E, int M, int nf, int with_backward) {
  Ws w;
  char* p = (char*)base;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* r = p + o;
    o += up16(bytes);
    return r;
  };
  const size_t e = (size_t)E, m = (size_t)M, n6 = 6 * (size_t)nf;
  w.status = (int*)take(sizeof(int) * kStatus);  // status and cnt: one memset
  w.cnt = (int*)take(sizeof(int) * m);
  w.start = (int*)take(sizeof(int) * (m + 1));
  w.cursor = (int*)take(sizeof(int) * m);
  w.ccnt = (int*)take(sizeof(int) * m);
  w.order = (int*)take(sizeof(int) * e);
  w.cpose = (int*)take(sizeof(int) * 2 * e);
  w.eopen = (int*)take(sizeof(int) * e);
  w.epose = (int2*)take(sizeof(int2) * e);
  w.ek = (int*)take(sizeof(int) * e);
  w.rec = (double*)take(sizeof(double) * kRec * e);
  w.Q = (double*)take(sizeof(double) * m);
  w.u = (double*)take(sizeof(double) * m);
  w.cvec = (double*)take(sizeof(double) * 12 * e);
  w.S = (double*)take(sizeof(double) * n6 * n6);
  w.y = (double*)take(sizeof(double) * n6);
  w.L = (double*)take(sizeof(double) * n6 * n6);
  w.dX = (double*)take(sizeof(double) * n6);
  if (with_backward) {
    w.rhs = (double*)take(sizeof(double) * n6);
    w.mu = (double*)take(sizeof(double) * n6);
    w.pb = (double*)take(sizeof(double) * kPb * m);
    w.bar = (double*)take(sizeof(double) * kBar * e);
    w.ge = (double*)take(sizeof(double) * kDir * e);
  } else {
    w.rhs = w.mu = w.pb = w.bar = w.ge = nullptr;
  }
  w.bytes = o;
  return w;
}

__device__ __forceinline__ int find_pose(const int* cpose, int base, int cc, int f) {
  for (int i = 0; i < cc; i++)
    if (cpose[base + i] == f) return base + i;
  return -1;
}

__device__ __forceinline__ int free_slot(int idx, int fixedp, int nf) {
  return (nf > 0 && idx >= fixedp) ? idx - fixedp : -1;
}

// ---- forward ------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kT)
    bal_lin(const T* __restrict__ poses, const T* __restrict__ patches,
            const T* __restrict__ intr, const T* __restrict__ targets,
            const T* __restrict__ weights, const int64_t* __restrict__ ii,
            const int64_t* __restrict__ jj, const int64_t* __restrict__ kk, int E, int M, int p,
            int n, double b0, double b1, double b2, double b3, Ws w) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= E) return;
  const int64_t i = ii[e], j = jj[e], k = kk[e];
  w.eopen[e] = 0;
  w.epose[e] = make_int2(-1, -1);
  w.ek[e] = 0;
  if (i < 0 || i >= n || j < 0 || j >= n || k < 0 || k >= M) {
    atomicAdd(&w.status[0], 1);
    return;
  }
  const T* pi = poses + 7 * (size_t)i;
  const T* pj = poses + 7 * (size_t)j;
  double ti[3], qi[4], tj[3], qj[4], Ki[4], Kj[4];
  for (int a = 0; a < 3; a++) ti[a] = (double)pi[a], tj[a] = (double)pj[a];
  for (int a = 0; a < 4; a++) {
    qi[a] = (double)pi[3 + a], qj[a] = (double)pj[3 + a];
    Ki[a] = (double)intr[4 * (size_t)i + a], Kj[a] = (double)intr[4 * (size_t)j + a];
  }
  const size_t pp = (size_t)p * p, c = (size_t)(p / 2) * p + p / 2;
  const T* pk = patches + (size_t)k * 3 * pp;
  Lin<double> o;
  linearise<double>(ti, qi, tj, qj, (double)pk[c], (double)pk[pp + c], (double)pk[2 * pp + c], Ki,
                    Kj, o);
  if (!(o.Z > 0.2)) return;  // closed (NaN included); proj is not formed from 1 / Z here
  const double r0 = (double)targets[2 * (size_t)e] - o.proj[0];
  const double r1 = (double)targets[2 * (size_t)e + 1] - o.proj[1];
  const bool open = sqrt(r0 * r0 + r1 * r1) < 250.0 && o.proj[0] > b0 && o.proj[1] > b1 &&
                    o.proj[0] < b2 && o.proj[1] < b3;
  if (!open) return;
  double* rec = w.rec + (size_t)e * kRec;
  rec[0] = (double)weights[2 * (size_t)e];
  rec[1] = (double)weights[2 * (size_t)e + 1];
  rec[2] = r0;
  rec[3] = r1;
  rec[4] = o.Jz[0];
  rec[5] = o.Jz[1];
  for (int cc = 0; cc < 2; cc++)
    for (int a = 0; a < 6; a++) {
      rec[6 + 6 * cc + a] = o.Ji[cc][a];
      rec[18 + 6 * cc + a] = o.Jj[cc][a];
    }
  w.eopen[e] = 1;
  w.epose[e] = make_int2((int)i, (int)j);
  w.ek[e] = (int)k;
  atomicAdd(&w.cnt[k], 1);
  atomicMax(&w.status[2], M - (int)k);  // M - kmin
  atomicMax(&w.status[3], (int)k + 1);  // kmax + 1
}

__global__ void __launch_bounds__(1024) bal_scan(Ws w, int M) {
  __shared__ int wt[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int per = (M + 1023) / 1024;
  const int s0 = min(tid * per, M), s1 = min(s0 + per, M);
  int sum = 0;
  for (int b = s0; b < s1; b++) sum += w.cnt[b];
  const int incl = wave_incl_sum(sum);
  if (lane == 63) wt[wid] = incl;
  __syncthreads();
  int run = incl - sum;
  for (int x = 0; x < wid; x++) run += wt[x];
  for (int b = s0; b < s1; b++) {
    w.start[b] = run;
    w.cursor[b] = run;
    run += w.cnt[b];
  }
  if (tid == 1023) w.start[M] = run;
}

__global__ void __launch_bounds__(kT) bal_place(Ws w, int E) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= E || !w.eopen[e]) return;
  w.order[atomicAdd(&w.cursor[w.ek[e]], 1)] = e;
}

template <typename T>
__global__ void __launch_bounds__(kT)
    bal_patch(Ws w, int M, int fixedp, int nf, const T* __restrict__ lmbda_dev, double lmbda) {
  const int k = blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  const double lm = lmbda_dev ? (double)lmbda_dev[0] : lmbda;
  const int s = w.start[k], len = w.cnt[k];
  int cc = 0;
  double C = 0, u = 0;
  int* ord = w.order + s;
  for (int a = 1; a < len; a++) {  // ascending edge id: a fixed order for every sum
    const int v = ord[a];
    int b = a - 1;
    while (b >= 0 && ord[b] > v) {
      ord[b + 1] = ord[b];
      b--;
    }
    ord[b + 1] = v;
  }
  const int base = 2 * s;
  for (int a = 0; a < len; a++) {
    const int e = ord[a];
    const double* rec = w.rec + (size_t)e * kRec;
    const double w0 = rec[0], w1 = rec[1], z0 = rec[4], z1 = rec[5];
    C += w0 * z0 * z0 + w1 * z1 * z1;
    u += w0 * z0 * rec[2] + w1 * z1 * rec[3];
    const int2 pe = w.epose[e];
    for (int sl = 0; sl < 2; sl++) {
      const int f = free_slot(sl ? pe.y : pe.x, fixedp, nf);
      if (f < 0) continue;
      int at = find_pose(w.cpose, base, cc, f);
      if (at < 0) {
        at = base + cc++;
        w.cpose[at] = f;
        for (int d = 0; d < 6; d++) w.cvec[(size_t)at * 6 + d] = 0.0;
      }
      const double* J = rec + 6 + 12 * sl;
      for (int d = 0; d < 6; d++) w.cvec[(size_t)at * 6 + d] += w0 * z0 * J[d] + w1 * z1 * J[6 + d];
    }
  }
  w.ccnt[k] = cc;
  w.Q[k] = 1.0 / (C + lm);
  w.u[k] = u;
}

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

// block (a, b), a >= b, of S (+ damping) for blockIdx.y < nf; the 6-row a of y
// for blockIdx.y == nf
__global__ void __launch_bounds__(kT) bal_schur(Ws w, int E, int M, int fixedp, int nf, double ep) {
  __shared__ double red[4 * 36];
  const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (b < nf && b > a) return;
  const int n6 = 6 * nf;
  const int kmin = M - w.status[2], kmax = w.status[3];
  double acc[36];
#pragma unroll
  for (int x = 0; x < 36; x++) acc[x] = 0.0;
  if (b < nf) {
    for (int e = tid; e < E; e += kT) {
      const int2 pe = w.epose[e];  // closed: (-1, -1), no free slot
      const int fi = free_slot(pe.x, fixedp, nf), fj = free_slot(pe.y, fixedp, nf);
      if ((fi != a && fj != a) || (fi != b && fj != b)) continue;
      const double* rec = w.rec + (size_t)e * kRec;
      for (int sa = 0; sa < 2; sa++) {
        if ((sa ? fj : fi) != a) continue;
        for (int sb = 0; sb < 2; sb++) {
          if ((sb ? fj : fi) != b) continue;
          for (int c = 0; c < 2; c++) {
            const double* Ja = rec + 6 + 12 * sa + 6 * c;
            const double* Jb = rec + 6 + 12 * sb + 6 * c;
            const double wc = rec[c];
#pragma unroll
            for (int r = 0; r < 6; r++)
#pragma unroll
              for (int q = 0; q < 6; q++) acc[6 * r + q] += wc * Ja[r] * Jb[q];
          }
        }
      }
    }
    for (int k = kmin + tid; k < kmax; k += kT) {
      const int cc = w.ccnt[k];
      if (!cc) continue;
      const int base = 2 * w.start[k];
      const int pa = find_pose(w.cpose, base, cc, a);
      if (pa < 0) continue;
      const int pb = a == b ? pa : find_pose(w.cpose, base, cc, b);
      if (pb < 0) continue;
      const double Qk = w.Q[k];
      const double* Ea = w.cvec + (size_t)pa * 6;
      const double* Eb = w.cvec + (size_t)pb * 6;
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int q = 0; q < 6; q++) acc[6 * r + q] -= Qk * Ea[r] * Eb[q];
    }
    block_sum<36>(acc, red);
    if (tid < 36) {
      const int r = tid / 6, q = tid % 6;
      double v = acc[tid];
      if (a == b && r == q) v = v + (ep + 1e-4 * v);
      w.S[(size_t)(6 * a + r) * n6 + 6 * b + q] = v;
    }
  } else {
    for (int e = tid; e < E; e += kT) {
      const int2 pe = w.epose[e];
      const int fi = free_slot(pe.x, fixedp, nf), fj = free_slot(pe.y, fixedp, nf);
      if (fi != a && fj != a) continue;
      const double* rec = w.rec + (size_t)e * kRec;
      for (int sa = 0; sa < 2; sa++) {
        if ((sa ? fj : fi) != a) continue;
        for (int c = 0; c < 2; c++) {
          const double* Ja = rec + 6 + 12 * sa + 6 * c;
          const double wr = rec[c] * rec[2 + c];
#pragma unroll
          for (int r = 0; r < 6; r++) acc[r] += wr * Ja[r];
        }
      }
    }
    for (int k = kmin + tid; k < kmax; k += kT) {
      const int cc = w.ccnt[k];
      if (!cc) continue;
      const int pa = find_pose(w.cpose, 2 * w.start[k], cc, a);
      if (pa < 0) continue;
      const double qu = w.Q[k] * w.u[k];
#pragma unroll
      for (int r = 0; r < 6; r++) acc[r] -= qu * w.cvec[(size_t)pa * 6 + r];
    }
    block_sum<6>(acc, red);
    if (tid < 6) w.y[6 * a + tid] = acc[tid];
  }
}

template <typename T>
__global__ void __launch_bounds__(kT) bal_dz(Ws w, int M, int nf, T* __restrict__ dX, T* __restrict__ dZ) {
  const int k = blockIdx.x * kT + threadIdx.x;
  if (k < 6 * nf) dX[k] = (T)w.dX[k];
  if (k >= M) return;
  const int cc = w.ccnt[k], base = 2 * w.start[k];
  double s = w.u[k];
  double ex = 0.0;
  for (int i = 0; i < cc; i++) {
    const int f = w.cpose[base + i];
    for (int d = 0; d < 6; d++) ex += w.cvec[(size_t)(base + i) * 6 + d] * w.dX[6 * f + d];
  }
  s -= ex;
  dZ[k] = (T)(w.Q[k] * s);
}

// ---- backward -----------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kT)
    bal_rhs(Ws w, int M, const T* __restrict__ gX, const T* __restrict__ gZ) {
  __shared__ double red[4 * 6];
  const int a = blockIdx.x, tid = threadIdx.x;
  const int kmin = M - w.status[2], kmax = w.status[3];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int k = kmin + tid; k < kmax; k += kT) {
    const int cc = w.ccnt[k];
    if (!cc) continue;
    const int pa = find_pose(w.cpose, 2 * w.start[k], cc, a);
    if (pa < 0) continue;
    const double qz = w.Q[k] * (double)gZ[k];
    for (int r = 0; r < 6; r++) acc[r] -= qz * w.cvec[(size_t)pa * 6 + r];
  }
  block_sum<6>(acc, red);
  if (tid < 6) w.rhs[6 * a + tid] = (double)gX[6 * a + tid] + acc[tid];
}

template <typename T>
__global__ void __launch_bounds__(kT) bal_pbar(Ws w, int M, int nf, const T* __restrict__ gZ) {
  const int k = blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  const bool ok = nf > 0 && w.status[1] == 0;
  const int cc = w.ccnt[k], base = 2 * w.start[k];
  double Emu = 0, EdX = 0, Edg = 0;
  if (ok)
    for (int i = 0; i < cc; i++) {
      const int f = w.cpose[base + i];
      for (int d = 0; d < 6; d++) {
        const double Ev = w.cvec[(size_t)(base + i) * 6 + d], m = w.mu[6 * f + d],
                     x = w.dX[6 * f + d];
        Emu += Ev * m;
        EdX += Ev * x;
        Edg += Ev * Ev * m * x;
      }
    }
  const double Q = w.Q[k], u = w.u[k], g = (double)gZ[k];
  const double qz = Q * g;
  const double ESE = -(Emu * EdX) - 1e-4 * Edg;
  const double Qbar = g * (u - EdX) - Emu * u - ESE;
  double* pb = w.pb + (size_t)k * kPb;
  pb[0] = qz;
  pb[1] = Q * u;
  pb[2] = Q;
  pb[3] = EdX;
  pb[4] = Emu;
  pb[5] = qz - Q * Emu;   // ubar
  pb[6] = -Q * Q * Qbar;  // Cbar
}

template <typename T>
__global__ void __launch_bounds__(kT)
    bal_ebar(Ws w, int E, int fixedp, int nf, T* __restrict__ gT, T* __restrict__ gW) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= E) return;
  if (!w.eopen[e]) {  // closed: exactly zero, nothing read
    gT[2 * (size_t)e] = gT[2 * (size_t)e + 1] = T(0);
    gW[2 * (size_t)e] = gW[2 * (size_t)e + 1] = T(0);
    return;
  }
  const bool ok = nf > 0 && w.status[1] == 0;
  const int k = w.ek[e];
  const double* rec = w.rec + (size_t)e * kRec;
  const double* pb = w.pb + (size_t)k * kPb;
  const double qz = pb[0], Qu = pb[1], Q = pb[2], EdX = pb[3], Emu = pb[4], ubar = pb[5],
               Cbar = pb[6];
  const int2 pe = w.epose[e];
  const int fi = ok ? free_slot(pe.x, fixedp, nf) : -1;
  const int fj = ok ? free_slot(pe.y, fixedp, nf) : -1;
  const bool same = fi >= 0 && fi == fj;  // one pose in both roles: a = Ji + Jj on its rows
  const int f[2] = {fi, same ? -1 : fj};
  // per effective slot: mu, dX, Ebar_k rows
  double mu[2][6], dx[2][6], Eb[2][6];
  const int cc = w.ccnt[k], base = 2 * w.start[k];
  for (int s = 0; s < 2; s++) {
    if (f[s] < 0) continue;
    const int at = find_pose(w.cpose, base, cc, f[s]);
    for (int d = 0; d < 6; d++) {
      const double m = w.mu[6 * f[s] + d], x = w.dX[6 * f[s] + d];
      const double Ev = w.cvec[(size_t)at * 6 + d];
      mu[s][d] = m;
      dx[s][d] = x;
      Eb[s][d] = -x * qz - m * Qu + Q * (m * EdX + x * Emu) + 2e-4 * Q * (m * x * Ev);
    }
  }
  double* bar = w.bar + (size_t)e * kBar;
  for (int c = 0; c < 2; c++) {
    const double wc = rec[c], r = rec[2 + c], z = rec[4 + c];
    double av[2][6];
    for (int d = 0; d < 6; d++) {
      av[0][d] = rec[6 + 6 * c + d] + (same ? rec[18 + 6 * c + d] : 0.0);
      av[1][d] = rec[18 + 6 * c + d];
    }
    double am = 0, ax = 0, dg = 0, aE = 0;
    for (int s = 0; s < 2; s++) {
      if (f[s] < 0) continue;
      for (int d = 0; d < 6; d++) {
        am += av[s][d] * mu[s][d];
        ax += av[s][d] * dx[s][d];
        dg += av[s][d] * av[s][d] * mu[s][d] * dx[s][d];
        aE += av[s][d] * Eb[s][d];
      }
    }
    const double wbar = (-(am * ax) - 1e-4 * dg) + z * aE + Cbar * z * z + r * am + ubar * z * r;
    const double rbar = wc * (am + ubar * z);
    gT[2 * (size_t)e + c] = (T)rbar;
    gW[2 * (size_t)e + c] = (T)wbar;
    bar[c] = -rbar;                                       // proj-bar
    bar[2 + c] = wc * (aE + 2.0 * Cbar * z + ubar * r);  // zbar
    double ab[2][6];
    for (int s = 0; s < 2; s++)
      for (int d = 0; d < 6; d++)
        ab[s][d] = f[s] < 0 ? 0.0
                            : wc * (-(mu[s][d] * ax + dx[s][d] * am) -
                                    2e-4 * (mu[s][d] * dx[s][d] * av[s][d]) + z * Eb[s][d] +
                                    r * mu[s][d]);
    for (int d = 0; d < 6; d++) {
      bar[4 + 6 * c + d] = ab[0][d];
      bar[16 + 6 * c + d] = same ? ab[0][d] : ab[1][d];
    }
  }
}

// one thread per (edge, direction): directions 0-5 the left tangent of pose i
// (tau, phi), 6-11 of pose j, 12-14 x, y, d of the patch centre
template <typename T>
__global__ void __launch_bounds__(kT)
    bal_egrad(const T* __restrict__ poses, const T* __restrict__ patches,
              const T* __restrict__ intr, int E, int p, Ws w) {
  const size_t id = (size_t)blockIdx.x * kT + threadIdx.x;
  if (id >= (size_t)E * kDir) return;
  const int e = (int)(id / kDir), dir = (int)(id % kDir);
  if (dir == 15) return;
  if (!w.eopen[e]) {
    w.ge[id] = 0.0;
    return;
  }
  const int i = w.epose[e].x, j = w.epose[e].y, k = w.ek[e];
  const T* pi = poses + 7 * (size_t)i;
  const T* pj = poses + 7 * (size_t)j;
  Du ti[3], qi[4], tj[3], qj[4];
  double Ki[4], Kj[4];
  for (int a = 0; a < 3; a++) ti[a] = Du((double)pi[a]), tj[a] = Du((double)pj[a]);
  for (int a = 0; a < 4; a++) {
    qi[a] = Du((double)pi[3 + a]), qj[a] = Du((double)pj[3 + a]);
    Ki[a] = (double)intr[4 * (size_t)i + a], Kj[a] = (double)intr[4 * (size_t)j + a];
  }
  const size_t pp = (size_t)p * p, c = (size_t)(p / 2) * p + p / 2;
  const T* pk = patches + (size_t)k * 3 * pp;
  Du x((double)pk[c]), y((double)pk[pp + c]), d((double)pk[2 * pp + c]);
  if (dir < 12) {
    // Exp(xi) T to first order: (t + tau + phi x t, q + 1/2 (phi, 0) q)
    Du* t = dir < 6 ? ti : tj;
    Du* q = dir < 6 ? qi : qj;
    const int a = dir % 6;
    if (a < 3) {
      t[a].d = 1.0;
    } else {
      double ph[3] = {0, 0, 0};
      ph[a - 3] = 1.0;
      const double tv[3] = {t[0].v, t[1].v, t[2].v};
      const double qv[4] = {q[0].v, q[1].v, q[2].v, q[3].v};
      t[0].d = ph[1] * tv[2] - ph[2] * tv[1];
      t[1].d = ph[2] * tv[0] - ph[0] * tv[2];
      t[2].d = ph[0] * tv[1] - ph[1] * tv[0];
      q[0].d = 0.5 * (ph[0] * qv[3] + ph[1] * qv[2] - ph[2] * qv[1]);
      q[1].d = 0.5 * (ph[1] * qv[3] + ph[2] * qv[0] - ph[0] * qv[2]);
      q[2].d = 0.5 * (ph[2] * qv[3] + ph[0] * qv[1] - ph[1] * qv[0]);
      q[3].d = 0.5 * (-ph[0] * qv[0] - ph[1] * qv[1] - ph[2] * qv[2]);
    }
  } else if (dir == 12) {
    x.d = 1.0;
  } else if (dir == 13) {
    y.d = 1.0;
  } else {
    d.d = 1.0;
  }
  Lin<Du> o;
  linearise<Du>(ti, qi, tj, qj, x, y, d, Ki, Kj, o);
  const double* bar = w.bar + (size_t)e * kBar;
  double g = 0.0;
  for (int cc = 0; cc < 2; cc++) {
    g += bar[cc] * o.proj[cc].d + bar[2 + cc] * o.Jz[cc].d;
    for (int a = 0; a < 6; a++)
      g += bar[4 + 6 * cc + a] * o.Ji[cc][a].d + bar[16 + 6 * cc + a] * o.Jj[cc][a].d;
  }
  w.ge[id] = g;
}

template <typename T>
__global__ void __launch_bounds__(kT) bal_gpose(Ws w, int E, int n, T* __restrict__ gP) {
  __shared__ double red[4 * 6];
  const int a = blockIdx.x, tid = threadIdx.x;
  if (a >= n) {
    if (tid < 6) gP[6 * (size_t)a + tid] = T(0);
    return;
  }
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int e = tid; e < E; e += kT) {
    const int2 pe = w.epose[e];  // closed: (-1, -1), never a pose row
    if (pe.x != a && pe.y != a) continue;
    const double* ge = w.ge + (size_t)e * kDir;
    if (pe.x == a)
      for (int d = 0; d < 6; d++) acc[d] += ge[d];
    if (pe.y == a)
      for (int d = 0; d < 6; d++) acc[d] += ge[6 + d];
  }
  block_sum<6>(acc, red);
  if (tid < 6) gP[6 * (size_t)a + tid] = (T)acc[tid];
}

template <typename T>
__global__ void __launch_bounds__(kT) bal_gpatch(Ws w, int M, T* __restrict__ gK) {
  const int k = blockIdx.x * kT + threadIdx.x;
  if (k >= M) return;
  const int s = w.start[k], len = w.cnt[k];
  double g[3] = {0, 0, 0};
  for (int a = 0; a < len; a++) {
    const double* ge = w.ge + (size_t)w.order[s + a] * kDir + 12;
    g[0] += ge[0];
    g[1] += ge[1];
    g[2] += ge[2];
  }
  for (int d = 0; d < 3; d++) gK[3 * (size_t)k + d] = (T)g[d];
}

inline int blocks(size_t n) { return (int)((n + kT - 1) / kT); }

struct Shape {
  int E, M, p, N, n, fixedp, nf;
};

// INVALID before UNSUPPORTED before WORKSPACE
int check(const Shape& s, int structure_only, int dtype, size_t ws_bytes, int with_backward,
          bool null_arg) {
  if (null_arg) return DPVO_ERR_INVALID;
  if (s.M < 1 || s.N < 1 || s.fixedp < 0 || s.n < s.fixedp || s.n > s.N) return DPVO_ERR_INVALID;
  if (s.p < 1 || s.p % 2 == 0) return DPVO_ERR_INVALID;
  if (dtype != DPVO_F32 && dtype != DPVO_F64) return DPVO_ERR_INVALID;
  (void)structure_only;
  if (6 * (int64_t)s.nf > DPVO_SPD_MAX_N_F64) return DPVO_ERR_UNSUPPORTED;  // dpvo_spd_solve's limit
  if ((int64_t)s.E * kRec > (int64_t)1 << 40) return DPVO_ERR_UNSUPPORTED;
  if (ws_bytes < dpvo_ba_layer_workspace_bytes(s.E, s.M, s.nf, with_backward))
    return DPVO_ERR_WORKSPACE;
  return DPVO_OK;
}

template <typename T>
int forward_t(const void* poses, const void* patches, const void* intr, const void* targets,
              const void* weights, const void* lmbda_dev, double lmbda, const int64_t* ii,
              const int64_t* jj, const int64_t* kk, const Shape& s, const double* bounds, double ep,
              void* dX, void* dZ, const Ws& w, hipStream_t st) {
  if (hipMemsetAsync(w.status, 0, (char*)w.start - (char*)w.status, st) != hipSuccess)
    return DPVO_ERR_LAUNCH;
  hipLaunchKernelGGL(bal_lin<T>, dim3(blocks(s.E)), dim3(kT), 0, st, (const T*)poses,
                     (const T*)patches, (const T*)intr, (const T*)targets, (const T*)weights, ii, jj,
                     kk, s.E, s.M, s.p, s.n, bounds[0], bounds[1], bounds[2], bounds[3], w);
  hipLaunchKernelGGL(bal_scan, dim3(1), dim3(1024), 0, st, w, s.M);
  hipLaunchKernelGGL(bal_place, dim3(blocks(s.E)), dim3(kT), 0, st, w, s.E);
  hipLaunchKernelGGL(bal_patch<T>, dim3(blocks(s.M)), dim3(kT), 0, st, w, s.M, s.fixedp, s.nf,
                     (const T*)lmbda_dev, lmbda);
  if (s.nf > 0) {
    hipLaunchKernelGGL(bal_schur, dim3(s.nf, s.nf + 1), dim3(kT), 0, st, w, s.E, s.M, s.fixedp,
                       s.nf, ep);
    if (launch_status() != DPVO_OK) return DPVO_ERR_LAUNCH;
    const int rc = dpvo_spd_solve(w.S, w.y, w.L, w.dX, w.status + 1, 1, 6 * s.nf, 1, 1, DPVO_F64,
                                  (void*)st);
    if (rc != DPVO_OK) return rc;
  }
  hipLaunchKernelGGL(bal_dz<T>, dim3(blocks((size_t)max(s.M, 6 * s.nf))), dim3(kT), 0, st, w, s.M,
                     s.nf, (T*)dX, (T*)dZ);
  return launch_status();
}

template <typename T>
int backward_t(const void* poses, const void* patches, const void* intr, const void* gX,
               const void* gZ, const Shape& s, void* gT, void* gW, void* gP, void* gK, const Ws& w,
               hipStream_t st) {
  if (s.nf > 0) {
    hipLaunchKernelGGL(bal_rhs<T>, dim3(s.nf), dim3(kT), 0, st, w, s.M, (const T*)gX,
                       (const T*)gZ);
    if (launch_status() != DPVO_OK) return DPVO_ERR_LAUNCH;
    const int rc = dpvo_spd_solve(w.L, w.rhs, nullptr, w.mu, nullptr, 1, 6 * s.nf, 1, 0, DPVO_F64,
                                  (void*)st);
    if (rc != DPVO_OK) return rc;
  }
  hipLaunchKernelGGL(bal_pbar<T>, dim3(blocks(s.M)), dim3(kT), 0, st, w, s.M, s.nf, (const T*)gZ);
  hipLaunchKernelGGL(bal_ebar<T>, dim3(blocks(s.E)), dim3(kT), 0, st, w, s.E, s.fixedp, s.nf,
                     (T*)gT, (T*)gW);
  hipLaunchKernelGGL(bal_egrad<T>, dim3(blocks((size_t)s.E * kDir)), dim3(kT), 0, st,
                     (const T*)poses, (const T*)patches, (const T*)intr, s.E, s.p, w);
  hipLaunchKernelGGL(bal_gpose<T>, dim3(s.N), dim3(kT), 0, st, w, s.E, s.n, (T*)gP);
  hipLaunchKernelGGL(bal_gpatch<T>, dim3(blocks(s.M)), dim3(kT), 0, st, w, s.M, (T*)gK);
  return launch_status();
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_ba_layer_workspace_bytes(int E, int M, int n_free, int with_backward) {
  if (E < 0 || M < 0 || n_free < 0) return 0;
  return layout(nullptr, E, M, n_free, with_backward).bytes;
}

DPVO_EXPORT int dpvo_ba_layer_forward(const void* poses, const void* patches,
                                      const void* intrinsics, const void* targets,
                                      const void* weights, const void* lmbda_dev, double lmbda,
                                      const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                                      int M, int p, int N, int n, int fixedp, int structure_only,
                                      const double* bounds, double ep, int dtype, void* dX, void* dZ,
                                      void* ws, size_t ws_bytes, int with_backward, void* stream) {
  if (E <= 0) return DPVO_OK;
  Shape s{E, M, p, N, n, fixedp, structure_only ? 0 : n - fixedp};
  const bool null_arg = !poses || !patches || !intrinsics || !targets || !weights || !ii || !jj ||
                        !kk || !bounds || !dZ || !ws || (s.nf > 0 && !dX);
  const int rc = check(s, structure_only, dtype, ws_bytes, with_backward, null_arg);
  if (rc != DPVO_OK) return rc;
  const Ws w = layout(ws, E, M, s.nf, with_backward);
  if (dtype == DPVO_F64)
    return forward_t<double>(poses, patches, intrinsics, targets, weights, lmbda_dev, lmbda, ii, jj,
                             kk, s, bounds, ep, dX, dZ, w, as_stream(stream));
  return forward_t<float>(poses, patches, intrinsics, targets, weights, lmbda_dev, lmbda, ii, jj, kk,
                          s, bounds, ep, dX, dZ, w, as_stream(stream));
}

DPVO_EXPORT int dpvo_ba_layer_backward(const void* poses, const void* patches,
                                       const void* intrinsics, const void* gX, const void* gZ, int E,
                                       int M, int p, int N, int n, int fixedp, int structure_only,
                                       int dtype, void* g_targets, void* g_weights, void* g_poses,
                                       void* g_patches, void* ws, size_t ws_bytes, void* stream) {
  if (E <= 0) return DPVO_OK;
  Shape s{E, M, p, N, n, fixedp, structure_only ? 0 : n - fixedp};
  const bool null_arg = !poses || !patches || !intrinsics || !gZ || !g_targets || !g_weights ||
                        !g_poses || !g_patches || !ws || (s.nf > 0 && !gX);
  const int rc = check(s, structure_only, dtype, ws_bytes, 1, null_arg);
  if (rc != DPVO_OK) return rc;
  const Ws w = layout(ws, E, M, s.nf, 1);
  if (dtype == DPVO_F64)
    return backward_t<double>(poses, patches, intrinsics, gX, gZ, s, g_targets, g_weights, g_poses,
                              g_patches, w, as_stream(stream));
  return backward_t<float>(poses, patches, intrinsics, gX, gZ, s, g_targets, g_weights, g_poses,
                           g_patches, w, as_stream(stream));
}
