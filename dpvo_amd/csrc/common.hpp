// common.hpp -- shared device/host helpers for the gfx950 DPVO hot path.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpvo_hot.h"

#define DPVO_EXPORT extern "C" __attribute__((visibility("default")))

namespace dpvo {

constexpr int kWave = 64;  // CDNA wavefront width (never 32)
constexpr int kMaxDevices = 64;  // per-device one-time host state (function attributes)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? DPVO_OK : DPVO_ERR_LAUNCH;
}

// --- element type helpers ---------------------------------------------------
template <typename T>
struct Acc { using type = float; };
template <>
struct Acc<double> { using type = double; };

__device__ __forceinline__ float to_acc(float v) { return v; }
__device__ __forceinline__ float to_acc(__half v) { return __half2float(v); }
__device__ __forceinline__ double to_acc(double v) { return v; }

template <typename T>
__device__ __forceinline__ T from_acc(float v);
template <>
__device__ __forceinline__ float from_acc<float>(float v) { return v; }
template <>
__device__ __forceinline__ __half from_acc<__half>(float v) { return __float2half(v); }
template <>
__device__ __forceinline__ double from_acc<double>(float v) { return (double)v; }

// static_cast<int>(floor(v)) with out-of-range values pushed far outside
// every map (the reference is undefined there; correlation_kernel.cu:156-157)
__device__ __forceinline__ int ifloor_safe(float v) {
  float f = floorf(v);
  f = fminf(fmaxf(f, -1.0e8f), 1.0e8f);  // NaN -> -1e8 (fmaxf drops NaN)
  return (int)f;
}

__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Order LDS traffic between lanes of ONE wave (a wave's DS ops execute in
// order; this stops the compiler from moving them across the point).  The
// fence is restricted to the LDS address space ("local"): a plain fence also
// orders global memory and makes the compiler wait for every outstanding
// global load (vmcnt(0)) at the point, which drains the load rings of the
// streaming kernels (A-CORR's tile ring) at every use.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
}

// --- 16-B write-through stores ------------------------------------------------
// raw buffer resources (gfx950 dword 3) and the buffer builtins' cache-policy
// bit for sc1 (agent-coherent: bypasses the CU's L1; stores write through L2)
constexpr int kBufDword3 = 0x00020000;
constexpr int kSc1 = 16;
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// A buffer of `bytes` bytes at `base` (wave-uniform).  Build it at the block or
// slot that is written, not at the tensor: offsets are 32-bit and a store past
// `bytes` is dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_buffer(void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, kBufDword3);
}
// 16 B of one lane at byte offset `off` (a multiple of 16), write-through: the
// line is not left dirty in the XCD's L2, so the bytes need no second trip at
// the end-of-kernel release (and no stale copy can be written back later).
// Only for 16 B per lane: a 4-B sc1 store costs about 6x, an 8-B one 2.7x per byte.
__device__ __forceinline__ void wt_store16(__amdgpu_buffer_rsrc_t rs, int off, v4u v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, kSc1);
}
__device__ __forceinline__ void wt_store16(__amdgpu_buffer_rsrc_t rs, int off, float4 v) {
  wt_store16(rs, off, __builtin_bit_cast(v4u, v));
}
// 16 B of one lane as a non-temporal store (the `nt` bit; not write-through: the
// end-of-kernel release still publishes the line).  Which bulk writer takes
// which flavour is decided by measurement: DESIGN.md, "What the bulk writers
// leave behind".
__device__ __forceinline__ void nt_store16(float* d, float4 v) {
  __builtin_nontemporal_store(__builtin_bit_cast(v4u, v), reinterpret_cast<v4u*>(d));
}

// wave-uniform per-level parameter without a dynamic index into the kernel
// argument struct (that would route every access through scratch / flat
// loads, which count in vmcnt and force full drains in the tile loop)
template <typename X>
__device__ __forceinline__ X sel4(int l, X a, X b, X c, X d) {
  return l == 0 ? a : l == 1 ? b : l == 2 ? c : d;
}

// Workgroup barrier that orders LDS traffic only (same reasoning one level
// up): global loads issued before it stay in flight across it.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// wave64 inclusive scan of ints with DPP (row shifts 1/2/4/8 inside each row
// of 16 lanes, then row_bcast:15 / row_bcast:31 across rows): six VALU ops
// with a DPP source.  A __shfl_* is a ds_bpermute, an LDS round trip per
// step.  `id` is op's identity (what an out-of-row source contributes).
template <typename Op>
__device__ __forceinline__ int wave_scan_dpp(int x, int id, Op op) {
  x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x111, 0xf, 0xf, false));  // row_shr:1
  x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x112, 0xf, 0xf, false));  // row_shr:2
  x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x114, 0xf, 0xf, false));  // row_shr:4
  x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x118, 0xf, 0xf, false));  // row_shr:8
  x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x142, 0xa, 0xf, false));  // row_bcast:15
  x = op(x, __builtin_amdgcn_update_dpp(id, x, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return x;
}
__device__ __forceinline__ int wave_incl_sum(int x) {
  return wave_scan_dpp(x, 0, [](int a, int b) { return a + b; });
}
// wave-wide reductions (every lane gets the result)
__device__ __forceinline__ int wave_sum_i(int x) {
  return __builtin_amdgcn_readlane(wave_incl_sum(x), 63);
}
__device__ __forceinline__ int wave_min_i(int x) {
  return __builtin_amdgcn_readlane(
      wave_scan_dpp(x, 0x7fffffff, [](int a, int b) { return a < b ? a : b; }), 63);
}
__device__ __forceinline__ int wave_max_i(int x) {
  return __builtin_amdgcn_readlane(
      wave_scan_dpp(x, (int)0x80000000, [](int a, int b) { return a > b ? a : b; }), 63);
}

// Workgroup exclusive scan of one int per thread, in thread order: returns the
// sum of v over the threads before this one, and in `total` the sum over all
// of them (every thread gets both).  Called by every thread of a workgroup
// of a multiple of 64 (at most 1024) threads.  One DPP scan per wave, the
// wave totals through scr (LDS, blockDim.x / 64 ints; the callers keep the
// blockDim.x / 64 + 1 of fscan), which every wave then scans for itself.
// Two LDS barriers: one after the totals are written, one after they are
// read -- so scr may be written again (the next call of a loop included) as
// soon as the call returns.  No barrier before the first write: the caller
// orders whatever it kept in scr before the call.
__device__ __forceinline__ int block_excl_sum(int v, int* scr, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int incl = wave_incl_sum(v);
  if (lane == 63) scr[wid] = incl;
  lds_barrier();
  const int t = lane < nw ? scr[lane] : 0;
  const int tincl = wave_incl_sum(t);
  lds_barrier();
  total = __builtin_amdgcn_readlane(tincl, 63);
  return __builtin_amdgcn_readlane(tincl - t, wave_uniform(wid)) + incl - v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// --- fp32 SE3 primitives of ba_cuda.cu:36-174 (restated, device) ---------------
// No FMA contraction here: the per-edge arithmetic then rounds exactly like the
// C oracle (x86, no FMA), which keeps the parity tests tight.
#pragma clang fp contract(off)
__device__ __forceinline__ void actSO3(const float* q, const float* X, float* Y) {
  float uv[3];
  uv[0] = 2.0f * (q[1] * X[2] - q[2] * X[1]);
  uv[1] = 2.0f * (q[2] * X[0] - q[0] * X[2]);
  uv[2] = 2.0f * (q[0] * X[1] - q[1] * X[0]);
  Y[0] = X[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
  Y[1] = X[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
  Y[2] = X[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}

__device__ __forceinline__ void actSE3(const float* t, const float* q, const float* X, float* Y) {
  actSO3(q, X, Y);
  Y[3] = X[3];
  Y[0] += X[3] * t[0];
  Y[1] += X[3] * t[1];
  Y[2] += X[3] * t[2];
}

// Ji = Adj(Gij)^T Jj (ba_cuda.cu:57-72)
__device__ __forceinline__ void adjSE3(const float* t, const float* q, const float* X, float* Y) {
  float qinv[4] = {-q[0], -q[1], -q[2], q[3]};
  actSO3(qinv, &X[0], &Y[0]);
  actSO3(qinv, &X[3], &Y[3]);
  float u[3], v[3];
  u[0] = t[2] * X[1] - t[1] * X[2];
  u[1] = t[0] * X[2] - t[2] * X[0];
  u[2] = t[1] * X[0] - t[0] * X[1];
  actSO3(qinv, u, v);
  Y[3] += v[0];
  Y[4] += v[1];
  Y[5] += v[2];
}

// Gij = Pj * Pi^-1 (ba_cuda.cu:74-85)
__device__ __forceinline__ void relSE3(const float* ti, const float* qi, const float* tj,
                                       const float* qj, float* tij, float* qij) {
  qij[0] = -qj[3] * qi[0] + qj[0] * qi[3] - qj[1] * qi[2] + qj[2] * qi[1];
  qij[1] = -qj[3] * qi[1] + qj[1] * qi[3] - qj[2] * qi[0] + qj[0] * qi[2];
  qij[2] = -qj[3] * qi[2] + qj[2] * qi[3] - qj[0] * qi[1] + qj[1] * qi[0];
  qij[3] = qj[3] * qi[3] + qj[0] * qi[0] + qj[1] * qi[1] + qj[2] * qi[2];
  actSO3(qij, ti, tij);
  tij[0] = tj[0] - tij[0];
  tij[1] = tj[1] - tij[1];
  tij[2] = tj[2] - tij[2];
}

__device__ __forceinline__ void expSO3(const float* phi, float* q) {  // ba_cuda.cu:88-110
  float theta_sq = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  float theta_p4 = theta_sq * theta_sq;
  float theta = sqrtf(theta_sq);
  float imag, real;
  if (theta_sq < 1e-8f) {
    imag = 0.5f - (1.0f / 48.0f) * theta_sq + (1.0f / 3840.0f) * theta_p4;
    real = 1.0f - (1.0f / 8.0f) * theta_sq + (1.0f / 384.0f) * theta_p4;
  } else {
    imag = sinf(0.5f * theta) / theta;
    real = cosf(0.5f * theta);
  }
  q[0] = imag * phi[0];
  q[1] = imag * phi[1];
  q[2] = imag * phi[2];
  q[3] = real;
}

__device__ __forceinline__ void crossInplace(const float* a, float* b) {
  float x0 = a[1] * b[2] - a[2] * b[1];
  float x1 = a[2] * b[0] - a[0] * b[2];
  float x2 = a[0] * b[1] - a[1] * b[0];
  b[0] = x0;
  b[1] = x1;
  b[2] = x2;
}

__device__ __forceinline__ void expSE3(const float* xi, float* t, float* q) {  // :125-153
  expSO3(xi + 3, q);
  float tau[3] = {xi[0], xi[1], xi[2]};
  float phi[3] = {xi[3], xi[4], xi[5]};
  float theta_sq = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
  float theta = sqrtf(theta_sq);
  t[0] = tau[0];
  t[1] = tau[1];
  t[2] = tau[2];
  if (theta > 1e-4f) {
    float a = (1.0f - cosf(theta)) / theta_sq;
    crossInplace(phi, tau);
    t[0] += a * tau[0];
    t[1] += a * tau[1];
    t[2] += a * tau[2];
    float b = (theta - sinf(theta)) / (theta * theta_sq);
    crossInplace(phi, tau);
    t[0] += b * tau[0];
    t[1] += b * tau[1];
    t[2] += b * tau[2];
  }
}

// pose <- Exp(xi) * pose, no renormalisation (ba_cuda.cu:156-174)
__device__ __forceinline__ void retrSE3(const float* xi, const float* t, const float* q, float* t1,
                                        float* q1) {
  float dt[3] = {0, 0, 0};
  float dq[4] = {0, 0, 0, 1};
  expSE3(xi, dt, dq);
  q1[0] = dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1];
  q1[1] = dq[3] * q[1] + dq[1] * q[3] + dq[2] * q[0] - dq[0] * q[2];
  q1[2] = dq[3] * q[2] + dq[2] * q[3] + dq[0] * q[1] - dq[1] * q[0];
  q1[3] = dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2];
  actSO3(dq, t, t1);
  t1[0] += dt[0];
  t1[1] += dt[1];
  t1[2] += dt[2];
}

// F-REPROJ of one (edge n, patch pixel pix) (ba_cuda.cu:379-429): shared by
// reproject_kernel (ba.hip) and the fused reproject + BA-plan launch
// (ba_window.hip), so both round identically.
// reprojected pixel (u, v) of patch pixel `pix` of edge n (ba_cuda.cu:379-429)
__device__ __forceinline__ void reproject_uv(const float* __restrict__ poses,
                                             const float* __restrict__ patches,
                                             const float* __restrict__ intrinsics,
                                             const int64_t* __restrict__ ii,
                                             const int64_t* __restrict__ jj,
                                             const int64_t* __restrict__ kk, int n, int pix, int P,
                                             int num_poses, int num_patches, float& u, float& v) {
  const int PP = P * P;
  const float fx = intrinsics[0], fy = intrinsics[1], cx = intrinsics[2], cy = intrinsics[3];
  const int ix = (int)min(max(ii[n], (int64_t)0), (int64_t)num_poses - 1);
  const int jx = (int)min(max(jj[n], (int64_t)0), (int64_t)num_poses - 1);
  const int64_t kx = min(max(kk[n], (int64_t)0), (int64_t)num_patches - 1);
  const float* pi = poses + 7 * (size_t)ix;
  const float* pj = poses + 7 * (size_t)jx;
  float ti[3] = {pi[0], pi[1], pi[2]}, qi[4] = {pi[3], pi[4], pi[5], pi[6]};
  float tj[3] = {pj[0], pj[1], pj[2]}, qj[4] = {pj[3], pj[4], pj[5], pj[6]};
  float tij[3], qij[4];
  relSE3(ti, qi, tj, qj, tij, qij);
  const float* pk = patches + (size_t)kx * 3 * PP;
  float Xi[4], Xj[4];
  Xi[0] = (pk[pix] - cx) / fx;
  Xi[1] = (pk[PP + pix] - cy) / fy;
  Xi[2] = 1.0f;
  Xi[3] = pk[2 * PP + pix];
  actSE3(tij, qij, Xi, Xj);
  u = fx * (Xj[0] / Xj[2]) + cx;
  v = fy * (Xj[1] / Xj[2]) + cy;
}

__device__ __forceinline__ void reproject_pixel(const float* __restrict__ poses,
                                                const float* __restrict__ patches,
                                                const float* __restrict__ intrinsics,
                                                const int64_t* __restrict__ ii,
                                                const int64_t* __restrict__ jj,
                                                const int64_t* __restrict__ kk, int n, int pix,
                                                int P, int num_poses, int num_patches,
                                                float* __restrict__ coords) {
  const int PP = P * P;
  float u, v;
  reproject_uv(poses, patches, intrinsics, ii, jj, kk, n, pix, P, num_poses, num_patches, u, v);
  coords[((size_t)n * 2 + 0) * PP + pix] = u;
  coords[((size_t)n * 2 + 1) * PP + pix] = v;
}

#pragma clang fp contract(fast)

// --- edge order for A-CORR (XCD-aware scheduling) -----------------------------
// One workgroup: order[p] = the edge at position p when edges are grouped by
// their target frame jj and, inside a frame, by the 16-pixel row band of the
// reprojected patch centre (counting sort; the order inside a (frame, band)
// bin is whatever the LDS atomics give -- A-CORR results do not depend on it,
// every edge is computed independently).  A-CORR gives each XCD an eighth of
// the positions: a frame's edges on one L2, and edges whose windows overlap
// near each other in the sequence, so the waves that share box lines run at
// the same time (cfg2 fp32: 41.3 -> 40.4 us, scripts/corr_order_probe.py).
// The centre is recomputed in both passes (no per-edge LDS: E is unbounded
// here).  bins: kOrderLds ints of LDS.  Frames outside
// [0, min(N2, kOrderBins / kOrderBands)) share the last frame's bins.
struct OrderIn {
  const float* poses;
  const float* patches;
  const float* intrinsics;
  const int64_t* ii;
  const int64_t* kk;
  int P, num_poses, num_patches;
};
constexpr int kOrderBins = 1024;
constexpr int kOrderBands = 16;  // row bands of 16 level-1 pixels (rows >= 240 share the last)
__device__ __forceinline__ int edge_order_key(const OrderIn& q, const int64_t* __restrict__ jj,
                                              int e, int nf) {
  const int64_t f = jj[e];
  float u, v;
  const int c = (q.P / 2) * q.P + q.P / 2;
  reproject_uv(q.poses, q.patches, q.intrinsics, q.ii, jj, q.kk, e, c, q.P, q.num_poses,
               q.num_patches, u, v);
  const int band = v >= 0.0f ? (int)fminf(v * (1.0f / 16.0f), (float)(kOrderBands - 1)) : 0;  // NaN: 0
  return ((f >= 0 && f < nf) ? (int)f : nf - 1) * kOrderBands + band;
}
// Keys of the groups after the first (E > 4 T only: recomputed in both
// passes), counted (order == null) or scattered.  One call site per pass
// behind an E > 4 T branch: the graphs of the update step (E <= 4 T) run
// straight through one copy of the key arithmetic.
__device__ __forceinline__ void edge_order_rest(const OrderIn& q, const int64_t* __restrict__ jj, int E,
                                             int nf, int* __restrict__ order, int* bins) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int e0 = tid + 4 * T; e0 < E; e0 += 4 * T) {
    int k[4];
#pragma unroll
    for (int r = 0; r < 4; r++) k[r] = edge_order_key(q, jj, min(e0 + r * T, E - 1), nf);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (e0 + r * T >= E) continue;
      const int p = atomicAdd(&bins[k[r]], 1);
      if (order) order[p] = e0 + r * T;
    }
  }
}
constexpr int kOrderLds = kOrderBins + 1 + 16;  // bins + the scan's wave totals (<= 1024 threads)
__device__ inline void edge_order_block(const OrderIn& q, const int64_t* __restrict__ jj, int E,
                                        int N2, int* __restrict__ order, int* bins) {
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wid = tid >> 6;
  const int nf = min(max(N2, 1), kOrderBins / kOrderBands), nb = nf * kOrderBands;
  int* scr = bins + kOrderBins + 1;
  if (E <= 0) return;
  // keys of the thread's first 4 edges (tid + r T), every load of the four
  // issued before the first use; they stay in registers for the scatter
  int k0[4];
#pragma unroll
  for (int r = 0; r < 4; r++) k0[r] = edge_order_key(q, jj, min(tid + r * T, E - 1), nf);
  for (int b = tid; b <= nb; b += T) bins[b] = 0;
  lds_barrier();
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (tid + r * T < E) atomicAdd(&bins[k0[r]], 1);
  if (__builtin_expect(E > 4 * T, 0)) edge_order_rest(q, jj, E, nf, nullptr, bins);
  lds_barrier();
  // exclusive scan of the nb <= 1024 bins by every wave: a run of `per` bins
  // per thread, one DPP scan per wave, the wave totals through LDS
  const int per = (nb + T - 1) / T, b0 = min(tid * per, nb), b1 = min(b0 + per, nb);
  int sum = 0;
  for (int b = b0; b < b1; b++) sum += bins[b];
  const int incl = wave_incl_sum(sum);
  if (lane == 63) scr[wid] = incl;
  lds_barrier();
  int run = incl - sum;
  for (int w = 0; w < wid; w++) run += scr[w];
  for (int b = b0; b < b1; b++) {
    const int c = bins[b];
    bins[b] = run;
    run += c;
  }
  lds_barrier();
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (tid + r * T < E) order[atomicAdd(&bins[k0[r]], 1)] = tid + r * T;
  if (__builtin_expect(E > 4 * T, 0)) edge_order_rest(q, jj, E, nf, order, bins);
}

}  // namespace dpvo
