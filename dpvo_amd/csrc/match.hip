// match.hip -- mutual-nearest-neighbour descriptor matching with a ratio test
// on gfx950: the stand-in for LightGlue between two DISK descriptor sets in
// the long-term loop closure (dpvo/loop_closure/long_term.py:82-88, 228-229).
//
//   sim[i, j] = sum_d a[i, d] b[j, d]                  (fp32, d ascending)
//   d2[i, j]  = max(|a_i|^2 + |b_j|^2 - 2 sim[i, j], 0)
//   (i, j) match  <=>  j is i's best column and i is j's best row (smaller d2,
//   then lower index), d2 <= r2 * second-best d2 on both sides, d2 <= max_d2.
//
// Two launches, no host sync, no float atomics, the [N0, N1] matrix never in
// memory:
//
// match_tile_kernel    one workgroup of four waves per 64 x 64 tile.  The two
//                      64 x 32 descriptor slabs of a step go through LDS; each
//                      wave accumulates one 32 x 32 quarter with
//                      v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fma
//                      chain), sixteen accumulator registers.  The squared
//                      norms are summed on the way into LDS.  Each wave then
//                      reduces its quarter to a (best d2, best index, second
//                      d2) triple per column (in registers: a column lives on
//                      one lane pair) and per row (through a 32 x 33 LDS image
//                      of the quarter), the two quarters of a row / column are
//                      merged in LDS, and the tile writes one triple per row
//                      and per column.
// match_finish_kernel  one workgroup: merges the tile triples of every row and
//                      column (the merge is keyed on (d2, index), so its order
//                      does not matter), applies the three tests, writes the
//                      dense partners and compacts the pairs in ascending row
//                      order with a workgroup scan.
#include <math.h>

#include "common.hpp"

namespace dpvo {
namespace match {

constexpr int kTile = 64;            // rows and columns of a workgroup's tile
constexpr int kKC = 32;              // descriptor elements staged per step
constexpr int kStride = kKC + 1;     // LDS row stride: the 32 rows of an operand on 32 banks
constexpr int kThreads = 256;
constexpr int kMaxN = 4096;
constexpr int kMaxD = 256;
constexpr int kFinT = 1024;
constexpr int kNone = 0x7fffffff;    // index of "no candidate": loses every tie

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Args {
  const void* a;  // [N0, D]
  const void* b;  // [N1, D]
  const int32_t* n0_dev;
  const int32_t* n1_dev;
  int n0, n1, N0, N1, D;
  float r2, md2;
  float* ws;
  int64_t* partner0;
  int64_t* partner1;
  int64_t* matches;
  float* dist2;
  int32_t* count;
};

// Triples of the workspace: row triples [T1][P0] then column triples [T0][P1],
// each as three planes (d2, index, second d2); P = tiles * kTile.
struct Layout {
  int T0, T1, P0, P1;
  size_t rows, cols;  // elements of one plane
  __host__ __device__ Layout(int N0, int N1) {
    T0 = (N0 + kTile - 1) / kTile;
    T1 = (N1 + kTile - 1) / kTile;
    P0 = T0 * kTile;
    P1 = T1 * kTile;
    rows = (size_t)T1 * P0;
    cols = (size_t)T0 * P1;
  }
  __host__ __device__ size_t bytes() const { return 3 * (rows + cols) * sizeof(float); }
};

struct Top2 {
  float d;  // best d2
  int i;    // its index
  float s;  // second-best d2
};

__device__ __forceinline__ Top2 top2_empty() { return Top2{INFINITY, kNone, INFINITY}; }

__device__ __forceinline__ bool before(float d, int i, float e, int j) {
  return d < e || (d == e && i < j);
}

__device__ __forceinline__ void top2_push(Top2& t, float d, int i) {
  if (before(d, i, t.d, t.i)) {
    t.s = t.d;
    t.d = d;
    t.i = i;
  } else {
    t.s = fminf(t.s, d);
  }
}

// order-independent: the best by (d2, index), the second the smallest of the rest
__device__ __forceinline__ Top2 top2_merge(Top2 a, Top2 b) {
  if (before(b.d, b.i, a.d, a.i)) {
    const Top2 t = a;
    a = b;
    b = t;
  }
  a.s = fminf(a.s, b.d);
  return a;
}

__device__ __forceinline__ Top2 top2_other_half(const Top2& t) {
  Top2 o;
  o.d = __shfl_xor(t.d, 32, kWave);
  o.i = __shfl_xor(t.i, 32, kWave);
  o.s = __shfl_xor(t.s, 32, kWave);
  return o;
}

__device__ __forceinline__ float4 load4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ float4 load4(const __half* p) {
  const uint2 u = *reinterpret_cast<const uint2*>(p);
  const __half2 lo = *reinterpret_cast<const __half2*>(&u.x);
  const __half2 hi = *reinterpret_cast<const __half2*>(&u.y);
  const float2 a = __half22float2(lo), b = __half22float2(hi);
  return make_float4(a.x, a.y, b.x, b.y);
}

__device__ __forceinline__ int row_limit(const int32_t* dev, int host, int N) {
  return min(max(dev ? *dev : host, 0), N);
}

__device__ __forceinline__ float sq_acc(float4 v, float s) {
  s = __fmaf_rn(v.x, v.x, s);
  s = __fmaf_rn(v.y, v.y, s);
  s = __fmaf_rn(v.z, v.z, s);
  return __fmaf_rn(v.w, v.w, s);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) match_tile_kernel(Args g) {
  // the two slabs of a step; after the last step the four 32 x 33 quarter images
  __shared__ float stage[2 * kTile * kStride];
  __shared__ float norm[2][kTile];
  __shared__ float pd[2][2][kTile];  // [rows / columns][quarter][element]
  __shared__ int pi[2][2][kTile];
  __shared__ float ps[2][2][kTile];
  static_assert(4 * 32 * 33 == 2 * kTile * kStride, "the quarter images reuse the slabs");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n0 = row_limit(g.n0_dev, g.n0, g.N0), n1 = row_limit(g.n1_dev, g.n1, g.N1);
  const int r0 = blockIdx.y * kTile, c0 = blockIdx.x * kTile;
  const Layout L(g.N0, g.N1);
  float* rowd = g.ws + (size_t)blockIdx.x * L.P0 + r0;
  float* cold = g.ws + 3 * L.rows + (size_t)blockIdx.y * L.P1 + c0;

  if (r0 >= n0 || c0 >= n1) {  // nothing valid in this tile: empty triples
    if (tid < 2 * kTile) {
      float* o = tid < kTile ? rowd + tid : cold + (tid - kTile);
      const size_t plane = tid < kTile ? L.rows : L.cols;
      o[0] = INFINITY;
      reinterpret_cast<int*>(o)[plane] = kNone;
      o[2 * plane] = INFINITY;
    }
    return;
  }

  const T* A = reinterpret_cast<const T*>(g.a);
  const T* B = reinterpret_cast<const T*>(g.b);
  float* As = stage;
  float* Bs = stage + kTile * kStride;
  const int D = g.D;
  const int rw = (w >> 1) * 32, cw = (w & 1) * 32;  // this wave's quarter
  const int ml = lane & 31, mh = lane >> 5;
  const int c4 = tid & 7, lrow = tid >> 3;  // this thread's float4 of rows lrow, lrow + 32

  f32x16 acc;
#pragma unroll
  for (int k = 0; k < 16; k++) acc[k] = 0.0f;
  float sa[2] = {0.0f, 0.0f}, sb[2] = {0.0f, 0.0f};

  for (int k0 = 0; k0 < D; k0 += kKC) {
    const int k = k0 + 4 * c4;
    float4 va[2], vb[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int ra = r0 + lrow + 32 * q, rb = c0 + lrow + 32 * q;
      // rows at or beyond the limit are never read
      va[q] = (ra < n0 && k < D) ? load4(A + (size_t)ra * D + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      vb[q] = (rb < n1 && k < D) ? load4(B + (size_t)rb * D + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      float* da = As + (lrow + 32 * q) * kStride + 4 * c4;
      float* db = Bs + (lrow + 32 * q) * kStride + 4 * c4;
      da[0] = va[q].x; da[1] = va[q].y; da[2] = va[q].z; da[3] = va[q].w;
      db[0] = vb[q].x; db[1] = vb[q].y; db[2] = vb[q].z; db[3] = vb[q].w;
      sa[q] = sq_acc(va[q], sa[q]);
      sb[q] = sq_acc(vb[q], sb[q]);
    }
    __syncthreads();
    const int steps = min(kKC, D - k0) / 2;
    const float* pa = As + (rw + ml) * kStride + mh;
    const float* pb = Bs + (cw + ml) * kStride + mh;
    for (int kk = 0; kk < steps; kk++)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * kk], pb[2 * kk], acc, 0, 0, 0);
    __syncthreads();
  }

  // squared norms: the eight threads of a row hold one slice each
#pragma unroll
  for (int q = 0; q < 2; q++) {
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
      sa[q] += __shfl_xor(sa[q], o, kWave);
      sb[q] += __shfl_xor(sb[q], o, kWave);
    }
    if (c4 == 0) {
      norm[0][lrow + 32 * q] = sa[q];
      norm[1][lrow + 32 * q] = sb[q];
    }
  }
  __syncthreads();

  // the quarter: C/D layout column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* img = stage + w * (32 * 33);
  {
    const int gcol = c0 + cw + ml;
    const bool cvalid = gcol < n1;
    const float nbv = norm[1][cw + ml];
    Top2 ct = top2_empty();
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
      const int row = (reg & 3) + 8 * (reg >> 2) + 4 * mh;
      const int grow = r0 + rw + row;
      const bool valid = cvalid && grow < n0;
      float v = __fsub_rn(__fadd_rn(norm[0][rw + row], nbv), __fmul_rn(2.0f, acc[reg]));
      v = v < 0.0f ? 0.0f : v;
      const float d = valid ? v : INFINITY;
      img[row * 33 + ml] = d;
      top2_push(ct, d, valid ? grow : kNone);
    }
    ct = top2_merge(ct, top2_other_half(ct));
    if (mh == 0) {
      pd[1][w >> 1][cw + ml] = ct.d;
      pi[1][w >> 1][cw + ml] = ct.i;
      ps[1][w >> 1][cw + ml] = ct.s;
    }
  }
  __syncthreads();
  {
    const int grow = r0 + rw + ml;
    const bool rvalid = grow < n0;
    Top2 rt = top2_empty();
#pragma unroll
    for (int c = 0; c < 16; c++) {
      const int col = 16 * mh + c, gcol = c0 + cw + col;
      top2_push(rt, img[ml * 33 + col], (rvalid && gcol < n1) ? gcol : kNone);
    }
    rt = top2_merge(rt, top2_other_half(rt));
    if (mh == 0) {
      pd[0][w & 1][rw + ml] = rt.d;
      pi[0][w & 1][rw + ml] = rt.i;
      ps[0][w & 1][rw + ml] = rt.s;
    }
  }
  __syncthreads();
  if (tid < 2 * kTile) {
    const int s = tid < kTile ? 0 : 1, e = tid & (kTile - 1);
    const Top2 t = top2_merge(Top2{pd[s][0][e], pi[s][0][e], ps[s][0][e]},
                              Top2{pd[s][1][e], pi[s][1][e], ps[s][1][e]});
    float* o = s == 0 ? rowd + e : cold + e;
    const size_t plane = s == 0 ? L.rows : L.cols;
    o[0] = t.d;
    reinterpret_cast<int*>(o)[plane] = t.i;
    o[2 * plane] = t.s;
  }
}

// merged triple of element e over its T tile triples (plane stride `plane`, tile stride P)
__device__ __forceinline__ Top2 merge_tiles(const float* base, size_t plane, int P, int T, int e) {
  Top2 t = top2_empty();
#pragma unroll 8
  for (int k = 0; k < T; k++) {
    const float* p = base + (size_t)k * P + e;
    t = top2_merge(t, Top2{p[0], reinterpret_cast<const int*>(p)[plane], p[2 * plane]});
  }
  return t;
}

__global__ void __launch_bounds__(kFinT) match_finish_kernel(Args g) {
  __shared__ int row_j[kMaxN];  // the row's best column if it passes its tests, else -1
  __shared__ int col_i[kMaxN];
  __shared__ float row_d[kMaxN];
  __shared__ int scr[kFinT / 64 + 1];
  const int tid = threadIdx.x;
  const int n0 = row_limit(g.n0_dev, g.n0, g.N0), n1 = row_limit(g.n1_dev, g.n1, g.N1);
  const Layout L(g.N0, g.N1);
  const float r2 = g.r2, md2 = g.md2;

  for (int i = tid; i < g.N0; i += kFinT) {
    int best = -1;
    float d = 0.0f;
    if (i < n0) {
      const Top2 t = merge_tiles(g.ws, L.rows, L.P0, L.T1, i);
      d = t.d;
      if (t.i != kNone && t.d <= __fmul_rn(r2, t.s) && t.d <= md2) best = t.i;
    }
    row_j[i] = best;
    row_d[i] = d;
  }
  for (int j = tid; j < g.N1; j += kFinT) {
    int best = -1;
    if (j < n1) {
      const Top2 t = merge_tiles(g.ws + 3 * L.rows, L.cols, L.P1, L.T0, j);
      if (t.i != kNone && t.d <= __fmul_rn(r2, t.s) && t.d <= md2) best = t.i;
    }
    col_i[j] = best;
  }
  __syncthreads();

  for (int j = tid; j < g.N1; j += kFinT) {
    const int i = col_i[j];
    g.partner1[j] = (i >= 0 && row_j[i] == j) ? (int64_t)i : (int64_t)-1;
  }
  // rows in runs of `per` per thread, so that the scan keeps them ascending
  const int per = (g.N0 + kFinT - 1) / kFinT;
  const int lo = min(tid * per, g.N0), hi = min(lo + per, g.N0);
  int cnt = 0;
  for (int i = lo; i < hi; i++) {
    const int j = row_j[i];
    cnt += (j >= 0 && col_i[j] == i) ? 1 : 0;
  }
  int total;
  int pos = block_excl_sum(cnt, scr, total);
  for (int i = lo; i < hi; i++) {
    const int j = row_j[i];
    const bool m = j >= 0 && col_i[j] == i;
    g.partner0[i] = m ? (int64_t)j : (int64_t)-1;
    if (m) {
      g.matches[2 * pos] = i;
      g.matches[2 * pos + 1] = j;
      g.dist2[pos] = row_d[i];
      pos++;
    }
  }
  const int K = min(g.N0, g.N1);
  for (int p = total + tid; p < K; p += kFinT) {
    g.matches[2 * p] = -1;
    g.matches[2 * p + 1] = -1;
    g.dist2[p] = -1.0f;
  }
  if (tid == 0) g.count[0] = total;
}

}  // namespace match
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_match_workspace_bytes(int N0, int N1) {
  if (N0 < 1 || N1 < 1 || N0 > match::kMaxN || N1 > match::kMaxN) return 0;
  return match::Layout(N0, N1).bytes();
}

DPVO_EXPORT int dpvo_match_descriptors(const void* desc0, const void* desc1, int dtype, int N0,
                                       int N1, int D, int n0, const int32_t* n0_dev, int n1,
                                       const int32_t* n1_dev, float ratio2, float max_dist2,
                                       int64_t* partner0, int64_t* partner1, int64_t* matches,
                                       float* dist2, int32_t* count, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (!desc0 || !desc1 || !partner0 || !partner1 || !matches || !dist2 || !count || !workspace)
    return DPVO_ERR_INVALID;
  if (N0 < 1 || N1 < 1 || D < 4 || (D & 3) != 0) return DPVO_ERR_INVALID;
  if (dtype != DPVO_F32 && dtype != DPVO_F16) return DPVO_ERR_INVALID;
  if ((!n0_dev && (n0 < 0 || n0 > N0)) || (!n1_dev && (n1 < 0 || n1 > N1))) return DPVO_ERR_INVALID;
  if (!(ratio2 >= 0.0f) || !(max_dist2 >= 0.0f)) return DPVO_ERR_INVALID;
  // rows are read as four elements at a time
  const uintptr_t al = dtype == DPVO_F16 ? 7 : 15;
  if (((uintptr_t)desc0 & al) || ((uintptr_t)desc1 & al)) return DPVO_ERR_INVALID;
  if (N0 > match::kMaxN || N1 > match::kMaxN || D > match::kMaxD) return DPVO_ERR_UNSUPPORTED;
  const match::Layout L(N0, N1);
  if (workspace_bytes < L.bytes()) return DPVO_ERR_WORKSPACE;
  match::Args g;
  g.a = desc0;
  g.b = desc1;
  g.n0_dev = n0_dev;
  g.n1_dev = n1_dev;
  g.n0 = n0; g.n1 = n1; g.N0 = N0; g.N1 = N1; g.D = D;
  g.r2 = ratio2;
  g.md2 = max_dist2;
  g.ws = reinterpret_cast<float*>(workspace);
  g.partner0 = partner0;
  g.partner1 = partner1;
  g.matches = matches;
  g.dist2 = dist2;
  g.count = count;
  const dim3 grid((unsigned)L.T1, (unsigned)L.T0);
  if (dtype == DPVO_F16)
    hipLaunchKernelGGL(match::match_tile_kernel<__half>, grid, dim3(match::kThreads), 0,
                       as_stream(stream), g);
  else
    hipLaunchKernelGGL(match::match_tile_kernel<float>, grid, dim3(match::kThreads), 0,
                       as_stream(stream), g);
  const int st = launch_status();
  if (st != DPVO_OK) return st;
  hipLaunchKernelGGL(match::match_finish_kernel, dim3(1), dim3(match::kFinT), 0, as_stream(stream),
                     g);
  return launch_status();
}
