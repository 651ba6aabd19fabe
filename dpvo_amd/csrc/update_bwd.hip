// update_bwd.hip -- backward of DPVO's update operator (update_op.hip) for
// gfx950: the gradients of net, inp, corr and of the 50 parameters from the
// planes that dpvo_update_forward_train kept (update_layout.hpp).
//
// The forward is walked in reverse.  Every linear y = x W^T + b gives up to
// three products, all on v_mfma_f32_16x16x4_f32 (exact fp32 products) through
// one tiled GEMM kernel (64 x 64 output tile, K step 16, operands staged in
// LDS, the next step's global loads in flight during the MFMAs):
//   dx = dy W            [E, 384] . [384, K]
//   dW = dy^T x          reduction over E, cut into chunks of kChunk edges; one
//                        partial per chunk, folded in ascending chunk order in
//                        fp64 by k_fold
//   db = column sums     fp64 per chunk of kColChunk edges, folded in fp64 in a
//                        fixed two-level order by k_fold_cols
// LayerNorm gain / bias gradients and the head gradients are column sums of
// the same kind.  What lies between the linears (LayerNorm, sigmoid gate, ReLU
// masks, group softmax, gathers) is one small kernel each; a row's statistics
// are recomputed from the saved pre-LayerNorm plane with the forward's formula.
//
// Determinism: no float atomics.  Sums over edges use the fixed chunking above
// (it depends on E only); sums over the members of a group, and over the edges
// that gathered one row (the adjoint of x[ix[e]]: plans of ix and jx, built here
// with the forward's plan kernels), run in ascending edge order, one workgroup
// per group.  Two calls on the same state are bit-identical.
//
// agg_*.g.bias: the group softmax is shift-invariant per channel, so this
// gradient is analytically zero; what is returned is what the arithmetic gives
// (rounding noise around 1e-7 of the largest parameter gradient).
#include "common.hpp"
#include "update_layout.hpp"

namespace dpvo {
namespace {

using namespace upd;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kChunk = 512;  // edges per partial of a weight gradient's reduction over E
inline int nchunks(int E) { return (E + kChunk - 1) / kChunk; }
constexpr int kColChunk = 64;  // edges per partial of a column sum
inline int ncolchunks(int E) { return (E + kColChunk - 1) / kColChunk; }
constexpr int kHeadPart = 4 * kD + 4;  // d.W, w.W rows, then d.b, w.b

// --- GEMM -------------------------------------------------------------------------
// C[z] (+)= A(:, kz) . B(kz, :) with kz = [z kchunk, min(K, (z + 1) kchunk)),
// z = blockIdx.z, C[z] = C + z cstride.  B is [K, N] row-major.  A is [M, K]
// row-major, or with TA [K, M] row-major (the reduction runs over A's rows).
// Lane maps of the MFMA (lane = 16 q + r): A[row r][k = q], B[k = q][col r],
// D[row 4 q + i][col r].  256 threads; wave w owns the 32 x 32 quadrant
// (w & 1, w >> 1) of the tile as 2 x 2 MFMA tiles.
constexpr int BM = 64, BN = 64, BK = 16, LP = 68;

template <bool TA>
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ A, int lda,
                                              const float* __restrict__ B, int ldb, float* C,
                                              int ldc, int M, int N, int K, int kchunk,
                                              size_t cstride, int accumulate) {
  __shared__ __align__(16) float As[BK * LP];
  __shared__ __align__(16) float Bs[BK * LP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int kb = blockIdx.z * kchunk, ke = min(K, kb + kchunk);
  C += (size_t)blockIdx.z * cstride;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const bool va = (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  const bool vb = (ldb & 3) == 0 && (reinterpret_cast<uintptr_t>(B) & 15) == 0;
  // this thread's four A and four B elements of a K step
  const int ar = TA ? tid / 16 : tid / 4, ac = TA ? (tid % 16) * 4 : (tid % 4) * 4;
  const int br = tid / 16, bc = (tid % 16) * 4;
  float ra[4], rb[4];
  auto load = [&](int k0) {
    if (TA) {  // A[k0 + ar][m0 + ac ..]
      const int gk = k0 + ar, gm = m0 + ac;
      if (va && gk < ke && gm + 3 < M) {
        const float4 v = *reinterpret_cast<const float4*>(A + (size_t)gk * lda + gm);
        ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          ra[j] = gk < ke && gm + j < M ? A[(size_t)gk * lda + gm + j] : 0.f;
      }
    } else {  // A[m0 + ar][k0 + ac ..]
      const int gm = m0 + ar, gk = k0 + ac;
      if (va && gm < M && gk + 3 < ke) {
        const float4 v = *reinterpret_cast<const float4*>(A + (size_t)gm * lda + gk);
        ra[0] = v.x; ra[1] = v.y; ra[2] = v.z; ra[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          ra[j] = gm < M && gk + j < ke ? A[(size_t)gm * lda + gk + j] : 0.f;
      }
    }
    const int gk = k0 + br, gn = n0 + bc;
    if (vb && gk < ke && gn + 3 < N) {
      const float4 v = *reinterpret_cast<const float4*>(B + (size_t)gk * ldb + gn);
      rb[0] = v.x; rb[1] = v.y; rb[2] = v.z; rb[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        rb[j] = gk < ke && gn + j < N ? B[(size_t)gk * ldb + gn + j] : 0.f;
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(kb);
  for (int k0 = kb; k0 < ke; k0 += BK) {
    if (TA) {
      *reinterpret_cast<float4*>(&As[ar * LP + ac]) = float4{ra[0], ra[1], ra[2], ra[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) As[(ac + j) * LP + ar] = ra[j];
    }
    *reinterpret_cast<float4*>(&Bs[br * LP + bc]) = float4{rb[0], rb[1], rb[2], rb[3]};
    __syncthreads();
    if (k0 + BK < ke) load(k0 + BK);
#pragma unroll
    for (int ks = 0; ks < BK / 4; ks++) {
      const float a0 = As[(4 * ks + q) * LP + wm + r], a1 = As[(4 * ks + q) * LP + wm + 16 + r];
      const float b0 = Bs[(4 * ks + q) * LP + wn + r], b1 = Bs[(4 * ks + q) * LP + wn + 16 + r];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int row = m0 + wm + i * 16 + 4 * q + v, col = n0 + wn + j * 16 + r;
        if (row < M && col < N) {
          float* c = C + (size_t)row * ldc + col;
          *c = accumulate ? *c + acc[i][j][v] : acc[i][j][v];
        }
      }
}

// dst[i] = sum over z, ascending, of part[z zstride + i], in fp64
__global__ __launch_bounds__(256) void k_fold(const float* __restrict__ part, int nz, size_t zstride,
                                              size_t n, float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int z = 0; z < nz; z++) s += (double)part[(size_t)z * zstride + i];
  dst[i] = (float)s;
}

// The same sum for few outputs and many partials (the column sums: n = 384,
// one partial per kColChunk edges), where a thread per output would walk a
// long chain alone: a workgroup owns 16 outputs, thread (zl, c) adds the
// partials z = zl, zl + 16, ... of output c in ascending order, and thread
// (0, c) adds the 16 sub-sums in ascending zl.  The order depends on nz only.
__global__ __launch_bounds__(256) void k_fold_cols(const float* __restrict__ part, int nz,
                                                   size_t zstride, int n, float* __restrict__ dst) {
  __shared__ double sub[16][17];
  const int c = threadIdx.x & 15, zl = threadIdx.x >> 4, i = blockIdx.x * 16 + c;
  double s = 0.0;
  if (i < n) {
#pragma unroll 4
    for (int z = zl; z < nz; z += 16) s += (double)part[(size_t)z * zstride + i];
  }
  sub[zl][c] = s;
  __syncthreads();
  if (zl == 0 && i < n) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 16; k++) t += sub[k][c];
    dst[i] = (float)t;
  }
}

// part[z][c] = sum of src[e][c] over the edges of chunk z, ascending, in fp64
__global__ __launch_bounds__(kD) void k_colsum_part(const float* __restrict__ src, int E,
                                                    float* __restrict__ part) {
  const int c = threadIdx.x, e0 = blockIdx.x * kColChunk, e1 = min(E, e0 + kColChunk);
  double s = 0.0;
#pragma unroll 8
  for (int e = e0; e < e1; e++) s += (double)src[(size_t)e * kD + c];
  part[(size_t)blockIdx.x * kD + c] = (float)s;
}

// --- the heads -----------------------------------------------------------------------
// d = Wd relu(x) + b, w = sigmoid(Ww relu(x) + b).  The cotangent of the two
// pre-activations of edge e: (g_d, g_w w (1 - w)); a null cotangent is zero.
__device__ __forceinline__ void head_cot(const float* __restrict__ g_d, const float* __restrict__ g_w,
                                         const float* __restrict__ w, size_t e, float (&z)[4]) {
  z[0] = g_d ? g_d[2 * e] : 0.f;
  z[1] = g_d ? g_d[2 * e + 1] : 0.f;
  const float w0 = w[2 * e], w1 = w[2 * e + 1];
  z[2] = (g_w ? g_w[2 * e] : 0.f) * (w0 * (1.f - w0));
  z[3] = (g_w ? g_w[2 * e + 1] : 0.f) * (w1 * (1.f - w1));
}
// gx = g_net_out + (x6 > 0) (z . [Wd; Ww])
__global__ __launch_bounds__(kD) void k_heads(const float* __restrict__ x6, const float* __restrict__ w,
                                              const float* __restrict__ g_net,
                                              const float* __restrict__ g_d,
                                              const float* __restrict__ g_w,
                                              const float* __restrict__ Wd,
                                              const float* __restrict__ Ww, float* __restrict__ gx) {
  const size_t e = blockIdx.x;
  const int c = threadIdx.x;
  float z[4];
  head_cot(g_d, g_w, w, e, z);
  const float v = z[0] * Wd[c] + z[1] * Wd[kD + c] + z[2] * Ww[c] + z[3] * Ww[kD + c];
  const size_t i = e * kD + c;
  gx[i] = (g_net ? g_net[i] : 0.f) + (x6[i] > 0.f ? v : 0.f);
}
// part[z]: [4][384] sums of z_o relu(x6) over chunk z, then the four sums of z_o
__global__ __launch_bounds__(kD) void k_heads_part(const float* __restrict__ x6,
                                                   const float* __restrict__ w,
                                                   const float* __restrict__ g_d,
                                                   const float* __restrict__ g_w, int E,
                                                   float* __restrict__ part) {
  const int c = threadIdx.x, e0 = blockIdx.x * kColChunk, e1 = min(E, e0 + kColChunk);
  double s[4] = {0.0, 0.0, 0.0, 0.0}, sb = 0.0;
  for (int e = e0; e < e1; e++) {
    float z[4];
    head_cot(g_d, g_w, w, (size_t)e, z);
    const float a = fmaxf(x6[(size_t)e * kD + c], 0.f);
#pragma unroll
    for (int o = 0; o < 4; o++) s[o] += (double)(z[o] * a);
    if (c < 4) sb += (double)(c == 0 ? z[0] : c == 1 ? z[1] : c == 2 ? z[2] : z[3]);
  }
  float* p = part + (size_t)blockIdx.x * kHeadPart;
#pragma unroll
  for (int o = 0; o < 4; o++) p[o * kD + c] = (float)s[o];
  if (c < 4) p[4 * kD + c] = (float)sb;
}

// --- between the linears -----------------------------------------------------------------
// GatedResidual x' = x + s r: gr = gx s, gg = gx r s (1 - s) (the gate's pre-activation)
__global__ __launch_bounds__(256) void k_gru_ew(const float* __restrict__ gx, const float* __restrict__ s,
                                                const float* __restrict__ r, size_t n,
                                                float* __restrict__ gr, float* __restrict__ gg) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float g = gx[i], sv = s[i];
  gr[i] = g * sv;
  gg[i] = g * r[i] * (sv * (1.f - sv));
}
// g *= (a > 0)
__global__ __launch_bounds__(256) void k_mask(float* __restrict__ g, const float* __restrict__ a,
                                              size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && !(a[i] > 0.f)) g[i] = 0.f;
}
__global__ __launch_bounds__(256) void k_copy(const float* __restrict__ src, float* __restrict__ dst,
                                              size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}
// out[e] = x[idx[e]], zeros where the index is outside [0, E)
__global__ __launch_bounds__(kD) void k_gather(const float* __restrict__ x,
                                               const int64_t* __restrict__ idx, int E,
                                               float* __restrict__ out) {
  const size_t e = blockIdx.x;
  const int64_t s = idx[e];
  const bool ok = s >= 0 && s < E;
  out[e * kD + threadIdx.x] = ok ? x[(size_t)s * kD + threadIdx.x] : 0.f;
}

// LayerNorm statistics of one row by one wave, the forward's formula
// (update_op.hip layer_norm): v <- x - mean, returns rstd
__device__ __forceinline__ float ln_stats(const float* __restrict__ x, int lane, float (&v)[6]) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    v[i] = x[lane + 64 * i];
    s += v[i];
  }
  const float mean = wave_sum(s) * (1.0f / kD);
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    v[i] -= mean;
    ss += v[i] * v[i];
  }
  return 1.0f / sqrtf(wave_sum(ss) * (1.0f / kD) + kEps);
}
// out = LN(x) (gain gb[0..384), bias gb[384..768) given separately); a wave per row
__global__ __launch_bounds__(512) void k_ln_fwd(const float* __restrict__ x,
                                                const float* __restrict__ gain,
                                                const float* __restrict__ bias, int E,
                                                float* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (row >= E) return;
  float v[6];
  const float rstd = ln_stats(x + (size_t)row * kD, lane, v);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int c = lane + 64 * i;
    out[(size_t)row * kD + c] = v[i] * rstd * gain[c] + bias[c];
  }
}
// y = xhat gain + bias: gx (+)= rstd (gh - mean(gh) - xhat mean(gh xhat)) with
// gh = gy gain; prod = gy xhat (its column sums are the gain's gradient)
__global__ __launch_bounds__(512) void k_ln_bwd(const float* __restrict__ gy,
                                                const float* __restrict__ x,
                                                const float* __restrict__ gain, int E, float* gx,
                                                int accumulate, float* __restrict__ prod) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 8 + (threadIdx.x >> 6);
  if (row >= E) return;
  float v[6], gh[6];
  const float rstd = ln_stats(x + (size_t)row * kD, lane, v);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const int c = lane + 64 * i;
    const float g = gy[(size_t)row * kD + c];
    v[i] *= rstd;  // xhat
    gh[i] = g * gain[c];
    s1 += gh[i];
    s2 += gh[i] * v[i];
    prod[(size_t)row * kD + c] = g * v[i];
  }
  const float m1 = wave_sum(s1) * (1.0f / kD), m2 = wave_sum(s2) * (1.0f / kD);
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const size_t o = (size_t)row * kD + lane + 64 * i;
    const float d = rstd * (gh[i] - m1 - v[i] * m2);
    gx[o] = accumulate ? gx[o] + d : d;
  }
}

// --- groups ---------------------------------------------------------------------------------
// out[g] = sum of gx over the members of group g, ascending; zero rows past the
// group count.  One workgroup per group, a thread per channel.
__global__ __launch_bounds__(kD) void k_group_sum(const float* __restrict__ gx, Plan p, int E,
                                                  float* __restrict__ out) {
  const int g = blockIdx.x, c = threadIdx.x;
  double s = 0.0;
  if (g < plan_count(p.off, E))
    for (int i = p.off[g], e = p.off[g + 1]; i < e; i++) s += (double)gx[(size_t)p.members[i] * kD + c];
  out[(size_t)g * kD + c] = (float)s;
}
// Y = sum_m p_m F_m with p = softmax over the group's members of G (k_agg):
// gF_m = p_m gY, gG_m = p_m (F_m - Y) gY.  p is recomputed the forward's way.
__global__ __launch_bounds__(kD) void k_agg_bwd(const float* __restrict__ F, const float* __restrict__ Gv,
                                                const float* __restrict__ Y,
                                                const float* __restrict__ gY, Plan p, int E,
                                                float* __restrict__ gF, float* __restrict__ gG) {
  const int g = blockIdx.x;
  if (g >= plan_count(p.off, E)) return;
  const int c = threadIdx.x, b = p.off[g], e = p.off[g + 1];
  float m = -INFINITY;
  for (int i = b; i < e; i++) m = fmaxf(m, Gv[(size_t)p.members[i] * kD + c]);
  float s = 0.f;
  for (int i = b; i < e; i++) s += expf(Gv[(size_t)p.members[i] * kD + c] - m);
  const float y = Y[(size_t)g * kD + c], gy = gY[(size_t)g * kD + c];
  for (int i = b; i < e; i++) {
    const size_t o = (size_t)p.members[i] * kD + c;
    const float pm = expf(Gv[o] - m) / s;
    gF[o] = pm * gy;
    gG[o] = pm * (F[o] - y) * gy;
  }
}
// the gather's adjoint: gx[r] += sum of gu over the edges e with idx[e] = r,
// ascending (p groups the edges by idx; a group whose index is outside [0, E)
// contributes nothing).  Groups have distinct rows: no two workgroups meet.
__global__ __launch_bounds__(kD) void k_scatter_add(float* gx, const float* __restrict__ gu,
                                                    const int64_t* __restrict__ idx, Plan p, int E) {
  const int g = blockIdx.x;
  if (g >= plan_count(p.off, E)) return;
  const int c = threadIdx.x, b = p.off[g], e = p.off[g + 1];
  const int64_t r = idx[p.members[b]];
  if (r < 0 || r >= E) return;
  double s = 0.0;
  for (int i = b; i < e; i++) s += (double)gu[(size_t)p.members[i] * kD + c];
  gx[(size_t)r * kD + c] += (float)s;
}

// --- host -------------------------------------------------------------------------------------
// workspace: six [E, 384] planes, the GEMM partials, the column-sum partials,
// the plans of ix and jx
struct Bws {
  float *A, *B, *C, *D, *N, *F, *part, *cpart;
  Plan plan[2];
};
inline size_t part_bytes(int E, int K0) {
  return r256((size_t)nchunks(E) * kD * (size_t)(K0 > kD ? K0 : kD) * 4);
}
inline size_t cpart_bytes(int E) { return r256((size_t)ncolchunks(E) * kHeadPart * 4); }
inline size_t bws_bytes(int E, int K0) {
  return 6 * rows_bytes(E) + part_bytes(E, K0) + cpart_bytes(E) + 12 * ints_bytes(E);
}
inline Bws bws_carve(void* base, int E, int K0) {
  char* p = (char*)base;
  Bws w;
  float** f[6] = {&w.A, &w.B, &w.C, &w.D, &w.N, &w.F};
  for (auto q : f) { *q = (float*)p; p += rows_bytes(E); }
  w.part = (float*)p; p += part_bytes(E, K0);
  w.cpart = (float*)p; p += cpart_bytes(E);
  carve_plans(p, E, w.plan);
  return w;
}

struct Run {
  int E;
  hipStream_t st;
  const float* const* P;  // parameters
  float* const* G;        // their gradients, or null
  Bws w;
  unsigned eblocks() const { return (unsigned)(((size_t)E * kD + 255) / 256); }
  void fold(const float* part, int nz, size_t zstride, size_t n, float* dst) const {
    hipLaunchKernelGGL(k_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, nz, zstride,
                       n, dst);
  }
  void fold_cols(const float* part, int nz, size_t zstride, int n, float* dst) const {
    hipLaunchKernelGGL(k_fold_cols, dim3((n + 15) / 16), dim3(256), 0, st, part, nz, zstride, n, dst);
  }
  void colsum(const float* src, float* dst) const {
    hipLaunchKernelGGL(k_colsum_part, dim3(ncolchunks(E)), dim3(kD), 0, st, src, E, w.cpart);
    fold_cols(w.cpart, ncolchunks(E), kD, kD, dst);
  }
  // the linear of tensor t (weight [384, K], bias): dx (+)= dy W when dx is
  // given; its weight and bias gradients when parameter gradients are wanted
  void linear(int t, int K, const float* dy, const float* x, float* dx, bool acc) const {
    if (dx)
      hipLaunchKernelGGL(k_gemm<false>, dim3((K + BN - 1) / BN, (E + BM - 1) / BM, 1), dim3(256), 0,
                         st, dy, kD, P[t], K, dx, K, E, K, kD, kD, (size_t)0, acc ? 1 : 0);
    if (!G) return;
    const int nz = nchunks(E);
    hipLaunchKernelGGL(k_gemm<true>, dim3((K + BN - 1) / BN, kD / BM, nz), dim3(256), 0, st, dy, kD,
                       x, K, w.part, K, kD, K, E, kChunk, (size_t)kD * K, 0);
    fold(w.part, nz, (size_t)kD * K, (size_t)kD * K, G[t]);
    colsum(dy, G[t + 1]);
  }
  void mask(float* g, const float* a) const {
    hipLaunchKernelGGL(k_mask, dim3(eblocks()), dim3(256), 0, st, g, a, (size_t)E * kD);
  }
  // LayerNorm of tensor t: gx (+)= through the norm, gain / bias gradients
  void ln_bwd(int t, const float* gy, const float* xpre, float* gx, bool acc, float* prod) const {
    hipLaunchKernelGGL(k_ln_bwd, dim3((E + 7) / 8), dim3(512), 0, st, gy, xpre, P[t], E, gx,
                       acc ? 1 : 0, prod);
    if (!G) return;
    colsum(prod, G[t]);
    colsum(gy, G[t + 1]);
  }
};

}  // namespace
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_update_backward_workspace_bytes(int E, int K0) {
  if (E < 1 || K0 < 1) return 0;
  return bws_bytes(E, K0);
}

DPVO_EXPORT int dpvo_update_backward(const float* const* params, int dim, int K0, const void* saved,
                                     size_t saved_size, const int64_t* ix, const int64_t* jx, int E,
                                     const float* g_net_out, const float* g_d, const float* g_w,
                                     float* g_net, float* g_inp, float* g_corr, float* const* grads,
                                     void* workspace, size_t workspace_size, void* stream) {
  if (dim != kD || E > 65535 * BM) return DPVO_ERR_UNSUPPORTED;  // the GEMM's grid
  if (K0 < 1) return DPVO_ERR_INVALID;
  if (E <= 0) return DPVO_OK;
  if (!params || !saved || !ix || !jx || !workspace) return DPVO_ERR_INVALID;
  for (int i = 0; i < kTensors; i++)
    if (!params[i] || (grads && !grads[i])) return DPVO_ERR_INVALID;
  if (saved_size < saved_bytes(E, K0) || workspace_size < bws_bytes(E, K0))
    return DPVO_ERR_WORKSPACE;
  const Saved sv = saved_carve(const_cast<void*>(saved), E, K0);
  const Run R{E, as_stream(stream), params, grads, bws_carve(workspace, E, K0)};
  const Bws& w = R.w;
  hipStream_t st = R.st;
  const float* const* P = params;
  const size_t n = (size_t)E * kD;
  auto pl = [&](int i) { return (const float*)sv.pl[i]; };

  launch_plans(ix, jx, E, w.plan[0], w.plan[1], st);

  // heads: A = the cotangent of x6
  hipLaunchKernelGGL(k_heads, dim3(E), dim3(kD), 0, st, pl(P_X6), (const float*)sv.w, g_net_out, g_d,
                     g_w, P[T_D], P[T_W], w.A);
  if (grads) {
    const int nz = ncolchunks(E);
    hipLaunchKernelGGL(k_heads_part, dim3(nz), dim3(kD), 0, st, pl(P_X6), (const float*)sv.w, g_d,
                       g_w, E, w.cpart);
    R.fold_cols(w.cpart, nz, kHeadPart, 2 * kD, grads[T_D]);
    R.fold_cols(w.cpart + 2 * kD, nz, kHeadPart, 2 * kD, grads[T_W]);
    R.fold_cols(w.cpart + 4 * kD, nz, kHeadPart, 2, grads[T_D + 1]);
    R.fold_cols(w.cpart + 4 * kD + 2, nz, kHeadPart, 2, grads[T_W + 1]);
  }

  // x' = n + sigmoid(gate n) res(n) with n = LN(x), twice, the second first;
  // gA holds the running cotangent of the residual stream
  float *gA = w.A, *gF = w.F;
  for (int blk = 1; blk >= 0; blk--) {
    const int ps = blk ? P_S2 : P_S1, tln = blk ? T_GRU2 : T_GRU0, tg = blk ? T_G3GATE : T_G1GATE;
    const float *S = pl(ps), *Aa = pl(ps + 1), *Rr = pl(ps + 2), *Xpre = pl(blk ? P_X5 : P_X4);
    hipLaunchKernelGGL(k_gru_ew, dim3(R.eblocks()), dim3(256), 0, st, (const float*)gA, S, Rr, n,
                       w.B, w.C);
    hipLaunchKernelGGL(k_ln_fwd, dim3((E + 7) / 8), dim3(512), 0, st, Xpre, P[tln], P[tln + 1], E,
                       w.N);
    R.linear(tg + 4, kD, w.B, Aa, w.D, false);  // res.2
    R.mask(w.D, Aa);
    R.linear(tg + 2, kD, w.D, w.N, gA, true);  // res.0: gA becomes the cotangent of n
    R.linear(tg, kD, w.C, w.N, gA, true);      // gate.0
    R.ln_bwd(tln, gA, Xpre, gF, false, w.B);
    float* t = gA;
    gA = gF;
    gF = t;
  }

  // the two soft-aggregations, ij first: x_out = x + h(Y)[group]
  for (int a = 1; a >= 0; a--) {
    const int tf = a ? T_IJF : T_KKF;
    const float *Fs = pl(a ? P_FIJ : P_FKK), *Gs = pl(a ? P_GIJ : P_GKK), *Y = pl(a ? P_YIJ : P_YKK);
    const float* Xin = pl(a ? P_X3 : P_X2);
    hipLaunchKernelGGL(k_group_sum, dim3(E), dim3(kD), 0, st, (const float*)gA, sv.plan[a], E, w.B);
    R.linear(tf + 4, kD, w.B, Y, w.C, false);  // h on the group rows
    hipLaunchKernelGGL(k_agg_bwd, dim3(E), dim3(kD), 0, st, Fs, Gs, Y, (const float*)w.C, sv.plan[a],
                       E, w.D, gF);
    R.linear(tf, kD, w.D, Xin, gA, true);
    R.linear(tf + 2, kD, gF, Xin, gA, true);
  }

  // c2 then c1: x_out = x + c.2(relu(c.0(m x[idx])))
  for (int c = 1; c >= 0; c--) {
    const int ta = c ? T_C2A : T_C1A;
    const float *Aa = pl(c ? P_A2 : P_A1), *Xs = pl(c ? P_X1 : P_X0);
    const int64_t* idx = c ? jx : ix;
    R.linear(ta + 2, kD, gA, Aa, w.B, false);
    R.mask(w.B, Aa);
    hipLaunchKernelGGL(k_gather, dim3(E), dim3(kD), 0, st, Xs, idx, E, w.C);
    R.linear(ta, kD, w.B, w.C, w.D, false);
    hipLaunchKernelGGL(k_scatter_add, dim3(E), dim3(kD), 0, st, gA, (const float*)w.D, idx,
                       w.plan[c], E);
  }

  // x0 = LN(net + inp + corr MLP)
  R.ln_bwd(T_NORM, gA, pl(P_S0), w.B, false, w.C);
  if (g_net) hipLaunchKernelGGL(k_copy, dim3(R.eblocks()), dim3(256), 0, st, (const float*)w.B, g_net, n);
  if (g_inp) hipLaunchKernelGGL(k_copy, dim3(R.eblocks()), dim3(256), 0, st, (const float*)w.B, g_inp, n);
  if (grads || g_corr) {
    R.linear(T_CORR5, kD, w.B, pl(P_A3), w.C, false);
    R.mask(w.C, pl(P_A3));
    R.ln_bwd(T_CORR3, w.C, pl(P_Z2), w.D, false, gF);
    R.linear(T_CORR2, kD, w.D, pl(P_A0), w.C, false);
    R.mask(w.C, pl(P_A0));
    R.linear(T_CORR0, K0, w.C, (const float*)sv.corr, g_corr, false);
  }
  return launch_status();
}
