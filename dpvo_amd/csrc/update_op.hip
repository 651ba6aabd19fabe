// update_op.hip -- DPVO's update operator (dpvo/net.py:175-339, `Update`) as
// fused gfx950 kernels on the matrix cores: the inference forward, the training
// forward (the same launches, every plane the backward needs kept in `saved`,
// update_layout.hpp) and the device pack.  The backward is update_bwd.hip.
//
// The operator is a residual stream x [E, 384] pushed through 19 linears of
// width 384 (the first reads corr [E, K0]), four LayerNorms, two neighbour
// gathers and two group soft-aggregations.  Rows depend on other rows only at
// the gathers and at the group reductions, so the work is cut there:
//
//   k_corr   corr MLP, + net + inp, LayerNorm                      -> xA
//   k_nbr    x + c1(m * x[ix])                       reads xA      -> xB
//   k_nbr    x + c2(m * x[jx]); f_kk(x), g_kk(x)     reads xB      -> xA, F, G
//   k_agg    per kk group: softmax_group(G) . F (ascending edges)  -> Y
//   k_h      h_kk on the dense group rows                          -> HY
//   k_addfg  x + HY[group]; f_ij(x), g_ij(x)                       -> xA, F, G
//   k_agg, k_h  (ij groups)
//   k_final  x + HY[group]; (LN, GatedResidual) x 2; d, w heads    -> net_out, d, w
//
// Inside a launch a workgroup owns T = 16 MT rows: their fp32 residual stream
// sits in LDS (X) across all of the launch's layers, next to one operand tile
// (tmp, in the weight type).  One GEMM core, templated on the weight type:
//   __half : v_mfma_f32_16x16x32_f16, activations rounded to fp16 (RNE) only
//            as MFMA operands, fp32 accumulation
//   float  : v_mfma_f32_16x16x4_f32, exact fp32 products
// Bias, LayerNorm, ReLU / sigmoid, softmax and residual adds are fp32.
//
// Lane maps (lane = 16 q + r): A[row r][k], B[k][col r], D[row 4 q + i][col r].
// The K elements of one MFMA may be assigned to (q, j) in any way as long as A
// and B agree, so both operands take the contiguous run k = KQ q + j of their
// K step (KQ = 8 halves / 4 floats = 16 B): one 16-B load each.
//
// Packed blob (host, dpvo_update_pack_weights; all offsets in bytes):
//   [0, 256)   header: int32 magic 'UPD1', wdtype, K0, K0pad (K0 rounded up to 128)
//   weights    layer 0 [384 x K0pad], layers 1..18 [384 x 384], element
//              (n, k) of a layer with KS = K / KK steps at 16-B unit
//              ((n / 16) KS + k / KK) 64 + 16 ((k % KK) / KQ) + n % 16, slot k % KQ
//              (KK = 32 halves or 16 floats).  The K tail of layer 0 is zero.
//   vectors    fp32: bias[19][384], ln[4][gain, bias][384], d.W[2][384],
//              w.W[2][384], d.b[2], w.b[2]  (head weights fp16-rounded when the
//              weights are fp16)
#include <string.h>

#include "common.hpp"
#include "update_layout.hpp"

namespace dpvo {
namespace {

using upd::kD;
using upd::kEps;
using upd::Plan;
using upd::plan_count;
using upd::rows_bytes;
using upd::ints_bytes;
constexpr int kThreads = 512, kWaves = 8, kNT = 3;  // a wave owns 48 output columns
constexpr int kXP = 388;                            // fp32 LDS row pitch (floats)
constexpr int kLayers = 19, kLN = 4;
constexpr int kHdr = 256;
constexpr int kUpdateBigTileE = 4096;  // E from which the 32-row tile is used

// GEMM layers and LayerNorms, blob order
enum { L_CORR0 = 0, L_CORR2, L_CORR5, L_C1A, L_C1B, L_C2A, L_C2B, L_KKF, L_KKG, L_KKH, L_IJF,
       L_IJG, L_IJH, L_G1GATE, L_G1RES0, L_G1RES2, L_G3GATE, L_G3RES0, L_G3RES2 };
enum { N_NORM = 0, N_CORR3, N_GRU0, N_GRU2 };

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// K0 up to a multiple of 128: four K steps of either weight type
inline int k0pad(int K0) { return (K0 + 127) & ~127; }
inline size_t esize(int wdtype) { return wdtype == DPVO_F16 ? 2 : 4; }
inline size_t w_off(int layer, int K0p, size_t es) {
  return kHdr + (layer == 0 ? 0 : es * kD * ((size_t)K0p + (size_t)(layer - 1) * kD));
}
inline size_t v_off(int K0p, size_t es) { return w_off(kLayers, K0p, es); }
constexpr size_t kVecFloats = (size_t)kLayers * kD + kLN * 2 * kD + 4 * kD + 4;
inline size_t blob_bytes(int K0, int wdtype) {
  return (v_off(k0pad(K0), esize(wdtype)) + kVecFloats * 4 + 255) & ~(size_t)255;
}

// vectors section, float offsets
constexpr int V_BIAS = 0, V_LN = kLayers * kD, V_DW = V_LN + kLN * 2 * kD, V_WW = V_DW + 2 * kD,
              V_DB = V_WW + 2 * kD, V_WB = V_DB + 2;

// --- workspace -----------------------------------------------------------------
// six [E, 384] fp32 arrays, then per grouping (kk, ij) six int arrays of E + 1
struct Ws {
  float *xA, *xB, *F, *G, *Y, *HY;
  Plan p[2];
};
inline size_t ws_bytes(int E) { return 6 * rows_bytes(E) + 12 * ints_bytes(E); }
inline Ws ws_carve(void* base, int E) {
  char* p = (char*)base;
  Ws w;
  float** f[6] = {&w.xA, &w.xB, &w.F, &w.G, &w.Y, &w.HY};
  for (auto q : f) { *q = (float*)p; p += rows_bytes(E); }
  upd::carve_plans(p, E, w.p);
  return w;
}
// the group count of a plan lives on the device at off[E + 1] (plan_count)

// --- group plan ------------------------------------------------------------------
// rep[e]: smallest edge with e's id; pos[e]: how many smaller edges share it.
// Block (x, y) compares the 256 edges of tile x with the kPlanChunk edges of
// chunk y and folds its partial result in with integer atomics (min / add:
// order-independent, so the plan is deterministic).
constexpr int kPlanChunk = 1024;
__global__ __launch_bounds__(256) void k_plan_init(int E, Plan p0, Plan p1) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < E) {
    p0.rep[e] = p1.rep[e] = e;
    p0.pos[e] = p1.pos[e] = 0;
  }
}
__global__ __launch_bounds__(256) void k_plan_rank(const int64_t* __restrict__ gk,
                                                   const int64_t* __restrict__ gij, int E,
                                                   Plan p0, Plan p1) {
  __shared__ int64_t tile[kPlanChunk];
  const int j0 = blockIdx.y * kPlanChunk;
  if (j0 >= (int)(blockIdx.x + 1) * 256) return;  // only smaller edges count
  const int64_t* ids = blockIdx.z ? gij : gk;
  const Plan p = blockIdx.z ? p1 : p0;
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int64_t my = e < E ? ids[e] : 0;
  for (int j = threadIdx.x; j < kPlanChunk; j += 256) tile[j] = j0 + j < E ? ids[j0 + j] : 0;
  __syncthreads();
  const int lim = min(kPlanChunk, min(E, e) - j0);
  int rep = -1, cnt = 0;
  for (int j = 0; j < lim; j++)
    if (tile[j] == my) {
      if (rep < 0) rep = j0 + j;
      cnt++;
    }
  if (e < E && cnt) {
    atomicMin(&p.rep[e], rep);
    atomicAdd(&p.pos[e], cnt);
  }
}

// exclusive scan of v(i), i < n, by one workgroup of 1024; returns the total
template <typename V, typename S>
__device__ int block_scan(int n, int* sh, V v, S store) {
  const int t = threadIdx.x, chunk = (n + 1023) / 1024;
  const int b = min(n, t * chunk), e = min(n, b + chunk);
  int s = 0;
  for (int i = b; i < e; i++) s += v(i);
  sh[t] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int add = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int total = sh[1023];
  int run = sh[t] - s;
  __syncthreads();
  for (int i = b; i < e; i++) {
    const int x = v(i);
    store(i, run);
    run += x;
  }
  __syncthreads();
  return total;
}

// dense group index (groups numbered by smallest member), CSR member lists in
// ascending edge order, group count at off[E + 1].  One workgroup per grouping.
__global__ __launch_bounds__(1024) void k_plan_build(int E, Plan p0, Plan p1) {
  __shared__ int sh[1024];
  const Plan p = blockIdx.x ? p1 : p0;
  const int t = threadIdx.x;
  const int G = block_scan(E, sh, [&](int i) { return p.rep[i] == i ? 1 : 0; },
                           [&](int i, int x) { if (p.rep[i] == i) p.dense[i] = x; });
  for (int i = t; i < E; i += 1024)
    if (p.rep[i] != i) p.dense[i] = p.dense[p.rep[i]];  // reads representatives only
  for (int i = t; i < G; i += 1024) p.size[i] = 0;
  __syncthreads();
  for (int i = t; i < E; i += 1024) atomicMax(&p.size[p.dense[i]], p.pos[i] + 1);
  __syncthreads();
  block_scan(G, sh, [&](int i) { return p.size[i]; }, [&](int i, int x) { p.off[i] = x; });
  if (t == 0) {
    p.off[G] = E;
    p.off[E + 1] = G;
  }
  __syncthreads();
  for (int i = t; i < E; i += 1024) p.members[p.off[p.dense[i]] + p.pos[i]] = i;
}

// --- group soft-aggregation --------------------------------------------------------
// Y[g][c] = sum_m softmax_m(G[m][c]) F[m][c] over the members m of group g in
// ascending edge order, with the per-(group, channel) maximum subtracted
// (torch_scatter.scatter_softmax).  One workgroup per group, a thread per channel.
// TRAIN: the rows of Y past the group count are zeroed (the backward's GEMMs
// read all E rows).
template <bool TRAIN>
__global__ __launch_bounds__(kD) void k_agg(const float* __restrict__ F, const float* __restrict__ Gv,
                                            Plan p, int E, float* __restrict__ Y) {
  const int g = blockIdx.x;
  if (g >= plan_count(p.off, E)) {
    if constexpr (TRAIN) Y[(size_t)g * kD + threadIdx.x] = 0.f;
    return;
  }
  const int c = threadIdx.x, b = p.off[g], e = p.off[g + 1];
  float m = -INFINITY;
  for (int i = b; i < e; i++) m = fmaxf(m, Gv[(size_t)p.members[i] * kD + c]);
  float s = 0.f, acc = 0.f;
  for (int i = b; i < e; i++) {
    const size_t o = (size_t)p.members[i] * kD + c;
    const float w = expf(Gv[o] - m);
    s += w;
    acc += w * F[o];
  }
  Y[(size_t)g * kD + c] = acc / s;
}

// --- the row-tile machinery -----------------------------------------------------------
template <typename WT>
struct WTraits;
template <>
struct WTraits<__half> {
  static constexpr int KK = 32, KQ = 8, TP = 392;  // K per step, per lane; tmp pitch
};
template <>
struct WTraits<float> {
  static constexpr int KK = 16, KQ = 4, TP = 388;
};

template <typename WT, int MT>
constexpr size_t lds_bytes() {
  return (size_t)16 * MT * (kXP * 4 + WTraits<WT>::TP * sizeof(WT));
}

__device__ __forceinline__ float to_w(float v, float) { return v; }
__device__ __forceinline__ __half to_w(float v, __half) { return __float2half_rn(v); }
// the value an operand of weight type WT carries, back in fp32
template <typename WT>
__device__ __forceinline__ float operand_round(float v) {
  if constexpr (sizeof(WT) == 2) return __half2float(__float2half_rn(v));
  else return v;
}

template <int MT>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[MT][kNT]) {
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < kNT; n++) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// acc += A[16 MT rows, nks K steps] . W^T for this wave's 48 columns.  A is an
// LDS tile (float: X, converted per operand; WT: tmp), W the layer's packed
// weights, ks0 the first K step of W to use, KS the layer's K steps.
template <typename WT, int MT, typename AT>
__device__ __forceinline__ void gemm(f32x4 (&acc)[MT][kNT], const AT* A, int pitch, int nks,
                                     const uint4* __restrict__ W, int KS, int ks0) {
  constexpr int KK = WTraits<WT>::KK, KQ = WTraits<WT>::KQ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const uint4* Wl = W + ((size_t)(wave * kNT) * KS + ks0) * 64 + lane;
  // ring of kPF K steps of B in flight: a step's loads are issued kPF steps
  // ahead (a single step ahead leaves every step waiting a full L2 round trip).
  // nks is a multiple of kPF.
  constexpr int kPF = 4;
  // two GEMMs that read the same X tile back to back must not share operand
  // registers (the compiler would keep a whole tile of fragments live and spill)
  asm volatile("" ::: "memory");
  // The workgroups of one XCD (blockIdx.x = XCD mod 8) start at different K
  // steps and wrap: walking the weights in one common order would have all of
  // them wait for the same L2 misses, one prefetch ring's worth at a time,
  // while a rotated start keeps nks times as many distinct lines in flight and
  // later visitors hit in L2.  A row's K order depends on its tile only, so
  // results stay reproducible.
  const int rot = (int)(blockIdx.x >> 3) % nks;
  auto wrap = [&](int k) { return k >= nks ? k - nks : k; };
  uint4 b[kPF][kNT];
#pragma unroll
  for (int p = 0; p < kPF; p++)
#pragma unroll
    for (int n = 0; n < kNT; n++) b[p][n] = Wl[((size_t)n * KS + wrap(rot + p)) * 64];
  for (int kb = 0; kb < nks; kb += kPF) {
#pragma unroll
    for (int p = 0; p < kPF; p++) {
      const int ks = wrap(rot + kb + p);
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const AT* ap = A + (m * 16 + r) * pitch + ks * KK + q * KQ;
        if constexpr (sizeof(WT) == 2) {
          f16x8 a;
          if constexpr (sizeof(AT) == 4) {
            const float4 lo = *reinterpret_cast<const float4*>(ap);
            const float4 hi = *reinterpret_cast<const float4*>(ap + 4);
            a = f16x8{(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w,
                      (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
          } else {
            a = *reinterpret_cast<const f16x8*>(ap);
          }
#pragma unroll
          for (int n = 0; n < kNT; n++)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                a, __builtin_bit_cast(f16x8, b[p][n]), acc[m][n], 0, 0, 0);
        } else {
          const float4 a = *reinterpret_cast<const float4*>(ap);
          const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
          for (int n = 0; n < kNT; n++) {
            const float4 bb = __builtin_bit_cast(float4, b[p][n]);
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
              acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc[m][n], 0, 0, 0);
          }
        }
      }
      const int kn = wrap(wrap(rot + kb + p + kPF));  // past the end: a step already done
#pragma unroll
      for (int n = 0; n < kNT; n++) b[p][n] = Wl[((size_t)n * KS + kn) * 64];
    }
  }
}

// f(row in tile, column, accumulator + bias) over this lane's D elements.  The
// lane's three bias values are loaded once, ahead of f's (possibly predicated)
// stores: a load per element would make every element wait for its own.
template <int MT, typename Fn>
__device__ __forceinline__ void epilogue(const f32x4 (&acc)[MT][kNT], const float* __restrict__ bias,
                                         Fn f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  float bv[kNT];
#pragma unroll
  for (int n = 0; n < kNT; n++) bv[n] = bias[wave * 48 + n * 16 + r];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < kNT; n++)
#pragma unroll
      for (int i = 0; i < 4; i++)
        f(m * 16 + q * 4 + i, wave * 48 + n * 16 + r, acc[m][n][i] + bv[n]);
}

// LayerNorm (eps 1e-3) of every row of X in place, optional ReLU; a wave per row
template <int MT>
__device__ __forceinline__ void layer_norm(float* X, const float* __restrict__ gb, bool relu) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = wave; row < 16 * MT; row += kWaves) {
    float v[6], s = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      v[i] = X[row * kXP + lane + 64 * i];
      s += v[i];
    }
    const float mean = wave_sum(s) * (1.0f / kD);
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) {
      v[i] -= mean;
      ss += v[i] * v[i];
    }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * (1.0f / kD) + kEps);
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const int c = lane + 64 * i;
      float o = v[i] * rstd * gb[c] + gb[kD + c];
      if (relu) o = fmaxf(o, 0.f);
      X[row * kXP + c] = o;
    }
  }
}

struct Blob {
  const char* base;
  int K0p;
  size_t es;
  __device__ __forceinline__ const uint4* w(int layer) const {
    return reinterpret_cast<const uint4*>(
        base + kHdr + (layer == 0 ? 0 : es * kD * ((size_t)K0p + (size_t)(layer - 1) * kD)));
  }
  __device__ __forceinline__ const float* vec() const {
    return reinterpret_cast<const float*>(base + kHdr +
                                          es * kD * ((size_t)K0p + (size_t)(kLayers - 1) * kD));
  }
  __device__ __forceinline__ const float* bias(int layer) const { return vec() + V_BIAS + layer * kD; }
  __device__ __forceinline__ const float* ln(int i) const { return vec() + V_LN + i * 2 * kD; }
};

__device__ __forceinline__ float io_load(const void* p, size_t i, int io16) {
  return io16 ? __half2float(reinterpret_cast<const __half*>(p)[i])
              : reinterpret_cast<const float*>(p)[i];
}

// rows [row0, row0 + T) of a [E, 384] fp32 array -> X, plus add[dense[row]]
template <int MT>
__device__ __forceinline__ void load_rows(float* X, const float* __restrict__ src, int row0, int E,
                                          const float* __restrict__ add, const int* __restrict__ dense) {
  // 3 MT float4 per thread; rows past E read a copy of row E - 1 (never
  // stored): unconditional loads, so all of a thread's loads are in flight at once
#pragma unroll
  for (int it = 0; it < 3 * MT; it++) {
    const int i = threadIdx.x + it * kThreads;
    const int row = i / (kD / 4), c4 = i % (kD / 4), e = min(row0 + row, E - 1);
    float4 v = reinterpret_cast<const float4*>(src + (size_t)e * kD)[c4];
    if (add) {
      const float4 h = reinterpret_cast<const float4*>(add + (size_t)dense[e] * kD)[c4];
      v.x += h.x; v.y += h.y; v.z += h.z; v.w += h.w;
    }
    *reinterpret_cast<float4*>(X + row * kXP + 4 * c4) = v;
  }
}
template <int MT>
__device__ __forceinline__ void store_rows(const float* X, float* __restrict__ dst, int row0, int E) {
  for (int i = threadIdx.x; i < 16 * MT * (kD / 4); i += kThreads) {
    const int row = i / (kD / 4), c4 = i % (kD / 4), e = row0 + row;
    if (e < E)
      reinterpret_cast<float4*>(dst + (size_t)e * kD)[c4] =
          *reinterpret_cast<const float4*>(X + row * kXP + 4 * c4);
  }
}
// tmp <- rows idx[row] of src as operands (zeros where the index is outside
// [0, n): missing neighbour; or identity rows when idx is null)
template <typename WT, int MT>
__device__ __forceinline__ void gather_rows(WT* tmp, const float* __restrict__ src, int row0, int E,
                                            const int64_t* __restrict__ idx, int n) {
  constexpr int TP = WTraits<WT>::TP;
#pragma unroll
  for (int it = 0; it < 3 * MT; it++) {
    const int i = threadIdx.x + it * kThreads;
    const int row = i / (kD / 4), c4 = i % (kD / 4), e = row0 + row;
    const int ec = min(e, E - 1);
    const int64_t s = idx ? idx[ec] : (int64_t)ec;
    const bool ok = e < E && s >= 0 && s < n;
    // the address is formed from a checked index only (row 0 otherwise)
    float4 v = reinterpret_cast<const float4*>(src + (size_t)(ok ? s : 0) * kD)[c4];
    if (!ok) v = float4{0.f, 0.f, 0.f, 0.f};
    WT* o = tmp + row * TP + 4 * c4;
    o[0] = to_w(v.x, WT{});
    o[1] = to_w(v.y, WT{});
    o[2] = to_w(v.z, WT{});
    o[3] = to_w(v.w, WT{});
  }
}

// f = Wf x + b, g = Wg x + b of the tile's rows straight from the accumulators
template <typename WT, int MT>
__device__ __forceinline__ void emit_fg(const float* X, const Blob& B, int lf, float* __restrict__ F,
                                        float* __restrict__ G, int row0, int E) {
  constexpr int KSD = kD / WTraits<WT>::KK;
  f32x4 acc[MT][kNT];
#pragma unroll 1
  for (int which = 0; which < 2; which++) {
    zero_acc<MT>(acc);
    gemm<WT, MT, float>(acc, X, kXP, KSD, B.w(lf + which), KSD, 0);
    float* out = which ? G : F;
    epilogue<MT>(acc, B.bias(lf + which), [&](int row, int col, float v) {
      if (row0 + row < E) out[(size_t)(row0 + row) * kD + col] = v;
    });
  }
}

#define UPD_SMEM()                                                       \
  extern __shared__ __align__(16) unsigned char smem[];                  \
  float* X = reinterpret_cast<float*>(smem);                             \
  WT* tmp = reinterpret_cast<WT*>(smem + (size_t)16 * MT * kXP * 4);     \
  constexpr int TP = WTraits<WT>::TP, KK = WTraits<WT>::KK, KSD = kD / KK; \
  const int row0 = blockIdx.x * 16 * MT;                                 \
  (void)tmp; (void)TP; (void)KSD

// What a training launch keeps on top of its outputs (planes of `saved`,
// update_layout.hpp); unused by the inference instantiations.
struct Keep {
  float *a, *b, *c, *d, *e;
  size_t stride;  // floats between consecutive planes of `saved`
};
template <int MT>
__device__ __forceinline__ void keep(float* __restrict__ dst, int row0, int E, int row, int col,
                                     float v) {
  if (row0 + row < E) dst[(size_t)(row0 + row) * kD + col] = v;
}

// x = LN(net + inp + corr MLP(corr))           (net.py:283-284, 201-208)
// TRAIN keeps corr (a), A0 (b), Z2 (c), A3 (d), S0 (e).
template <typename WT, int MT, bool TRAIN = false>
__global__ __launch_bounds__(kThreads) void k_corr(Blob B, const void* __restrict__ net,
                                                   const void* __restrict__ inp,
                                                   const void* __restrict__ corr, int io16, int E,
                                                   int K0, float* __restrict__ xout, Keep kp) {
  UPD_SMEM();
  f32x4 acc[MT][kNT];
  zero_acc<MT>(acc);
  const int KS0 = B.K0p / KK;
  for (int c0 = 0; c0 < B.K0p; c0 += kD) {
    const int kc = min(kD, B.K0p - c0);  // multiple of 128
#pragma unroll 4
    for (int i = threadIdx.x; i < 16 * MT * kD; i += kThreads) {
      const int row = i / kD, col = i % kD, e = row0 + row, k = c0 + col;
      // clamped address, value zeroed past E / K0: unconditional loads
      const float v = io_load(corr, (size_t)min(e, E - 1) * K0 + min(k, K0 - 1), io16);
      if (col < kc) tmp[row * TP + col] = to_w(e < E && k < K0 ? v : 0.f, WT{});
      if constexpr (TRAIN)
        if (col < kc && e < E && k < K0) kp.a[(size_t)e * K0 + k] = v;
    }
    __syncthreads();
    gemm<WT, MT, WT>(acc, tmp, TP, kc / KK, B.w(L_CORR0), KS0, c0 / KK);
    __syncthreads();
  }
  epilogue<MT>(acc, B.bias(L_CORR0), [&](int row, int col, float v) {
    X[row * kXP + col] = fmaxf(v, 0.f);
    if constexpr (TRAIN) keep<MT>(kp.b, row0, E, row, col, fmaxf(v, 0.f));
  });
  __syncthreads();
  zero_acc<MT>(acc);
  gemm<WT, MT, float>(acc, X, kXP, KSD, B.w(L_CORR2), KSD, 0);
  __syncthreads();
  epilogue<MT>(acc, B.bias(L_CORR2), [&](int row, int col, float v) {
    X[row * kXP + col] = v;
    if constexpr (TRAIN) keep<MT>(kp.c, row0, E, row, col, v);
  });
  __syncthreads();
  layer_norm<MT>(X, B.ln(N_CORR3), true);
  __syncthreads();
  if constexpr (TRAIN) store_rows<MT>(X, kp.d, row0, E);
  zero_acc<MT>(acc);
  gemm<WT, MT, float>(acc, X, kXP, KSD, B.w(L_CORR5), KSD, 0);
  __syncthreads();
  epilogue<MT>(acc, B.bias(L_CORR5), [&](int row, int col, float v) {
    // rows past E take a copy of row E - 1 (never stored): unconditional loads
    const size_t o = (size_t)min(row0 + row, E - 1) * kD + col;
    const float s = io_load(net, o, io16) + io_load(inp, o, io16) + v;
    X[row * kXP + col] = s;
    if constexpr (TRAIN) keep<MT>(kp.e, row0, E, row, col, s);
  });
  __syncthreads();
  layer_norm<MT>(X, B.ln(N_NORM), false);
  __syncthreads();
  store_rows<MT>(X, xout, row0, E);
}

// x_new = x + c(m * x[idx]) from x_old (double-buffered: xin is never written
// here), optionally f/g of the first aggregation      (net.py:305-306, 179-187)
// TRAIN keeps the hidden layer's post-activation (a).
template <typename WT, int MT, bool FG, bool TRAIN = false>
__global__ __launch_bounds__(kThreads) void k_nbr(Blob B, const float* __restrict__ xin,
                                                  const int64_t* __restrict__ idx, int E, int la,
                                                  float* __restrict__ xout, float* __restrict__ F,
                                                  float* __restrict__ G, Keep kp) {
  UPD_SMEM();
  load_rows<MT>(X, xin, row0, E, nullptr, nullptr);
  gather_rows<WT, MT>(tmp, xin, row0, E, idx, E);
  __syncthreads();
  f32x4 acc[MT][kNT];
  zero_acc<MT>(acc);
  gemm<WT, MT, WT>(acc, tmp, TP, KSD, B.w(la), KSD, 0);
  __syncthreads();
  epilogue<MT>(acc, B.bias(la), [&](int row, int col, float v) {
    tmp[row * TP + col] = to_w(fmaxf(v, 0.f), WT{});
    if constexpr (TRAIN) keep<MT>(kp.a, row0, E, row, col, fmaxf(v, 0.f));
  });
  __syncthreads();
  zero_acc<MT>(acc);
  gemm<WT, MT, WT>(acc, tmp, TP, KSD, B.w(la + 1), KSD, 0);
  epilogue<MT>(acc, B.bias(la + 1), [&](int row, int col, float v) { X[row * kXP + col] += v; });
  __syncthreads();
  store_rows<MT>(X, xout, row0, E);
  if constexpr (FG) emit_fg<WT, MT>(X, B, L_KKF, F, G, row0, E);
}

// HY = h(Y) on the dense group rows                    (net.py:714)
template <typename WT, int MT>
__global__ __launch_bounds__(kThreads) void k_h(Blob B, const float* __restrict__ Y, Plan p, int E,
                                                int lh, float* __restrict__ HY) {
  UPD_SMEM();
  const int ng = plan_count(p.off, E);
  if (row0 >= ng) return;
  gather_rows<WT, MT>(tmp, Y, row0, ng, nullptr, ng);
  __syncthreads();
  f32x4 acc[MT][kNT];
  zero_acc<MT>(acc);
  gemm<WT, MT, WT>(acc, tmp, TP, KSD, B.w(lh), KSD, 0);
  epilogue<MT>(acc, B.bias(lh), [&](int row, int col, float v) {
    if (row0 + row < ng) HY[(size_t)(row0 + row) * kD + col] = v;
  });
}

// x += HY[group]; f/g of the second aggregation        (net.py:319-320)
template <typename WT, int MT>
// (xout may be xin: a workgroup reads and writes its own rows only)
__global__ __launch_bounds__(kThreads) void k_addfg(Blob B, const float* xin, float* xout,
                                                    const float* __restrict__ HY, Plan p, int E,
                                                    float* __restrict__ F, float* __restrict__ G) {
  UPD_SMEM();
  load_rows<MT>(X, xin, row0, E, HY, p.dense);
  __syncthreads();
  store_rows<MT>(X, xout, row0, E);  // own rows only
  emit_fg<WT, MT>(X, B, L_IJF, F, G, row0, E);
}

// x += HY[group]; gru; heads                            (net.py:320-326, 194-219)
// TRAIN keeps X4 (a), then per block S, A, R and the block's output, four
// consecutive planes from b (b + 4 stride for the second block), and w (c).
template <typename WT, int MT, bool TRAIN = false>
__global__ __launch_bounds__(kThreads) void k_final(Blob B, const float* __restrict__ x,
                                                    const float* __restrict__ HY, Plan p, int E,
                                                    int io16, void* __restrict__ net_out,
                                                    float* __restrict__ dout, float* __restrict__ wout,
                                                    Keep kp) {
  UPD_SMEM();
  load_rows<MT>(X, x, row0, E, HY, p.dense);
  __syncthreads();
  if constexpr (TRAIN) {
    store_rows<MT>(X, kp.a, row0, E);
    __syncthreads();  // the LayerNorm below rewrites X
  }
  f32x4 gate[MT][kNT], acc[MT][kNT];
#pragma unroll 1
  for (int blk = 0; blk < 2; blk++) {
    const int l0 = blk ? L_G3GATE : L_G1GATE;
    layer_norm<MT>(X, B.ln(blk ? N_GRU2 : N_GRU0), false);
    __syncthreads();
    zero_acc<MT>(gate);
    gemm<WT, MT, float>(gate, X, kXP, KSD, B.w(l0), KSD, 0);
    zero_acc<MT>(acc);
    gemm<WT, MT, float>(acc, X, kXP, KSD, B.w(l0 + 1), KSD, 0);
    float* kb = nullptr;
    if constexpr (TRAIN) kb = kp.b + (size_t)blk * 4 * kp.stride;
    epilogue<MT>(acc, B.bias(l0 + 1), [&](int row, int col, float v) {
      tmp[row * TP + col] = to_w(fmaxf(v, 0.f), WT{});
      if constexpr (TRAIN) keep<MT>(kb + kp.stride, row0, E, row, col, fmaxf(v, 0.f));
    });
    __syncthreads();  // tmp complete; every read of X by the two GEMMs is done
    zero_acc<MT>(acc);
    gemm<WT, MT, WT>(acc, tmp, TP, KSD, B.w(l0 + 2), KSD, 0);
    {
      const float* bg = B.bias(l0);
      const float* br = B.bias(l0 + 2);
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
      float bgv[kNT], brv[kNT];
#pragma unroll
      for (int n = 0; n < kNT; n++) {
        bgv[n] = bg[wave * 48 + n * 16 + r];
        brv[n] = br[wave * 48 + n * 16 + r];
      }
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < kNT; n++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int row = m * 16 + q * 4 + i, col = wave * 48 + n * 16 + r;
            const float s = 1.0f / (1.0f + expf(-(gate[m][n][i] + bgv[n])));
            X[row * kXP + col] += s * (acc[m][n][i] + brv[n]);
            if constexpr (TRAIN) {
              keep<MT>(kb, row0, E, row, col, s);
              keep<MT>(kb + 2 * kp.stride, row0, E, row, col, acc[m][n][i] + brv[n]);
            }
          }
    }
    __syncthreads();
    if constexpr (TRAIN) {
      store_rows<MT>(X, kb + 3 * kp.stride, row0, E);
      __syncthreads();
    }
  }
  // net_out, then the two heads on relu(x): a wave per row
  for (int i = threadIdx.x; i < 16 * MT * kD; i += kThreads) {
    const int row = i / kD, col = i % kD, e = row0 + row;
    if (e < E) {
      const float v = X[row * kXP + col];
      if (io16) reinterpret_cast<__half*>(net_out)[(size_t)e * kD + col] = __float2half_rn(v);
      else reinterpret_cast<float*>(net_out)[(size_t)e * kD + col] = v;
    }
  }
  const float* V = B.vec();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = wave; row < 16 * MT; row += kWaves) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const int c = lane + 64 * i;
      const float v = operand_round<WT>(fmaxf(X[row * kXP + c], 0.f));
#pragma unroll
      for (int o = 0; o < 4; o++) s[o] += v * V[V_DW + o * kD + c];
    }
#pragma unroll
    for (int o = 0; o < 4; o++) s[o] = wave_sum(s[o]);
    const int e = row0 + row;
    if (lane == 0 && e < E) {
      dout[2 * e] = s[0] + V[V_DB];
      dout[2 * e + 1] = s[1] + V[V_DB + 1];
      wout[2 * e] = 1.0f / (1.0f + expf(-(s[2] + V[V_WB])));
      wout[2 * e + 1] = 1.0f / (1.0f + expf(-(s[3] + V[V_WB + 1])));
      if constexpr (TRAIN) {
        kp.c[2 * e] = wout[2 * e];
        kp.c[2 * e + 1] = wout[2 * e + 1];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_copy_ints(const int* __restrict__ src,
                                                   int* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// the six ReLU masks of a training forward, uint8 [6, E, 384]
__global__ __launch_bounds__(256) void k_relu_masks(const float* __restrict__ planes, size_t stride,
                                                    int E, uint8_t* __restrict__ out) {
  constexpr int which[6] = {upd::P_A0, upd::P_A3, upd::P_A1, upd::P_A2, upd::P_A4, upd::P_A5};
  const size_t n = (size_t)E * kD, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int m = blockIdx.y;
  const int pl = m == 0 ? which[0] : m == 1 ? which[1] : m == 2 ? which[2] : m == 3 ? which[3]
                 : m == 4 ? which[4] : which[5];
  out[(size_t)m * n + i] = planes[(size_t)pl * stride + i] > 0.f ? 1 : 0;
}

// --- host ---------------------------------------------------------------------------
// dynamic LDS past the default 64 KB, set once per device and kernel
template <auto K>
bool ensure_lds(size_t lds) {
  if (lds <= 64 * 1024) return true;
  static bool attr_set[kMaxDevices] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return false;
  if (!attr_set[dev]) {
    if (hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    attr_set[dev] = true;
  }
  return true;
}

#define UPD_LAUNCH(kern, ...)                                                          \
  do {                                                                                 \
    if (!ensure_lds<kern>(lds)) return DPVO_ERR_LAUNCH;                                \
    hipLaunchKernelGGL(kern, dim3(tiles), dim3(kThreads), lds, st, __VA_ARGS__);        \
  } while (0)

// TRAIN: the same launches with every intermediate written to a plane of
// `saved` (x0..x3, f, g and the group rows directly, the on-chip ones through
// Keep), then a copy of the two group plans.
template <typename WT, int MT, bool TRAIN>
int forward_t(const Blob& B, const void* net, const void* inp, const void* corr, const int64_t* ix,
              const int64_t* jx, int E, int K0, int io16, const Ws& w, const upd::Saved* sv,
              void* net_out, float* d, float* wo, hipStream_t st) {
  constexpr size_t lds = lds_bytes<WT, MT>();
  const int tiles = (E + 16 * MT - 1) / (16 * MT);
  auto P = [&](int i) { return TRAIN ? sv->pl[i] : nullptr; };
  float* x0 = TRAIN ? P(upd::P_X0) : w.xA;
  float* x1 = TRAIN ? P(upd::P_X1) : w.xB;
  float* x2 = TRAIN ? P(upd::P_X2) : w.xA;
  float* x3 = TRAIN ? P(upd::P_X3) : w.xA;
  float* F0 = TRAIN ? P(upd::P_FKK) : w.F, *G0 = TRAIN ? P(upd::P_GKK) : w.G;
  float* F1 = TRAIN ? P(upd::P_FIJ) : w.F, *G1 = TRAIN ? P(upd::P_GIJ) : w.G;
  float* Y0 = TRAIN ? P(upd::P_YKK) : w.Y, *Y1 = TRAIN ? P(upd::P_YIJ) : w.Y;
  const size_t stride = rows_bytes(E) / 4;
  Keep kc{}, k1{}, k2{}, kf{};
  if (TRAIN) {
    kc = Keep{sv->corr, P(upd::P_A0), P(upd::P_Z2), P(upd::P_A3), P(upd::P_S0), stride};
    k1.a = P(upd::P_A1);
    k2.a = P(upd::P_A2);
    kf = Keep{P(upd::P_X4), P(upd::P_S1), sv->w, nullptr, nullptr, stride};
  }
  UPD_LAUNCH((k_corr<WT, MT, TRAIN>), B, net, inp, corr, io16, E, K0, x0, kc);
  UPD_LAUNCH((k_nbr<WT, MT, false, TRAIN>), B, (const float*)x0, ix, E, (int)L_C1A, x1, F0, G0, k1);
  UPD_LAUNCH((k_nbr<WT, MT, true, TRAIN>), B, (const float*)x1, jx, E, (int)L_C2A, x2, F0, G0, k2);
  hipLaunchKernelGGL(k_agg<TRAIN>, dim3(E), dim3(kD), 0, st, (const float*)F0, (const float*)G0,
                     w.p[0], E, Y0);
  UPD_LAUNCH((k_h<WT, MT>), B, (const float*)Y0, w.p[0], E, (int)L_KKH, w.HY);
  UPD_LAUNCH((k_addfg<WT, MT>), B, (const float*)x2, x3, (const float*)w.HY, w.p[0], E, F1, G1);
  hipLaunchKernelGGL(k_agg<TRAIN>, dim3(E), dim3(kD), 0, st, (const float*)F1, (const float*)G1,
                     w.p[1], E, Y1);
  UPD_LAUNCH((k_h<WT, MT>), B, (const float*)Y1, w.p[1], E, (int)L_IJH, w.HY);
  UPD_LAUNCH((k_final<WT, MT, TRAIN>), B, (const float*)x3, (const float*)w.HY, w.p[1], E, io16,
             net_out, d, wo, kf);
  if (TRAIN) {
    // the plan arrays are contiguous in both buffers
    const int n = (int)(12 * ints_bytes(E) / 4);
    hipLaunchKernelGGL(k_copy_ints, dim3((n + 255) / 256), dim3(256), 0, st,
                       (const int*)w.p[0].rep, sv->plan[0].rep, n);
  }
  return launch_status();
}

// RNE float -> half bits, host and device (the device pack writes the host pack's bytes)
__host__ __device__ inline uint16_t half_bits(float f) {
  uint32_t x = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u : 0));
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // rounds to >= 65520: inf
  if (x < 0x38800000u) {                                     // subnormal half or zero
    if (x < 0x33000000u) return (uint16_t)sign;              // < 2^-25
    const int shift = 126 - (int)(x >> 23);                  // 14..24
    const uint32_t m = (x & 0x7fffffu) | 0x800000u;
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (h & 1))) h++;
    return (uint16_t)(sign | h);
  }
  uint32_t h = ((x >> 23) - 112) << 10 | ((x >> 13) & 0x3ffu);
  const uint32_t rem = x & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) h++;
  return (uint16_t)(sign | h);
}
__host__ __device__ inline float half_value(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu, x;
  if (e == 0) {
    if (m == 0) x = sign;
    else {
      e = 113;
      while (!(m & 0x400u)) { m <<= 1; e--; }
      x = sign | (e << 23) | ((m & 0x3ffu) << 13);
    }
  } else if (e == 31) x = sign | 0x7f800000u | (m << 13);
  else x = sign | ((e + 112) << 23) | (m << 13);
  return __builtin_bit_cast(float, x);
}

// PyTorch state_dict order of Update (net.py:179-219): weight, bias pairs
// tensor index of each GEMM layer's weight and of each LayerNorm's gain
constexpr int kLayerTensor[kLayers] = {38, 40, 44, 0, 2, 4, 6, 10, 12, 14, 16, 18, 20,
                                       24, 26, 28, 32, 34, 36};
constexpr int kLNTensor[kLN] = {8, 42, 22, 30};
constexpr int kTensorDW = 46, kTensorWW = 48;

// --- device pack ------------------------------------------------------------------------
// blockIdx.y < 19: the weights of that layer, a 4-byte word per thread
// (grid-stride); 19..49: one 384-float vector of the vectors section each;
// 50: the header, the head biases and the zero tail.  The tensor a block reads
// is block-uniform.
struct PackArgs {
  const float* t[upd::kTensors];
  int wdtype, K0, K0p;
  unsigned tail_words;  // words from the end of the vectors to the end of the blob
};
constexpr int kPackVecs = kLayers + 2 * kLN + 4;

__device__ __forceinline__ float pack_elem(const float* __restrict__ W, int K, int KS, int KK,
                                           int KQ, unsigned slot) {
  const unsigned unit = slot / KQ, j = slot % KQ, u = unit % 64, blk = unit / 64;
  const int n = (int)(blk / KS) * 16 + (int)(u % 16), k = (int)(blk % KS) * KK + (int)(u / 16) * KQ + j;
  return k < K ? W[(size_t)n * K + k] : 0.f;
}

__global__ __launch_bounds__(256) void k_pack(PackArgs a, uint32_t* __restrict__ blob) {
  constexpr int lt[kLayers] = {38, 40, 44, 0, 2, 4, 6, 10, 12, 14, 16, 18, 20, 24, 26, 28, 32, 34, 36};
  constexpr int lnt[kLN] = {8, 42, 22, 30};
  const bool h16 = a.wdtype == DPVO_F16;
  const Blob B{reinterpret_cast<const char*>(blob), a.K0p, h16 ? (size_t)2 : (size_t)4};
  const int y = blockIdx.y;
  if (y < kLayers) {
    const int K = y == 0 ? a.K0 : kD, Kp = y == 0 ? a.K0p : kD;
    const int KK = h16 ? 32 : 16, KQ = KK / 4, KS = Kp / KK;
    const float* W = a.t[lt[y]];
    uint32_t* out = blob + (reinterpret_cast<const char*>(B.w(y)) - B.base) / 4;
    const unsigned words = (unsigned)kD * Kp / (h16 ? 2 : 1);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) {
      if (h16) {
        const uint32_t lo = half_bits(pack_elem(W, K, KS, KK, KQ, 2 * i));
        const uint32_t hi = half_bits(pack_elem(W, K, KS, KK, KQ, 2 * i + 1));
        out[i] = lo | (hi << 16);
      } else {
        out[i] = __builtin_bit_cast(uint32_t, pack_elem(W, K, KS, KK, KQ, i));
      }
    }
    return;
  }
  if (blockIdx.x != 0) return;
  float* V = reinterpret_cast<float*>(blob) + (reinterpret_cast<const char*>(B.vec()) - B.base) / 4;
  const int v = y - kLayers;
  if (v < kPackVecs) {
    const float* src;
    float* dst;
    bool round = false;
    if (v < kLayers) {
      src = a.t[lt[v] + 1];
      dst = V + V_BIAS + v * kD;
    } else if (v < kLayers + 2 * kLN) {
      const int i = (v - kLayers) / 2, gb = (v - kLayers) % 2;
      src = a.t[lnt[i] + gb];
      dst = V + V_LN + i * 2 * kD + gb * kD;
    } else {
      const int h = v - kLayers - 2 * kLN;  // d.W rows 0, 1, then w.W rows 0, 1
      src = a.t[h < 2 ? 46 : 48] + (h & 1) * kD;
      dst = V + V_DW + h * kD;
      round = h16;
    }
    for (int i = threadIdx.x; i < kD; i += 256)
      dst[i] = round ? half_value(half_bits(src[i])) : src[i];
    return;
  }
  for (int i = threadIdx.x; i < kHdr / 4; i += 256)
    blob[i] = i == 0 ? 0x31445055u : i == 1 ? (uint32_t)a.wdtype : i == 2 ? (uint32_t)a.K0
              : i == 3 ? (uint32_t)a.K0p : 0u;
  if (threadIdx.x < 2) {
    V[V_DB + threadIdx.x] = a.t[47][threadIdx.x];
    V[V_WB + threadIdx.x] = a.t[49][threadIdx.x];
  }
  for (unsigned i = threadIdx.x; i < a.tail_words; i += 256) V[kVecFloats + i] = 0.f;
}

}  // namespace

void upd::launch_plans(const int64_t* ids0, const int64_t* ids1, int E, const Plan& p0,
                       const Plan& p1, hipStream_t st) {
  hipLaunchKernelGGL(k_plan_init, dim3((E + 255) / 256), dim3(256), 0, st, E, p0, p1);
  hipLaunchKernelGGL(k_plan_rank, dim3((E + 255) / 256, (E + kPlanChunk - 1) / kPlanChunk, 2),
                     dim3(256), 0, st, ids0, ids1, E, p0, p1);
  hipLaunchKernelGGL(k_plan_build, dim3(2), dim3(1024), 0, st, E, p0, p1);
}

}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_update_packed_bytes(int K0, int wdtype) {
  if (K0 < 1 || (wdtype != DPVO_F32 && wdtype != DPVO_F16)) return 0;
  return blob_bytes(K0, wdtype);
}

DPVO_EXPORT int dpvo_update_pack_weights(const float* const* tensors, int ntensors, int dim, int K0,
                                         int wdtype, void* blob, size_t blob_size) {
  if (dim != kD || (wdtype != DPVO_F32 && wdtype != DPVO_F16)) return DPVO_ERR_UNSUPPORTED;
  if (K0 < 1 || ntensors != 50 || !tensors || !blob) return DPVO_ERR_INVALID;
  for (int i = 0; i < 50; i++)
    if (!tensors[i]) return DPVO_ERR_INVALID;
  if (blob_size < blob_bytes(K0, wdtype)) return DPVO_ERR_WORKSPACE;
  const int K0p = k0pad(K0);
  const size_t es = esize(wdtype);
  memset(blob, 0, blob_bytes(K0, wdtype));
  int32_t hdr[4] = {0x31445055, wdtype, K0, K0p};
  memcpy(blob, hdr, sizeof(hdr));
  const int KK = wdtype == DPVO_F16 ? 32 : 16, KQ = KK / 4;
  for (int l = 0; l < kLayers; l++) {
    const int K = l == 0 ? K0 : kD, KS = (l == 0 ? K0p : kD) / KK;
    const float* W = tensors[kLayerTensor[l]];
    char* out = (char*)blob + w_off(l, K0p, es);
    for (int n = 0; n < kD; n++)
      for (int k = 0; k < K; k++) {
        const size_t unit = ((size_t)(n / 16) * KS + k / KK) * 64 + 16 * ((k % KK) / KQ) + n % 16;
        const size_t slot = unit * KQ + k % KQ;
        const float v = W[(size_t)n * K + k];
        if (wdtype == DPVO_F16) ((uint16_t*)out)[slot] = half_bits(v);
        else ((float*)out)[slot] = v;
      }
  }
  float* V = (float*)((char*)blob + v_off(K0p, es));
  for (int l = 0; l < kLayers; l++) memcpy(V + V_BIAS + l * kD, tensors[kLayerTensor[l] + 1], kD * 4);
  for (int i = 0; i < kLN; i++) {
    memcpy(V + V_LN + i * 2 * kD, tensors[kLNTensor[i]], kD * 4);
    memcpy(V + V_LN + i * 2 * kD + kD, tensors[kLNTensor[i] + 1], kD * 4);
  }
  for (int i = 0; i < 2 * kD; i++) {
    const float dv = tensors[kTensorDW][i], wv = tensors[kTensorWW][i];
    V[V_DW + i] = wdtype == DPVO_F16 ? half_value(half_bits(dv)) : dv;
    V[V_WW + i] = wdtype == DPVO_F16 ? half_value(half_bits(wv)) : wv;
  }
  memcpy(V + V_DB, tensors[kTensorDW + 1], 8);
  memcpy(V + V_WB, tensors[kTensorWW + 1], 8);
  return DPVO_OK;
}

DPVO_EXPORT size_t dpvo_update_workspace_bytes(int E, int K0) {
  if (E < 1 || K0 < 1) return 0;
  return ws_bytes(E);
}

DPVO_EXPORT int dpvo_update_plan(const int64_t* gk, const int64_t* gij, int E, void* workspace,
                                 size_t workspace_size, void* stream) {
  if (E <= 0) return DPVO_OK;
  if (!gk || !gij || !workspace) return DPVO_ERR_INVALID;
  if (workspace_size < ws_bytes(E)) return DPVO_ERR_WORKSPACE;
  const Ws w = ws_carve(workspace, E);
  upd::launch_plans(gk, gij, E, w.p[0], w.p[1], as_stream(stream));
  return launch_status();
}

DPVO_EXPORT int dpvo_update_forward(const void* blob, int wdtype, const void* net, const void* inp,
                                    const void* corr, const int64_t* ix, const int64_t* jx, int E,
                                    int dim, int K0, int iodtype, void* workspace,
                                    size_t workspace_size, void* net_out, float* d, float* w,
                                    void* stream) {
  if (dim != kD) return DPVO_ERR_UNSUPPORTED;
  if (wdtype != DPVO_F32 && wdtype != DPVO_F16) return DPVO_ERR_UNSUPPORTED;
  if (iodtype != DPVO_F32 && !(iodtype == DPVO_F16 && wdtype == DPVO_F16))
    return DPVO_ERR_UNSUPPORTED;
  if (K0 < 1) return DPVO_ERR_INVALID;
  if (E <= 0) return DPVO_OK;
  if (!blob || !net || !inp || !corr || !ix || !jx || !workspace || !net_out || !d || !w)
    return DPVO_ERR_INVALID;
  if (workspace_size < ws_bytes(E)) return DPVO_ERR_WORKSPACE;
  const Ws ws = ws_carve(workspace, E);
  const Blob B{(const char*)blob, k0pad(K0), esize(wdtype)};
  const int io16 = iodtype == DPVO_F16;
  hipStream_t st = as_stream(stream);
  // row tile: 32 rows halve the weight traffic per row, 16 rows fill the CUs
  // at small E.  (A 64-row tile with fp16 operand tiles fits the 160 KB of
  // LDS, but only one workgroup per CU then: measured slower)
  const bool big = E >= kUpdateBigTileE;
  if (wdtype == DPVO_F16)
    return big ? forward_t<__half, 2, false>(B, net, inp, corr, ix, jx, E, K0, io16, ws, nullptr,
                                             net_out, d, w, st)
               : forward_t<__half, 1, false>(B, net, inp, corr, ix, jx, E, K0, io16, ws, nullptr,
                                             net_out, d, w, st);
  return big ? forward_t<float, 2, false>(B, net, inp, corr, ix, jx, E, K0, io16, ws, nullptr,
                                          net_out, d, w, st)
             : forward_t<float, 1, false>(B, net, inp, corr, ix, jx, E, K0, io16, ws, nullptr,
                                          net_out, d, w, st);
}

DPVO_EXPORT int dpvo_update_pack_weights_device(const float* const* params, int dim, int K0,
                                                int wdtype, void* blob, size_t blob_size,
                                                void* stream) {
  if (dim != kD || (wdtype != DPVO_F32 && wdtype != DPVO_F16)) return DPVO_ERR_UNSUPPORTED;
  if (K0 < 1 || !params || !blob) return DPVO_ERR_INVALID;
  for (int i = 0; i < upd::kTensors; i++)
    if (!params[i]) return DPVO_ERR_INVALID;
  if (blob_size < blob_bytes(K0, wdtype)) return DPVO_ERR_WORKSPACE;
  PackArgs a{};
  for (int i = 0; i < upd::kTensors; i++) a.t[i] = params[i];
  a.wdtype = wdtype;
  a.K0 = K0;
  a.K0p = k0pad(K0);
  a.tail_words =
      (unsigned)((blob_bytes(K0, wdtype) - v_off(a.K0p, esize(wdtype)) - kVecFloats * 4) / 4);
  const unsigned words = (unsigned)(kD * (size_t)a.K0p * esize(wdtype) / 4);
  hipLaunchKernelGGL(k_pack, dim3((words + 255) / 256, kLayers + kPackVecs + 1), dim3(256), 0,
                     as_stream(stream), a, (uint32_t*)blob);
  return launch_status();
}

DPVO_EXPORT size_t dpvo_update_saved_bytes(int E, int K0) {
  if (E < 1 || K0 < 1) return 0;
  return upd::saved_bytes(E, K0);
}

DPVO_EXPORT int dpvo_update_forward_train(const void* blob, int wdtype, const void* net,
                                          const void* inp, const void* corr, const int64_t* ix,
                                          const int64_t* jx, int E, int dim, int K0, int iodtype,
                                          void* workspace, size_t workspace_size, void* saved,
                                          size_t saved_size, void* net_out, float* d, float* w,
                                          void* stream) {
  if (dim != kD || wdtype != DPVO_F32 || iodtype != DPVO_F32) return DPVO_ERR_UNSUPPORTED;
  if (K0 < 1) return DPVO_ERR_INVALID;
  if (E <= 0) return DPVO_OK;
  if (!blob || !net || !inp || !corr || !ix || !jx || !workspace || !saved || !net_out || !d || !w)
    return DPVO_ERR_INVALID;
  if (workspace_size < ws_bytes(E) || saved_size < upd::saved_bytes(E, K0))
    return DPVO_ERR_WORKSPACE;
  const Ws ws = ws_carve(workspace, E);
  const upd::Saved sv = upd::saved_carve(saved, E, K0);
  const Blob B{(const char*)blob, k0pad(K0), 4};
  hipStream_t st = as_stream(stream);
  return E >= kUpdateBigTileE
             ? forward_t<float, 2, true>(B, net, inp, corr, ix, jx, E, K0, 0, ws, &sv, net_out, d, w, st)
             : forward_t<float, 1, true>(B, net, inp, corr, ix, jx, E, K0, 0, ws, &sv, net_out, d, w, st);
}

DPVO_EXPORT int dpvo_update_saved_relu_masks(const void* saved, size_t saved_size, int E, int K0,
                                             uint8_t* masks, void* stream) {
  if (K0 < 1) return DPVO_ERR_INVALID;
  if (E <= 0) return DPVO_OK;
  if (!saved || !masks) return DPVO_ERR_INVALID;
  if (saved_size < upd::saved_bytes(E, K0)) return DPVO_ERR_WORKSPACE;
  const upd::Saved sv = upd::saved_carve(const_cast<void*>(saved), E, K0);
  const size_t n = (size_t)E * kD;
  hipLaunchKernelGGL(k_relu_masks, dim3((unsigned)((n + 255) / 256), 6), dim3(256), 0,
                     as_stream(stream), (const float*)sv.pl[0], rows_bytes(E) / 4, E, masks);
  return launch_status();
}
