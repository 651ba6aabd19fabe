// encoder.hip -- DPVO's feature encoders (dpvo/extractor.py:200-264,
// `BasicEncoder4`, the fnet / inet of net.py's Patchifier) as implicit-GEMM
// convolutions on the gfx950 matrix cores: the inference forward, the training
// forward that keeps its planes, and the device pack.  The backward is
// encoder_bwd.hip.
//
// An encoder is eleven convolutions (all with bias):
//
//   0      conv1            7x7 s2 p3   3 -> 32      H  x W  -> H1 x W1
//   1..4   layer1.{0,1}     3x3 s1 p1  32 -> 32      two residual blocks
//   5      layer2.0.conv1   3x3 s2 p1  32 -> 64      H1 x W1 -> H2 x W2
//   6      layer2.0.conv2   3x3 s1 p1  64 -> 64
//   7      layer2.0.downsample.0  1x1 s2  32 -> 64   the strided block's skip
//   8, 9   layer2.1         3x3 s1 p1  64 -> 64
//   10     conv2            1x1 s1     64 -> out_dim, result / 4
//
// Activations live channels-last in fp32 between launches.  One launch is one
// convolution: a workgroup of four waves owns a tile of 4 MT x 16 output
// pixels (a wave: MT rows of 16), stages the tile's input window in LDS in the
// weight type and walks K = taps * Cin in steps of one MFMA.  One GEMM core,
// templated on the weight type:
//   __half : v_mfma_f32_16x16x32_f16, activations rounded to fp16 (RNE) only
//            as MFMA operands, fp32 accumulation
//   float  : v_mfma_f32_16x16x4_f32, exact fp32 products
// Bias, statistics, normalisation, ReLU, residual adds and the final / 4 are
// fp32 (statistics are combined in fp64).
//
// The weights are the MFMA's A operand and the pixels its B operand, so that
// D[row 4 q + i][col r] is (channel 16 n + 4 q + i, pixel r) for lane 16 q + r:
// a lane stores four consecutive channels of one pixel (one 16-B store
// channels-last) and the 16 lanes of a row are 16 consecutive pixels (one 64-B
// run in NCHW).  Both operands take the contiguous K run KQ q + j of a K step
// (KQ = 8 halves / 4 floats): one 16-B load each.
//
// norm_fn = 'none': bias, ReLU and the residual add run in the conv epilogue:
// eleven launches.
// norm_fn = 'instance': a conv stores its raw output and, per workgroup, the
// (count, sum, sum of squares about zero built from per-wave centred sums) of
// every channel over the tile's valid pixels.  k_stat_final combines the
// partials of a plane in a fixed order in fp64 into (mean, 1 / sqrt(var + eps));
// the consumer normalises and applies ReLU while it stages its operand, and
// k_residual writes a block's output relu(skip + relu(norm(y))).  No float
// atomics: two calls on the same input are bit-identical.  25 launches.
//
// Packed blob (host, dpvo_encoder_pack_weights; offsets in bytes):
//   [0, 256)   header: int32 magic 'ENC1', wdtype, out_dim, norm
//   weights    convs 0..10 in the order above, [Cout x Kpad] each with
//              k = (ky KW + kx) Cin + c (Kpad = K but for conv 0: 147 -> 160,
//              tail zero); element (n, k) of a conv with KS = Kpad / KK steps at
//              16-B unit ((n / 16) KS + k / KK) 64 + 16 ((k % KK) / KQ) + n % 16,
//              slot k % KQ (KK = 32 halves or 16 floats)
//   biases     fp32, convs 0..10
// dpvo_encoder_pack_weights_device (k_pack, one launch, one 4-byte word per
// thread) writes the same bytes from device parameters.
//
// Saved buffer (dpvo_encoder_forward_train; carved in encoder_layout.hpp).  The
// training forward is the launches above with every destination a plane of its
// own, so the output is bit-identical to the inference forward.  Channels-last
// fp32 planes, each rounded up to 256 B, in this order:
//   'instance'  y0..y4 [n, H1, W1, 32] raw outputs of convs 0..4, then the
//               outputs of layer1.0 and layer1.1; y5..y9 [n, H2, W2, 64] raw
//               outputs of convs 5..9, then the outputs of layer2.0 and
//               layer2.1; the statistic partials (scratch of the forward);
//               ten (mean, rstd) sets, conv i at set i, [n, Cout, 2] each in a
//               slot of n 64 2 floats
//   'none'      o0..o4 [n, H1, W1, 32] and o5..o9 [n, H2, W2, 64]: the
//               post-epilogue outputs of convs 0..9 (o2, o4, o6, o9 are the
//               block outputs; o7 is the skip conv, no ReLU).  out > 0 is the
//               mask of relu(conv) and of the block's outer ReLU.
#include <string.h>

#include "encoder_layout.hpp"

namespace dpvo {
namespace {

using namespace enc;

constexpr int kHdr = 256;
constexpr int kThreads = 256, kWaves = 4;

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

inline int conv_kpad(int ci, int out_dim) {
  const ConvShape s = conv_shape(ci, out_dim);
  return ci == 0 ? kK0Pad : s.kh * s.kh * s.cin;
}
inline size_t esize(int wdtype) { return wdtype == DPVO_F16 ? 2 : 4; }
inline size_t w_off(int ci, int out_dim, size_t es) {
  size_t o = kHdr;
  for (int i = 0; i < ci; i++) o += es * conv_shape(i, out_dim).cout * conv_kpad(i, out_dim);
  return o;
}
inline size_t b_off(int ci, int out_dim, size_t es) {
  size_t o = w_off(kConvs, out_dim, es);
  for (int i = 0; i < ci; i++) o += 4 * (size_t)conv_shape(i, out_dim).cout;
  return o;
}
inline size_t blob_bytes(int out_dim, int wdtype) {
  return (b_off(kConvs, out_dim, esize(wdtype)) + 255) & ~(size_t)255;
}

// --- workspace -------------------------------------------------------------------
// three channels-last fp32 planes at half resolution (32 channels), three at
// quarter resolution (64), the statistic partials and the ten (mean, rstd) sets
struct Ws {
  float* a1[3];
  float* a2[3];
  double* part;
  float* stat;
};
inline size_t ws_bytes(int n, int H, int W) {
  const int H1 = down(H), W1 = down(W), H2 = down(H1), W2 = down(W1);
  return 3 * r256((size_t)n * H1 * W1 * 32 * 4) + 3 * r256((size_t)n * H2 * W2 * 64 * 4) +
         r256((size_t)n * max_parts(H1, W1) * 64 * 3 * 8) + r256((size_t)10 * n * 64 * 2 * 4);
}
inline Ws ws_carve(void* base, int n, int H, int W) {
  const int H1 = down(H), W1 = down(W), H2 = down(H1), W2 = down(W1);
  char* p = (char*)base;
  Ws w;
  for (int i = 0; i < 3; i++) { w.a1[i] = (float*)p; p += r256((size_t)n * H1 * W1 * 32 * 4); }
  for (int i = 0; i < 3; i++) { w.a2[i] = (float*)p; p += r256((size_t)n * H2 * W2 * 64 * 4); }
  w.part = (double*)p;
  p += r256((size_t)n * max_parts(H1, W1) * 64 * 3 * 8);
  w.stat = (float*)p;
  return w;
}

// --- device ----------------------------------------------------------------------
template <typename WT>
struct WTraits;
template <>
struct WTraits<__half> { static constexpr int KK = 32, KQ = 8; };
template <>
struct WTraits<float> { static constexpr int KK = 16, KQ = 4; };

__device__ __forceinline__ float to_w(float v, float) { return v; }
__device__ __forceinline__ __half to_w(float v, __half) { return __float2half_rn(v); }

// sum over the 16 lanes of a DPP row (the 16 pixels of a tile row): every lane
// of the row gets it.  row_ror:8, 4, 2, 1.
__device__ __forceinline__ float row_sum(float x) {
#define DPVO_ROR(n)                                                                         \
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), \
                                                             0x120 + n, 0xf, 0xf, false))
  DPVO_ROR(8);
  DPVO_ROR(4);
  DPVO_ROR(2);
  DPVO_ROR(1);
#undef DPVO_ROR
  return x;
}

struct ConvArgs {
  const float* src;      // conv 0: the NCHW image; else channels-last fp32 [n, Hi, Wi, CIN]
  const float* in_stat;  // (mean, rstd) [n, CIN] of src: stage relu(norm(src)); null: src as is
  const uint4* W;        // packed weights
  const float* bias;
  float* dst;            // channels-last fp32 [n, Ho, Wo, COUT] (FINAL: see nchw)
  const float* skip;     // null, or [n, Ho, Wo, COUT]: dst = relu(skip + relu(conv))
  double* part;          // null, or the statistic partials [n, COUT, tiles, 3]
  int Hi, Wi, Ho, Wo;
  int relu;              // dst = relu(conv) (without skip)
  int cout;              // FINAL: the runtime output dim (a multiple of 64)
  int nchw;              // FINAL: 1 = NCHW-contiguous, 0 = channels-last memory
};

// One convolution.  KH: taps per side (pad KH / 2), S: stride, MT: tile rows
// per wave, NT: 16-channel tiles per pass.  FINAL: conv2 (any multiple of 64
// output channels in passes of 64, result / 4, either output layout).
template <typename WT, int KH, int S, int CIN, int COUT, int MT, bool FINAL>
__global__ __launch_bounds__(kThreads) void k_conv(ConvArgs a) {
  constexpr int KK = WTraits<WT>::KK, KQ = WTraits<WT>::KQ;
  constexpr bool IM2COL = CIN == 3;  // conv 0: the tile's K rows are laid out in LDS
  constexpr int TH = kWaves * MT, TW = 16, PAD = KH / 2;
  constexpr int IH = (TH - 1) * S + KH, IW = (TW - 1) * S + KH;
  constexpr int CP = IM2COL ? kK0Pad + KQ : CIN + KQ;  // LDS pitch of a pixel (elements)
  constexpr int KS = (IM2COL ? kK0Pad : KH * KH * CIN) / KK;
  constexpr int NT = COUT >= 64 ? 4 : COUT / 16;
  constexpr int kLdsElems = IM2COL ? TH * TW * CP + IH * IW * 3 : IH * IW * CP;
  constexpr int kStatFloats = kWaves * 64 * 2;
  static_assert(kLdsElems * sizeof(WT) <= 64 * 1024, "tile window exceeds static LDS");
  static_assert(kLdsElems * sizeof(WT) >= kStatFloats * 4, "statistics reuse the tile's LDS");
  __shared__ __align__(16) WT tile[kLdsElems];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int img = blockIdx.z, oy0 = blockIdx.y * TH, ox0 = blockIdx.x * TW;
  const int Hi = a.Hi, Wi = a.Wi, Ho = a.Ho, Wo = a.Wo;

  // --- stage the input window ---
  if constexpr (IM2COL) {
    // the image window [IH][IW][3] (coalesced row loads, zero outside the
    // image), then the tile's K rows k = 3 tap + c expanded from it inside LDS
    const float* im = a.src + (size_t)img * 3 * Hi * Wi;
    WT* win = tile + TH * TW * CP;
    for (int i = tid; i < 3 * IH * IW; i += kThreads) {
      const int c = i / (IH * IW), rem = i % (IH * IW), ly = rem / IW, lx = rem % IW;
      const int iy = oy0 * S - PAD + ly, ix = ox0 * S - PAD + lx;
      const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
      // the address is formed from checked indices only (element 0 otherwise)
      const float v = im[ok ? ((size_t)c * Hi + iy) * Wi + ix : 0];
      win[(ly * IW + lx) * 3 + c] = to_w(ok ? v : 0.f, WT{});
    }
    __syncthreads();
    for (int i = tid; i < TH * TW * KH * KH; i += kThreads) {
      const int tap = i / (TH * TW), p = i % (TH * TW), ky = tap / KH, kx = tap % KH;
      const WT* w3 = win + (((p / TW) * S + ky) * IW + (p % TW) * S + kx) * 3;
      WT* o = tile + p * CP + tap * 3;
      o[0] = w3[0];
      o[1] = w3[1];
      o[2] = w3[2];
    }
    for (int i = tid; i < TH * TW * (kK0Pad - kK0); i += kThreads)
      tile[(i / (kK0Pad - kK0)) * CP + kK0 + i % (kK0Pad - kK0)] = to_w(0.f, WT{});
  } else {
    const float* src = a.src + (size_t)img * Hi * Wi * CIN;
    const float* st = a.in_stat ? a.in_stat + (size_t)img * CIN * 2 : nullptr;
    constexpr int C4 = CIN / 4;
    for (int i = tid; i < IH * IW * C4; i += kThreads) {
      const int p = i / C4, c4 = i % C4, ly = p / IW, lx = p % IW;
      if (KH == 1 && S == 2 && ((ly | lx) & 1)) continue;  // never read by a 1x1 stride-2 conv
      const int iy = oy0 * S - PAD + ly, ix = ox0 * S - PAD + lx;
      const bool ok = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
      float4 v = reinterpret_cast<const float4*>(src + (ok ? ((size_t)iy * Wi + ix) * CIN : 0))[c4];
      if (st) {
        const float4 s0 = reinterpret_cast<const float4*>(st)[2 * c4];      // mean, rstd, mean, rstd
        const float4 s1 = reinterpret_cast<const float4*>(st)[2 * c4 + 1];
        v.x = fmaxf((v.x - s0.x) * s0.y, 0.f);
        v.y = fmaxf((v.y - s0.z) * s0.w, 0.f);
        v.z = fmaxf((v.z - s1.x) * s1.y, 0.f);
        v.w = fmaxf((v.w - s1.z) * s1.w, 0.f);
      }
      if (!ok) v = float4{0.f, 0.f, 0.f, 0.f};  // zero padding of the activation
      WT* o = tile + p * CP + 4 * c4;
      o[0] = to_w(v.x, WT{});
      o[1] = to_w(v.y, WT{});
      o[2] = to_w(v.z, WT{});
      o[3] = to_w(v.w, WT{});
    }
  }
  __syncthreads();

  // this lane's pixel operand of tile row m at K step ks
  auto bptr = [&](int m, int ks) -> const WT* {
    const int ty = wave * MT + m;
    if constexpr (IM2COL) {
      return tile + (ty * TW + r) * CP + ks * KK + q * KQ;
    } else {
      const int k = ks * KK, tap = k / CIN, c = k % CIN + q * KQ, ky = tap / KH, kx = tap % KH;
      return tile + ((ty * S + ky) * IW + r * S + kx) * CP + c;
    }
  };

  const int npass = FINAL ? a.cout / 64 : 1;
#pragma unroll 1
  for (int np = 0; np < npass; np++) {
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint4* Wl = a.W + (size_t)(np * NT) * KS * 64 + lane;
    uint4 w[NT], wn[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) w[n] = Wl[(size_t)n * KS * 64];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const int kn = ks + 1 < KS ? ks + 1 : ks;
#pragma unroll
      for (int n = 0; n < NT; n++) wn[n] = Wl[((size_t)n * KS + kn) * 64];
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const WT* bp = bptr(m, ks);
        if constexpr (sizeof(WT) == 2) {
          const f16x8 b = *reinterpret_cast<const f16x8*>(bp);
#pragma unroll
          for (int n = 0; n < NT; n++)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w[n]), b,
                                                               acc[m][n], 0, 0, 0);
        } else {
          const float4 b = *reinterpret_cast<const float4*>(bp);
          const float bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int n = 0; n < NT; n++) {
            const float4 ww = __builtin_bit_cast(float4, w[n]);
            const float wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
            for (int j = 0; j < 4; j++)
              acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[j], bv[j], acc[m][n], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int n = 0; n < NT; n++) w[n] = wn[n];
    }

    // --- epilogue: lane (q, r) holds channels 16 n + 4 q + i of pixel r ---
    const int cstride = FINAL ? a.cout : COUT;
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int c0 = (np * NT + n) * 16 + 4 * q;
      const float4 bias = *reinterpret_cast<const float4*>(a.bias + c0);
      const float bv[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const int oy = oy0 + wave * MT + m, ox = ox0 + r;
        const bool ok = oy < Ho && ox < Wo;
        const size_t pix = ok ? ((size_t)img * Ho + oy) * Wo + ox : 0;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = acc[m][n][i] + bv[i];
        if (a.skip) {
          const float4 s = *reinterpret_cast<const float4*>(a.skip + pix * cstride + c0);
          const float sv[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
          for (int i = 0; i < 4; i++) v[i] = fmaxf(sv[i] + fmaxf(v[i], 0.f), 0.f);
        } else if (a.relu) {
#pragma unroll
          for (int i = 0; i < 4; i++) v[i] = fmaxf(v[i], 0.f);
        }
        if constexpr (FINAL) {
#pragma unroll
          for (int i = 0; i < 4; i++) v[i] *= 0.25f;
          if (ok && a.nchw) {
#pragma unroll
            for (int i = 0; i < 4; i++)
              a.dst[(((size_t)img * cstride + c0 + i) * Ho + oy) * Wo + ox] = v[i];
          }
        }
        if (ok && !(FINAL && a.nchw))
          *reinterpret_cast<float4*>(a.dst + pix * cstride + c0) = float4{v[0], v[1], v[2], v[3]};
#pragma unroll
        for (int i = 0; i < 4; i++) acc[m][n][i] = ok ? v[i] : 0.f;  // for the statistics
      }
    }

    if constexpr (!FINAL) {
      if (a.part) {  // uniform
        // per wave and channel: sum, and the sum of squares about the wave's own
        // mean (two passes over the registers), over the wave's valid pixels
        float* sst = reinterpret_cast<float*>(tile);
        const int rows = min(max(Ho - (oy0 + wave * MT), 0), MT), cols = min(Wo - ox0, TW);
        const float cnt = (float)(rows * cols);
        __syncthreads();  // every wave is done reading the tile
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < MT; m++) s += acc[m][n][i];
            s = row_sum(s);
            const float mean = cnt > 0.f ? s / cnt : 0.f;
            float m2 = 0.f;
#pragma unroll
            for (int m = 0; m < MT; m++) {
              const bool ok = oy0 + wave * MT + m < Ho && ox0 + r < Wo;
              const float d = ok ? acc[m][n][i] - mean : 0.f;
              m2 += d * d;
            }
            m2 = row_sum(m2);
            if (r == 0) {
              const int c = n * 16 + 4 * q + i;
              sst[(wave * 64 + c) * 2] = s;
              sst[(wave * 64 + c) * 2 + 1] = m2;
            }
          }
        __syncthreads();
        if (tid < COUT) {
          double N = 0.0, S1 = 0.0, S2 = 0.0;
          for (int w8 = 0; w8 < kWaves; w8++) {  // fixed order
            const int rw = min(max(Ho - (oy0 + w8 * MT), 0), MT);
            const double nw = (double)(rw * cols);
            if (nw > 0.0) {
              const double s = sst[(w8 * 64 + tid) * 2], m2 = sst[(w8 * 64 + tid) * 2 + 1];
              N += nw;
              S1 += s;
              S2 += m2 + s * s / nw;
            }
          }
          // [image][channel][tile][3]: a channel's partials are one contiguous run
          const size_t P = (size_t)gridDim.x * gridDim.y, p = blockIdx.y * gridDim.x + blockIdx.x;
          double* o = a.part + (((size_t)img * COUT + tid) * P + p) * 3;
          o[0] = N;
          o[1] = S1;
          o[2] = S2;
        }
      }
    }
  }
}

// (mean, 1 / sqrt(var + eps)) of one (image, channel) from the P partials of
// its plane, summed in a fixed order in fp64: thread t takes partials t, t + 256,
// ..., then a fixed tree over the threads.  One workgroup per (channel, image).
__global__ __launch_bounds__(256) void k_stat_final(const double* __restrict__ part, int P, int C,
                                                    float* __restrict__ stat) {
  __shared__ double sh[256 * 3];
  const int tid = threadIdx.x, c = blockIdx.x, img = blockIdx.y;
  const double* base = part + ((size_t)img * C + c) * P * 3;
  double N = 0.0, S1 = 0.0, S2 = 0.0;
  for (int p = tid; p < P; p += 256) {
    N += base[p * 3];
    S1 += base[p * 3 + 1];
    S2 += base[p * 3 + 2];
  }
  sh[tid * 3] = N;
  sh[tid * 3 + 1] = S1;
  sh[tid * 3 + 2] = S2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 3; k++) sh[tid * 3 + k] += sh[(tid + o) * 3 + k];
    __syncthreads();
  }
  if (tid == 0) {
    N = sh[0];
    const double mean = sh[1] / N;
    const double var = fmax(sh[2] / N - mean * mean, 0.0);  // biased, as InstanceNorm2d
    stat[((size_t)img * C + c) * 2] = (float)mean;
    stat[((size_t)img * C + c) * 2 + 1] = (float)(1.0 / sqrt(var + (double)kInEps));
  }
}

// A residual block's output with instance norm: relu(skip' + relu(norm(y))),
// skip' = skip (skip_stat null), norm(skip) (mode 1: the downsample path) or
// relu(norm(skip)) (mode 2: the stem).  Channels-last fp32, four channels per
// thread; out may be skip or y (element-wise).
__global__ __launch_bounds__(256) void k_residual(const float* skip, const float* __restrict__ skip_stat,
                                                  int skip_mode, const float* y,
                                                  const float* __restrict__ y_stat, size_t n4,
                                                  size_t plane4, int C4, float* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int c4 = (int)(i % C4);
  const size_t img = i / plane4;
  float4 s = reinterpret_cast<const float4*>(skip)[i];
  const float4 v = reinterpret_cast<const float4*>(y)[i];
  const float4* ys = reinterpret_cast<const float4*>(y_stat + img * C4 * 8) + 2 * c4;
  const float4 y0 = ys[0], y1 = ys[1];
  float sv[4] = {s.x, s.y, s.z, s.w};
  if (skip_mode) {
    const float4* ss = reinterpret_cast<const float4*>(skip_stat + img * C4 * 8) + 2 * c4;
    const float4 s0 = ss[0], s1 = ss[1];
    sv[0] = (sv[0] - s0.x) * s0.y;
    sv[1] = (sv[1] - s0.z) * s0.w;
    sv[2] = (sv[2] - s1.x) * s1.y;
    sv[3] = (sv[3] - s1.z) * s1.w;
    if (skip_mode == 2)
      for (int k = 0; k < 4; k++) sv[k] = fmaxf(sv[k], 0.f);
  }
  float4 o;
  o.x = fmaxf(sv[0] + fmaxf((v.x - y0.x) * y0.y, 0.f), 0.f);
  o.y = fmaxf(sv[1] + fmaxf((v.y - y0.z) * y0.w, 0.f), 0.f);
  o.z = fmaxf(sv[2] + fmaxf((v.z - y1.x) * y1.y, 0.f), 0.f);
  o.w = fmaxf(sv[3] + fmaxf((v.w - y1.z) * y1.w, 0.f), 0.f);
  reinterpret_cast<float4*>(out)[i] = o;
}

// --- host ---------------------------------------------------------------------------
template <typename WT>
struct Runner {
  const char* blob;
  int out_dim, instance;
  Dims d;
  Ws w;
  hipStream_t st;
  size_t es = sizeof(WT);

  const uint4* W(int ci) const { return (const uint4*)(blob + w_off(ci, out_dim, es)); }
  const float* B(int ci) const { return (const float*)(blob + b_off(ci, out_dim, es)); }
  float* stat(int i) const { return w.stat + (size_t)i * d.n * 64 * 2; }

  // conv ci: src (normalised by in_stat when given) -> dst; with instance norm
  // the raw output and its statistics `so`; without, relu / the residual add
  template <int KH, int S, int CIN, int COUT, int MT>
  void conv(int ci, const float* src, int in_stat, int Hi, int Wi, int Ho, int Wo, float* dst,
            int so, bool relu, const float* skip) {
    ConvArgs a{};
    a.src = src;
    a.in_stat = in_stat >= 0 ? stat(in_stat) : nullptr;
    a.W = W(ci);
    a.bias = B(ci);
    a.dst = dst;
    a.skip = skip;
    a.part = so >= 0 ? w.part : nullptr;
    a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
    a.relu = relu;
    a.cout = COUT;
    const dim3 grid((Wo + 15) / 16, (Ho + 4 * MT - 1) / (4 * MT), d.n);
    hipLaunchKernelGGL((k_conv<WT, KH, S, CIN, COUT, MT, false>), grid, dim3(kThreads), 0, st, a);
    if (so >= 0)
      hipLaunchKernelGGL(k_stat_final, dim3(COUT, d.n), dim3(256), 0, st, (const double*)w.part,
                         (int)(grid.x * grid.y), COUT, stat(so));
  }
  void residual(const float* skip, int skip_stat, int mode, const float* y, int y_stat, int Hh,
                int Ww, int C, float* out) {
    const size_t plane4 = (size_t)Hh * Ww * C / 4, n4 = plane4 * d.n;
    hipLaunchKernelGGL(k_residual, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, skip,
                       skip_stat >= 0 ? stat(skip_stat) : nullptr, mode, y, (const float*)stat(y_stat),
                       n4, plane4, C / 4, out);
  }
  void final_conv(const float* src, float* out, int nchw) {
    ConvArgs a{};
    a.src = src;
    a.W = W(10);
    a.bias = B(10);
    a.dst = out;
    a.Hi = a.Ho = d.H2;
    a.Wi = a.Wo = d.W2;
    a.cout = out_dim;
    a.nchw = nchw;
    const dim3 grid((d.W2 + 15) / 16, (d.H2 + 3) / 4, d.n);
    hipLaunchKernelGGL((k_conv<WT, 1, 1, 64, 64, 1, true>), grid, dim3(kThreads), 0, st, a);
  }

  int run(const float* images, float* out, int nchw) {
    const int H = d.H, Wd = d.W, H1 = d.H1, W1 = d.W1, H2 = d.H2, W2 = d.W2;
    float *A1 = w.a1[0], *B1 = w.a1[1], *C1 = w.a1[2], *A2 = w.a2[0], *B2 = w.a2[1], *C2 = w.a2[2];
    if (instance) {
      conv<7, 2, 3, 32, 1>(0, images, -1, H, Wd, H1, W1, A1, 0, false, nullptr);
      conv<3, 1, 32, 32, 2>(1, A1, 0, H1, W1, H1, W1, B1, 1, false, nullptr);
      conv<3, 1, 32, 32, 2>(2, B1, 1, H1, W1, H1, W1, C1, 2, false, nullptr);
      residual(A1, 0, 2, C1, 2, H1, W1, 32, C1);                           // layer1.0 -> C1
      conv<3, 1, 32, 32, 2>(3, C1, -1, H1, W1, H1, W1, B1, 3, false, nullptr);
      conv<3, 1, 32, 32, 2>(4, B1, 3, H1, W1, H1, W1, A1, 4, false, nullptr);
      residual(C1, -1, 0, A1, 4, H1, W1, 32, A1);                          // layer1.1 -> A1
      conv<3, 2, 32, 64, 1>(5, A1, -1, H1, W1, H2, W2, A2, 5, false, nullptr);
      conv<3, 1, 64, 64, 1>(6, A2, 5, H2, W2, H2, W2, B2, 6, false, nullptr);
      conv<1, 2, 32, 64, 1>(7, A1, -1, H1, W1, H2, W2, C2, 7, false, nullptr);
      residual(C2, 7, 1, B2, 6, H2, W2, 64, C2);                           // layer2.0 -> C2
      conv<3, 1, 64, 64, 1>(8, C2, -1, H2, W2, H2, W2, A2, 8, false, nullptr);
      conv<3, 1, 64, 64, 1>(9, A2, 8, H2, W2, H2, W2, B2, 9, false, nullptr);
      residual(C2, -1, 0, B2, 9, H2, W2, 64, B2);                          // layer2.1 -> B2
      final_conv(B2, out, nchw);
    } else {
      conv<7, 2, 3, 32, 1>(0, images, -1, H, Wd, H1, W1, A1, -1, true, nullptr);
      conv<3, 1, 32, 32, 2>(1, A1, -1, H1, W1, H1, W1, B1, -1, true, nullptr);
      conv<3, 1, 32, 32, 2>(2, B1, -1, H1, W1, H1, W1, C1, -1, false, A1);  // layer1.0 -> C1
      conv<3, 1, 32, 32, 2>(3, C1, -1, H1, W1, H1, W1, B1, -1, true, nullptr);
      conv<3, 1, 32, 32, 2>(4, B1, -1, H1, W1, H1, W1, A1, -1, false, C1);  // layer1.1 -> A1
      conv<3, 2, 32, 64, 1>(5, A1, -1, H1, W1, H2, W2, A2, -1, true, nullptr);
      conv<1, 2, 32, 64, 1>(7, A1, -1, H1, W1, H2, W2, C2, -1, false, nullptr);
      conv<3, 1, 64, 64, 1>(6, A2, -1, H2, W2, H2, W2, B2, -1, false, C2);  // layer2.0 -> B2
      conv<3, 1, 64, 64, 1>(8, B2, -1, H2, W2, H2, W2, A2, -1, true, nullptr);
      conv<3, 1, 64, 64, 1>(9, A2, -1, H2, W2, H2, W2, C2, -1, false, B2);  // layer2.1 -> C2
      final_conv(C2, out, nchw);
    }
    return launch_status();
  }

  // The training forward: the same launches with every destination a plane of
  // its own inside `s` (encoder_layout.hpp), so the backward finds them.
  // w.part / w.stat point into `s` too.
  int run_train(const float* images, float* out, int nchw, const Saved& s) {
    const int H = d.H, Wd = d.W, H1 = d.H1, W1 = d.W1, H2 = d.H2, W2 = d.W2;
    float* const* h = s.h;
    float* const* q = s.q;
    if (instance) {
      conv<7, 2, 3, 32, 1>(0, images, -1, H, Wd, H1, W1, h[0], 0, false, nullptr);
      conv<3, 1, 32, 32, 2>(1, h[0], 0, H1, W1, H1, W1, h[1], 1, false, nullptr);
      conv<3, 1, 32, 32, 2>(2, h[1], 1, H1, W1, H1, W1, h[2], 2, false, nullptr);
      residual(h[0], 0, 2, h[2], 2, H1, W1, 32, h[5]);                     // layer1.0
      conv<3, 1, 32, 32, 2>(3, h[5], -1, H1, W1, H1, W1, h[3], 3, false, nullptr);
      conv<3, 1, 32, 32, 2>(4, h[3], 3, H1, W1, H1, W1, h[4], 4, false, nullptr);
      residual(h[5], -1, 0, h[4], 4, H1, W1, 32, h[6]);                    // layer1.1
      conv<3, 2, 32, 64, 1>(5, h[6], -1, H1, W1, H2, W2, q[0], 5, false, nullptr);
      conv<3, 1, 64, 64, 1>(6, q[0], 5, H2, W2, H2, W2, q[1], 6, false, nullptr);
      conv<1, 2, 32, 64, 1>(7, h[6], -1, H1, W1, H2, W2, q[2], 7, false, nullptr);
      residual(q[2], 7, 1, q[1], 6, H2, W2, 64, q[5]);                     // layer2.0
      conv<3, 1, 64, 64, 1>(8, q[5], -1, H2, W2, H2, W2, q[3], 8, false, nullptr);
      conv<3, 1, 64, 64, 1>(9, q[3], 8, H2, W2, H2, W2, q[4], 9, false, nullptr);
      residual(q[5], -1, 0, q[4], 9, H2, W2, 64, q[6]);                    // layer2.1
      final_conv(q[6], out, nchw);
    } else {
      conv<7, 2, 3, 32, 1>(0, images, -1, H, Wd, H1, W1, h[0], -1, true, nullptr);
      conv<3, 1, 32, 32, 2>(1, h[0], -1, H1, W1, H1, W1, h[1], -1, true, nullptr);
      conv<3, 1, 32, 32, 2>(2, h[1], -1, H1, W1, H1, W1, h[2], -1, false, h[0]);  // layer1.0
      conv<3, 1, 32, 32, 2>(3, h[2], -1, H1, W1, H1, W1, h[3], -1, true, nullptr);
      conv<3, 1, 32, 32, 2>(4, h[3], -1, H1, W1, H1, W1, h[4], -1, false, h[2]);  // layer1.1
      conv<3, 2, 32, 64, 1>(5, h[4], -1, H1, W1, H2, W2, q[0], -1, true, nullptr);
      conv<1, 2, 32, 64, 1>(7, h[4], -1, H1, W1, H2, W2, q[2], -1, false, nullptr);
      conv<3, 1, 64, 64, 1>(6, q[0], -1, H2, W2, H2, W2, q[1], -1, false, q[2]);  // layer2.0
      conv<3, 1, 64, 64, 1>(8, q[1], -1, H2, W2, H2, W2, q[3], -1, true, nullptr);
      conv<3, 1, 64, 64, 1>(9, q[3], -1, H2, W2, H2, W2, q[4], -1, false, q[1]);  // layer2.1
      final_conv(q[4], out, nchw);
    }
    return launch_status();
  }
};

// RNE float -> half bits (host pack and device pack: one definition)
__host__ __device__ inline uint16_t half_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
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

// The packed blob written on the device, one 4-byte word per thread: the
// inverse of the host pack's index map, so the bytes are the same.
struct PackArgs {
  const float* w[kConvs];
  const float* b[kConvs];
  int woff[kConvs + 1];  // first word of each conv's weights; [kConvs]: of the biases
  int boff[kConvs + 1];  // first word of each conv's bias; [kConvs]: of the zero tail
  int cin[kConvs], taps[kConvs], ks[kConvs];
  int wdtype, out_dim, norm, words;
};

__device__ inline float pack_elem(const PackArgs& a, int ci, int slot, int KK, int KQ) {
  const int unit = slot / KQ, kslot = slot % KQ, KS = a.ks[ci];
  const int n16 = unit / (KS * 64), rem = unit % (KS * 64), u = rem % 64;
  const int k = (rem / 64) * KK + (u / 16) * KQ + kslot, n = n16 * 16 + u % 16;
  const int cin = a.cin[ci], taps = a.taps[ci];
  if (k >= taps * cin) return 0.f;  // conv 0's padded K tail
  return a.w[ci][((size_t)n * cin + k % cin) * taps + k / cin];
}

__global__ __launch_bounds__(256) void k_pack(PackArgs a, uint32_t* __restrict__ blob) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.words) return;
  uint32_t v = 0;
  if (i < kHdr / 4) {
    v = i == 0 ? 0x31434e45u : i == 1 ? (uint32_t)a.wdtype : i == 2 ? (uint32_t)a.out_dim
        : i == 3 ? (uint32_t)a.norm : 0u;
  } else if (i < a.woff[kConvs]) {
    int ci = 0;
    while (i >= a.woff[ci + 1]) ci++;
    const int wi = i - a.woff[ci];
    if (a.wdtype == DPVO_F16) {
      const uint32_t lo = half_bits(pack_elem(a, ci, 2 * wi, 32, 8));
      const uint32_t hi = half_bits(pack_elem(a, ci, 2 * wi + 1, 32, 8));
      v = lo | hi << 16;
    } else {
      v = __builtin_bit_cast(uint32_t, pack_elem(a, ci, wi, 16, 4));
    }
  } else if (i < a.boff[kConvs]) {
    int ci = 0;
    while (i >= a.boff[ci + 1]) ci++;
    v = __builtin_bit_cast(uint32_t, a.b[ci][i - a.boff[ci]]);
  }
  blob[i] = v;
}

}  // namespace
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_encoder_packed_bytes(int out_dim, int wdtype) {
  if (!out_dim_ok(out_dim) || (wdtype != DPVO_F32 && wdtype != DPVO_F16)) return 0;
  return blob_bytes(out_dim, wdtype);
}

DPVO_EXPORT int dpvo_encoder_pack_weights(const float* const* tensors, int ntensors, int out_dim,
                                          int norm, int wdtype, void* blob, size_t blob_size) {
  if (ntensors != 2 * kConvs || !tensors || !blob) return DPVO_ERR_INVALID;
  for (int i = 0; i < 2 * kConvs; i++)
    if (!tensors[i]) return DPVO_ERR_INVALID;
  if (!out_dim_ok(out_dim) || (wdtype != DPVO_F32 && wdtype != DPVO_F16) ||
      (norm != DPVO_ENCODER_NORM_NONE && norm != DPVO_ENCODER_NORM_INSTANCE))
    return DPVO_ERR_UNSUPPORTED;
  if (blob_size < blob_bytes(out_dim, wdtype)) return DPVO_ERR_WORKSPACE;
  const size_t es = esize(wdtype);
  memset(blob, 0, blob_bytes(out_dim, wdtype));
  int32_t hdr[4] = {0x31434e45, wdtype, out_dim, norm};
  memcpy(blob, hdr, sizeof(hdr));
  const int KK = wdtype == DPVO_F16 ? 32 : 16, KQ = KK / 4;
  for (int ci = 0; ci < kConvs; ci++) {
    const ConvShape s = conv_shape(ci, out_dim);
    const int taps = s.kh * s.kh, K = taps * s.cin, KS = conv_kpad(ci, out_dim) / KK;
    const float* Wt = tensors[2 * ci];  // [cout][cin][kh][kw]
    char* out = (char*)blob + w_off(ci, out_dim, es);
    for (int n = 0; n < s.cout; n++)
      for (int k = 0; k < K; k++) {
        const int tap = k / s.cin, c = k % s.cin;
        const float v = Wt[((size_t)n * s.cin + c) * taps + tap];
        const size_t unit = ((size_t)(n / 16) * KS + k / KK) * 64 + 16 * ((k % KK) / KQ) + n % 16;
        const size_t slot = unit * KQ + k % KQ;
        if (wdtype == DPVO_F16) ((uint16_t*)out)[slot] = half_bits(v);
        else ((float*)out)[slot] = v;
      }
    memcpy((char*)blob + b_off(ci, out_dim, es), tensors[2 * ci + 1], 4 * (size_t)s.cout);
  }
  return DPVO_OK;
}

DPVO_EXPORT size_t dpvo_encoder_workspace_bytes(int n_images, int H, int W, int out_dim) {
  if (n_images < 1 || H < 1 || W < 1 || !out_dim_ok(out_dim) || !dims_ok(n_images, H, W)) return 0;
  return ws_bytes(n_images, H, W);
}

DPVO_EXPORT int dpvo_encoder_forward(const void* blob, int wdtype, int norm, int out_dim,
                                     const float* images, int n_images, int H, int W, float* out,
                                     int out_layout, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  if (!blob || !images || !out || !workspace || n_images < 1 || H < 1 || W < 1)
    return DPVO_ERR_INVALID;
  if (out_layout != DPVO_ENCODER_NCHW && out_layout != DPVO_ENCODER_NHWC) return DPVO_ERR_INVALID;
  if ((wdtype != DPVO_F32 && wdtype != DPVO_F16) || !out_dim_ok(out_dim) ||
      (norm != DPVO_ENCODER_NORM_NONE && norm != DPVO_ENCODER_NORM_INSTANCE) ||
      !dims_ok(n_images, H, W))
    return DPVO_ERR_UNSUPPORTED;
  if (workspace_bytes < ws_bytes(n_images, H, W)) return DPVO_ERR_WORKSPACE;
  const Dims d{n_images, H, W, down(H), down(W), down(down(H)), down(down(W))};
  const Ws ws = ws_carve(workspace, n_images, H, W);
  const int nchw = out_layout == DPVO_ENCODER_NCHW;
  if (wdtype == DPVO_F16) {
    Runner<__half> r{(const char*)blob, out_dim, norm == DPVO_ENCODER_NORM_INSTANCE, d, ws,
                     as_stream(stream)};
    return r.run(images, out, nchw);
  }
  Runner<float> r{(const char*)blob, out_dim, norm == DPVO_ENCODER_NORM_INSTANCE, d, ws,
                  as_stream(stream)};
  return r.run(images, out, nchw);
}

DPVO_EXPORT int dpvo_encoder_pack_weights_device(const float* const* params, int out_dim, int norm,
                                                 int wdtype, void* blob, size_t blob_size,
                                                 void* stream) {
  if (!params || !blob) return DPVO_ERR_INVALID;
  for (int i = 0; i < 2 * kConvs; i++)
    if (!params[i]) return DPVO_ERR_INVALID;
  if (!out_dim_ok(out_dim) || (wdtype != DPVO_F32 && wdtype != DPVO_F16) || !norm_ok(norm))
    return DPVO_ERR_UNSUPPORTED;
  if (blob_size < blob_bytes(out_dim, wdtype)) return DPVO_ERR_WORKSPACE;
  const size_t es = esize(wdtype);
  PackArgs a{};
  for (int ci = 0; ci < kConvs; ci++) {
    const ConvShape s = conv_shape(ci, out_dim);
    a.w[ci] = params[2 * ci];
    a.b[ci] = params[2 * ci + 1];
    a.woff[ci] = (int)(w_off(ci, out_dim, es) / 4);
    a.boff[ci] = (int)(b_off(ci, out_dim, es) / 4);
    a.cin[ci] = s.cin;
    a.taps[ci] = s.kh * s.kh;
    a.ks[ci] = conv_kpad(ci, out_dim) / (wdtype == DPVO_F16 ? 32 : 16);
  }
  a.woff[kConvs] = (int)(w_off(kConvs, out_dim, es) / 4);
  a.boff[kConvs] = (int)(b_off(kConvs, out_dim, es) / 4);
  a.wdtype = wdtype;
  a.out_dim = out_dim;
  a.norm = norm;
  a.words = (int)(blob_bytes(out_dim, wdtype) / 4);
  hipLaunchKernelGGL(k_pack, dim3((a.words + 255) / 256), dim3(256), 0, as_stream(stream), a,
                     (uint32_t*)blob);
  return launch_status();
}

DPVO_EXPORT size_t dpvo_encoder_saved_bytes(int n_images, int H, int W, int out_dim, int norm) {
  if (n_images < 1 || H < 1 || W < 1 || !out_dim_ok(out_dim) || !norm_ok(norm) ||
      !dims_ok(n_images, H, W))
    return 0;
  return saved_bytes(make_dims(n_images, H, W), norm == DPVO_ENCODER_NORM_INSTANCE);
}

DPVO_EXPORT int dpvo_encoder_forward_train(const void* blob, int wdtype, int norm, int out_dim,
                                           const float* images, int n_images, int H, int W,
                                           float* out, int out_layout, void* saved,
                                           size_t saved_size, void* stream) {
  if (!blob || !images || !out || !saved || n_images < 1 || H < 1 || W < 1)
    return DPVO_ERR_INVALID;
  if (out_layout != DPVO_ENCODER_NCHW && out_layout != DPVO_ENCODER_NHWC) return DPVO_ERR_INVALID;
  if ((wdtype != DPVO_F32 && wdtype != DPVO_F16) || !out_dim_ok(out_dim) || !norm_ok(norm) ||
      !dims_ok(n_images, H, W))
    return DPVO_ERR_UNSUPPORTED;
  const bool instance = norm == DPVO_ENCODER_NORM_INSTANCE;
  const Dims d = make_dims(n_images, H, W);
  if (saved_size < saved_bytes(d, instance)) return DPVO_ERR_WORKSPACE;
  const Saved s = saved_carve(saved, d, instance);
  Ws ws{};
  ws.part = s.part;
  ws.stat = s.stat;
  const int nchw = out_layout == DPVO_ENCODER_NCHW;
  if (wdtype == DPVO_F16) {
    Runner<__half> r{(const char*)blob, out_dim, instance, d, ws, as_stream(stream)};
    return r.run_train(images, out, nchw, s);
  }
  Runner<float> r{(const char*)blob, out_dim, instance, d, ws, as_stream(stream)};
  return r.run_train(images, out, nchw, s);
}
