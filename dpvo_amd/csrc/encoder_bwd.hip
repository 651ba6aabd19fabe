// encoder_bwd.hip -- the backward pass of the feature encoders (encoder.hip):
// the gradients of the 22 parameters of a BasicEncoder4 from the planes that
// dpvo_encoder_forward_train kept (encoder_layout.hpp).  The image gradient is
// not computed.  Exact fp32 throughout (v_mfma_f32_16x16x4_f32 in both GEMMs),
// every sum that spans workgroups is a fixed-order fp64 sum of per-workgroup
// partials, and there is no float atomic: two calls on the same saved state
// are bit-identical.  The fp32 master parameters are read as they are
// (PyTorch layout); the only copy is a [tap][Cout][Cin] transpose of the
// weights of convs 1..10 that the backward makes for itself in its workspace.
//
// With g_out the cotangent of the encoder's output (conv 10 / 4), per conv k:
//
//   k_gout      g10 = g_out / 4 as a channels-last plane, from NCHW-contiguous
//               (a 32 x 32 LDS transpose) or channels-last memory
//   k_gz        the gradient at a conv's output before the norm: the incoming
//               plane times the block's outer ReLU mask (out > 0; the masked
//               plane is also kept as the skip path's gradient), times the
//               inner ReLU mask, and per workgroup the fp64 plane sums
//               (sum g_z, sum g_z z) of every channel.  'instance': inner mask
//               z > 0, z = (y - mean) rstd as the forward's consumer builds
//               it.  'none': inner mask out > 0, or out > skip for the second
//               conv of a block (out = skip + relu(conv) there, so out > skip
//               is relu(conv) > 0 but where relu(conv) is below half an ulp
//               of skip).  ReLU at exactly 0 passes 0.
//   k_gz_final  the partials of a plane in a fixed order in fp64: 'instance'
//               the two means per (image, channel); 'none' and conv 10 the bias
//               gradient (summed over the images too)
//   k_in_bwd    'instance': g_y = rstd (g_z - mean(g_z) - z mean(g_z z)), in place
//   k_wgrad     the weight gradient as a GEMM with M = Cout, N = taps Cin,
//               K = pixels.  A[m][k] = g_y[pixel k][channel m], B[k][n] = the
//               shifted input pixel's channel n, both one 4-byte element per
//               lane straight from the channels-last planes (conv 0: B from
//               the NCHW image, N = 147 padded to 160 in PyTorch's (c, ky, kx)
//               order); the input of a normalised layer is rebuilt
//               relu((y - mean) rstd) on the way.  grid = (K chunks, taps,
//               images); a wave keeps the whole [Cout x Cin] tile of its part
//               of the chunk, the four waves' tiles are added through LDS in
//               wave order and the workgroup writes one partial
//   k_wreduce   sums the partials over (image, chunk) in a fixed order in fp64
//               into the PyTorch-layout gradient
//   k_dgrad     the data gradient of convs 1..10 as a GEMM with M = 16 input
//               pixels, N = Cin, K = taps Cout: an input pixel (iy, ix) takes
//               tap (ky, kx) where iy + pad - ky and ix + pad - kx are
//               multiples of the stride with the quotient inside Ho x Wo
//               (other lanes feed 0).  An optional plane is added to the
//               result by the lane that owns the element (the skip path's
//               gradient; conv 7 adds onto conv 5's plane): a fixed order
//   k_wt        the [tap][Cout][Cin] transposes, one launch for the ten convs
//
// 'instance': the bias of convs 0..9 cancels in the mean subtraction, so its
// gradient is identically zero and exact zeros are written (one memset each).
//
// Launches: 'instance' 66 (k_gout, k_wt; per conv 0..9 k_gz, k_gz_final,
// k_in_bwd, k_wgrad, k_wreduce; conv 10 k_gz, k_gz_final, k_wgrad, k_wreduce;
// ten k_dgrad) plus ten memsets; 'none' 56 (no k_in_bwd, no memsets).
//
// Workspace (dpvo_encoder_backward_workspace_bytes): g10 [n, H2, W2, out_dim],
// three gradient planes per resolution, the weight-gradient partials of the
// largest conv, the plane-sum partials and means, and the transposes.
#include <algorithm>

#include "encoder_layout.hpp"

namespace dpvo {
namespace {

using namespace enc;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kThreads = 256;

// pixels of one image per workgroup of the K-split kernels: at least 512, and
// few enough chunks that all images together make about 256 partials
inline int chunk_of(int HW, int n) {
  const size_t c = ((size_t)HW * n + 255) / 256;
  return (int)((std::max<size_t>(c, 512) + 3) & ~(size_t)3);
}
inline int chunks_of(int HW, int n) {
  const int c = chunk_of(HW, n);
  return (HW + c - 1) / c;
}
// k_wgrad: pixels of one image per wave (a workgroup: four times that), at
// least 64, and about 300 workgroups over all images
inline int wg_chunk_of(int HW, int n) {
  const size_t c = ((size_t)HW * n + 299) / 300;
  return (int)(((std::max<size_t>(c, 256) + 15) & ~(size_t)15) / 4);
}
inline int wg_chunks_of(int HW, int n) {
  const int c = 4 * wg_chunk_of(HW, n);
  return (HW + c - 1) / c;
}

// --- k_gout -------------------------------------------------------------------------
// NCHW-contiguous [n, C, HW] -> channels-last [n, HW, C], times 0.25
__global__ __launch_bounds__(256) void k_gout_nchw(const float* __restrict__ g, int C, int HW,
                                                   float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5, img = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int j = ty; j < 32; j += 8) {
    const int c = c0 + j, p = p0 + tx;
    const bool ok = p < HW;  // C is a multiple of 64
    const float v = g[ok ? ((size_t)img * C + c) * HW + p : 0];
    tile[j][tx] = ok ? v : 0.f;
  }
  __syncthreads();
  for (int j = ty; j < 32; j += 8) {
    const int p = p0 + j, c = c0 + tx;
    if (p < HW) out[((size_t)img * HW + p) * C + c] = 0.25f * tile[tx][j];
  }
}
__global__ __launch_bounds__(256) void k_gout_nhwc(const float4* __restrict__ g, size_t n4,
                                                   float4* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 v = g[i];
  out[i] = float4{0.25f * v.x, 0.25f * v.y, 0.25f * v.z, 0.25f * v.w};
}

// --- k_gz ---------------------------------------------------------------------------
struct GzArgs {
  const float* g;      // incoming gradient plane
  const float* outer;  // null, or the block's output: g *= outer > 0
  float* t_out;        // null, or where the outer-masked gradient goes
  const float* y;      // inner 1, or stat given: the raw conv output; inner 2, 3: the saved output
  const float* skip;   // inner 3
  const float* stat;   // null, or (mean, rstd) [n, C] of y
  float* gz;           // null (sums only), or the result plane (may be g)
  double* part;        // [n, Ctot, chunks, 2]
  int HW, chunk, chunks;
  int inner;           // 0 none, 1 z > 0, 2 y > 0, 3 y > skip
  int C;               // channels of this launch's group (32 or 64)
  int Ctot;            // channel stride of the planes (C, or out_dim for conv 10)
};

__global__ __launch_bounds__(kThreads) void k_gz(GzArgs a) {
  __shared__ double sh[kThreads * 8];
  const int tid = threadIdx.x, C4 = a.C / 4, PL = kThreads / C4;
  const int c4 = tid % C4, pl = tid / C4, img = blockIdx.y, cbase = blockIdx.z * a.C;
  const int p0 = blockIdx.x * a.chunk, p1 = min(p0 + a.chunk, a.HW);
  float mean[4] = {0.f, 0.f, 0.f, 0.f}, rstd[4] = {1.f, 1.f, 1.f, 1.f};
  if (a.stat) {
    const float4* st = reinterpret_cast<const float4*>(a.stat + ((size_t)img * a.Ctot + cbase) * 2) + 2 * c4;
    const float4 s0 = st[0], s1 = st[1];
    mean[0] = s0.x; rstd[0] = s0.y; mean[1] = s0.z; rstd[1] = s0.w;
    mean[2] = s1.x; rstd[2] = s1.y; mean[3] = s1.z; rstd[3] = s1.w;
  }
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = p0 + pl; p < p1; p += PL) {
    const size_t i = (((size_t)img * a.HW + p) * a.Ctot + cbase) / 4 + c4;
    const float4 gv = reinterpret_cast<const float4*>(a.g)[i];
    float g[4] = {gv.x, gv.y, gv.z, gv.w};
    if (a.outer) {
      const float4 o = reinterpret_cast<const float4*>(a.outer)[i];
      const float ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int k = 0; k < 4; k++) g[k] = ov[k] > 0.f ? g[k] : 0.f;
      if (a.t_out) reinterpret_cast<float4*>(a.t_out)[i] = float4{g[0], g[1], g[2], g[3]};
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.y) {
      const float4 yv = reinterpret_cast<const float4*>(a.y)[i];
      const float y[4] = {yv.x, yv.y, yv.z, yv.w};
      if (a.stat) {
#pragma unroll
        for (int k = 0; k < 4; k++) z[k] = (y[k] - mean[k]) * rstd[k];
      }
      if (a.inner == 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = z[k] > 0.f ? g[k] : 0.f;
      } else if (a.inner == 2) {
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = y[k] > 0.f ? g[k] : 0.f;
      } else if (a.inner == 3) {
        const float4 sv = reinterpret_cast<const float4*>(a.skip)[i];
        const float s[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
        for (int k = 0; k < 4; k++) g[k] = y[k] > s[k] ? g[k] : 0.f;
      }
    }
    if (a.gz) reinterpret_cast<float4*>(a.gz)[i] = float4{g[0], g[1], g[2], g[3]};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      s1[k] += (double)g[k];
      s2[k] += (double)g[k] * (double)z[k];
    }
  }
  // sh[pl][channel][2]; then channel sums over the pixel lanes in a fixed order
#pragma unroll
  for (int k = 0; k < 4; k++) {
    sh[((pl * a.C) + 4 * c4 + k) * 2] = s1[k];
    sh[((pl * a.C) + 4 * c4 + k) * 2 + 1] = s2[k];
  }
  __syncthreads();
  if (tid < 2 * a.C) {
    double s = 0.0;
    for (int l = 0; l < PL; l++) s += sh[l * a.C * 2 + tid];
    const int c = tid >> 1, which = tid & 1;
    a.part[(((size_t)img * a.Ctot + cbase + c) * a.chunks + blockIdx.x) * 2 + which] = s;
  }
}

// the partials of a plane summed in a fixed order in fp64, one wave per
// result: lane l takes entries l, l + 64, ..., then a fixed xor tree.  bias
// null: result (img, c, which) -> msum = (sum g_z, sum g_z z) / HW.  bias
// given: result c -> bias[c] = sum g_z over images and chunks.
__global__ __launch_bounds__(64) void k_gz_final(const double* __restrict__ part, int n, int C,
                                                 int chunks, int HW, float* __restrict__ msum,
                                                 float* __restrict__ bias) {
  const int i = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  if (bias) {
    for (int k = lane; k < n * chunks; k += 64)
      s += part[(((size_t)(k / chunks) * C + i) * chunks + k % chunks) * 2];
    s = wave_sum(s);
    if (lane == 0) bias[i] = (float)s;
    return;
  }
  const int which = i & 1;
  const size_t ic = (size_t)(i >> 1);
  for (int k = lane; k < chunks; k += 64) s += part[(ic * chunks + k) * 2 + which];
  s = wave_sum(s);
  if (lane == 0) msum[i] = (float)(s / (double)HW);
}

// g_y = rstd (g_z - mean(g_z) - z mean(g_z z)), z = (y - mean) rstd; in place
__global__ __launch_bounds__(256) void k_in_bwd(float* gz, const float* __restrict__ y,
                                                const float* __restrict__ stat,
                                                const float* __restrict__ msum, size_t n4,
                                                size_t plane4, int C4) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int c4 = (int)(i % C4);
  const size_t img = i / plane4;
  const float4 g = reinterpret_cast<const float4*>(gz)[i];
  const float4 v = reinterpret_cast<const float4*>(y)[i];
  const float4* st = reinterpret_cast<const float4*>(stat + img * C4 * 8) + 2 * c4;
  const float4* ms = reinterpret_cast<const float4*>(msum + img * C4 * 8) + 2 * c4;
  const float4 s0 = st[0], s1 = st[1], m0 = ms[0], m1 = ms[1];
  float4 o;
  o.x = s0.y * (g.x - m0.x - (v.x - s0.x) * s0.y * m0.y);
  o.y = s0.w * (g.y - m0.z - (v.y - s0.z) * s0.w * m0.w);
  o.z = s1.y * (g.z - m1.x - (v.z - s1.x) * s1.y * m1.y);
  o.w = s1.w * (g.w - m1.z - (v.w - s1.z) * s1.w * m1.w);
  reinterpret_cast<float4*>(gz)[i] = o;
}

// --- k_wgrad ------------------------------------------------------------------------
struct WgArgs {
  const float* gy;    // [n, Ho, Wo, gC] channels-last
  const float* x;     // the conv's input [n, Hi, Wi, CIN] channels-last (IMG: the NCHW image)
  const float* stat;  // null, or (mean, rstd) [n, CIN] of x: the input is relu(norm(x))
  float* part;        // [n chunks][gridDim.y][COUT][NB]
  int Hi, Wi, Ho, Wo, chunk, chunks;
  int gC;             // channel stride of gy (COUT, or out_dim for conv 10)
  int final;          // conv 10: blockIdx.y is a group of 64 output channels, not a tap
};

// A workgroup owns 4 a.chunk pixels of one image and one tap, a wave a.chunk of
// them and the whole [COUT x NB] tile (CT x NT accumulators, every A and B
// element loaded once per wave).  The four waves' tiles are summed through LDS
// in wave order, so a workgroup writes one partial.  IMG (conv 0): NB = 160
// columns, column j < 147 is (c, ky, kx) = (j / 49, j % 49 / 7, j % 7) of the
// image, gridDim.y = 1.
template <int KH, int S, int CIN, int COUT, bool IMG>
__global__ __launch_bounds__(kThreads) void k_wgrad(WgArgs a) {
  constexpr int PAD = KH / 2;
  constexpr int NB = IMG ? kK0Pad : CIN, CT = COUT / 16, NT = NB / 16;
  static_assert(COUT * NB * 4 <= 64 * 1024, "the workgroup's tile exceeds static LDS");
  __shared__ float red[COUT * NB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int img = blockIdx.z, HWo = a.Ho * a.Wo;
  const int tap = a.final ? 0 : blockIdx.y, ky = tap / KH, kx = tap % KH;
  const int cbase = a.final ? blockIdx.y * COUT : 0;
  const int p0 = min((blockIdx.x * 4 + wave) * a.chunk, HWo), p1 = min(p0 + a.chunk, HWo);

  // this lane's column of every tile: the channel (and its statistics), or
  // the image tap of conv 0
  int col[NT], dy[NT], dx[NT];
  bool colok[NT];
  float mean[NT], rstd[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int n = j * 16 + r;
    if constexpr (IMG) {
      colok[j] = n < kK0;
      const int nn = colok[j] ? n : 0;
      col[j] = nn / 49;
      dy[j] = (nn % 49) / 7 - PAD;
      dx[j] = nn % 7 - PAD;
    } else {
      colok[j] = true;
      col[j] = n;
      dy[j] = ky - PAD;
      dx[j] = kx - PAD;
    }
    mean[j] = 0.f;
    rstd[j] = 1.f;
    if (!IMG && a.stat) {
      mean[j] = a.stat[((size_t)img * CIN + n) * 2];
      rstd[j] = a.stat[((size_t)img * CIN + n) * 2 + 1];
    }
  }

  f32x4 acc[CT][NT];
#pragma unroll
  for (int c = 0; c < CT; c++)
#pragma unroll
    for (int j = 0; j < NT; j++) acc[c][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // this lane's pixel of the first K step; a step moves it on by 4
  int oy = (p0 + q) / a.Wo, ox = (p0 + q) % a.Wo;
#pragma unroll 2
  for (int pb = p0; pb < p1; pb += 4) {  // wave-uniform trip count
    const bool ok = pb + q < p1;
    // every address is formed from checked indices only (element 0 otherwise)
    const float* gp = a.gy + (ok ? ((size_t)img * HWo + pb + q) * a.gC + cbase + r : 0);
    float A[CT], B[NT];
#pragma unroll
    for (int c = 0; c < CT; c++) A[c] = gp[ok ? c * 16 : 0];
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const int iy = oy * S + dy[j], ix = ox * S + dx[j];
      const bool in = ok && colok[j] && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      float v;
      if constexpr (IMG) {
        v = a.x[in ? (((size_t)img * 3 + col[j]) * a.Hi + iy) * a.Wi + ix : 0];
      } else {
        v = a.x[in ? (((size_t)img * a.Hi + iy) * a.Wi + ix) * CIN + col[j] : 0];
        if (a.stat) v = fmaxf((v - mean[j]) * rstd[j], 0.f);
      }
      B[j] = in ? v : 0.f;  // zero padding of the activation
    }
#pragma unroll
    for (int c = 0; c < CT; c++) {
      const float av = ok ? A[c] : 0.f;
#pragma unroll
      for (int j = 0; j < NT; j++)
        acc[c][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, B[j], acc[c][j], 0, 0, 0);
    }
    ox += 4;
    while (ox >= a.Wo) {
      ox -= a.Wo;
      oy++;
    }
  }

  // D[row 4 q + i][col r]: output channel 16 c + 4 q + i, column 16 j + r.
  // red = wave 0's tile + wave 1's + wave 2's + wave 3's, in that order.
#pragma unroll 1
  for (int w = 0; w < 4; w++) {
    if (wave == w) {
#pragma unroll
      for (int c = 0; c < CT; c++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            float* o = red + (c * 16 + 4 * q + i) * NB + j * 16 + r;
            *o = w == 0 ? acc[c][j][i] : *o + acc[c][j][i];
          }
    }
    __syncthreads();
  }
  const size_t split = (size_t)img * a.chunks + blockIdx.x;
  float* o = a.part + (split * gridDim.y + blockIdx.y) * COUT * NB;
  for (int e = tid; e < COUT * NB; e += kThreads) o[e] = red[e];
}

// grad[...] = sum over the splits, in split order, in fp64.  e = (y, co, nb) of
// one partial [Y][COUT][NB].  mode 0: y is the tap: grad[co][nb][y].  mode 1
// (conv 10): y is the channel group: grad[y COUT + co][nb].  mode 2 (conv 0):
// grad[co][nb], nb < 147.
// A workgroup: 32 elements x 8 split lanes (lane l takes splits l, l + 8, ...),
// the eight sums added through LDS in lane order.
__global__ __launch_bounds__(256) void k_wreduce(const float* __restrict__ part, int splits, int Y,
                                                 int COUT, int NB, int mode,
                                                 float* __restrict__ grad) {
  __shared__ double sh[8][32];
  const int el = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int e = blockIdx.x * 32 + el, E = Y * COUT * NB;
  double s = 0.0;
  if (e < E)
    for (int k = rl; k < splits; k += 8) s += (double)part[(size_t)k * E + e];
  sh[rl][el] = s;
  __syncthreads();
  if (rl != 0 || e >= E) return;
  for (int l = 1; l < 8; l++) s += sh[l][el];
  const int nb = e % NB, co = (e / NB) % COUT, y = e / (NB * COUT);
  if (mode == 0) grad[((size_t)co * NB + nb) * Y + y] = (float)s;
  else if (mode == 1) grad[((size_t)y * COUT + co) * NB + nb] = (float)s;
  else if (nb < kK0) grad[(size_t)co * kK0 + nb] = (float)s;
}

// --- k_wt ---------------------------------------------------------------------------
struct WtArgs {
  const float* w[kConvs];  // PyTorch [cout][cin][taps]
  int off[kConvs];         // element offset of conv ci's transpose in wt
  int cin[kConvs], cout[kConvs], taps[kConvs];
};
// wt[ci][tap][co][c] = w[ci][co][c][tap]; blockIdx.y = conv 1..10
__global__ __launch_bounds__(256) void k_wt(WtArgs a, float* __restrict__ wt) {
  const int ci = blockIdx.y + 1, cin = a.cin[ci], cout = a.cout[ci], taps = a.taps[ci];
  const int E = cin * cout * taps;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < E; e += gridDim.x * 256) {
    const int c = e % cin, co = (e / cin) % cout, tap = e / (cin * cout);
    wt[(size_t)a.off[ci] + e] = a.w[ci][((size_t)co * cin + c) * taps + tap];
  }
}

// --- k_dgrad ------------------------------------------------------------------------
struct DgArgs {
  const float* gy;   // [n, Ho, Wo, cout] channels-last
  const float* wt;   // [taps][cout][CIN]
  const float* add;  // null, or [n, Hi, Wi, CIN] added to the result (may be out)
  float* out;        // [n, Hi, Wi, CIN]
  int Hi, Wi, Ho, Wo, cout;
};

// A workgroup owns 4 MT rows of 16 input pixels, a wave MT rows.  The pixels
// are the MFMA's A rows (16 output channels of g_y per K block, a 16-B load:
// lane group q takes channels 4 q + j in step j, and so does B), the input
// channels its columns.
template <int KH, int S, int CIN, int MT>
__global__ __launch_bounds__(kThreads) void k_dgrad(DgArgs a) {
  constexpr int PAD = KH / 2, NT = CIN / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  const int img = blockIdx.z, ix0 = blockIdx.x * 16, iy0 = blockIdx.y * 4 * MT + wave * MT;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; m++)
#pragma unroll
    for (int n = 0; n < NT; n++) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int tap = 0; tap < KH * KH; tap++) {
    const int ky = tap / KH, kx = tap % KH;
    bool ok[MT];
    size_t base[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const int iy = iy0 + m, ix = ix0 + r, ny = iy + PAD - ky, nx = ix + PAD - kx;
      ok[m] = iy < a.Hi && ix < a.Wi && ny >= 0 && nx >= 0 && ny % S == 0 && nx % S == 0 &&
              ny / S < a.Ho && nx / S < a.Wo;
      // the address is formed from checked indices only (element 0 otherwise)
      base[m] = ok[m] ? (((size_t)img * a.Ho + ny / S) * a.Wo + nx / S) * a.cout : 0;
    }
    const float* wtap = a.wt + (size_t)tap * a.cout * CIN;
#pragma unroll 1
    for (int cb = 0; cb < a.cout; cb += 16) {
      float av[MT][4];
#pragma unroll
      for (int m = 0; m < MT; m++) {
        const float4 v = *reinterpret_cast<const float4*>(a.gy + base[m] + (ok[m] ? cb + 4 * q : 0));
        av[m][0] = ok[m] ? v.x : 0.f;
        av[m][1] = ok[m] ? v.y : 0.f;
        av[m][2] = ok[m] ? v.z : 0.f;
        av[m][3] = ok[m] ? v.w : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float* wrow = wtap + (size_t)(cb + 4 * q + j) * CIN + r;
#pragma unroll
        for (int n = 0; n < NT; n++) {
          const float b = wrow[n * 16];
#pragma unroll
          for (int m = 0; m < MT; m++)
            acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][j], b, acc[m][n], 0, 0, 0);
        }
      }
    }
  }

  // D[row 4 q + i][col r]: input pixel ix0 + 4 q + i, channel 16 n + r
#pragma unroll
  for (int m = 0; m < MT; m++) {
    const int iy = iy0 + m;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int ix = ix0 + 4 * q + i;
      if (iy >= a.Hi || ix >= a.Wi) continue;
      const size_t o = (((size_t)img * a.Hi + iy) * a.Wi + ix) * CIN + r;
#pragma unroll
      for (int n = 0; n < NT; n++) {
        float v = acc[m][n][i];
        if (a.add) v = a.add[o + n * 16] + v;
        a.out[o + n * 16] = v;
      }
    }
  }
}

// --- host ---------------------------------------------------------------------------
struct BwdWs {
  float* g10;
  float *ga1, *gb1, *t1, *ga2, *gb2, *t2;
  float* wpart;
  double* spart;
  float* msum;
  float* wt;
};

inline size_t wt_elems(int ci, int out_dim) {
  const ConvShape s = conv_shape(ci, out_dim);
  return (size_t)s.cout * s.cin * s.kh * s.kh;
}
inline size_t wpart_bytes(const Dims& d, int out_dim) {
  const int HW1 = d.H1 * d.W1, HW2 = d.H2 * d.W2;
  const size_t s1 = (size_t)d.n * wg_chunks_of(HW1, d.n), s2 = (size_t)d.n * wg_chunks_of(HW2, d.n);
  size_t m = s1 * 32 * kK0Pad;                     // conv 0
  m = std::max(m, s1 * 9 * 32 * 32);               // convs 1..4
  m = std::max(m, s2 * 9 * 64 * 64);               // convs 5 (64 x 32), 6, 8, 9; 7
  m = std::max(m, s2 * (size_t)out_dim * 64);      // conv 10
  return r256(m * 4);
}
inline size_t spart_bytes(const Dims& d, int out_dim) {
  const size_t a = (size_t)d.n * 32 * chunks_of(d.H1 * d.W1, d.n);
  const size_t b = (size_t)d.n * out_dim * chunks_of(d.H2 * d.W2, d.n);
  return r256(std::max(a, b) * 2 * 8);
}
inline size_t bwd_ws_bytes(const Dims& d, int out_dim) {
  size_t wt = 0;
  for (int ci = 1; ci < kConvs; ci++) wt += wt_elems(ci, out_dim);
  return r256((size_t)d.n * d.H2 * d.W2 * out_dim * 4) + 3 * half_plane_bytes(d) +
         3 * quarter_plane_bytes(d) + wpart_bytes(d, out_dim) + spart_bytes(d, out_dim) +
         r256((size_t)d.n * 64 * 2 * 4) + r256(wt * 4);
}
inline BwdWs bwd_ws_carve(void* base, const Dims& d, int out_dim) {
  char* p = (char*)base;
  BwdWs w;
  auto take = [&](size_t bytes) { char* q = p; p += bytes; return q; };
  w.g10 = (float*)take(r256((size_t)d.n * d.H2 * d.W2 * out_dim * 4));
  w.ga1 = (float*)take(half_plane_bytes(d));
  w.gb1 = (float*)take(half_plane_bytes(d));
  w.t1 = (float*)take(half_plane_bytes(d));
  w.ga2 = (float*)take(quarter_plane_bytes(d));
  w.gb2 = (float*)take(quarter_plane_bytes(d));
  w.t2 = (float*)take(quarter_plane_bytes(d));
  w.wpart = (float*)take(wpart_bytes(d, out_dim));
  w.spart = (double*)take(spart_bytes(d, out_dim));
  w.msum = (float*)take(r256((size_t)d.n * 64 * 2 * 4));
  w.wt = (float*)p;
  return w;
}

struct Bwd {
  bool instance;
  int out_dim;
  Dims d;
  Saved s;
  BwdWs w;
  const float* const* params;
  float* const* grads;
  const float* images;
  hipStream_t st;
  size_t wt_off[kConvs];

  const float* stat(int i) const { return instance ? saved_stat(s, d, i) : nullptr; }

  // g -> gz (and the skip path's t), the plane sums, and for conv ci either
  // the InstanceNorm backward ('instance') or the bias gradient ('none')
  void gz(int ci, const float* g, const float* outer, float* t_out, const float* y,
          const float* skip, int inner, float* out, int HW, int C) {
    GzArgs a{};
    a.g = g; a.outer = outer; a.t_out = t_out; a.y = y; a.skip = skip;
    a.stat = stat(ci);
    a.gz = out; a.part = w.spart;
    a.HW = HW; a.chunk = chunk_of(HW, d.n); a.chunks = chunks_of(HW, d.n);
    a.inner = inner; a.C = C; a.Ctot = C;
    hipLaunchKernelGGL(k_gz, dim3(a.chunks, d.n, 1), dim3(kThreads), 0, st, a);
    if (instance) {
      hipLaunchKernelGGL(k_gz_final, dim3(d.n * C * 2), dim3(64), 0, st, (const double*)w.spart,
                         d.n, C, a.chunks, HW, w.msum, (float*)nullptr);
      const size_t plane4 = (size_t)HW * C / 4, n4 = plane4 * d.n;
      hipLaunchKernelGGL(k_in_bwd, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, out, y,
                         stat(ci), (const float*)w.msum, n4, plane4, C / 4);
      hipMemsetAsync(grads[2 * ci + 1], 0, 4 * (size_t)C, st);  // the bias cancels: exact zeros
    } else {
      hipLaunchKernelGGL(k_gz_final, dim3(C), dim3(64), 0, st, (const double*)w.spart, d.n, C,
                         a.chunks, HW, (float*)nullptr, grads[2 * ci + 1]);
    }
  }

  template <int KH, int S, int CIN, int COUT, bool IMG>
  void wgrad(int ci, const float* gy, const float* x, int x_stat, int Hi, int Wi, int Ho, int Wo) {
    WgArgs a{};
    a.gy = gy; a.x = x;
    a.stat = x_stat >= 0 ? stat(x_stat) : nullptr;
    a.part = w.wpart;
    a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo;
    a.chunk = wg_chunk_of(Ho * Wo, d.n); a.chunks = wg_chunks_of(Ho * Wo, d.n);
    const bool fin = ci == 10;
    a.gC = fin ? out_dim : COUT;
    a.final = fin;
    const int Y = fin ? out_dim / 64 : IMG ? 1 : KH * KH;
    hipLaunchKernelGGL((k_wgrad<KH, S, CIN, COUT, IMG>), dim3(a.chunks, Y, d.n), dim3(kThreads), 0,
                       st, a);
    constexpr int NB = IMG ? kK0Pad : CIN;
    const int E = Y * COUT * NB;
    hipLaunchKernelGGL(k_wreduce, dim3((E + 31) / 32), dim3(256), 0, st, (const float*)w.wpart,
                       d.n * a.chunks, Y, COUT, NB, IMG ? 2 : fin ? 1 : 0, grads[2 * ci]);
  }

  template <int KH, int S, int CIN>
  void dgrad(int ci, const float* gy, int cout, const float* add, float* out, int Hi, int Wi,
             int Ho, int Wo) {
    DgArgs a{};
    a.gy = gy; a.wt = w.wt + wt_off[ci]; a.add = add; a.out = out;
    a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.cout = cout;
    constexpr int MT = 2;
    hipLaunchKernelGGL((k_dgrad<KH, S, CIN, MT>), dim3((Wi + 15) / 16, (Hi + 4 * MT - 1) / (4 * MT), d.n),
                       dim3(kThreads), 0, st, a);
  }

  int run(const float* grad_out, int nchw) {
    const int H1 = d.H1, W1 = d.W1, H2 = d.H2, W2 = d.W2, HW1 = H1 * W1, HW2 = H2 * W2;
    // g10 = grad_out / 4, channels-last
    if (nchw) {
      hipLaunchKernelGGL(k_gout_nchw, dim3((HW2 + 31) / 32, out_dim / 32, d.n), dim3(256), 0, st,
                         grad_out, out_dim, HW2, w.g10);
    } else {
      const size_t n4 = (size_t)d.n * HW2 * out_dim / 4;
      hipLaunchKernelGGL(k_gout_nhwc, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                         (const float4*)grad_out, n4, (float4*)w.g10);
    }
    {  // the transposed weights of convs 1..10
      WtArgs a{};
      size_t off = 0;
      for (int ci = 1; ci < kConvs; ci++) {
        const ConvShape cs = conv_shape(ci, out_dim);
        a.w[ci] = params[2 * ci];
        a.off[ci] = (int)off;
        a.cin[ci] = cs.cin; a.cout[ci] = cs.cout; a.taps[ci] = cs.kh * cs.kh;
        wt_off[ci] = off;
        off += wt_elems(ci, out_dim);
      }
      hipLaunchKernelGGL(k_wt, dim3(64, kConvs - 1), dim3(256), 0, st, a, w.wt);
    }
    float* const* h = s.h;
    float* const* q = s.q;
    // the planes by role.  'instance': y[k] raw conv outputs, b[] block outputs;
    // 'none': o[k] the saved outputs, block outputs among them
    const float *b0, *b1, *b2, *b3;
    if (instance) { b0 = h[5]; b1 = h[6]; b2 = q[5]; b3 = q[6]; }
    else { b0 = h[2]; b1 = h[4]; b2 = q[1]; b3 = q[4]; }
    const float* y[10] = {h[0], h[1], h[2], h[3], h[4], q[0], q[1], q[2], q[3], q[4]};
    // the inner ReLU of a conv that feeds a conv (1, 3, 5, 8, 0) and of the
    // second conv of a block (2, 4, 6, 9), and what the next conv reads
    const int in_plain = instance ? 1 : 2, in_block = instance ? 1 : 3;
    const int sx = instance ? 0 : -100;  // x_stat = conv index ('instance') or none

    {  // conv 10: bias (plane sums of g10 per group of 64 channels), weights, data
      GzArgs a{};
      a.g = w.g10; a.part = w.spart;
      a.HW = HW2; a.chunk = chunk_of(HW2, d.n); a.chunks = chunks_of(HW2, d.n);
      a.C = 64; a.Ctot = out_dim;
      hipLaunchKernelGGL(k_gz, dim3(a.chunks, d.n, out_dim / 64), dim3(kThreads), 0, st, a);
      hipLaunchKernelGGL(k_gz_final, dim3(out_dim), dim3(64), 0, st, (const double*)w.spart, d.n,
                         out_dim, a.chunks, HW2, (float*)nullptr, grads[21]);
    }
    wgrad<1, 1, 64, 64, false>(10, w.g10, b3, -1, H2, W2, H2, W2);
    dgrad<1, 1, 64>(10, w.g10, out_dim, nullptr, w.ga2, H2, W2, H2, W2);
    // layer2.1
    gz(9, w.ga2, b3, w.t2, y[9], b2, in_block, w.gb2, HW2, 64);
    wgrad<3, 1, 64, 64, false>(9, w.gb2, y[8], sx + 8, H2, W2, H2, W2);
    dgrad<3, 1, 64>(9, w.gb2, 64, nullptr, w.ga2, H2, W2, H2, W2);
    gz(8, w.ga2, nullptr, nullptr, y[8], nullptr, in_plain, w.gb2, HW2, 64);
    wgrad<3, 1, 64, 64, false>(8, w.gb2, b2, -1, H2, W2, H2, W2);
    dgrad<3, 1, 64>(8, w.gb2, 64, w.t2, w.ga2, H2, W2, H2, W2);
    // layer2.0: y[7] is the skip (conv 7, no ReLU of its own)
    gz(6, w.ga2, b2, w.t2, y[6], y[7], in_block, w.gb2, HW2, 64);
    wgrad<3, 1, 64, 64, false>(6, w.gb2, y[5], sx + 5, H2, W2, H2, W2);
    dgrad<3, 1, 64>(6, w.gb2, 64, nullptr, w.ga2, H2, W2, H2, W2);
    gz(5, w.ga2, nullptr, nullptr, y[5], nullptr, in_plain, w.gb2, HW2, 64);
    wgrad<3, 2, 32, 64, false>(5, w.gb2, b1, -1, H1, W1, H2, W2);
    dgrad<3, 2, 32>(5, w.gb2, 64, nullptr, w.ga1, H1, W1, H2, W2);
    gz(7, w.t2, nullptr, nullptr, y[7], nullptr, 0, w.gb2, HW2, 64);
    wgrad<1, 2, 32, 64, false>(7, w.gb2, b1, -1, H1, W1, H2, W2);
    dgrad<1, 2, 32>(7, w.gb2, 64, w.ga1, w.ga1, H1, W1, H2, W2);
    // layer1.1
    gz(4, w.ga1, b1, w.t1, y[4], b0, in_block, w.gb1, HW1, 32);
    wgrad<3, 1, 32, 32, false>(4, w.gb1, y[3], sx + 3, H1, W1, H1, W1);
    dgrad<3, 1, 32>(4, w.gb1, 32, nullptr, w.ga1, H1, W1, H1, W1);
    gz(3, w.ga1, nullptr, nullptr, y[3], nullptr, in_plain, w.gb1, HW1, 32);
    wgrad<3, 1, 32, 32, false>(3, w.gb1, b0, -1, H1, W1, H1, W1);
    dgrad<3, 1, 32>(3, w.gb1, 32, w.t1, w.ga1, H1, W1, H1, W1);
    // layer1.0: its skip is the stem's output
    gz(2, w.ga1, b0, w.t1, y[2], y[0], in_block, w.gb1, HW1, 32);
    wgrad<3, 1, 32, 32, false>(2, w.gb1, y[1], sx + 1, H1, W1, H1, W1);
    dgrad<3, 1, 32>(2, w.gb1, 32, nullptr, w.ga1, H1, W1, H1, W1);
    gz(1, w.ga1, nullptr, nullptr, y[1], nullptr, in_plain, w.gb1, HW1, 32);
    wgrad<3, 1, 32, 32, false>(1, w.gb1, y[0], sx + 0, H1, W1, H1, W1);
    dgrad<3, 1, 32>(1, w.gb1, 32, w.t1, w.ga1, H1, W1, H1, W1);
    // the stem
    gz(0, w.ga1, nullptr, nullptr, y[0], nullptr, in_plain, w.gb1, HW1, 32);
    wgrad<7, 2, 3, 32, true>(0, w.gb1, images, -1, d.H, d.W, H1, W1);
    return launch_status();
  }
};

}  // namespace
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_encoder_backward_workspace_bytes(int n_images, int H, int W, int out_dim) {
  if (n_images < 1 || H < 1 || W < 1 || !out_dim_ok(out_dim) || !dims_ok(n_images, H, W)) return 0;
  return bwd_ws_bytes(make_dims(n_images, H, W), out_dim);
}

DPVO_EXPORT int dpvo_encoder_backward(int norm, int out_dim, const float* const* params,
                                      const float* images, int n_images, int H, int W,
                                      const void* saved, const float* grad_out, int grad_layout,
                                      float* const* grads, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (!params || !images || !saved || !grad_out || !grads || !workspace || n_images < 1 || H < 1 ||
      W < 1)
    return DPVO_ERR_INVALID;
  for (int i = 0; i < 2 * kConvs; i++)
    if (!params[i] || !grads[i]) return DPVO_ERR_INVALID;
  if (grad_layout != DPVO_ENCODER_NCHW && grad_layout != DPVO_ENCODER_NHWC) return DPVO_ERR_INVALID;
  if (!out_dim_ok(out_dim) || !norm_ok(norm) || !dims_ok(n_images, H, W)) return DPVO_ERR_UNSUPPORTED;
  const Dims d = make_dims(n_images, H, W);
  if (workspace_bytes < bwd_ws_bytes(d, out_dim)) return DPVO_ERR_WORKSPACE;
  const bool instance = norm == DPVO_ENCODER_NORM_INSTANCE;
  Bwd b{};
  b.instance = instance;
  b.out_dim = out_dim;
  b.d = d;
  b.s = saved_carve(const_cast<void*>(saved), d, instance);
  b.w = bwd_ws_carve(workspace, d, out_dim);
  b.params = params;
  b.grads = grads;
  b.images = images;
  b.st = as_stream(stream);
  return b.run(grad_out, grad_layout == DPVO_ENCODER_NCHW);
}
