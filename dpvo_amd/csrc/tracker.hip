// tracker.hip -- the pieces of DPVO's frame path (dpvo/dpvo.py) that sit between
// the larger kernels, on gfx950.  Four small memory-bound kernels, each one
// launch on the caller's stream, none synchronising with the host:
//
// dpvo_frame_sample    Patchifier.forward after the two encoders (net.py:388-399)
//                      and the ring writes of DPVO.__call__ (dpvo.py:937-938,
//                      965-969): the P x P fmap window and the imap pixel of
//                      every patch centre straight into ring rows of gmap_ /
//                      imap_, the (x, y, 1) patch grid and the B, G, R colours.
//                      The reference builds an h x w coordinate grid and makes
//                      four patchify launches plus index copies.
// dpvo_probe_median    torch.quantile(delta.norm(dim=-1).float(), 0.5) of the
//                      motion probe (dpvo.py:584): rank select in LDS.
// dpvo_update_targets  target = coords[..., P/2, P/2] + delta, weight = w
//                      (dpvo.py:805-810) written into the patch graph.
// dpvo_map_points      the centre pixel of pops.point_cloud (dpvo.py:834-836):
//                      one thread per patch, not the P x P cloud.
//
// The fp32 chains that must round like the reference's torch ops are written
// with the __f*_rn intrinsics, which the compiler never contracts.
#include <math.h>

#include "common.hpp"

namespace dpvo {
namespace tracker {

// ---- frame sample ---------------------------------------------------------------
struct FrameSample {
  const float* fmap;    // [C, h, w]
  const float* imap;    // [DIM, h, w]
  const float* image;   // [3, H, W], normalised
  const float* coords;  // [M, 2] (x, y)
  void* gmap_ring;      // [pmem * M, C, P, P]
  void* imap_ring;      // [pmem * M, DIM]
  float* patches;       // [M, 3, P, P]
  uint8_t* colors;      // [N, M, 3]
  const int32_t* n_dev;
  int h, w, H, W, C, DIM, M, P, res, pmem, N, n;
};

__device__ __forceinline__ void ring_store(float* d, size_t i, float v) { d[i] = v; }
__device__ __forceinline__ void ring_store(__half* d, size_t i, float v) {
  d[i] = __float2half_rn(v);  // round to nearest even, as .to(torch.half)
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// One wave per patch.  Lane t of pass k owns output element k * 64 + t of the
// patch's ring row: consecutive lanes write consecutive addresses, and read P
// consecutive floats of one fmap row before stepping to the next row / channel
// plane.  Every load of a patch is independent of the others.
template <typename T>
__global__ void __launch_bounds__(kWave) frame_sample_kernel(FrameSample a) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int n = a.n_dev ? *a.n_dev : a.n;
  if (n < 0 || n >= a.N) return;  // a device value outside the buffers: nothing written
  const int P = a.P, PP = P * P, r = P / 2;
  // integer-valued centres; clamped so that no window leaves the maps
  const int x = clampi((int)a.coords[2 * m], r, a.w - 1 - r);
  const int y = clampi((int)a.coords[2 * m + 1], r, a.h - 1 - r);
  const size_t row = (size_t)(n % a.pmem) * a.M + m;
  const size_t plane = (size_t)a.h * a.w;

  T* g = reinterpret_cast<T*>(a.gmap_ring) + row * a.C * PP;
  const float* f0 = a.fmap + (size_t)(y - r) * a.w + (x - r);
  const int total = a.C * PP;
#pragma unroll 6
  for (int i = lane; i < total; i += kWave) {
    const int c = i / PP, p = i - c * PP, py = p / P, px = p - py * P;
    ring_store(g, i, f0[c * plane + (size_t)py * a.w + px]);
  }
  T* im = reinterpret_cast<T*>(a.imap_ring) + row * a.DIM;
  const float* i0 = a.imap + (size_t)y * a.w + x;
#pragma unroll 6
  for (int c = lane; c < a.DIM; c += kWave) ring_store(im, c, i0[c * plane]);

  // (x, y, 1) of every patch pixel: utils.py:39-54 gathered at the centre
  float* pt = a.patches + (size_t)m * 3 * PP;
  for (int i = lane; i < 3 * PP; i += kWave) {
    const int ch = i / PP, p = i - ch * PP, py = p / P, px = p - py * P;
    pt[i] = ch == 0 ? (float)(x + px - r) : ch == 1 ? (float)(y + py - r) : 1.0f;
  }
  // colours: clr[[2, 1, 0]] at (res x + res / 2, res y + res / 2), then
  // (v + 0.5) * (255 / 2) truncated (dpvo.py:937-938), fp32, two roundings
  if (lane < 3) {
    const int cx = clampi(a.res * x + a.res / 2, 0, a.W - 1);
    const int cy = clampi(a.res * y + a.res / 2, 0, a.H - 1);
    const float v = a.image[(size_t)(2 - lane) * a.H * a.W + (size_t)cy * a.W + cx];
    const float s = __fmul_rn(__fadd_rn(v, 0.5f), 127.5f);
    a.colors[((size_t)n * a.M + m) * 3 + lane] = (uint8_t)(int)s;
  }
}

// ---- probe median ---------------------------------------------------------------
constexpr int kMedMax = 1024;

// order-preserving key of a float: a < b  <=>  key(a) < key(b)
__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup of M rounded up to whole waves.  Thread i ranks its norm among
// all M (ties broken by index, so the ranks are a permutation): M LDS reads of
// one address per wave-instruction, a broadcast.
template <typename T>
__global__ void __launch_bounds__(kMedMax)
    probe_median_kernel(const T* __restrict__ delta, int M, float* __restrict__ out) {
  __shared__ uint32_t keys[kMedMax];
  __shared__ float mid[2];
  __shared__ int any_nan;
  const int tid = threadIdx.x;
  if (tid == 0) any_nan = 0;
  float v = 0.f;
  uint32_t key = 0;
  if (tid < M) {
    const float x = to_acc(delta[2 * tid]), y = to_acc(delta[2 * tid + 1]);
    // the accumulation of torch's norm: acc = fma(v, v, acc) from acc = 0
    v = __fsqrt_rn(__fmaf_rn(y, y, __fmul_rn(x, x)));
    key = float_key(v);
    keys[tid] = key;
  }
  __syncthreads();
  if (tid < M) {
    if (v != v) any_nan = 1;
    int rank = 0;
    for (int j = 0; j < M; j++) {
      const uint32_t k = keys[j];
      rank += (k < key || (k == key && j < tid)) ? 1 : 0;
    }
    if (rank == (M - 1) / 2) mid[0] = v;
    if (rank == M / 2) mid[1] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const float lo = mid[0], hi = mid[1];
    // torch.lerp at weight 0.5: b - (b - a) * 0.5; an odd M has lo == hi
    float q = (M & 1) ? lo : __fsub_rn(hi, __fmul_rn(__fsub_rn(hi, lo), 0.5f));
    if (any_nan) q = __uint_as_float(0x7fc00000u);
    out[0] = q;
  }
}

// ---- update targets -------------------------------------------------------------
constexpr int kUtT = 256;

template <typename T>
__global__ void __launch_bounds__(kUtT)
    update_targets_kernel(const float* __restrict__ coords, const T* __restrict__ delta,
                          const T* __restrict__ w, float* __restrict__ target,
                          float* __restrict__ weight, int P, int E,
                          const int32_t* __restrict__ E_dev, int cap) {
  const int count = E_dev ? min(max(*E_dev, 0), cap) : E;
  const int i = blockIdx.x * kUtT + threadIdx.x;  // (edge, component)
  if (i >= 2 * count) return;
  const int PP = P * P, centre = (P / 2) * P + P / 2;
  target[i] = __fadd_rn(coords[(size_t)i * PP + centre], to_acc(delta[i]));
  weight[i] = to_acc(w[i]);
}

// ---- map points -----------------------------------------------------------------
constexpr int kMpT = 256;

// X = pose^-1 * ((x - cx) / fx, (y - cy) / fy, 1, d); out = X.xyz / X.w.  fp64
// from the fp32 rows, the quaternion normalised, one rounding on store.
__global__ void __launch_bounds__(kMpT)
    map_points_kernel(const float* __restrict__ poses, const float* __restrict__ patches,
                      const float* __restrict__ intrinsics, const int64_t* __restrict__ ix,
                      float* __restrict__ points, int N, int P, int m,
                      const int32_t* __restrict__ m_dev, int cap) {
  const int count = m_dev ? min(max(*m_dev, 0), cap) : m;
  const int k = blockIdx.x * kMpT + threadIdx.x;
  if (k >= count) return;
  const int PP = P * P, centre = (P / 2) * P + P / 2;
  const int f = (int)min(max(ix[k], (int64_t)0), (int64_t)N - 1);
  const float* pk = patches + (size_t)k * 3 * PP + centre;
  const float* K = intrinsics + 4 * (size_t)f;
  const float* T = poses + 7 * (size_t)f;
  const double X[3] = {((double)pk[0] - (double)K[2]) / (double)K[0],
                       ((double)pk[PP] - (double)K[3]) / (double)K[1], 1.0};
  const double d = (double)pk[2 * PP];
  double q[4] = {(double)T[3], (double)T[4], (double)T[5], (double)T[6]};
  const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int c = 0; c < 4; c++) q[c] /= qn;
  // v = X - d t;  out = R^T v / d, with R^T the rotation by the conjugate
  const double v[3] = {X[0] - d * (double)T[0], X[1] - d * (double)T[1], X[2] - d * (double)T[2]};
  const double qx = -q[0], qy = -q[1], qz = -q[2], qw = q[3];
  const double ux = 2.0 * (qy * v[2] - qz * v[1]);
  const double uy = 2.0 * (qz * v[0] - qx * v[2]);
  const double uz = 2.0 * (qx * v[1] - qy * v[0]);
  const double Y[3] = {v[0] + qw * ux + (qy * uz - qz * uy), v[1] + qw * uy + (qz * ux - qx * uz),
                       v[2] + qw * uz + (qx * uy - qy * ux)};
  float* o = points + 3 * (size_t)k;
  o[0] = (float)(Y[0] / d);
  o[1] = (float)(Y[1] / d);
  o[2] = (float)(Y[2] / d);
}

}  // namespace tracker
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT int dpvo_frame_sample(const float* fmap, const float* imap, const float* image,
                                  const float* coords, void* gmap_ring, void* imap_ring,
                                  int ring_dtype, float* patches_out, uint8_t* colors, int h,
                                  int w, int H, int W, int C, int DIM, int M, int P, int res,
                                  int pmem, int N, int n, const int32_t* n_dev, void* stream) {
  if (!fmap || !imap || !image || !coords || !gmap_ring || !imap_ring || !patches_out || !colors)
    return DPVO_ERR_INVALID;
  if (h <= 0 || w <= 0 || H <= 0 || W <= 0 || C <= 0 || DIM <= 0 || M <= 0 || res <= 0 ||
      pmem <= 0 || N <= 0)
    return DPVO_ERR_INVALID;
  if (P < 1 || (P & 1) == 0 || P > h || P > w) return DPVO_ERR_INVALID;
  if (!n_dev && (n < 0 || n >= N)) return DPVO_ERR_INVALID;
  if (ring_dtype != DPVO_F32 && ring_dtype != DPVO_F16) return DPVO_ERR_UNSUPPORTED;
  // element indices inside one map / one ring row are ints
  if ((long long)(C > DIM ? C : DIM) * h * w >= (1ll << 31) || (long long)C * P * P >= (1ll << 31) ||
      (long long)3 * H * W >= (1ll << 31))
    return DPVO_ERR_UNSUPPORTED;
  tracker::FrameSample a;
  a.fmap = fmap;
  a.imap = imap;
  a.image = image;
  a.coords = coords;
  a.gmap_ring = gmap_ring;
  a.imap_ring = imap_ring;
  a.patches = patches_out;
  a.colors = colors;
  a.n_dev = n_dev;
  a.h = h; a.w = w; a.H = H; a.W = W; a.C = C; a.DIM = DIM; a.M = M; a.P = P;
  a.res = res; a.pmem = pmem; a.N = N; a.n = n;
  if (ring_dtype == DPVO_F16)
    hipLaunchKernelGGL(tracker::frame_sample_kernel<__half>, dim3((unsigned)M), dim3(kWave), 0,
                       as_stream(stream), a);
  else
    hipLaunchKernelGGL(tracker::frame_sample_kernel<float>, dim3((unsigned)M), dim3(kWave), 0,
                       as_stream(stream), a);
  return launch_status();
}

DPVO_EXPORT int dpvo_probe_median(const void* delta, int dtype, int M, float* out, void* stream) {
  if (!delta || !out || M <= 0) return DPVO_ERR_INVALID;
  if (dtype != DPVO_F32 && dtype != DPVO_F16) return DPVO_ERR_INVALID;
  if (M > tracker::kMedMax) return DPVO_ERR_UNSUPPORTED;
  const unsigned T = (unsigned)((M + kWave - 1) / kWave * kWave);
  if (dtype == DPVO_F16)
    hipLaunchKernelGGL(tracker::probe_median_kernel<__half>, dim3(1), dim3(T), 0,
                       as_stream(stream), reinterpret_cast<const __half*>(delta), M, out);
  else
    hipLaunchKernelGGL(tracker::probe_median_kernel<float>, dim3(1), dim3(T), 0,
                       as_stream(stream), reinterpret_cast<const float*>(delta), M, out);
  return launch_status();
}

DPVO_EXPORT int dpvo_update_targets(const float* coords, const void* delta, const void* w,
                                    int dtype, float* target, float* weight, int P, int E,
                                    const int32_t* E_dev, int cap, void* stream) {
  if (cap < 0 || (!E_dev && (E < 0 || E > cap))) return DPVO_ERR_INVALID;
  if (P < 1 || (P & 1) == 0) return DPVO_ERR_INVALID;
  if (dtype != DPVO_F32 && dtype != DPVO_F16) return DPVO_ERR_INVALID;
  const int launch = E_dev ? cap : E;
  if (launch == 0) return DPVO_OK;
  if (!coords || !delta || !w || !target || !weight) return DPVO_ERR_INVALID;
  if ((long long)launch * 2 >= (1ll << 31)) return DPVO_ERR_UNSUPPORTED;
  const unsigned grid = (unsigned)((2 * launch + tracker::kUtT - 1) / tracker::kUtT);
  if (dtype == DPVO_F16)
    hipLaunchKernelGGL(tracker::update_targets_kernel<__half>, dim3(grid), dim3(tracker::kUtT), 0,
                       as_stream(stream), coords, reinterpret_cast<const __half*>(delta),
                       reinterpret_cast<const __half*>(w), target, weight, P, E, E_dev, cap);
  else
    hipLaunchKernelGGL(tracker::update_targets_kernel<float>, dim3(grid), dim3(tracker::kUtT), 0,
                       as_stream(stream), coords, reinterpret_cast<const float*>(delta),
                       reinterpret_cast<const float*>(w), target, weight, P, E, E_dev, cap);
  return launch_status();
}

DPVO_EXPORT int dpvo_map_points(const float* poses, const float* patches, const float* intrinsics,
                                const int64_t* ix, float* points, int N, int P, int m,
                                const int32_t* m_dev, int cap, void* stream) {
  if (cap < 0 || (!m_dev && (m < 0 || m > cap))) return DPVO_ERR_INVALID;
  if (N <= 0 || P < 1 || (P & 1) == 0) return DPVO_ERR_INVALID;
  const int launch = m_dev ? cap : m;
  if (launch == 0) return DPVO_OK;
  if (!poses || !patches || !intrinsics || !ix || !points) return DPVO_ERR_INVALID;
  const unsigned grid = (unsigned)((launch + tracker::kMpT - 1) / tracker::kMpT);
  hipLaunchKernelGGL(tracker::map_points_kernel, dim3(grid), dim3(tracker::kMpT), 0,
                     as_stream(stream), poses, patches, intrinsics, ix, points, N, P, m, m_dev,
                     cap);
  return launch_status();
}
