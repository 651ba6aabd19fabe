// RANSAC over 3-point Umeyama models and the refit on the winner's inliers
// (loop-closure measurement, dpvo/loop_closure/optim_utils.py:64-150, where it
// is numba on the CPU over points copied off the GPU).
//
// Two launches, no atomics on floats, no host read:
//   score:  one wave per hypothesis.  Every lane forms the Umeyama model of
//           the hypothesis' three points in fp64 (the same few hundred
//           operations in all 64 lanes: no divergence, no broadcast), then the
//           lanes stride over the N points and count |c R x + t - y| <
//           threshold; the count goes to counts[h], -1 for a degenerate sample.
//   select: one workgroup.  It replays the reference's sequential loop on
//           counts[]: stop = first h with counts[h] > early_exit (else H - 1),
//           winner = lowest h <= stop with the largest positive count.  It
//           recomputes the winner's model with the code of the score launch
//           (so the mask has exactly counts[winner] points), writes the inlier
//           mask and refits Umeyama on the inliers in two passes (means, then
//           centred covariance and variance), each reduced in a fixed tree
//           order: bit-identical from run to run.
//
// The fit itself (one-sided Jacobi SVD completed by cross products) is
// umeyama.hpp, shared with the trajectory evaluation.
#include "common.hpp"
#include "umeyama.hpp"

namespace dpvo {
namespace {

constexpr int kSelectThreads = 256;
using umeyama::Model;
using umeyama::umeyama_from_moments;

// model of the three points smp[3]; an index outside [0, N) gives no model
// (the extension validates the samples; nothing is ever read out of range)
template <typename S>
__device__ inline Model sample_model(const S* __restrict__ src, const S* __restrict__ dst, int N,
                                     const int32_t* __restrict__ smp) {
  double x[3][3], y[3][3];
  bool in_range = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int p = smp[k];
    in_range = in_range && p >= 0 && p < N;
    const int pc = min(max(p, 0), N - 1);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      x[k][r] = (double)src[(size_t)pc * 3 + r];
      y[k][r] = (double)dst[(size_t)pc * 3 + r];
    }
  }
  double mx[3], my[3], cov[9], sx = 0.0;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    mx[r] = (x[0][r] + x[1][r] + x[2][r]) / 3.0;
    my[r] = (y[0][r] + y[1][r] + y[2][r]) / 3.0;
  }
#pragma unroll
  for (int e = 0; e < 9; e++) cov[e] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double xr = x[k][r] - mx[r];
      sx += xr * xr;
#pragma unroll
      for (int c = 0; c < 3; c++) cov[c * 3 + r] += (y[k][c] - my[c]) * xr;
    }
#pragma unroll
  for (int e = 0; e < 9; e++) cov[e] /= 3.0;
  Model m = umeyama_from_moments(mx, my, sx / 3.0, cov);
  m.ok = m.ok && in_range;
  return m;
}

template <typename S>
__device__ __forceinline__ bool is_inlier(const Model& m, const S* __restrict__ src,
                                          const S* __restrict__ dst, int p, double threshold) {
  const double x0 = (double)src[(size_t)p * 3], x1 = (double)src[(size_t)p * 3 + 1],
               x2 = (double)src[(size_t)p * 3 + 2];
  double sq = 0.0;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double e = m.c * (m.R[r * 3] * x0 + m.R[r * 3 + 1] * x1 + m.R[r * 3 + 2] * x2) + m.t[r] -
                     (double)dst[(size_t)p * 3 + r];
    sq += e * e;
  }
  return sqrt(sq) < threshold;
}

template <typename S>
__global__ void __launch_bounds__(kWave)
    ransac_score_kernel(const S* __restrict__ src, const S* __restrict__ dst, int N,
                        const int32_t* __restrict__ samples, int H, double threshold,
                        int32_t* __restrict__ counts) {
  const int h = blockIdx.x, lane = threadIdx.x;
  if (h >= H) return;
  const Model m = sample_model(src, dst, N, samples + (size_t)h * 3);
  int cnt = 0;
  if (m.ok)
    for (int p = lane; p < N; p += kWave) cnt += is_inlier(m, src, dst, p, threshold) ? 1 : 0;
  cnt = wave_sum_i(cnt);
  if (lane == 0) counts[h] = m.ok ? cnt : -1;
}

// sum of K doubles per thread over the workgroup, fixed order: xor tree in
// each wave, then the waves in ascending order.  red: kSelectThreads / 64 * K.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red) {
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = wave_sum(v[k]);
  __syncthreads();  // red may still be read from the previous call
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; k++) red[w * K + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; k++) {
    double s = red[k];
    for (int ww = 1; ww < kSelectThreads / kWave; ww++) s += red[ww * K + k];
    v[k] = s;
  }
}

__device__ __forceinline__ long long block_max_ll(long long x, long long* red) {
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long y = __shfl_xor(x, o, kWave);
    x = y > x ? y : x;
  }
  __syncthreads();
  if (lane == 0) red[w] = x;
  __syncthreads();
  x = red[0];
  for (int ww = 1; ww < kSelectThreads / kWave; ww++) x = red[ww] > x ? red[ww] : x;
  return x;
}

// rotation matrix -> unit quaternion (x, y, z, w), w >= 0: the largest of the
// four squared components is formed first, so no branch divides by a small number
__device__ inline void quat_of(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    w = 1.0 + tr;
    x = R[7] - R[5];
    y = R[2] - R[6];
    z = R[3] - R[1];
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    x = 1.0 + R[0] - R[4] - R[8];
    y = R[1] + R[3];
    z = R[2] + R[6];
    w = R[7] - R[5];
  } else if (R[4] >= R[8]) {
    x = R[1] + R[3];
    y = 1.0 - R[0] + R[4] - R[8];
    z = R[5] + R[7];
    w = R[2] - R[6];
  } else {
    x = R[2] + R[6];
    y = R[5] + R[7];
    z = 1.0 - R[0] - R[4] + R[8];
    w = R[3] - R[1];
  }
  const double sg = w < 0.0 ? -1.0 : 1.0;
  const double inv = sg / sqrt(x * x + y * y + z * z + w * w);
  q[0] = x * inv;
  q[1] = y * inv;
  q[2] = z * inv;
  q[3] = w * inv;
}

__device__ inline void write_model(double* __restrict__ model, const double* R, const double* t,
                                   double s) {
  for (int e = 0; e < 9; e++) model[e] = R[e];
  for (int e = 0; e < 3; e++) model[9 + e] = t[e];
  model[12] = s;
  double q[4];
  quat_of(R, q);
  for (int e = 0; e < 3; e++) model[13 + e] = t[e];
  for (int e = 0; e < 4; e++) model[16 + e] = q[e];
  model[20] = s;
}

template <typename S>
__global__ void __launch_bounds__(kSelectThreads)
    ransac_select_kernel(const S* __restrict__ src, const S* __restrict__ dst, int N,
                         const int32_t* __restrict__ samples, int H, double threshold,
                         int early_exit, const int32_t* __restrict__ counts,
                         double* __restrict__ model, int32_t* __restrict__ info,
                         uint8_t* __restrict__ mask) {
  __shared__ double red[kSelectThreads / kWave * 10];
  __shared__ long long redl[kSelectThreads / kWave];
  const int tid = threadIdx.x;
  const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, zero3[3] = {0, 0, 0};

  // stop: the first hypothesis whose count exceeds early_exit ends the loop
  long long key = -(long long)(H - 1);
  for (int h = tid; h < H; h += kSelectThreads)
    if (counts[h] > early_exit && -(long long)h > key) key = -(long long)h;
  const int stop = (int)-block_max_ll(key, redl);
  // winner: largest count, lowest index (the reference replaces only on >)
  key = 0;
  for (int h = tid; h <= stop; h += kSelectThreads) {
    const int c = counts[h];
    const long long k = ((long long)c << 32) | (long long)(0x7fffffff - h);
    if (c > 0 && k > key) key = k;
  }
  key = block_max_ll(key, redl);
  const int best = (int)(key >> 32);
  const int win = best > 0 ? 0x7fffffff - (int)(key & 0x7fffffff) : -1;
  if (win < 0) {  // status 1: nothing to fit
    for (int p = tid; p < N; p += kSelectThreads) mask[p] = 0;
    if (tid == 0) {
      write_model(model, ident, zero3, 1.0);
      info[0] = 0;
      info[1] = -1;
      info[2] = stop;
      info[3] = 1;
    }
    return;
  }

  const Model m = sample_model(src, dst, N, samples + (size_t)win * 3);
  // pass 1: mask, number of inliers and the sums of the means
  double a[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int p = tid; p < N; p += kSelectThreads) {
    const bool in = m.ok && is_inlier(m, src, dst, p, threshold);
    mask[p] = in ? 1 : 0;
    if (in) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        a[r] += (double)src[(size_t)p * 3 + r];
        a[3 + r] += (double)dst[(size_t)p * 3 + r];
      }
      a[6] += 1.0;
    }
  }
  block_sum<7>(a, red);
  const double n = a[6];
  double mx[3], my[3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    mx[r] = a[r] / n;
    my[r] = a[3 + r] / n;
  }
  // pass 2: centred covariance and variance (each thread rereads its own mask bytes)
  double b[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int p = tid; p < N; p += kSelectThreads) {
    if (!mask[p]) continue;
    double xr[3], yr[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      xr[r] = (double)src[(size_t)p * 3 + r] - mx[r];
      yr[r] = (double)dst[(size_t)p * 3 + r] - my[r];
      b[9] += xr[r] * xr[r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) b[r * 3 + c] += yr[r] * xr[c];
  }
  block_sum<10>(b, red);
  if (tid != 0) return;
  double cov[9];
#pragma unroll
  for (int e = 0; e < 9; e++) cov[e] = b[e] / n;
  const Model f = umeyama_from_moments(mx, my, b[9] / n, cov);
  if (f.ok)
    write_model(model, f.R, f.t, f.c);
  else
    write_model(model, ident, zero3, 1.0);
  info[0] = (int)n;
  info[1] = win;
  info[2] = stop;
  info[3] = f.ok ? 0 : 2;
}

size_t counts_bytes(int H) { return (((size_t)(H > 0 ? H : 0) * sizeof(int32_t)) + 255) & ~(size_t)255; }

template <typename S>
int launch_ransac(const void* src, const void* dst, int N, const int32_t* samples, int H,
                  double threshold, int early_exit, double* model, int32_t* info, uint8_t* mask,
                  int32_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL((ransac_score_kernel<S>), dim3((unsigned)H), dim3(kWave), 0, stream,
                     (const S*)src, (const S*)dst, N, samples, H, threshold, counts);
  hipLaunchKernelGGL((ransac_select_kernel<S>), dim3(1), dim3(kSelectThreads), 0, stream,
                     (const S*)src, (const S*)dst, N, samples, H, threshold, early_exit, counts,
                     model, info, mask);
  return launch_status();
}

}  // namespace
}  // namespace dpvo

DPVO_EXPORT size_t dpvo_ransac_umeyama_workspace_bytes(int N, int H) {
  if (N < 3 || H < 1) return 0;
  return dpvo::counts_bytes(H);
}

DPVO_EXPORT int dpvo_ransac_umeyama(const void* src, const void* dst, int N, int dtype,
                                    const int32_t* samples, int H, double threshold,
                                    int early_exit, double* model, int32_t* info,
                                    uint8_t* inlier_mask, void* ws, size_t ws_bytes,
                                    void* stream) {
  if (!src || !dst || !samples || !model || !info || !inlier_mask || !ws || N < 3 || H < 1 ||
      !(threshold > 0.0))
    return DPVO_ERR_INVALID;
  if (dtype != DPVO_F32 && dtype != DPVO_F64) return DPVO_ERR_UNSUPPORTED;
  if (H > (1 << 24) || N > (1 << 28)) return DPVO_ERR_UNSUPPORTED;
  if (ws_bytes < dpvo::counts_bytes(H)) return DPVO_ERR_WORKSPACE;
  hipStream_t s = dpvo::as_stream(stream);
  int32_t* counts = (int32_t*)ws;  // counts[H] is the whole workspace
  if (dtype == DPVO_F32)
    return dpvo::launch_ransac<float>(src, dst, N, samples, H, threshold, early_exit, model, info,
                                      inlier_mask, counts, s);
  return dpvo::launch_ransac<double>(src, dst, N, samples, H, threshold, early_exit, model, info,
                                     inlier_mask, counts, s);
}
