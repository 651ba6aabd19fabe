// evaluate.hip -- the back of a run on a sequence: the absolute trajectory
// error of DPVO.terminate's output against a ground-truth trajectory, as
// evaluate_euroc.py:109-119 takes it from evo (associate by timestamp, Sim(3)
// Umeyama alignment, RMSE of the translation error), on the device.
//
// One launch of one workgroup, no host read, no float atomics:
//   associate  every stamp of the shorter trajectory looks up the nearest stamp
//              of the longer one by binary search (ties: the lower index); the
//              pairs within max_diff are compacted in order, a block scan per
//              chunk of kThreads stamps
//   align      means, then centred covariance and variance of the matched
//              points, each reduced in a fixed tree order in fp64 (xor tree in
//              the wave, waves in ascending order); umeyama.hpp gives c, R, t
//   errors     e_i = |c R x_i + t - y_i| to the workspace; sum, squares,
//              min, max; a second pass for the population deviation
//   median     exact: an 8-pass radix select over the bit patterns of the
//              (non-negative) errors, once per middle rank
// Every reduction has a fixed order: two runs give identical bytes.
#include <math.h>

#include "common.hpp"
#include "umeyama.hpp"

namespace dpvo {
namespace evaluate {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxStamps = 65536;

struct Ate {
  const void* est_xyz;
  const double* est_t;
  const double* ref_xyz;
  const double* ref_t;
  double* stats;
  double* model;
  int32_t* pairs;
  int32_t* status;
  double* err;
  double max_diff;
  int n, m, align;
};

// sum of K doubles per thread over the workgroup in a fixed order; every
// thread gets the result.  red: kWaves * K doubles.
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
    for (int ww = 1; ww < kWaves; ww++) s += red[ww * K + k];
    v[k] = s;
  }
}

// min of v over the workgroup (max: negate); a NaN is the caller's to flag
__device__ __forceinline__ double block_min(double v, double* red) {
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, kWave));
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  v = red[0];
  for (int ww = 1; ww < kWaves; ww++) v = fmin(v, red[ww]);
  return v;
}

// first index in [0, len) with a[index] >= key (len when there is none)
__device__ __forceinline__ int lower_bound(const double* __restrict__ a, int len, double key) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// the value of sorted rank `rank` among err[0, count): err >= 0, so the bit
// patterns order like the values.  hist: 256 ints, sel: 2 x 64-bit words.
__device__ double select_rank(const double* __restrict__ err, int count, int rank, int* hist,
                              int* wtot, unsigned long long* sel) {
  const int tid = threadIdx.x;
  unsigned long long prefix = 0;
  __syncthreads();
  if (tid == 0) {
    sel[0] = 0;
    sel[1] = (unsigned long long)rank;
  }
#pragma unroll 1
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 56 - 8 * pass;
    const unsigned long long himask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < count; i += kThreads) {
      const unsigned long long k = (unsigned long long)__double_as_longlong(err[i]);
      if ((k & himask) == prefix) atomicAdd(&hist[(int)((k >> shift) & 255ull)], 1);
    }
    __syncthreads();
    // exclusive scan of the 256 bins by the first four waves; the bin holding the rank is selected
    const int c = tid < 256 ? hist[tid] : 0;
    const int incl = wave_incl_sum(c);
    if (tid < 256 && (tid & 63) == 63) wtot[tid >> 6] = incl;
    __syncthreads();
    int excl = incl - c;
    for (int w = 0; w < (tid >> 6) && w < 4; w++) excl += wtot[w];
    const int r = (int)sel[1];
    __syncthreads();  // every thread has read the rank
    if (tid < 256 && c > 0 && r >= excl && r < excl + c) {
      sel[0] = prefix | ((unsigned long long)tid << shift);
      sel[1] = (unsigned long long)(r - excl);
    }
    __syncthreads();
    prefix = sel[0];
  }
  return __longlong_as_double((long long)prefix);
}

template <typename S>
__global__ void __launch_bounds__(kThreads) trajectory_ate_kernel(Ate a) {
  __shared__ double red[kWaves * 10];
  __shared__ double smodel[13];
  __shared__ int scr[kWaves + 1];
  __shared__ int hist[256];
  __shared__ int wtot[4];
  __shared__ unsigned long long sel[2];
  __shared__ int sflag;
  const int tid = threadIdx.x;
  const S* __restrict__ ex = (const S*)a.est_xyz;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const bool est_long = a.n > a.m;
  const double* __restrict__ lt = est_long ? a.est_t : a.ref_t;
  const double* __restrict__ st = est_long ? a.ref_t : a.est_t;
  const int nl = est_long ? a.n : a.m, ns = est_long ? a.m : a.n;

  // ---- both stamp arrays non-decreasing (a NaN stamp counts as unsorted) ----
  int bad = 0;
  for (int i = tid; i + 1 < a.n; i += kThreads) bad |= !(a.est_t[i] <= a.est_t[i + 1]);
  for (int i = tid; i + 1 < a.m; i += kThreads) bad |= !(a.ref_t[i] <= a.ref_t[i + 1]);
  if (a.n == 1 && tid == 0) bad |= a.est_t[0] != a.est_t[0];
  if (a.m == 1 && tid == 0) bad |= a.ref_t[0] != a.ref_t[0];
  const int unsorted = __syncthreads_or(bad);

  // ---- association, compacted in short-side order ----
  int count = 0;
  if (!unsorted) {
    for (int base = 0; base < ns; base += kThreads) {
      const int s = base + tid;
      int keep = 0, l = 0;
      if (s < ns) {
        const double ts = st[s];
        const int j = lower_bound(lt, nl, ts);  // lt[j - 1] < ts <= lt[j]
        const double dhi = j < nl ? fabs(lt[j] - ts) : INFINITY;
        const double dlo = j > 0 ? fabs(lt[j - 1] - ts) : INFINITY;
        double dt;
        // a tie goes to the lower index: the first of the equal stamps below
        if (j > 0 && (j >= nl || dlo <= dhi)) {
          dt = dlo;
          l = lower_bound(lt, nl, lt[j - 1]);
        } else {
          dt = dhi;
          l = j;
        }
        keep = dt <= a.max_diff ? 1 : 0;
      }
      int total;
      const int off = block_excl_sum(keep, scr, total);
      if (keep) {
        a.pairs[2 * (size_t)(count + off)] = est_long ? l : s;
        a.pairs[2 * (size_t)(count + off) + 1] = est_long ? s : l;
      }
      count += total;
    }
  }
  for (int i = count + tid; i < ns; i += kThreads) {
    a.pairs[2 * (size_t)i] = -1;
    a.pairs[2 * (size_t)i + 1] = -1;
  }
  __syncthreads();  // the pairs of other threads are read from here on

  // ---- alignment ----
  int status = (unsorted ? 4 : 0) | (count < 3 ? 1 : 0);
  if (tid == 0) {
#pragma unroll
    for (int e = 0; e < 9; e++) smodel[e] = (e % 4 == 0) ? 1.0 : 0.0;
    smodel[9] = smodel[10] = smodel[11] = 0.0;
    smodel[12] = 1.0;
    sflag = 0;
  }
  if (status == 0 && a.align) {
    double s1[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < count; i += kThreads) {
      const int ie = a.pairs[2 * (size_t)i], ir = a.pairs[2 * (size_t)i + 1];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        s1[r] += (double)ex[(size_t)ie * 3 + r];
        s1[3 + r] += a.ref_xyz[(size_t)ir * 3 + r];
      }
    }
    block_sum<6>(s1, red);
    const double cn = (double)count;
    double mx[3], my[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      mx[r] = s1[r] / cn;
      my[r] = s1[3 + r] / cn;
    }
    double b[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < count; i += kThreads) {
      const int ie = a.pairs[2 * (size_t)i], ir = a.pairs[2 * (size_t)i + 1];
      double xr[3], yr[3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        xr[r] = (double)ex[(size_t)ie * 3 + r] - mx[r];
        yr[r] = a.ref_xyz[(size_t)ir * 3 + r] - my[r];
        b[9] += xr[r] * xr[r];
      }
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) b[r * 3 + c] += yr[r] * xr[c];
    }
    block_sum<10>(b, red);
    if (tid == 0) {
      double cov[9];
#pragma unroll
      for (int e = 0; e < 9; e++) cov[e] = b[e] / cn;
      const umeyama::Model f = umeyama::umeyama_from_moments(mx, my, b[9] / cn, cov);
      if (f.ok) {
#pragma unroll
        for (int e = 0; e < 9; e++) smodel[e] = f.R[e];
#pragma unroll
        for (int e = 0; e < 3; e++) smodel[9 + e] = f.t[e];
        smodel[12] = f.c;
      } else {
        sflag = 2;
      }
    }
  }
  __syncthreads();
  status |= sflag;
  if (tid < 13) a.model[tid] = smodel[tid];
  if (tid == 0) a.status[0] = status;
  if (status != 0) {
    if (tid < 7) a.stats[tid] = nan;
    if (tid == 7) a.stats[7] = (double)count;
    return;
  }

  // ---- errors ----
  double R[9], t[3];
#pragma unroll
  for (int e = 0; e < 9; e++) R[e] = smodel[e];
#pragma unroll
  for (int e = 0; e < 3; e++) t[e] = smodel[9 + e];
  const double c = smodel[12];
  double s2[2] = {0, 0};
  double emin = INFINITY, emax = -INFINITY;
  int isnan_ = 0;
  for (int i = tid; i < count; i += kThreads) {
    const int ie = a.pairs[2 * (size_t)i], ir = a.pairs[2 * (size_t)i + 1];
    const double x0 = (double)ex[(size_t)ie * 3], x1 = (double)ex[(size_t)ie * 3 + 1],
                 x2 = (double)ex[(size_t)ie * 3 + 2];
    double sq = 0.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double d = c * (R[r * 3] * x0 + R[r * 3 + 1] * x1 + R[r * 3 + 2] * x2) + t[r] -
                       a.ref_xyz[(size_t)ir * 3 + r];
      sq += d * d;
    }
    const double e = sqrt(sq);
    a.err[i] = e;
    s2[0] += e;
    s2[1] += sq;
    emin = fmin(emin, e);
    emax = fmax(emax, e);
    isnan_ |= e != e;
  }
  const int any_nan = __syncthreads_or(isnan_);  // also publishes err[] to the workgroup
  block_sum<2>(s2, red);
  emin = block_min(emin, red);
  emax = -block_min(-emax, red);
  const double cn = (double)count, mean = s2[0] / cn;
  double s3[1] = {0};
  for (int i = tid; i < count; i += kThreads) {
    const double d = a.err[i] - mean;
    s3[0] += d * d;
  }
  block_sum<1>(s3, red);
  double med = nan;
  if (!any_nan) {
    med = select_rank(a.err, count, count / 2, hist, wtot, sel);
    if ((count & 1) == 0)
      med = 0.5 * (select_rank(a.err, count, count / 2 - 1, hist, wtot, sel) + med);
  }
  if (tid == 0) {
    a.stats[0] = sqrt(s2[1] / cn);
    a.stats[1] = mean;
    a.stats[2] = med;
    a.stats[3] = sqrt(s3[0] / cn);
    a.stats[4] = any_nan ? nan : emin;
    a.stats[5] = any_nan ? nan : emax;
    a.stats[6] = s2[1];
    a.stats[7] = cn;
  }
}

}  // namespace evaluate
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT size_t dpvo_trajectory_ate_workspace_bytes(int n, int m) {
  const int s = n < m ? n : m;
  return sizeof(double) * (size_t)(s > 1 ? s : 1);
}

DPVO_EXPORT int dpvo_trajectory_ate(const void* est_xyz, int est_dtype, const double* est_t, int n,
                                    const double* ref_xyz, const double* ref_t, int m,
                                    double max_diff, int align, double* stats, double* model,
                                    int32_t* pairs, int32_t* status, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (!est_xyz || !est_t || !ref_xyz || !ref_t || !stats || !model || !pairs || !status ||
      !workspace)
    return DPVO_ERR_INVALID;
  if (n <= 0 || m <= 0 || !(max_diff >= 0.0) || align < 0 || align > 1) return DPVO_ERR_INVALID;
  if (est_dtype != DPVO_F32 && est_dtype != DPVO_F64) return DPVO_ERR_UNSUPPORTED;
  if (n > evaluate::kMaxStamps || m > evaluate::kMaxStamps) return DPVO_ERR_UNSUPPORTED;
  if (workspace_bytes < dpvo_trajectory_ate_workspace_bytes(n, m)) return DPVO_ERR_WORKSPACE;
  evaluate::Ate a;
  a.est_xyz = est_xyz;
  a.est_t = est_t;
  a.ref_xyz = ref_xyz;
  a.ref_t = ref_t;
  a.stats = stats;
  a.model = model;
  a.pairs = pairs;
  a.status = status;
  a.err = (double*)workspace;
  a.max_diff = max_diff;
  a.n = n;
  a.m = m;
  a.align = align;
  hipStream_t s = as_stream(stream);
  if (est_dtype == DPVO_F32)
    hipLaunchKernelGGL(evaluate::trajectory_ate_kernel<float>, dim3(1),
                       dim3(evaluate::kThreads), 0, s, a);
  else
    hipLaunchKernelGGL(evaluate::trajectory_ate_kernel<double>, dim3(1),
                       dim3(evaluate::kThreads), 0, s, a);
  return launch_status();
}
