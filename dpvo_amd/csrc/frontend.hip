// frontend.hip -- the head of DPVO.__call__ (dpvo/dpvo.py:931-965) and the
// trajectory read-out of DPVO.terminate / get_pose (dpvo.py:385-417) on gfx950.
//
// dpvo_frame_init: one launch of one workgroup seeds the new frame: timestamp
// index, intrinsics / RES, the pose from the motion model and the patches with
// their depth set to the median depth of the last three frames.  The
// reference spends about eight lietorch launches and a sort (torch.median) on
// it; here the median is a radix select (no sort) and n / counter may be
// device scalars, so the call replays from a captured graph.
//
// dpvo_trajectory: get_pose(t) for every t in [0, counter) from the keyframe
// poses and the pg.delta log that dpvo_kf_shift records.  The reference
// recurses in Python, one lietorch call per frame; here the chains are
// followed by pointer jumping, 2 + ceil(log2(counter)) launches in all.
//
// All group arithmetic is fp64 (lie_se3.hpp instantiated for double): fp32
// rows are loaded, the quaternion normalised in fp64, and the result rounded
// to fp32 once, on store.
#include <math.h>

#include "common.hpp"
#include "lie_se3.hpp"
#include "radix_select.hpp"

namespace dpvo {
namespace frontend {

using G = lie::SE3g<double>;

__device__ __forceinline__ G load_pose(const float* __restrict__ p) {
  double d[7];
#pragma unroll
  for (int c = 0; c < 7; c++) d[c] = (double)p[c];
  return lie::se3_load<double>(d);
}
__device__ __forceinline__ G load_pose(const double* __restrict__ p) {
  G g;
  g.t[0] = p[0]; g.t[1] = p[1]; g.t[2] = p[2];
  g.q = {p[3], p[4], p[5], p[6]};  // workspace rows are normalised already
  return g;
}
__device__ __forceinline__ void store_pose(const G& g, double* __restrict__ p) {
  p[0] = g.t[0]; p[1] = g.t[1]; p[2] = g.t[2];
  p[3] = g.q.x; p[4] = g.q.y; p[5] = g.q.z; p[6] = g.q.w;
}
__device__ __forceinline__ void store_pose(const G& g, float* __restrict__ p) {
  p[0] = (float)g.t[0]; p[1] = (float)g.t[1]; p[2] = (float)g.t[2];
  p[3] = (float)g.q.x; p[4] = (float)g.q.y; p[5] = (float)g.q.z; p[6] = (float)g.q.w;
}

// ---- frame init ---------------------------------------------------------------
constexpr int kFiT = 256;

struct FrameInit {
  float* poses;
  float* patches;
  float* intrinsics;
  int64_t* tstamps;
  const double* times;
  const float* new_patches;
  const float* new_intrinsics;
  const int32_t* n_dev;
  const int32_t* counter_dev;
  int N, M, P, times_cap, n, counter, motion_model, median;
  double damping;
  float res;
};

// dpvo.py:943-957.  Thread-serial: a handful of fp64 group operations.
__device__ void seed_pose(const FrameInit& a, int n, int counter) {
  float* out = a.poses + 7 * (size_t)n;
  const float* p1 = a.poses + 7 * (size_t)(n - 1);
  if (a.motion_model == 0) {
#pragma unroll
    for (int c = 0; c < 7; c++) out[c] = p1[c];
    return;
  }
  // *_, a, b, c = [1] * 3 + tlist (dpvo.py:949): missing times read as 1
  double t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int i = counter - 2 + k;
    t[k] = i >= 0 ? a.times[i] : 1.0;
  }
  const double den = t[1] - t[0];
  const double fac = den == 0.0 ? 1.0 : (t[2] - t[1]) / den;  // the reference raises at b == a
  const G P1 = load_pose(p1), P2 = load_pose(a.poses + 7 * (size_t)(n - 2));
  double xi[6];
  lie::se3_log(lie::se3_mul(P1, lie::se3_inv(P2)), xi);
  const double s = a.damping * fac;
#pragma unroll
  for (int c = 0; c < 6; c++) xi[c] *= s;
  store_pose(lie::se3_mul(lie::se3_exp(xi), P1), out);
}

__global__ void __launch_bounds__(kFiT) frame_init_kernel(FrameInit a) {
  __shared__ RadixSelectLds sel;
  __shared__ int any_nan;
  const int tid = threadIdx.x;
  const int n = a.n_dev ? *a.n_dev : a.n;
  const int counter = a.counter_dev ? *a.counter_dev : a.counter;
  // host values were validated before the launch; device values outside the
  // buffers leave everything untouched
  if (n < 0 || n >= a.N || counter < 0 || counter >= a.times_cap) return;
  const int PP = a.P * a.P;

  if (tid == 0) {
    a.tstamps[n] = counter;
    if (n > 1) seed_pose(a, n, counter);
    any_nan = 0;
  }
  if (tid >= kWave && tid < kWave + 4)
    a.intrinsics[4 * (size_t)n + (tid - kWave)] = a.new_intrinsics[tid - kWave] / a.res;

  // ---- lower median of the depths of frames [max(n - 3, 0), n): radix select ----
  const bool med = a.median && n >= 1;
  float s = 0.f;
  if (med) {
    const int f0 = max(n - 3, 0);
    const int count = (n - f0) * a.M * PP;
    const float* base = a.patches + (size_t)f0 * a.M * 3 * PP + 2 * PP;  // channel 2 of patch f0 M
    bool nan = false;
    const uint32_t key = block_radix_select(count, (count - 1) / 2, [&](int i) {
      const int patch = i / PP, pix = i - patch * PP;
      const float v = base[(size_t)patch * 3 * PP + pix];
      nan |= v != v;
      return float_key(v);
    }, sel);
    if (nan) any_nan = 1;
    __syncthreads();
    s = any_nan ? __uint_as_float(0x7fc00000u) : key_float(key);
  }

  // ---- patches_[n] = patches, depth channel replaced by the median ----
  float* dst = a.patches + (size_t)n * a.M * 3 * PP;
  const int total = a.M * 3 * PP;
  for (int i = tid; i < total; i += kFiT) {
    const int ch = (i / PP) % 3;
    dst[i] = (med && ch == 2) ? s : a.new_patches[i];
  }
}

// ---- trajectory ---------------------------------------------------------------
// Workspace (128 bytes per frame): T[2][counter][7] fp64, then int32 tables
// par[2][counter], rec[counter], kfi[counter].
//   rec[t]  index of the last valid pg.delta record with t1 == t, or -1
//   kfi[t]  largest i < n with tstamps[i] == t, or -1
//   par[t]  >= 0: pose(t) = T[t] * pose(par[t]), still to be followed;
//           <  0: T[t] is pose(t), hanging on keyframe -par[t] - 2 (-1: unresolved)
constexpr int kTrT = 256;
constexpr int kTrScatterT = 1024;

struct TrajWs {
  double* T[2];
  int* par[2];
  int* rec;
  int* kfi;
};
__host__ __device__ inline TrajWs traj_ws(void* ws, int counter) {
  TrajWs w;
  const size_t C = (size_t)counter;
  w.T[0] = reinterpret_cast<double*>(ws);
  w.T[1] = w.T[0] + 7 * C;
  w.par[0] = reinterpret_cast<int*>(w.T[1] + 7 * C);
  w.par[1] = w.par[0] + C;
  w.rec = w.par[1] + C;
  w.kfi = w.rec + C;
  return w;
}

// One workgroup: reset the tables, then scatter the records and the keyframes
// with atomicMax (the last record in log order and the last keyframe row win,
// as later dict assignments do).
__global__ void __launch_bounds__(kTrScatterT)
    traj_scatter_kernel(const int64_t* __restrict__ tstamps, int n_host,
                        const int32_t* __restrict__ n_dev, int N,
                        const int64_t* __restrict__ pairs, const int32_t* __restrict__ count,
                        int cap, int counter, int* __restrict__ rec, int* __restrict__ kfi,
                        int32_t* __restrict__ info) {
  const int tid = threadIdx.x;
  for (int t = tid; t < counter; t += kTrScatterT) {
    rec[t] = -1;
    kfi[t] = -1;
  }
  if (tid < 2) info[tid] = 0;
  __threadfence();
  __syncthreads();
  const int n = min(max(n_dev ? *n_dev : n_host, 0), N);
  const int cnt = min(max(*count, 0), cap);
  int ignored = 0;
  for (int r = tid; r < cnt; r += kTrScatterT) {
    const int64_t t1 = pairs[2 * (size_t)r], t0 = pairs[2 * (size_t)r + 1];
    if (t0 >= t1 || t0 < 0 || t1 >= counter)
      ignored++;
    else
      atomicMax(&rec[t1], r);
  }
  for (int i = tid; i < n; i += kTrScatterT) {
    const int64_t t = tstamps[i];
    if (t >= 0 && t < counter) atomicMax(&kfi[t], i);
  }
  ignored = wave_sum_i(ignored);
  if ((tid & 63) == 0 && ignored) atomicAdd(&info[1], ignored);
}

// traj[t] / root[t] from a finished entry (par < 0)
__device__ __forceinline__ void traj_emit(int t, const G& g, int par, int inverse,
                                          float* __restrict__ traj, int64_t* __restrict__ root,
                                          int32_t* __restrict__ info) {
  const int r = par < 0 ? -par - 2 : -1;
  const bool bad = r < 0;
  float* o = traj + 7 * (size_t)t;
  if (bad) {
#pragma unroll
    for (int c = 0; c < 7; c++) o[c] = __uint_as_float(0x7fc00000u);
  } else {
    store_pose(inverse ? lie::se3_inv(g) : g, o);
  }
  root[t] = r;
  const int nbad = __popcll(__ballot(bad));
  if (bad && (__ffsll((long long)__ballot(bad)) - 1) == (int)(threadIdx.x & 63))
    atomicAdd(&info[0], nbad);
}

__global__ void __launch_bounds__(kTrT)
    traj_build_kernel(const float* __restrict__ poses, const float* __restrict__ dlog,
                      const int64_t* __restrict__ pairs, int counter, const int* __restrict__ rec,
                      const int* __restrict__ kfi, double* __restrict__ T, int* __restrict__ par,
                      int last, int inverse, float* __restrict__ traj, int64_t* __restrict__ root,
                      int32_t* __restrict__ info) {
  const int t = blockIdx.x * kTrT + threadIdx.x;
  if (t >= counter) return;
  const int k = kfi[t], r = rec[t];
  G g;
  int p;
  if (k >= 0) {  // `if t in self.traj` comes first (dpvo.py:386)
    g = load_pose(poses + 7 * (size_t)k);
    p = -k - 2;
  } else if (r >= 0) {
    g = load_pose(dlog + 7 * (size_t)r);
    p = (int)pairs[2 * (size_t)r + 1];
  } else {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    g.t[0] = g.t[1] = g.t[2] = nan;
    g.q = {nan, nan, nan, nan};
    p = -1;
  }
  if (last) {
    traj_emit(t, g, p, inverse, traj, root, info);
  } else {
    store_pose(g, T + 7 * (size_t)t);
    par[t] = p;
  }
}

// One round of pointer jumping: T[t] <- T[t] * T[par], par[t] <- par[par].
__global__ void __launch_bounds__(kTrT)
    traj_jump_kernel(int counter, const double* __restrict__ Tin, const int* __restrict__ pin,
                     double* __restrict__ Tout, int* __restrict__ pout, int last, int inverse,
                     float* __restrict__ traj, int64_t* __restrict__ root,
                     int32_t* __restrict__ info) {
  const int t = blockIdx.x * kTrT + threadIdx.x;
  if (t >= counter) return;
  int p = pin[t];
  G g = load_pose(Tin + 7 * (size_t)t);
  if (p >= 0) {  // p < t < counter by construction
    g = lie::se3_mul(g, load_pose(Tin + 7 * (size_t)p));
    p = pin[p];
  }
  if (last) {
    traj_emit(t, g, p, inverse, traj, root, info);
  } else {
    store_pose(g, Tout + 7 * (size_t)t);
    pout[t] = p;
  }
}

inline int jump_rounds(int counter) {  // ceil(log2(counter)): chains are at most counter - 1 long
  int r = 0;
  while ((1ll << r) < counter) r++;
  return r;
}

}  // namespace frontend
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT int dpvo_frame_init(float* poses, float* patches, float* intrinsics, int64_t* tstamps,
                                const double* times, int times_cap, const float* new_patches,
                                const float* new_intrinsics, int N, int M, int P, int n,
                                const int32_t* n_dev, int counter, const int32_t* counter_dev,
                                int motion_model, double damping, double res, int median,
                                void* stream) {
  if (!poses || !patches || !intrinsics || !tstamps || !times || !new_patches || !new_intrinsics)
    return DPVO_ERR_INVALID;
  if (N <= 0 || M <= 0 || P <= 0 || times_cap <= 0) return DPVO_ERR_INVALID;
  if (!n_dev && (n < 0 || n >= N)) return DPVO_ERR_INVALID;
  if (!counter_dev && (counter < 0 || counter >= times_cap)) return DPVO_ERR_INVALID;
  if (motion_model < 0 || motion_model > 1 || median < 0 || median > 1) return DPVO_ERR_INVALID;
  if (!(res == res) || res == 0.0 || !(damping == damping)) return DPVO_ERR_INVALID;
  // the select counts in int: 3 frames of M P P depths (far above 3 x 1024 x 9)
  if ((long long)3 * M * P * P > (1ll << 30)) return DPVO_ERR_UNSUPPORTED;
  frontend::FrameInit a;
  a.poses = poses;
  a.patches = patches;
  a.intrinsics = intrinsics;
  a.tstamps = tstamps;
  a.times = times;
  a.new_patches = new_patches;
  a.new_intrinsics = new_intrinsics;
  a.n_dev = n_dev;
  a.counter_dev = counter_dev;
  a.N = N;
  a.M = M;
  a.P = P;
  a.times_cap = times_cap;
  a.n = n;
  a.counter = counter;
  a.motion_model = motion_model;
  a.median = median;
  a.damping = damping;
  a.res = (float)res;
  hipLaunchKernelGGL(frontend::frame_init_kernel, dim3(1), dim3(frontend::kFiT), 0,
                     as_stream(stream), a);
  return launch_status();
}

DPVO_EXPORT size_t dpvo_trajectory_workspace_bytes(int counter) {
  return (size_t)128 * (size_t)(counter > 1 ? counter : 1);
}

DPVO_EXPORT int dpvo_trajectory(const float* poses, const int64_t* tstamps, int N, int n,
                                const int32_t* n_dev, const float* delta_log,
                                const int64_t* delta_pairs, const int32_t* delta_count,
                                int delta_cap, int counter, int inverse, float* traj,
                                int64_t* root, int32_t* info, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (counter < 0) return DPVO_ERR_INVALID;
  if (counter == 0) return DPVO_OK;
  if (N <= 0 || delta_cap < 0 || inverse < 0 || inverse > 1) return DPVO_ERR_INVALID;
  if (!n_dev && (n < 0 || n > N)) return DPVO_ERR_INVALID;
  if (!poses || !tstamps || !delta_count || !traj || !root || !info || !workspace)
    return DPVO_ERR_INVALID;
  if (delta_cap > 0 && (!delta_log || !delta_pairs)) return DPVO_ERR_INVALID;
  if (workspace_bytes < dpvo_trajectory_workspace_bytes(counter)) return DPVO_ERR_WORKSPACE;
  hipStream_t s = as_stream(stream);
  const frontend::TrajWs w = frontend::traj_ws(workspace, counter);
  const int R = frontend::jump_rounds(counter);
  const unsigned grid = (unsigned)((counter + frontend::kTrT - 1) / frontend::kTrT);
  hipLaunchKernelGGL(frontend::traj_scatter_kernel, dim3(1), dim3(frontend::kTrScatterT), 0, s,
                     tstamps, n, n_dev, N, delta_pairs, delta_count, delta_cap, counter, w.rec,
                     w.kfi, info);
  hipLaunchKernelGGL(frontend::traj_build_kernel, dim3(grid), dim3(frontend::kTrT), 0, s, poses,
                     delta_log, delta_pairs, counter, (const int*)w.rec, (const int*)w.kfi, w.T[0],
                     w.par[0], R == 0 ? 1 : 0, inverse, traj, root, info);
  for (int r = 0; r < R; r++) {
    const int in = r & 1, out = in ^ 1;
    hipLaunchKernelGGL(frontend::traj_jump_kernel, dim3(grid), dim3(frontend::kTrT), 0, s, counter,
                       (const double*)w.T[in], (const int*)w.par[in], w.T[out], w.par[out],
                       r == R - 1 ? 1 : 0, inverse, traj, root, info);
  }
  return launch_status();
}
