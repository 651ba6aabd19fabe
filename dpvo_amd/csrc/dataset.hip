// dataset.hip -- the device half of the training data readers
// (dpvo/data_readers/base.py, rgbd_utils.py, augmentation.py):
//
//   dpvo_frame_flow_distance   rgbd_utils.compute_distance_matrix_flow: the mean
//                              clamped flow magnitude between every pair of
//                              frames, both directions pooled.  One launch.
//   dpvo_frame_graph_count /   base.py:77-80: the rows of d = f D below max_flow
//   dpvo_frame_graph_fill      as CSR (count, scan, fill)
//   dpvo_rgbd_augment          augmentation.py: colour jitter / gray / invert,
//                              then scale (bicubic image, nearest depth) and
//                              centre crop, parameters by value
//   dpvo_normalize_depth       base.py:171-173: s = 0.7 quantile(disps, 0.98)
//
// Flow distance: a workgroup owns source frame i against a tile of kFdTile
// frames j >= i; one wave per pair strides over the h w grid points of both
// directions (i -> j first) and ends in a fixed xor tree, all in fp64.  Frame
// i's disparities (4.8 KB at TartanAir's 30 x 40) are read by every wave of the
// workgroup and stay in the CU's L1; the rays are two divisions from the lane's
// (x, y) and are recomputed.  Only i <= j is computed and stored twice.
//
// Augmentation: colour is evaluated once per source pixel and resampled from a
// scratch image (the bicubic has 16 taps per output pixel: colour per tap
// would repeat the hue's RGB -> HSV -> RGB 16 times).  The contrast mean is a
// reduction over all frames with a launch of its own: fp64 partials per
// workgroup, summed in one fixed order by every workgroup of the next launch.
// Every sum here has a fixed order: two calls give identical bits.
#include <math.h>

#include "common.hpp"
#include "radix_select.hpp"

namespace dpvo {
namespace dataset {

constexpr int kMaxFrames = 8192;
constexpr int kMaxPoints = 65536;
constexpr int kMaxSide = 16384;

// ---- frame flow distance ---------------------------------------------------------
constexpr int kFdThreads = 256;
constexpr int kFdWaves = kFdThreads / kWave;
constexpr int kFdTile = 64;

// SE3 with the quaternion formulas of lie_se3.hpp (qact, qmul, se3_inv,
// se3_mul), fp64, without the renormalisation
struct Pose {
  double t[3];
  double q[4];  // x y z w
};
__device__ __forceinline__ void q_act(const double* q, const double* p, double* o) {
  double uv[3], uv2[3];
  uv[0] = q[1] * p[2] - q[2] * p[1];
  uv[1] = q[2] * p[0] - q[0] * p[2];
  uv[2] = q[0] * p[1] - q[1] * p[0];
  uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
  uv2[0] = q[1] * uv[2] - q[2] * uv[1];
  uv2[1] = q[2] * uv[0] - q[0] * uv[2];
  uv2[2] = q[0] * uv[1] - q[1] * uv[0];
#pragma unroll
  for (int c = 0; c < 3; c++) o[c] = p[c] + q[3] * uv[c] + uv2[c];
}
__device__ __forceinline__ Pose pose_load(const float* __restrict__ p) {
  Pose g;
#pragma unroll
  for (int c = 0; c < 3; c++) g.t[c] = (double)p[c];
#pragma unroll
  for (int c = 0; c < 4; c++) g.q[c] = (double)p[3 + c];
  return g;
}
__device__ __forceinline__ Pose pose_inv(const Pose& g) {
  Pose o;
  o.q[0] = -g.q[0]; o.q[1] = -g.q[1]; o.q[2] = -g.q[2]; o.q[3] = g.q[3];
  double t[3];
  q_act(o.q, g.t, t);
  o.t[0] = -t[0]; o.t[1] = -t[1]; o.t[2] = -t[2];
  return o;
}
__device__ __forceinline__ Pose pose_mul(const Pose& a, const Pose& b) {
  Pose o;
  const double *p = a.q, *q = b.q;
  o.q[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
  o.q[1] = p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2];
  o.q[2] = p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0];
  o.q[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
  double t[3];
  q_act(a.q, b.t, t);
#pragma unroll
  for (int c = 0; c < 3; c++) o.t[c] = a.t[c] + t[c];
  return o;
}

struct FlowDist {
  const float* poses;
  const float* disps;
  const float* intrinsics;
  float* D;
  int N, h, w;
};

// the lane's share of one direction: points lane, lane + 64, .. of the source
// frame, in that order, onto the running sum and count
__device__ __forceinline__ void flow_accumulate(const Pose& G, const double* Ks, const double* Kd,
                                                const float* __restrict__ disp, int hw, int w,
                                                int lane, double& sum, int& k) {
  for (int p = lane; p < hw; p += kWave) {
    const int y = p / w, x = p - y * w;
    const double d = (double)disp[p];
    const double X0[3] = {((double)x - Ks[2]) / Ks[0], ((double)y - Ks[3]) / Ks[1], 1.0};
    double X1[3];
    q_act(G.q, X0, X1);
#pragma unroll
    for (int c = 0; c < 3; c++) X1[c] += G.t[c] * d;
    const double Z = X1[2], zc = fmax(Z, 0.1);
    const double u = Kd[0] * (X1[0] / zc) + Kd[2], v = Kd[1] * (X1[1] / zc) + Kd[3];
    const double fu = u - (double)x, fv = v - (double)y;
    const double mag = fmin(sqrt(fu * fu + fv * fv), 100.0);  // a NaN flow counts as the clamp
    if (Z > 0.2) {  // false for a NaN depth
      sum += mag;
      k++;
    }
  }
}

__global__ void __launch_bounds__(kFdThreads) flow_distance_kernel(FlowDist a) {
  const int i = blockIdx.x, j0 = blockIdx.y * kFdTile;
  if (j0 + kFdTile <= i) return;  // every j of the tile is below i: the mirror's
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int hw = a.h * a.w;
  const Pose Gi = pose_inv(pose_load(a.poses + 7 * (size_t)i));
  const Pose Gi_inv = pose_inv(Gi);
  double Ki[4], Kj[4];
#pragma unroll
  for (int c = 0; c < 4; c++) Ki[c] = (double)a.intrinsics[4 * (size_t)i + c];
  const int jend = min(j0 + kFdTile, a.N);
  for (int j = j0 + wid; j < jend; j += kFdWaves) {
    if (j < i) continue;
    const Pose Gj = pose_inv(pose_load(a.poses + 7 * (size_t)j));
    const Pose Gij = pose_mul(Gj, Gi_inv), Gji = pose_mul(Gi, pose_inv(Gj));
#pragma unroll
    for (int c = 0; c < 4; c++) Kj[c] = (double)a.intrinsics[4 * (size_t)j + c];
    double sum = 0.0;
    int k = 0;
    flow_accumulate(Gij, Ki, Kj, a.disps + (size_t)i * hw, hw, a.w, lane, sum, k);
    flow_accumulate(Gji, Kj, Ki, a.disps + (size_t)j * hw, hw, a.w, lane, sum, k);
    sum = wave_sum(sum);
    k = wave_sum_i(k);
    if (lane == 0) {
      const float share = (float)k / (float)(2 * hw);
      const float v = share < 0.7f ? INFINITY : (float)(sum / (double)k);
      a.D[(size_t)i * a.N + j] = v;
      a.D[(size_t)j * a.N + i] = v;
    }
  }
}

// ---- frame graph: CSR of the entries f D < max_flow -----------------------------------
constexpr int kFgThreads = 256;
constexpr int kFgScanThreads = 1024;

// d = f * D as numpy's float32 product (one rounding)
__global__ void __launch_bounds__(kFgThreads)
    graph_count_kernel(const float* __restrict__ D, int N, float f, float max_flow,
                       int* __restrict__ rowptr) {
  __shared__ int scr[kFgThreads / kWave + 1];
  const float* row = D + (size_t)blockIdx.x * N;
  int c = 0;
  for (int j = threadIdx.x; j < N; j += kFgThreads) c += (f * row[j] < max_flow) ? 1 : 0;
  int total;
  block_excl_sum(c, scr, total);
  if (threadIdx.x == 0) rowptr[blockIdx.x] = total;
}

// rowptr[0, N) counts -> exclusive prefix, rowptr[N] = nnz; one workgroup, in place
// (every thread reads and writes its own elements only)
__global__ void __launch_bounds__(kFgScanThreads) graph_scan_kernel(int* __restrict__ rowptr, int N) {
  __shared__ int scr[kFgScanThreads / kWave + 1];
  int run = 0;
  for (int base = 0; base < N; base += kFgScanThreads) {
    const int idx = base + threadIdx.x;
    const int v = idx < N ? rowptr[idx] : 0;
    int total;
    const int off = block_excl_sum(v, scr, total);
    if (idx < N) rowptr[idx] = run + off;
    run += total;
  }
  if (threadIdx.x == 0) rowptr[N] = run;
}

__global__ void __launch_bounds__(kFgThreads)
    graph_fill_kernel(const float* __restrict__ D, int N, float f, float max_flow,
                      const int* __restrict__ rowptr, int* __restrict__ col,
                      float* __restrict__ dist, int cap) {
  __shared__ int scr[kFgThreads / kWave + 1];
  const float* row = D + (size_t)blockIdx.x * N;
  int run = rowptr[blockIdx.x];
  for (int base = 0; base < N; base += kFgThreads) {
    const int j = base + threadIdx.x;
    const float d = j < N ? f * row[j] : 0.f;
    const int keep = (j < N && d < max_flow) ? 1 : 0;
    int total;
    const int pos = run + block_excl_sum(keep, scr, total);
    if (keep && pos >= 0 && pos < cap) {  // a rowptr that is not this D's writes nothing outside
      col[pos] = j;
      dist[pos] = d;
    }
    run += total;
  }
}

// ---- RGB-D augmentation ----------------------------------------------------------------
constexpr int kAugThreads = 256;
constexpr int kAugWaves = kAugThreads / kWave;
constexpr int kMeanBlocks = 256;  // == kAugThreads: one partial per thread of the next launch

struct Augment {
  const float* images;   // [N, 3, H, W]
  const float* disps;    // [N, H, W]
  const float* intrinsics;
  float* images_out;     // [N, 3, ch, cw]
  float* disps_out;      // [N, ch, cw]
  float* intrinsics_out;
  double* partial;       // [kMeanBlocks]
  float* scratch;        // [N, 3, H, W]
  dpvo_augment_params p;
  int N, H, W, ch, cw, ht1, wd1, y0, x0;
  int n_pre;             // jitter operations before contrast
};

// fp32 as the header states it, no contraction: the host restatement (torch on
// the CPU, no FMA) rounds the same way
#pragma clang fp contract(off)
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) {
  return 0.299f * r + 0.587f * g + 0.114f * b;
}
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float delta) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const float cr = maxc - minc;
  float h = 0.f, s = 0.f;
  if (cr > 0.f) {
    s = cr / maxc;
    const float rc = (maxc - r) / cr, gc = (maxc - g) / cr, bc = (maxc - b) / cr;
    if (maxc == r)
      h = bc - gc;
    else if (maxc == g)
      h = 2.f + rc - bc;
    else
      h = 4.f + gc - rc;
    h = fmodf(h / 6.f + 1.f, 1.f);
  }
  h = h + delta;
  h = h - floorf(h);  // mod 1
  const float v = maxc;
  const float h6 = h * 6.f, fl = floorf(h6), f = h6 - fl;
  const int sector = ((int)fl) % 6;
  const float p = v * (1.f - s), q = v * (1.f - f * s), t = v * (1.f - (1.f - f) * s);
  switch (sector) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
  r = clamp01(r); g = clamp01(g); b = clamp01(b);
}
// jitter operation `op` (0 brightness, 1 contrast, 2 saturation, 3 hue), clamped
__device__ __forceinline__ void jitter(int op, const dpvo_augment_params& p, float m, float& r,
                                       float& g, float& b) {
  if (op == 0) {
    r = clamp01(r * p.brightness); g = clamp01(g * p.brightness); b = clamp01(b * p.brightness);
  } else if (op == 1) {
    const float c = p.contrast, o = (1.f - c) * m;
    r = clamp01(c * r + o); g = clamp01(c * g + o); b = clamp01(c * b + o);
  } else if (op == 2) {
    const float s = p.saturation, o = (1.f - s) * gray_of(r, g, b);
    r = clamp01(s * r + o); g = clamp01(s * g + o); b = clamp01(s * b + o);
  } else {
    hue_shift(r, g, b, p.hue);
  }
}
// the whole colour map of one pixel, 0..255 in and out
__device__ __forceinline__ void color_pixel(const dpvo_augment_params& p, float m, float& r, float& g,
                                            float& b) {
  r = r / 255.f; g = g / 255.f; b = b / 255.f;
#pragma unroll
  for (int k = 0; k < 4; k++) jitter(p.order[k], p, m, r, g, b);
  if (p.gray) r = g = b = gray_of(r, g, b);
  if (p.invert) { r = 1.f - r; g = 1.f - g; b = 1.f - b; }
  r = r * 255.f; g = g * 255.f; b = b * 255.f;
}
__device__ __forceinline__ float intrinsic_out(const Augment& a, int g) {
  const int c = g & 3;
  const float v = (float)a.p.scale * a.intrinsics[g];
  return c == 2 ? v - (float)a.x0 : c == 3 ? v - (float)a.y0 : v;
}
#pragma clang fp contract(fast)

// sum of one double per thread over a workgroup of kAugThreads in a fixed order
// (xor tree in the wave, waves ascending); every thread gets it
__device__ __forceinline__ double aug_block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < kAugWaves; w++) s += red[w];
  return s;
}

// partial[b] = workgroup b's share of the sum of gray(x) over all N frames, x as
// it stands when contrast's turn comes
__global__ void __launch_bounds__(kAugThreads) color_mean_kernel(Augment a) {
  __shared__ double red[kAugWaves];
  const size_t plane = (size_t)a.H * a.W, total = (size_t)a.N * plane;
  const int ir = a.p.swap_rb ? 2 : 0, ib = 2 - ir;
  double acc = 0.0;
  for (size_t t = (size_t)blockIdx.x * kAugThreads + threadIdx.x; t < total;
       t += (size_t)kMeanBlocks * kAugThreads) {
    const size_t n = t / plane, o = n * 3 * plane + (t - n * plane);
    float r = a.images[o + ir * plane] / 255.f, g = a.images[o + plane] / 255.f,
          b = a.images[o + ib * plane] / 255.f;
    for (int k = 0; k < a.n_pre; k++) jitter(a.p.order[k], a.p, 0.f, r, g, b);
    acc += (double)gray_of(r, g, b);
  }
  acc = aug_block_sum(acc, red);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = acc;
}

// Colour (or a plain copy with do_color = 0) of the window [y0, y0 + dh) x
// [x0, x0 + dw) of every frame into dst [N, 3, dh, dw].  FINAL: the window is
// the crop (scale 1): the depth window and the intrinsics are written too.
template <bool FINAL>
__global__ void __launch_bounds__(kAugThreads)
    color_kernel(Augment a, float* __restrict__ dst, int dh, int dw, int y0, int x0) {
  __shared__ double red[kAugWaves];
  float m = 0.f;
  if (a.p.do_color) {  // the same fixed-order sum in every workgroup
    const double s = aug_block_sum(a.partial[threadIdx.x], red);
    m = (float)(s / ((double)a.N * (double)a.H * (double)a.W));
  }
  const size_t gid = (size_t)blockIdx.x * kAugThreads + threadIdx.x;
  if (FINAL && gid < 4 * (size_t)a.N) a.intrinsics_out[gid] = intrinsic_out(a, (int)gid);
  const size_t win = (size_t)dh * dw, total = (size_t)a.N * win;
  if (gid >= total) return;
  const size_t n = gid / win, rem = gid - n * win;
  const int y = (int)(rem / dw), x = (int)(rem - (size_t)y * dw);
  const size_t plane = (size_t)a.H * a.W;
  const size_t so = n * 3 * plane + (size_t)(y0 + y) * a.W + (x0 + x), dof = n * 3 * win + rem;
  float c0 = a.images[so], c1 = a.images[so + plane], c2 = a.images[so + 2 * plane];
  if (a.p.do_color) {
    if (a.p.swap_rb)
      color_pixel(a.p, m, c2, c1, c0);
    else
      color_pixel(a.p, m, c0, c1, c2);
  }
  dst[dof] = c0;
  dst[dof + win] = c1;
  dst[dof + 2 * win] = c2;
  if (FINAL) a.disps_out[n * win + rem] = a.disps[n * plane + (size_t)(y0 + y) * a.W + (x0 + x)];
}

// F.interpolate(mode='bicubic', align_corners=False) in fp32: A = -0.75, source
// index clamped at the border
__device__ __forceinline__ void cubic_coeffs(float t, float* c) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
  c[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  c[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  c[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  c[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

// the crop window of the resized frame: image bicubic from src [N, 3, H, W],
// depth nearest, intrinsics.  One thread per output pixel.
__global__ void __launch_bounds__(kAugThreads)
    resample_kernel(Augment a, const float* __restrict__ src) {
  const size_t gid = (size_t)blockIdx.x * kAugThreads + threadIdx.x;
  if (gid < 4 * (size_t)a.N) a.intrinsics_out[gid] = intrinsic_out(a, (int)gid);
  const size_t win = (size_t)a.ch * a.cw, total = (size_t)a.N * win;
  if (gid >= total) return;
  const size_t n = gid / win, rem = gid - n * win;
  const int y = (int)(rem / a.cw), x = (int)(rem - (size_t)y * a.cw);
  const int oy = a.y0 + y, ox = a.x0 + x;
  const float sh = (float)a.H / (float)a.ht1, sw = (float)a.W / (float)a.wd1;
  const float ry = sh * ((float)oy + 0.5f) - 0.5f, rx = sw * ((float)ox + 0.5f) - 0.5f;
  const float fy = floorf(ry), fx = floorf(rx);
  const int iy = (int)fy, ix = (int)fx;
  float cy[4], cx[4];
  cubic_coeffs(ry - fy, cy);
  cubic_coeffs(rx - fx, cx);
  int xs[4], ys[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    xs[k] = min(max(ix - 1 + k, 0), a.W - 1);
    ys[k] = min(max(iy - 1 + k, 0), a.H - 1);
  }
  const size_t plane = (size_t)a.H * a.W;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float* P = src + (n * 3 + c) * plane;
    float out = 0.f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float* row = P + (size_t)ys[r] * a.W;
      const float v = row[xs[0]] * cx[0] + row[xs[1]] * cx[1] + row[xs[2]] * cx[2] + row[xs[3]] * cx[3];
      out += v * cy[r];
    }
    a.images_out[(n * 3 + c) * win + rem] = out;
  }
  const int dy = min((int)floorf((float)oy * sh), a.H - 1), dx = min((int)floorf((float)ox * sw), a.W - 1);
  a.disps_out[n * win + rem] = a.disps[n * plane + (size_t)dy * a.W + dx];
}

// ---- normalize_depth ---------------------------------------------------------------
constexpr int kQtThreads = 1024;
constexpr int kNdThreads = 256;

// out[0] = s = 0.7 lerp(lo, hi, weight), out[1] = lo, out[2] = hi: the values of
// sorted ranks rank_lo and rank_hi.  One workgroup.
__global__ void __launch_bounds__(kQtThreads)
    depth_scale_kernel(const float* __restrict__ disps, int n, int rank_lo, int rank_hi, float weight,
                       float* __restrict__ out) {
  __shared__ RadixSelectLds sel;
  bool nan = false;
  const uint32_t klo = block_radix_select(n, rank_lo, [&](int i) {
    const float v = disps[i];
    nan |= v != v;
    return float_key(v);
  }, sel);
  const uint32_t khi = rank_hi == rank_lo ? klo : block_radix_select(n, rank_hi, [&](int i) {
    return float_key(disps[i]);
  }, sel);
  const int any_nan = __syncthreads_or(nan ? 1 : 0);
  if (threadIdx.x == 0) {
    const float lo = key_float(klo), hi = key_float(khi);
    float q;
    {
#pragma clang fp contract(off)
      q = weight < 0.5f ? lo + weight * (hi - lo) : hi - (hi - lo) * (1.f - weight);  // torch's lerp
    }
    const float qnan = __uint_as_float(0x7fc00000u);
    out[0] = any_nan ? qnan : 0.7f * q;
    out[1] = any_nan ? qnan : lo;
    out[2] = any_nan ? qnan : hi;
  }
}

__global__ void __launch_bounds__(kNdThreads)
    depth_apply_kernel(const float* __restrict__ disps, const float* __restrict__ poses, int n,
                       int nposes, const float* __restrict__ scale, float* __restrict__ disps_out,
                       float* __restrict__ poses_out) {
  const float s = scale[0];
  const size_t gid = (size_t)blockIdx.x * kNdThreads + threadIdx.x;
  if (gid < (size_t)n) disps_out[gid] = disps[gid] / s;
  if (gid < 7 * (size_t)nposes) poses_out[gid] = (gid % 7) < 3 ? poses[gid] * s : poses[gid];
}

inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace dataset
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT int dpvo_frame_flow_distance(const float* poses, const float* disps,
                                         const float* intrinsics, int N, int h, int w, float* D,
                                         void* stream) {
  if (!poses || !disps || !intrinsics || !D) return DPVO_ERR_INVALID;
  if (dataset::misaligned(poses, 4) || dataset::misaligned(disps, 4) ||
      dataset::misaligned(intrinsics, 4) || dataset::misaligned(D, 4))
    return DPVO_ERR_INVALID;
  if (N <= 0 || h <= 0 || w <= 0) return DPVO_ERR_INVALID;
  if (N > dataset::kMaxFrames || (long long)h * w > dataset::kMaxPoints) return DPVO_ERR_UNSUPPORTED;
  dataset::FlowDist a{poses, disps, intrinsics, D, N, h, w};
  const dim3 grid((unsigned)N, (unsigned)((N + dataset::kFdTile - 1) / dataset::kFdTile));
  hipLaunchKernelGGL(dataset::flow_distance_kernel, grid, dim3(dataset::kFdThreads), 0,
                     as_stream(stream), a);
  return launch_status();
}

static int graph_args(const float* D, int N, float f, float max_flow) {
  if (!D || dataset::misaligned(D, 4) || N <= 0) return DPVO_ERR_INVALID;
  if (!isfinite(f) || !(f > 0.f) || max_flow != max_flow) return DPVO_ERR_INVALID;
  return DPVO_OK;
}

DPVO_EXPORT int dpvo_frame_graph_count(const float* D, int N, float f, float max_flow,
                                       int32_t* rowptr, void* stream) {
  const int st = graph_args(D, N, f, max_flow);
  if (st != DPVO_OK || !rowptr || dataset::misaligned(rowptr, 4)) return DPVO_ERR_INVALID;
  if (N > dataset::kMaxFrames) return DPVO_ERR_UNSUPPORTED;
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(dataset::graph_count_kernel, dim3(N), dim3(dataset::kFgThreads), 0, s, D, N, f,
                     max_flow, rowptr);
  hipLaunchKernelGGL(dataset::graph_scan_kernel, dim3(1), dim3(dataset::kFgScanThreads), 0, s, rowptr,
                     N);
  return launch_status();
}

DPVO_EXPORT int dpvo_frame_graph_fill(const float* D, int N, float f, float max_flow,
                                      const int32_t* rowptr, int32_t* col, float* dist, int nnz,
                                      void* stream) {
  const int st = graph_args(D, N, f, max_flow);
  if (st != DPVO_OK || !rowptr || dataset::misaligned(rowptr, 4) || nnz < 0)
    return DPVO_ERR_INVALID;
  if (nnz > 0 && (!col || !dist || dataset::misaligned(col, 4) || dataset::misaligned(dist, 4)))
    return DPVO_ERR_INVALID;
  if (N > dataset::kMaxFrames) return DPVO_ERR_UNSUPPORTED;
  if (nnz == 0) return DPVO_OK;
  hipLaunchKernelGGL(dataset::graph_fill_kernel, dim3(N), dim3(dataset::kFgThreads), 0,
                     as_stream(stream), D, N, f, max_flow, rowptr, col, dist, nnz);
  return launch_status();
}

// the checks of dpvo_rgbd_augment that need no pointer; fills the resized size and the crop origin
static int augment_geometry(int N, int H, int W, int ch, int cw, const dpvo_augment_params* p,
                            int* ht1, int* wd1, int* y0, int* x0) {
  if (!p || N <= 0 || H <= 0 || W <= 0 || ch <= 0 || cw <= 0) return DPVO_ERR_INVALID;
  if (p->do_color < 0 || p->do_color > 1 || p->gray < 0 || p->gray > 1 || p->invert < 0 ||
      p->invert > 1 || p->swap_rb < 0 || p->swap_rb > 1)
    return DPVO_ERR_INVALID;
  int seen = 0;
  for (int k = 0; k < 4; k++) {
    if (p->order[k] < 0 || p->order[k] > 3) return DPVO_ERR_INVALID;
    seen |= 1 << p->order[k];
  }
  if (seen != 15) return DPVO_ERR_INVALID;
  if (!isfinite(p->brightness) || !isfinite(p->contrast) || !isfinite(p->saturation) ||
      !isfinite(p->hue) || !isfinite(p->scale) || !(p->scale > 0.0))
    return DPVO_ERR_INVALID;
  if (p->brightness < 0.f || p->contrast < 0.f || p->saturation < 0.f) return DPVO_ERR_INVALID;
  const bool small = H <= dataset::kMaxSide && W <= dataset::kMaxSide;
  const double sh = p->scale * H, sw = p->scale * W;
  if (small && sh <= 4.0 * dataset::kMaxSide && sw <= 4.0 * dataset::kMaxSide) {
    *ht1 = (int)sh;
    *wd1 = (int)sw;
    // scale 1 resamples nothing and takes any crop inside the frame; a resized
    // frame must be larger than the crop (augmentation.py's (crop + 1) / size)
    const int room = p->scale == 1.0 ? 0 : 1;
    if (ch > *ht1 - room || cw > *wd1 - room) return DPVO_ERR_INVALID;
  }
  if (!small || sh > 4.0 * dataset::kMaxSide || sw > 4.0 * dataset::kMaxSide)
    return DPVO_ERR_UNSUPPORTED;
  if ((long long)N * H * W >= (1ll << 31) / 3) return DPVO_ERR_UNSUPPORTED;
  *y0 = (*ht1 - ch) / 2;
  *x0 = (*wd1 - cw) / 2;
  return DPVO_OK;
}

DPVO_EXPORT size_t dpvo_rgbd_augment_workspace_bytes(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return sizeof(double) * dataset::kMeanBlocks + sizeof(float) * 3 * (size_t)N * H * W;
}

DPVO_EXPORT int dpvo_rgbd_augment(const float* images, const float* disps, const float* intrinsics,
                                  int N, int H, int W, int crop_h, int crop_w,
                                  const dpvo_augment_params* params, float* images_out,
                                  float* disps_out, float* intrinsics_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!images || !disps || !intrinsics || !images_out || !disps_out || !intrinsics_out || !workspace)
    return DPVO_ERR_INVALID;
  if (dataset::misaligned(images, 4) || dataset::misaligned(disps, 4) ||
      dataset::misaligned(intrinsics, 4) || dataset::misaligned(images_out, 4) ||
      dataset::misaligned(disps_out, 4) || dataset::misaligned(intrinsics_out, 4) ||
      dataset::misaligned(workspace, 8))
    return DPVO_ERR_INVALID;
  dataset::Augment a;
  const int st = augment_geometry(N, H, W, crop_h, crop_w, params, &a.ht1, &a.wd1, &a.y0, &a.x0);
  if (st != DPVO_OK) return st;
  const bool scratch = params->do_color && params->scale != 1.0;
  if (workspace_bytes < (scratch ? dpvo_rgbd_augment_workspace_bytes(N, H, W)
                                 : sizeof(double) * dataset::kMeanBlocks))
    return DPVO_ERR_WORKSPACE;
  a.images = images;
  a.disps = disps;
  a.intrinsics = intrinsics;
  a.images_out = images_out;
  a.disps_out = disps_out;
  a.intrinsics_out = intrinsics_out;
  a.partial = reinterpret_cast<double*>(workspace);
  a.scratch = reinterpret_cast<float*>(a.partial + dataset::kMeanBlocks);
  a.p = *params;
  a.N = N; a.H = H; a.W = W; a.ch = crop_h; a.cw = crop_w;
  a.n_pre = 0;
  while (a.p.order[a.n_pre] != 1) a.n_pre++;
  hipStream_t s = as_stream(stream);
  const bool resample = a.p.scale != 1.0;
  auto blocks = [](size_t threads) {
    return dim3((unsigned)((threads + dataset::kAugThreads - 1) / dataset::kAugThreads));
  };
  if (a.p.do_color)
    hipLaunchKernelGGL(dataset::color_mean_kernel, dim3(dataset::kMeanBlocks),
                       dim3(dataset::kAugThreads), 0, s, a);
  const size_t out_threads = (size_t)N * crop_h * crop_w > 4 * (size_t)N ? (size_t)N * crop_h * crop_w
                                                                           : 4 * (size_t)N;
  if (!resample) {
    hipLaunchKernelGGL((dataset::color_kernel<true>), blocks(out_threads), dim3(dataset::kAugThreads),
                       0, s, a, images_out, crop_h, crop_w, a.y0, a.x0);
  } else {
    if (a.p.do_color)
      hipLaunchKernelGGL((dataset::color_kernel<false>), blocks((size_t)N * H * W),
                         dim3(dataset::kAugThreads), 0, s, a, a.scratch, H, W, 0, 0);
    hipLaunchKernelGGL(dataset::resample_kernel, blocks(out_threads), dim3(dataset::kAugThreads), 0,
                       s, a, a.p.do_color ? (const float*)a.scratch : images);
  }
  return launch_status();
}

DPVO_EXPORT int dpvo_normalize_depth(const float* disps, int n, const float* poses, int nposes,
                                     float* disps_out, float* poses_out, float* scale,
                                     void* stream) {
  if (!disps || !poses || !disps_out || !poses_out || !scale) return DPVO_ERR_INVALID;
  if (dataset::misaligned(disps, 4) || dataset::misaligned(poses, 4) ||
      dataset::misaligned(disps_out, 4) || dataset::misaligned(poses_out, 4) ||
      dataset::misaligned(scale, 4))
    return DPVO_ERR_INVALID;
  if (n <= 0 || nposes <= 0) return DPVO_ERR_INVALID;
  if (n > (1 << 30) || nposes > (1 << 24)) return DPVO_ERR_UNSUPPORTED;
  // torch.quantile's rank arithmetic, in the tensor's dtype
  const float pos = 0.98f * (float)(n - 1);
  const float below = floorf(pos);
  const int lo = (int)below, hi = (int)ceilf(pos);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(dataset::depth_scale_kernel, dim3(1), dim3(dataset::kQtThreads), 0, s, disps, n,
                     lo, hi < n ? hi : n - 1, pos - below, scale);
  const size_t threads = (size_t)n > 7 * (size_t)nposes ? (size_t)n : 7 * (size_t)nposes;
  hipLaunchKernelGGL(dataset::depth_apply_kernel,
                     dim3((unsigned)((threads + dataset::kNdThreads - 1) / dataset::kNdThreads)),
                     dim3(dataset::kNdThreads), 0, s, disps, poses, n, nposes,
                     (const float*)scale, disps_out, poses_out);
  return launch_status();
}
