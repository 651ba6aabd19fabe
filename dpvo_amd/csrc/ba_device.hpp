// ba_device.hpp -- the device helpers the BA kernels share: ba.hip (multi-kernel
// path), ba_large.hip (large graphs) and ba_window.hip (through ba_solve.hpp)
// include it.  It holds the index helpers of the packed lower 6x6 blocks
// (lblk, tri_of), the workgroup scan of an LDS array (fscan), the reference's
// fp32 edge linearisation (lin_edge) and the fp64 pivot reciprocal (rcp64).
// The dense solves are elsewhere: ba_solve.hpp (window), ba.hip (multi-kernel),
// ba_bgj.hpp (large graphs).
#pragma once

#include "common.hpp"

namespace dpvo {
namespace bad {

__device__ __forceinline__ int lblk(int a, int b) { return a * (a + 1) / 2 + b; }  // a >= b

__device__ __forceinline__ void tri_of(int bt, int& a, int& b) {  // bt -> (a, b), a >= b
  int r = (int)((sqrtf(8.0f * bt + 1.0f) - 1.0f) * 0.5f);
  while (r * (r + 1) / 2 > bt) r--;
  while ((r + 1) * (r + 2) / 2 <= bt) r++;
  a = r;
  b = bt - r * (r + 1) / 2;
}

// block-wide exclusive scan of LDS ints data[0..n), returns the total.  Each
// thread owns a contiguous run of at most kScanRun elements whose loads are
// all issued before the first add (one LDS latency, not one per element).
constexpr int kScanRun = 16;
// pack_shift > 0: each input c is first replaced by (c << pack_shift) | (c > 0),
// so one scan gives both the exclusive prefix of c (high bits) and the number
// of nonzero entries before (low bits) -- bucket starts and bucket indices.
__device__ inline int fscan(int* data, int n, int* scr, int pack_shift = 0) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (n <= 0) {
    // keep the barrier of every other path: callers rely on it to order their
    // LDS atomics before reading the results
    __syncthreads();
    return 0;
  }
  if (n <= 64 * kScanRun) {
    // small scans (the plan's shard ranges, the BA setup's patch counts at
    // cfg2): wave 0 alone, one DPP scan, two barriers instead of three
    if (tid < 64) {
      const int per = (n + 63) / 64;
      const int lo = min(tid * per, n), hi = min(lo + per, n);
      int v[kScanRun];
#pragma unroll
      for (int k = 0; k < kScanRun; k++) {
        const int d = data[min(lo + k, max(n - 1, 0))];
        v[k] = (lo + k < hi) ? d : 0;
        if (pack_shift > 0) v[k] = (v[k] << pack_shift) | (v[k] > 0 ? 1 : 0);
      }
      int sum = 0;
#pragma unroll
      for (int k = 0; k < kScanRun; k++) sum += v[k];
      const int x = wave_incl_sum(sum);
      int run = x - sum;
#pragma unroll
      for (int k = 0; k < kScanRun; k++)
        if (lo + k < hi) {
          data[lo + k] = run;
          run += v[k];
        }
      if (tid == 63) scr[0] = x;
    }
    __syncthreads();
    const int total = scr[0];
    __syncthreads();  // scr[0] read everywhere before the next scan writes it
    return total;
  }
  const int per = (n + nt - 1) / nt;
  int total = 0;
  for (int base = 0; base < n; base += nt * kScanRun) {  // chunks of nt * kScanRun
    const int cn = min(n - base, nt * kScanRun);
    const int cper = min(per, kScanRun);
    const int lo = base + min(tid * cper, cn), hi = base + min(tid * cper + cper, cn);
    int v[kScanRun];
#pragma unroll
    for (int k = 0; k < kScanRun; k++) {  // unconditional read, then select (no branch per load)
      const int d = data[min(lo + k, n - 1)];
      v[k] = (lo + k < hi) ? d : 0;
    }
    if (pack_shift > 0) {
#pragma unroll
      for (int k = 0; k < kScanRun; k++) v[k] = (v[k] << pack_shift) | (v[k] > 0 ? 1 : 0);
    }
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanRun; k++) s += v[k];
    const int lane = tid & 63, wid = tid >> 6, nw = nt / 64;
    const int x = wave_incl_sum(s);  // DPP: no LDS round trip per step
    if (lane == 63) scr[wid] = x;
    __syncthreads();
    if (wid == 0) {  // exclusive prefix of the (<= 16) wave totals, one DPP scan
      const int y = lane < nw ? scr[lane] : 0;
      const int inc = wave_incl_sum(y);
      if (lane < nw) scr[lane] = inc - y;
      if (lane == nw - 1) scr[nw] = inc;
    }
    __syncthreads();
    int run = total + scr[wid] + x - s;
#pragma unroll
    for (int k = 0; k < kScanRun; k++)
      if (lo + k < hi) {
        data[lo + k] = run;
        run += v[k];
      }
    total += scr[nt / 64];
    __syncthreads();
  }
  return total;
}

// ---------------------------------------------------------------------------
// fp32 edge linearisation, ba_cuda.cu:265-333 (operation order of the C
// oracle; no contraction).
// ---------------------------------------------------------------------------
struct Lin {
  float w[2], r[2], Jz[2], Ji[2][6], Jj[2][6];
};

#pragma clang fp contract(off)
__device__ __forceinline__ void lin_edge(const float* Pi, const float* Pj, float nx, float ny,
                                         float depth, float tx, float ty, float wx, float wy,
                                         float fx, float fy, float cx, float cy, Lin& o) {
  float ti[3] = {Pi[0], Pi[1], Pi[2]}, qi[4] = {Pi[3], Pi[4], Pi[5], Pi[6]};
  float tj[3] = {Pj[0], Pj[1], Pj[2]}, qj[4] = {Pj[3], Pj[4], Pj[5], Pj[6]};
  float Xi[4], Xj[4];
  Xi[0] = nx;  // (x - cx) / fx, per patch
  Xi[1] = ny;
  Xi[2] = 1.0f;
  Xi[3] = depth;
  float tij[3], qij[4];
  relSE3(ti, qi, tj, qj, tij, qij);
  actSE3(tij, qij, Xi, Xj);
  const float X = Xj[0], Y = Xj[1], Z = Xj[2], W = Xj[3];
  const float d = ((double)Z >= 0.2) ? (float)(1.0 / (double)Z) : 0.0f;  // ba_cuda.cu:296
  const float d2 = d * d;
  const float x1 = fx * (X / Z) + cx;
  const float y1 = fy * (Y / Z) + cy;
  const float rx = tx - x1, ry = ty - y1;
  const bool in_bounds = (sqrtf(rx * rx + ry * ry) < 128.0f) && ((double)Z > 0.2) &&
                         (x1 > -64.0f) && (y1 > -64.0f) && (x1 < 2.0f * cx + 64.0f) &&
                         (y1 < 2.0f * cy + 64.0f);  // :305-306
  const float mask = in_bounds ? 1.0f : 0.0f;
  o.w[0] = mask * wx;
  o.w[1] = mask * wy;
  o.r[0] = rx;
  o.r[1] = ry;
  o.Jz[0] = fx * (tij[0] * d - tij[2] * (X * d2));
  o.Jz[1] = fy * (tij[1] * d - tij[2] * (Y * d2));
  o.Jj[0][0] = fx * W * d;
  o.Jj[0][1] = 0.0f;
  o.Jj[0][2] = fx * -X * W * d2;
  o.Jj[0][3] = fx * -X * Y * d2;
  o.Jj[0][4] = fx * (1 + X * X * d2);
  o.Jj[0][5] = fx * -Y * d;
  o.Jj[1][0] = 0.0f;
  o.Jj[1][1] = fy * W * d;
  o.Jj[1][2] = fy * -Y * W * d2;
  o.Jj[1][3] = fy * (-1 - Y * Y * d2);
  o.Jj[1][4] = fy * (X * Y * d2);
  o.Jj[1][5] = fy * X * d;
  adjSE3(tij, qij, o.Jj[0], o.Ji[0]);
  adjSE3(tij, qij, o.Jj[1], o.Ji[1]);
}
#pragma clang fp contract(fast)

// v_rcp_f64 (~2^-24 relative) + one Newton step (~2^-48): the pivot
// reciprocals sit on the solve's dependency chain, where each dependent fp64
// FMA costs ~36 cycles on gfx950.  gba::rcp_f64 (ba_bgj.hpp) is a different
// function: two Newton steps.
__device__ __forceinline__ double rcp64(double d) {
  const double r = __builtin_amdgcn_rcp(d);
  return __builtin_fma(r, __builtin_fma(-d, r, 1.0), r);
}

}  // namespace bad
}  // namespace dpvo
