// stream.hip -- the front of a run on a sequence as it sits on disk
// (dpvo/stream.py:24-39 and :75-83): undistort, halve and crop a decoded frame
// in one launch, from the raw uint8 frame to the [3, H, W] planes that
// DPVO.__call__ takes and the float32 intrinsics that go with them.
//
// The reference does this on the host with cv2 (undistort -> resize INTER_AREA
// -> crop to a multiple of 16) in a reader process.  Here every output pixel is
// computed from the source directly: the distortion map of the 1 (scale 1) or
// 4 (scale 0.5) undistorted pixels under it is evaluated in fp64 in the
// thread, about 30 operations each, so there is no map table, no state and
// nothing between the calls of a captured graph.
//
//   map      OpenCV's camera model (k1 k2 p1 p2 [k3]) in the order the header
//            gives, FMA contraction off, quantised to 1/32 pixel
//   sample   bilinear in exact integers: 5-bit weights, + 512 >> 10, taps
//            outside the source read 0 (BORDER_CONSTANT)
//   halve    (a + b + c + d + 2) >> 2 over the 2 x 2 block of rounded
//            undistorted pixels: undistort, then INTER_AREA at 1/2
//   crop     top-left, to multiples of 16
//
// Each thread produces 4 x-adjacent output pixels of the three planes and
// stores one 32-bit word per plane (W % 16 == 0 keeps it aligned).  The source
// is a few MB at the most and is read through ordinary cached byte loads.
#include <math.h>

#include "common.hpp"

namespace dpvo {
namespace stream {

constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;  // H0, W0: every index stays far inside int

struct Prepare {
  const uint8_t* raw;
  uint8_t* image;
  float* intrinsics;
  double fx, fy, cx, cy, k1, k2, p1, p2, k3, scale;
  int H0, W0, H, W, swap_rb;
};

// The header's arithmetic, operation for operation: no contraction, so the
// host restatement (numpy, no FMA) rounds identically.
#pragma clang fp contract(off)
__device__ __forceinline__ void distort_q(const Prepare& a, int u, int v, int& qx, int& qy) {
  const double x = ((double)u - a.cx) / a.fx, y = ((double)v - a.cy) / a.fy;
  const double r2 = x * x + y * y;
  const double kr = 1.0 + r2 * (a.k1 + r2 * (a.k2 + r2 * a.k3));
  const double xd = x * kr + (2.0 * a.p1 * x * y + a.p2 * (r2 + 2.0 * x * x));
  const double yd = y * kr + (a.p1 * (r2 + 2.0 * y * y) + 2.0 * a.p2 * x * y);
  const double mx = a.fx * xd + a.cx, my = a.fy * yd + a.cy;
  // a map that leaves the int range (or is NaN) is pinned far outside the source
  const double lim = 1073741824.0;  // 2^30
  qx = (int)fmin(fmax(floor(mx * 32.0 + 0.5), -lim), lim);
  qy = (int)fmin(fmax(floor(my * 32.0 + 0.5), -lim), lim);
}
#pragma clang fp contract(fast)

// the undistorted pixel (u, v) of the C source channels, rounded
template <int C, bool DISTORT>
__device__ __forceinline__ void undistorted(const Prepare& a, int u, int v, int (&val)[C]) {
  const uint8_t* __restrict__ S = a.raw;
  if (!DISTORT) {  // u < W0, v < H0 by the crop
    const size_t o = ((size_t)v * a.W0 + u) * C;
#pragma unroll
    for (int c = 0; c < C; c++) val[c] = S[o + c];
    return;
  }
  int qx, qy;
  distort_q(a, u, v, qx, qy);
  const int ix = qx >> 5, ax = qx & 31, iy = qy >> 5, ay = qy & 31;
  const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
  const bool x0 = ix >= 0 && ix < a.W0, x1 = ix + 1 >= 0 && ix + 1 < a.W0;
  const bool y0 = iy >= 0 && iy < a.H0, y1 = iy + 1 >= 0 && iy + 1 < a.H0;
  // clamped addresses: a tap outside is never read out of bounds, its value is dropped
  const int cx0 = min(max(ix, 0), a.W0 - 1), cx1 = min(max(ix + 1, 0), a.W0 - 1);
  const int cy0 = min(max(iy, 0), a.H0 - 1), cy1 = min(max(iy + 1, 0), a.H0 - 1);
  const size_t o00 = ((size_t)cy0 * a.W0 + cx0) * C, o01 = ((size_t)cy0 * a.W0 + cx1) * C;
  const size_t o10 = ((size_t)cy1 * a.W0 + cx0) * C, o11 = ((size_t)cy1 * a.W0 + cx1) * C;
#pragma unroll
  for (int c = 0; c < C; c++) {
    const int s00 = (y0 && x0) ? S[o00 + c] : 0, s01 = (y0 && x1) ? S[o01 + c] : 0;
    const int s10 = (y1 && x0) ? S[o10 + c] : 0, s11 = (y1 && x1) ? S[o11 + c] : 0;
    val[c] = (w00 * s00 + w01 * s01 + w10 * s10 + w11 * s11 + 512) >> 10;
  }
}

template <int C, bool DISTORT, bool HALF>
__global__ void __launch_bounds__(kThreads) frame_prepare_kernel(Prepare a) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t == 0) {
    a.intrinsics[0] = (float)(a.fx * a.scale);
    a.intrinsics[1] = (float)(a.fy * a.scale);
    a.intrinsics[2] = (float)(a.cx * a.scale);
    a.intrinsics[3] = (float)(a.cy * a.scale);
  }
  const int wq = a.W >> 2;  // words per output row
  if (t >= a.H * wq) return;
  const int row = t / wq, x0 = (t - row * wq) << 2;
  uint32_t word[C] = {};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int px[C];
    if (HALF) {
      int s[C] = {};
#pragma unroll
      for (int d = 0; d < 4; d++) {
        int one[C];
        undistorted<C, DISTORT>(a, 2 * (x0 + k) + (d & 1), 2 * row + (d >> 1), one);
#pragma unroll
        for (int c = 0; c < C; c++) s[c] += one[c];
      }
#pragma unroll
      for (int c = 0; c < C; c++) px[c] = (s[c] + 2) >> 2;
    } else {
      undistorted<C, DISTORT>(a, x0 + k, row, px);
    }
#pragma unroll
    for (int c = 0; c < C; c++) word[c] |= (uint32_t)px[c] << (8 * k);
  }
  const size_t plane = (size_t)a.H * a.W, o = (size_t)row * a.W + x0;
#pragma unroll
  for (int p = 0; p < 3; p++) {
    // grey is replicated into the three planes (what cv2.imread delivers)
    const int c = C == 1 ? 0 : (a.swap_rb ? 2 - p : p);
    *reinterpret_cast<uint32_t*>(a.image + p * plane + o) = word[C == 1 ? 0 : c];
  }
}

template <int C>
void launch(const Prepare& a, bool distort, bool half, hipStream_t s) {
  const unsigned grid = (unsigned)(((size_t)a.H * (a.W >> 2) + kThreads - 1) / kThreads);
  if (distort && half)
    hipLaunchKernelGGL((frame_prepare_kernel<C, true, true>), dim3(grid), dim3(kThreads), 0, s, a);
  else if (distort)
    hipLaunchKernelGGL((frame_prepare_kernel<C, true, false>), dim3(grid), dim3(kThreads), 0, s, a);
  else if (half)
    hipLaunchKernelGGL((frame_prepare_kernel<C, false, true>), dim3(grid), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((frame_prepare_kernel<C, false, false>), dim3(grid), dim3(kThreads), 0, s, a);
}

}  // namespace stream
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT int dpvo_frame_prepare_shape(int H0, int W0, double scale, int* H, int* W) {
  if (!H || !W || H0 <= 0 || W0 <= 0) return DPVO_ERR_INVALID;
  if (scale != 1.0 && scale != 0.5) return DPVO_ERR_UNSUPPORTED;
  if (H0 > stream::kMaxSide || W0 > stream::kMaxSide) return DPVO_ERR_UNSUPPORTED;
  if (scale == 0.5 && ((H0 | W0) & 1)) return DPVO_ERR_UNSUPPORTED;
  const int H1 = scale == 0.5 ? H0 / 2 : H0, W1 = scale == 0.5 ? W0 / 2 : W0;
  *H = H1 - H1 % 16;
  *W = W1 - W1 % 16;
  if (*H <= 0 || *W <= 0) return DPVO_ERR_UNSUPPORTED;
  return DPVO_OK;
}

DPVO_EXPORT int dpvo_frame_prepare(const uint8_t* raw, int H0, int W0, int channels,
                                   const double* calib, int ncalib, double scale, int swap_rb,
                                   uint8_t* image, float* intrinsics, void* stream) {
  if (!raw || !calib || !image || !intrinsics) return DPVO_ERR_INVALID;
  if (H0 <= 0 || W0 <= 0 || (channels != 1 && channels != 3)) return DPVO_ERR_INVALID;
  if (swap_rb < 0 || swap_rb > 1) return DPVO_ERR_INVALID;
  if (((uintptr_t)image & 3) != 0) return DPVO_ERR_INVALID;  // one 32-bit word per store
  const bool count_ok = ncalib == 4 || ncalib == 8 || ncalib == 9;
  if (count_ok && (!isfinite(calib[0]) || !isfinite(calib[1]) || calib[0] == 0.0 || calib[1] == 0.0))
    return DPVO_ERR_INVALID;
  if (!count_ok) return DPVO_ERR_UNSUPPORTED;
  stream::Prepare a;
  const int st = dpvo_frame_prepare_shape(H0, W0, scale, &a.H, &a.W);
  if (st != DPVO_OK) return st;
  a.raw = raw;
  a.image = image;
  a.intrinsics = intrinsics;
  a.fx = calib[0];
  a.fy = calib[1];
  a.cx = calib[2];
  a.cy = calib[3];
  a.k1 = ncalib > 4 ? calib[4] : 0.0;
  a.k2 = ncalib > 4 ? calib[5] : 0.0;
  a.p1 = ncalib > 4 ? calib[6] : 0.0;
  a.p2 = ncalib > 4 ? calib[7] : 0.0;
  a.k3 = ncalib > 8 ? calib[8] : 0.0;
  a.scale = scale;
  a.H0 = H0;
  a.W0 = W0;
  a.swap_rb = swap_rb;
  if (channels == 1)
    stream::launch<1>(a, ncalib > 4, scale == 0.5, as_stream(stream));
  else
    stream::launch<3>(a, ncalib > 4, scale == 0.5, as_stream(stream));
  return launch_status();
}
