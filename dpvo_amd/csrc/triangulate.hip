// triangulate.hip -- the 3-D keypoints of the long-term loop closure
// (dpvo/loop_closure/long_term.py:90-136 joined with :213-217) on gfx950, one
// launch, no host sync.
//
// A keypoint of frame i with a partner in frame i-1 and in frame i+1 is a
// track.  Its inverse depth starts at the lower median of the frame's patch
// depths (torch.median) and takes `iterations` steps of the reference's
// structure-only bundle adjustment over its two observations, weight 1
// (ba_cuda.cu:521-531: dZ = u / (C + lmbda)); the linearisation (residual, Jz,
// the outlier and depth gates) is bad::lin_edge, the one the BA kernels use, the
// C / u sums are fp64 and the retraction is clamped as theirs is.  Then the
// reprojection residual into both neighbours, the camera-frame point and the
// keep rule, and the kept indices compacted in ascending order.
//
// One workgroup: a keypoint per lane, kTriT lanes, every lane of the launch in
// one scan for the ordered compaction.  The median is a rank count in LDS.
#include <math.h>

#include "ba_device.hpp"

namespace dpvo {
namespace tri {

constexpr int kTriT = 1024;
constexpr int kMaxTracks = 4096;
constexpr int kMaxM = 1024;

struct Args {
  const float* poses;       // [3, 7] frames i-1, i, i+1
  const float* intrinsics;  // [3, 4] at image resolution
  const float* disps;       // [M] with stride
  const float* kps0;        // [N0, 2]
  const float* kps1;        // [N1, 2]
  const float* kps2;        // [N2, 2]
  const int64_t* m10;       // [N1] partner in kps0 or -1
  const int64_t* m12;       // [N1] partner in kps2 or -1
  int disp_stride, M, N0, N1, N2, iterations;
  float max_depth, max_residual, lmbda;
  float* points;  // [N1, 3]
  float* disp;    // [N1]
  uint8_t* keep;  // [N1]
  int64_t* sel;   // [N1]
  int32_t* count;
};

__device__ __forceinline__ uint32_t float_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kTriT) triangulate_kernel(Args a) {
  __shared__ float dval[kMaxM];
  __shared__ uint8_t kept[kMaxTracks];
  __shared__ float med;
  __shared__ int scr[kTriT / 64 + 1];
  const int tid = threadIdx.x;

  // lower median of the M depths: the value of rank (M - 1) / 2
  if (tid < a.M) dval[tid] = a.disps[(size_t)tid * a.disp_stride];
  __syncthreads();
  if (tid < a.M) {
    const float v = dval[tid];
    const uint32_t key = float_key(v);
    int rank = 0;
    for (int j = 0; j < a.M; j++) {
      const uint32_t k = float_key(dval[j]);
      rank += (k < key || (k == key && j < tid)) ? 1 : 0;
    }
    if (rank == (a.M - 1) / 2) med = v;
  }
  __syncthreads();
  const float d0 = med;

  const float* K = a.intrinsics;
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];  // the BA reads row 0 (ba_cuda.cu:277)
  const double lam = (double)a.lmbda;

  for (int n = tid; n < a.N1; n += kTriT) {
    const int64_t p0 = a.m10[n], p2 = a.m12[n];
    const bool track = p0 >= 0 && p0 < a.N0 && p2 >= 0 && p2 < a.N2;
    float X[3] = {0.f, 0.f, 0.f}, d = 0.f;
    bool keep = false;
    if (track) {
      const float u1 = a.kps1[2 * n], v1 = a.kps1[2 * n + 1];
      const float t[2][2] = {{a.kps0[2 * p0], a.kps0[2 * p0 + 1]},
                             {a.kps2[2 * p2], a.kps2[2 * p2 + 1]}};
      const float nx = (u1 - cx) / fx, ny = (v1 - cy) / fy;
      d = d0;
      bad::Lin L;
      for (int it = 0; it < a.iterations; it++) {
        double C = 0.0, U = 0.0;
#pragma unroll
        for (int o = 0; o < 2; o++) {
          bad::lin_edge(a.poses + 7, a.poses + 14 * o, nx, ny, d, t[o][0], t[o][1], 1.0f, 1.0f, fx,
                        fy, cx, cy, L);
#pragma unroll
          for (int row = 0; row < 2; row++) {  // ba_cuda.cu:352-373
            const double wr = L.w[row];
            const double wz = wr * L.Jz[row];
            C += wz * L.Jz[row];
            U += wr * L.r[row] * L.Jz[row];
          }
        }
        const float dz = (float)((1.0 / (C + lam)) * U);  // Q = 1 / (C + lmbda) (:519)
        d = d + dz;
        d = (d > 20.0f) ? 1.0f : d;  // patch_retr_kernel :225-228
        d = (float)fmax((double)d, 1e-4);
      }
      float res = 0.f;
#pragma unroll
      for (int o = 0; o < 2; o++) {
        bad::lin_edge(a.poses + 7, a.poses + 14 * o, nx, ny, d, t[o][0], t[o][1], 1.0f, 1.0f, fx, fy,
                      cx, cy, L);
        const float r = sqrtf(L.r[0] * L.r[0] + L.r[1] * L.r[1]);
        res = (r > res || r != r) ? r : res;  // a NaN residual is never kept
      }
      // pops.iproj with the intrinsics of frame i (row 1), divided by the depth
      X[0] = ((u1 - K[6]) / K[4]) / d;
      X[1] = ((v1 - K[7]) / K[5]) / d;
      X[2] = 1.0f / d;
      keep = res < a.max_residual && X[2] < a.max_depth;
    }
    a.points[3 * n] = X[0];
    a.points[3 * n + 1] = X[1];
    a.points[3 * n + 2] = X[2];
    a.disp[n] = d;
    a.keep[n] = keep ? 1 : 0;
    kept[n] = keep ? 1 : 0;
  }
  __syncthreads();

  // kept indices in ascending order: runs of `per` keypoints per thread
  const int per = (a.N1 + kTriT - 1) / kTriT;
  const int lo = min(tid * per, a.N1), hi = min(lo + per, a.N1);
  int cnt = 0;
  for (int n = lo; n < hi; n++) cnt += kept[n];
  int total;
  int pos = block_excl_sum(cnt, scr, total);
  for (int n = lo; n < hi; n++)
    if (kept[n]) a.sel[pos++] = n;
  for (int p = total + tid; p < a.N1; p += kTriT) a.sel[p] = -1;
  if (tid == 0) a.count[0] = total;
}

}  // namespace tri
}  // namespace dpvo

using namespace dpvo;

DPVO_EXPORT int dpvo_triangulate_tracks(const float* poses, const float* intrinsics,
                                        const float* disps, int disp_stride, int M,
                                        const float* kps0, int N0, const float* kps1, int N1,
                                        const float* kps2, int N2, const int64_t* m10,
                                        const int64_t* m12, float max_depth, float max_residual,
                                        int iterations, float lmbda, float* points, float* disp,
                                        uint8_t* keep, int64_t* sel, int32_t* count, void* stream) {
  if (!poses || !intrinsics || !disps || !kps0 || !kps1 || !kps2 || !m10 || !m12 || !points ||
      !disp || !keep || !sel || !count)
    return DPVO_ERR_INVALID;
  if (M < 1 || N0 < 1 || N1 < 1 || N2 < 1 || disp_stride < 1 || iterations < 0)
    return DPVO_ERR_INVALID;
  if (!(lmbda >= 0.0f)) return DPVO_ERR_INVALID;
  if (M > tri::kMaxM || N1 > tri::kMaxTracks) return DPVO_ERR_UNSUPPORTED;
  tri::Args a;
  a.poses = poses;
  a.intrinsics = intrinsics;
  a.disps = disps;
  a.kps0 = kps0;
  a.kps1 = kps1;
  a.kps2 = kps2;
  a.m10 = m10;
  a.m12 = m12;
  a.disp_stride = disp_stride;
  a.M = M; a.N0 = N0; a.N1 = N1; a.N2 = N2; a.iterations = iterations;
  a.max_depth = max_depth;
  a.max_residual = max_residual;
  a.lmbda = lmbda;
  a.points = points;
  a.disp = disp;
  a.keep = keep;
  a.sel = sel;
  a.count = count;
  hipLaunchKernelGGL(tri::triangulate_kernel, dim3(1), dim3(tri::kTriT), 0, as_stream(stream), a);
  return launch_status();
}
