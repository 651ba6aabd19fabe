// lie.hip -- lietorch SO3 (group 1) / SE3 (group 3) / Sim3 (group 4) on gfx950
// (L-SE3).  The Sim3 math lives in sim3.hpp (shared with pgo.hip), the SO3 /
// SE3 device functions in lie_se3.hpp (shared with frontend.hip).
//
// Reference semantics: dpvo/lietorch/include/so3.h, se3.h and the kernels of
// dpvo/lietorch/src/lietorch_gpu.cu:20-294 (one thread per group element,
// Eigen math).  Restated here without Eigen: plain fixed-size register math,
// templated on float/double, quaternion (x, y, z, w) normalised on load
// (so3.h:95-97), tangent ordering (tau, phi).
#include <type_traits>

#include "common.hpp"
#include "lie_se3.hpp"
#include "sim3.hpp"

namespace dpvo {
namespace lie {

enum { OP_EXP = 0, OP_LOG, OP_INV, OP_MUL, OP_ADJ, OP_ADJT, OP_ACT, OP_ACT4, OP_MATRIX, OP_PROJ,
       OP_JINV };

// ---- SE3 forward, one element (lietorch_gpu.cu:20-294) ----
template <typename S>
__device__ void se3_fwd(int op, const S* X, const S* Y, S* out) {
  switch (op) {
    case OP_EXP: se3_store(se3_exp(X), out); break;
    case OP_LOG: se3_log(se3_load(X), out); break;
    case OP_INV: se3_store(se3_inv(se3_load(X)), out); break;
    case OP_MUL: se3_store(se3_mul(se3_load(X), se3_load(Y)), out); break;
    case OP_ADJ: { S A[36]; se3_Adj(se3_load(X), A); mat_vec(A, Y, 6, 6, out); } break;
    case OP_ADJT: { S A[36]; se3_Adj(se3_load(X), A); rowvec_mat(Y, A, 6, 6, out); } break;
    case OP_ACT: {
      const SE3g<S> g = se3_load(X);
      S p[3];
      qact(g.q, Y, p);
      for (int i = 0; i < 3; i++) out[i] = p[i] + g.t[i];
    } break;
    case OP_ACT4: {
      const SE3g<S> g = se3_load(X);
      S p[3];
      qact(g.q, Y, p);
      for (int i = 0; i < 3; i++) out[i] = p[i] + g.t[i] * Y[3];
      out[3] = Y[3];
    } break;
    case OP_MATRIX: {
      const SE3g<S> g = se3_load(X);
      S R[9];
      qmat(g.q, R);
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[i * 4 + j] = R[i * 3 + j];
        out[i * 4 + 3] = g.t[i];
        out[12 + i] = 0;
      }
      out[15] = 1;
    } break;
    case OP_PROJ: {  // se3.h:403-411, so3.h:141-151
      const SE3g<S> g = se3_load(X);
      for (int i = 0; i < 49; i++) out[i] = 0;
      S mt[3] = {-g.t[0], -g.t[1], -g.t[2]}, H[9];
      hat(mt, H);
      for (int i = 0; i < 3; i++) {
        out[i * 7 + i] = 1;
        for (int j = 0; j < 3; j++) out[i * 7 + 3 + j] = H[i * 3 + j];
      }
      S mv[3] = {-g.q.x, -g.q.y, -g.q.z}, Hq[9];
      hat(mv, Hq);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
          out[(3 + i) * 7 + 3 + j] = S(0.5) * ((i == j ? g.q.w : S(0)) + Hq[i * 3 + j]);
      out[6 * 7 + 3] = S(0.5) * -g.q.x;
      out[6 * 7 + 4] = S(0.5) * -g.q.y;
      out[6 * 7 + 5] = S(0.5) * -g.q.z;
    } break;
    case OP_JINV: {
      S a[6], J[36];
      se3_log(se3_load(X), a);
      se3_jl_inv(a, J);
      mat_vec(J, Y, 6, 6, out);
    } break;
  }
}

// ---- SE3 backward, one element (lietorch_gpu.cu:32-256) ----
template <typename S>
__device__ void se3_bwd(int op, const S* g, const S* X, const S* Y, S* o0, S* o1) {
  S A[36], T[6], b[6];
  switch (op) {
    case OP_EXP: se3_jl(X, A); rowvec_mat(g, A, 6, 6, o0); break;
    case OP_LOG:
      se3_log(se3_load(X), b);
      se3_jl_inv(b, A);
      rowvec_mat(g, A, 6, 6, o0);
      o0[6] = 0;
      break;
    case OP_INV:
      se3_Adj(se3_inv(se3_load(X)), A);
      rowvec_mat(g, A, 6, 6, T);
      for (int i = 0; i < 6; i++) o0[i] = -T[i];
      o0[6] = 0;
      break;
    case OP_MUL:
      for (int i = 0; i < 6; i++) o0[i] = g[i];
      o0[6] = 0;
      se3_Adj(se3_load(X), A);
      rowvec_mat(g, A, 6, 6, o1);
      o1[6] = 0;
      break;
    case OP_ADJ:
      se3_Adj(se3_load(X), A);
      mat_vec(A, Y, 6, 6, b);
      rowvec_mat(g, A, 6, 6, o1);
      se3_adj_small(b, A);
      rowvec_mat(g, A, 6, 6, T);
      for (int i = 0; i < 6; i++) o0[i] = -T[i];
      o0[6] = 0;
      break;
    case OP_ADJT:
      se3_Adj(se3_load(X), A);
      mat_vec(A, g, 6, 6, b);
      for (int i = 0; i < 6; i++) o1[i] = b[i];
      se3_adj_small(b, A);
      rowvec_mat(Y, A, 6, 6, T);
      for (int i = 0; i < 6; i++) o0[i] = -T[i];
      o0[6] = 0;
      break;
    case OP_ACT: {
      const SE3g<S> G = se3_load(X);
      S R[9], q[3];
      qmat(G.q, R);
      rowvec_mat(g, R, 3, 3, o1);
      qact(G.q, Y, q);
      for (int i = 0; i < 3; i++) q[i] = -(q[i] + G.t[i]);
      S H[9], J[18];
      hat(q, H);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          J[i * 6 + j] = (i == j) ? S(1) : S(0);
          J[i * 6 + 3 + j] = H[i * 3 + j];
        }
      rowvec_mat(g, J, 3, 6, o0);
      o0[6] = 0;
    } break;
    case OP_ACT4: {
      const SE3g<S> G = se3_load(X);
      S R[9], M4[16], q[3];
      qmat(G.q, R);
      for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) M4[i * 4 + j] = R[i * 3 + j];
        M4[i * 4 + 3] = G.t[i];
        M4[12 + i] = 0;
      }
      M4[15] = 1;
      rowvec_mat(g, M4, 4, 4, o1);
      qact(G.q, Y, q);
      for (int i = 0; i < 3; i++) q[i] = -(q[i] + G.t[i] * Y[3]);
      S H[9], J[24];
      hat(q, H);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          J[i * 6 + j] = (i == j) ? Y[3] : S(0);
          J[i * 6 + 3 + j] = H[i * 3 + j];
        }
      for (int j = 0; j < 6; j++) J[18 + j] = 0;
      rowvec_mat(g, J, 4, 6, o0);
      o0[6] = 0;
    } break;
  }
}

// ---- SO3 forward / backward, one element ----
template <typename S>
__device__ void so3_fwd(int op, const S* X, const S* Y, S* out) {
  auto ld = [](const S* d) { return qnorm<S>(d[0], d[1], d[2], d[3]); };
  auto st = [](const Q4<S>& q, S* d) { d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w; };
  S R[9];
  switch (op) {
    case OP_EXP: st(so3_exp(X), out); break;
    case OP_LOG: so3_log(ld(X), out); break;
    case OP_INV: { const Q4<S> q = ld(X); st(qnorm<S>(-q.x, -q.y, -q.z, q.w), out); } break;
    case OP_MUL: st(qmul(ld(X), ld(Y)), out); break;
    case OP_ADJ: qmat(ld(X), R); mat_vec(R, Y, 3, 3, out); break;
    case OP_ADJT: qmat(ld(X), R); rowvec_mat(Y, R, 3, 3, out); break;
    case OP_ACT: qact(ld(X), Y, out); break;
    case OP_ACT4: qact(ld(X), Y, out); out[3] = Y[3]; break;
    case OP_MATRIX:
      qmat(ld(X), R);
      for (int i = 0; i < 16; i++) out[i] = 0;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[i * 4 + j] = R[i * 3 + j];
      out[15] = 1;
      break;
    case OP_PROJ: {
      const Q4<S> q = ld(X);
      for (int i = 0; i < 16; i++) out[i] = 0;
      S mv[3] = {-q.x, -q.y, -q.z}, H[9];
      hat(mv, H);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[i * 4 + j] = S(0.5) * ((i == j ? q.w : S(0)) + H[i * 3 + j]);
      out[12] = S(0.5) * -q.x; out[13] = S(0.5) * -q.y; out[14] = S(0.5) * -q.z;
    } break;
    case OP_JINV: {
      S a[3], J[9];
      so3_log(ld(X), a);
      so3_jl_inv(a, J);
      mat_vec(J, Y, 3, 3, out);
    } break;
  }
}

template <typename S>
__device__ void so3_bwd(int op, const S* g, const S* X, const S* Y, S* o0, S* o1) {
  auto ld = [](const S* d) { return qnorm<S>(d[0], d[1], d[2], d[3]); };
  S R[9], J[9], a[3], T[3];
  switch (op) {
    case OP_EXP: so3_jl(X, J); rowvec_mat(g, J, 3, 3, o0); break;
    case OP_LOG: so3_log(ld(X), a); so3_jl_inv(a, J); rowvec_mat(g, J, 3, 3, o0); o0[3] = 0; break;
    case OP_INV: {
      const Q4<S> q = ld(X);
      qmat(qnorm<S>(-q.x, -q.y, -q.z, q.w), R);
      rowvec_mat(g, R, 3, 3, T);
      for (int i = 0; i < 3; i++) o0[i] = -T[i];
      o0[3] = 0;
    } break;
    case OP_MUL:
      for (int i = 0; i < 3; i++) o0[i] = g[i];
      o0[3] = 0;
      qmat(ld(X), R);
      rowvec_mat(g, R, 3, 3, o1);
      o1[3] = 0;
      break;
    case OP_ADJ:
      qmat(ld(X), R);
      mat_vec(R, Y, 3, 3, a);
      rowvec_mat(g, R, 3, 3, o1);
      hat(a, J);
      rowvec_mat(g, J, 3, 3, T);
      for (int i = 0; i < 3; i++) o0[i] = -T[i];
      o0[3] = 0;
      break;
    case OP_ADJT:
      qmat(ld(X), R);
      mat_vec(R, g, 3, 3, a);
      for (int i = 0; i < 3; i++) o1[i] = a[i];
      hat(a, J);
      rowvec_mat(Y, J, 3, 3, T);
      for (int i = 0; i < 3; i++) o0[i] = -T[i];
      o0[3] = 0;
      break;
    case OP_ACT: {
      const Q4<S> q = ld(X);
      qmat(q, R);
      rowvec_mat(g, R, 3, 3, o1);
      qact(q, Y, a);
      for (int i = 0; i < 3; i++) a[i] = -a[i];
      hat(a, J);
      rowvec_mat(g, J, 3, 3, o0);
      o0[3] = 0;
    } break;
    case OP_ACT4: {
      const Q4<S> q = ld(X);
      qmat(q, R);
      S M4[16];
      for (int i = 0; i < 16; i++) M4[i] = 0;
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M4[i * 4 + j] = R[i * 3 + j];
      M4[15] = 1;
      rowvec_mat(g, M4, 4, 4, o1);
      qact(q, Y, a);
      for (int i = 0; i < 3; i++) a[i] = -a[i];
      S J4[12];
      hat(a, J);
      for (int i = 0; i < 9; i++) J4[i] = J[i];
      J4[9] = J4[10] = J4[11] = 0;
      rowvec_mat(g, J4, 4, 3, o0);
      o0[3] = 0;
    } break;
  }
}

struct Dims {
  int xin, yin, out, gin, o0, o1;
};

__host__ __device__ constexpr int dim_K(int group) { return group == 1 ? 3 : group == 3 ? 6 : 7; }
__host__ __device__ constexpr int dim_N(int group) { return dim_K(group) + 1; }

__host__ __device__ constexpr Dims fwd_dims(int group, int op) {
  const int K = dim_K(group), N = dim_N(group);
  return op == OP_EXP    ? Dims{K, 0, N, 0, 0, 0}
         : op == OP_LOG  ? Dims{N, 0, K, 0, 0, 0}
         : op == OP_INV  ? Dims{N, 0, N, 0, 0, 0}
         : op == OP_MUL  ? Dims{N, N, N, 0, 0, 0}
         : op == OP_ACT  ? Dims{N, 3, 3, 0, 0, 0}
         : op == OP_ACT4 ? Dims{N, 4, 4, 0, 0, 0}
         : op == OP_MATRIX ? Dims{N, 0, 16, 0, 0, 0}
         : op == OP_PROJ ? Dims{N, 0, N * N, 0, 0, 0}
                         : Dims{N, K, K, 0, 0, 0};  // ADJ, ADJT, JINV
}
__host__ __device__ constexpr Dims bwd_dims(int group, int op) {
  const int K = dim_K(group), N = dim_N(group);
  return op == OP_EXP    ? Dims{K, 0, 0, N, K, 0}
         : op == OP_LOG  ? Dims{N, 0, 0, K, N, 0}
         : op == OP_INV  ? Dims{N, 0, 0, N, N, 0}
         : op == OP_MUL  ? Dims{N, N, 0, N, N, N}
         : op == OP_ACT  ? Dims{N, 3, 0, 3, N, 3}
         : op == OP_ACT4 ? Dims{N, 4, 0, 4, N, 4}
                         : Dims{N, K, 0, K, N, K};  // ADJ, ADJT
}

// One thread per group element; (group, op) are template parameters so every
// loop bound is a compile-time constant and the operands stay in registers.
// Sim3 (G == 4) computes in fp64 whatever the tensors' dtype (sim3.hpp).
template <typename S, int G>
using Compute = typename std::conditional<G == 4, double, S>::type;

template <typename S, int G, int OP>
__global__ void __launch_bounds__(256)
    lie_fwd_kernel(int n, const S* __restrict__ X, const S* __restrict__ Y, S* __restrict__ out) {
  constexpr Dims d = fwd_dims(G, OP);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    Compute<S, G> x[8], y[8], o[64];
#pragma unroll
    for (int k = 0; k < d.xin; k++) x[k] = X[(size_t)i * d.xin + k];
#pragma unroll
    for (int k = 0; k < d.yin; k++) y[k] = Y[(size_t)i * d.yin + k];
    if constexpr (G == 4)
      sim3::fwd(OP, x, y, o);
    else if constexpr (G == 3)
      se3_fwd<S>(OP, x, y, o);
    else
      so3_fwd<S>(OP, x, y, o);
#pragma unroll
    for (int k = 0; k < d.out; k++) out[(size_t)i * d.out + k] = (S)o[k];
  }
}

template <typename S, int G, int OP>
__global__ void __launch_bounds__(256)
    lie_bwd_kernel(int n, const S* __restrict__ Gr, const S* __restrict__ X,
                   const S* __restrict__ Y, S* __restrict__ o0, S* __restrict__ o1) {
  constexpr Dims d = bwd_dims(G, OP);
  constexpr int K = dim_K(G);
  // gradient rows of group elements are N-strided, their first K entries used
  constexpr int gread = (OP == OP_EXP || OP == OP_INV || OP == OP_MUL) ? K : d.gin;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    Compute<S, G> x[8], y[8], g[8], a[8], b[8];
#pragma unroll
    for (int k = 0; k < d.xin; k++) x[k] = X[(size_t)i * d.xin + k];
#pragma unroll
    for (int k = 0; k < d.yin; k++) y[k] = Y[(size_t)i * d.yin + k];
#pragma unroll
    for (int k = 0; k < gread; k++) g[k] = Gr[(size_t)i * d.gin + k];
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = b[k] = 0;
    if constexpr (G == 4)
      sim3::bwd(OP, g, x, y, a, b);
    else if constexpr (G == 3)
      se3_bwd<S>(OP, g, x, y, a, b);
    else
      so3_bwd<S>(OP, g, x, y, a, b);
#pragma unroll
    for (int k = 0; k < d.o0; k++) o0[(size_t)i * d.o0 + k] = (S)a[k];
#pragma unroll
    for (int k = 0; k < d.o1; k++) o1[(size_t)i * d.o1 + k] = (S)b[k];
  }
}

template <typename S, int G>
int launch_fwd(int op, int n, const void* X, const void* Y, void* out, hipStream_t s,
               unsigned grid) {
#define DPVO_LIE_F(OPV)                                                                        \
  case OPV:                                                                                    \
    hipLaunchKernelGGL((lie_fwd_kernel<S, G, OPV>), dim3(grid), dim3(256), 0, s, n,            \
                       (const S*)X, (const S*)Y, (S*)out);                                     \
    break;
  switch (op) {
    DPVO_LIE_F(OP_EXP) DPVO_LIE_F(OP_LOG) DPVO_LIE_F(OP_INV) DPVO_LIE_F(OP_MUL)
    DPVO_LIE_F(OP_ADJ) DPVO_LIE_F(OP_ADJT) DPVO_LIE_F(OP_ACT) DPVO_LIE_F(OP_ACT4)
    DPVO_LIE_F(OP_MATRIX) DPVO_LIE_F(OP_PROJ) DPVO_LIE_F(OP_JINV)
    default: return DPVO_ERR_INVALID;
  }
#undef DPVO_LIE_F
  return launch_status();
}

template <typename S, int G>
int launch_bwd(int op, int n, const void* Gr, const void* X, const void* Y, void* o0, void* o1,
               hipStream_t s, unsigned grid) {
#define DPVO_LIE_B(OPV)                                                                        \
  case OPV:                                                                                    \
    hipLaunchKernelGGL((lie_bwd_kernel<S, G, OPV>), dim3(grid), dim3(256), 0, s, n,            \
                       (const S*)Gr, (const S*)X, (const S*)Y, (S*)o0, (S*)o1);                \
    break;
  switch (op) {
    DPVO_LIE_B(OP_EXP) DPVO_LIE_B(OP_LOG) DPVO_LIE_B(OP_INV) DPVO_LIE_B(OP_MUL)
    DPVO_LIE_B(OP_ADJ) DPVO_LIE_B(OP_ADJT) DPVO_LIE_B(OP_ACT) DPVO_LIE_B(OP_ACT4)
    default: return DPVO_ERR_INVALID;
  }
#undef DPVO_LIE_B
  return launch_status();
}

}  // namespace lie
}  // namespace dpvo

using namespace dpvo;

static unsigned lie_grid(int n) {
  int g = (n + 255) / 256;
  if (g > 65536) g = 65536;
  return g > 0 ? g : 1;
}

DPVO_EXPORT int dpvo_lie_forward(int group, int op, int dtype, int n, const void* X, const void* Y,
                                 void* out, void* stream) {
  if (group != 1 && group != 3 && group != 4) return DPVO_ERR_UNSUPPORTED;  // 2 = RxSO3
  if (op < 0 || op > lie::OP_JINV || n < 0) return DPVO_ERR_INVALID;
  if (n == 0) return DPVO_OK;
  hipStream_t s = as_stream(stream);
  const unsigned g = lie_grid(n);
  if (dtype == DPVO_F32)
    return group == 4   ? lie::launch_fwd<float, 4>(op, n, X, Y, out, s, g)
           : group == 3 ? lie::launch_fwd<float, 3>(op, n, X, Y, out, s, g)
                        : lie::launch_fwd<float, 1>(op, n, X, Y, out, s, g);
  if (dtype == DPVO_F64)
    return group == 4   ? lie::launch_fwd<double, 4>(op, n, X, Y, out, s, g)
           : group == 3 ? lie::launch_fwd<double, 3>(op, n, X, Y, out, s, g)
                        : lie::launch_fwd<double, 1>(op, n, X, Y, out, s, g);
  return DPVO_ERR_UNSUPPORTED;
}

DPVO_EXPORT int dpvo_lie_backward(int group, int op, int dtype, int n, const void* grad,
                                  const void* X, const void* Y, void* out0, void* out1,
                                  void* stream) {
  if (group != 1 && group != 3 && group != 4) return DPVO_ERR_UNSUPPORTED;  // 2 = RxSO3
  if (op < 0 || op > lie::OP_ACT4 || n < 0) return DPVO_ERR_INVALID;
  if (n == 0) return DPVO_OK;
  hipStream_t s = as_stream(stream);
  const unsigned g = lie_grid(n);
  if (dtype == DPVO_F32)
    return group == 4   ? lie::launch_bwd<float, 4>(op, n, grad, X, Y, out0, out1, s, g)
           : group == 3 ? lie::launch_bwd<float, 3>(op, n, grad, X, Y, out0, out1, s, g)
                        : lie::launch_bwd<float, 1>(op, n, grad, X, Y, out0, out1, s, g);
  if (dtype == DPVO_F64)
    return group == 4   ? lie::launch_bwd<double, 4>(op, n, grad, X, Y, out0, out1, s, g)
           : group == 3 ? lie::launch_bwd<double, 3>(op, n, grad, X, Y, out0, out1, s, g)
                        : lie::launch_bwd<double, 1>(op, n, grad, X, Y, out0, out1, s, g);
  return DPVO_ERR_UNSUPPORTED;
}

DPVO_EXPORT const char* dpvo_status_string(int status) {
  switch (status) {
    case DPVO_OK: return "ok";
    case DPVO_ERR_INVALID: return "invalid argument";
    case DPVO_ERR_LAUNCH: return "kernel launch failed";
    case DPVO_ERR_UNSUPPORTED: return "unsupported configuration";
    case DPVO_ERR_WORKSPACE: return "workspace too small";
  }
  return "unknown status";
}

#ifndef DPVO_GIT_REV
#define DPVO_GIT_REV "dev"
#endif
DPVO_EXPORT const char* dpvo_version(void) { return "dpvo_hot gfx950 " DPVO_GIT_REV; }
