// update_layout.hpp -- what update_op.hip (forward) and update_bwd.hip
// (backward) share: the group plan, the parameter tensor indices and the layout
// of the `saved` buffer that dpvo_update_forward_train fills and
// dpvo_update_backward reads.
#pragma once

#include "common.hpp"

namespace dpvo {
namespace upd {

constexpr int kD = 384;
constexpr float kEps = 1e-3f;
constexpr int kTensors = 50;

// group plan of one id array: members[off[g] + pos] = edge, ascending inside a
// group; off[E + 1]: the group count
struct Plan {
  int *rep, *pos, *dense, *off, *size, *members;
};
inline size_t rows_bytes(int E) { return ((size_t)E * kD * 4 + 255) & ~(size_t)255; }
inline size_t ints_bytes(int E) { return ((size_t)(E + 2) * 4 + 255) & ~(size_t)255; }
inline size_t r256(size_t n) { return (n + 255) & ~(size_t)255; }
inline char* carve_plans(char* p, int E, Plan (&pl)[2]) {
  for (int g = 0; g < 2; g++) {
    int** a[6] = {&pl[g].rep, &pl[g].pos, &pl[g].dense, &pl[g].off, &pl[g].size, &pl[g].members};
    for (auto q : a) { *q = (int*)p; p += ints_bytes(E); }
  }
  return p;
}
__device__ __forceinline__ int plan_count(const int* off, int E) { return off[E + 1]; }

// the plans of two id arrays, built on `st` without a host sync (update_op.hip)
void launch_plans(const int64_t* ids0, const int64_t* ids1, int E, const Plan& p0, const Plan& p1,
                  hipStream_t st);

// state_dict index of each tensor the kernels name (weight; the bias follows)
enum {
  T_C1A = 0, T_C1B = 2, T_C2A = 4, T_C2B = 6, T_NORM = 8, T_KKF = 10, T_KKG = 12, T_KKH = 14,
  T_IJF = 16, T_IJG = 18, T_IJH = 20, T_GRU0 = 22, T_G1GATE = 24, T_G1RES0 = 26, T_G1RES2 = 28,
  T_GRU2 = 30, T_G3GATE = 32, T_G3RES0 = 34, T_G3RES2 = 36, T_CORR0 = 38, T_CORR2 = 40,
  T_CORR3 = 42, T_CORR5 = 44, T_D = 46, T_W = 48
};

// --- the saved buffer --------------------------------------------------------------
// 25 fp32 planes [E, 384] (each rounded up to 256 B), then corr [E, K0], the
// w head's output [E, 2] and a copy of the two group plans (12 int arrays of
// E + 2): 25 * 1536 + 4 K0 + 8 + 48 bytes per edge, 42 KB at K0 = 882.
//   A0  relu(corr.0)            Z2  corr.2 output (before corr.3's LayerNorm)
//   A3  relu(LN(Z2))            S0  net + inp + corr MLP (before `norm`)
//   X0  LN(S0)                  A1  relu(c1.0(m x0[ix]))      X1  x0 + c1.2(A1)
//   A2  relu(c2.0(m x1[jx]))    X2  x1 + c2.2(A2)
//   FKK, GKK  f, g of agg_kk    YKK the group rows (rows past the group count: 0)
//   X3  x2 + h_kk(YKK)[group]   FIJ, GIJ, YIJ as above for agg_ij
//   X4  x3 + h_ij(YIJ)[group]
//   S1, A4, R1  sigmoid(gate), relu(res.0), res.2 output of gru.1;  X5 its output
//   S2, A5, R2  the same of gru.3;  X6 = net_out
// The six ReLU masks are A0, A3, A1, A2, A4, A5 > 0.
enum {
  P_A0 = 0, P_Z2, P_A3, P_S0, P_X0, P_A1, P_X1, P_A2, P_X2, P_FKK, P_GKK, P_YKK, P_X3, P_FIJ,
  P_GIJ, P_YIJ, P_X4, P_S1, P_A4, P_R1, P_X5, P_S2, P_A5, P_R2, P_X6, kPlanes
};
struct Saved {
  float* pl[kPlanes];
  float* corr;
  float* w;
  Plan plan[2];
};
inline size_t saved_bytes(int E, int K0) {
  return kPlanes * rows_bytes(E) + r256((size_t)E * K0 * 4) + r256((size_t)E * 8) +
         12 * ints_bytes(E);
}
inline Saved saved_carve(void* base, int E, int K0) {
  char* p = (char*)base;
  Saved s;
  for (int i = 0; i < kPlanes; i++) { s.pl[i] = (float*)p; p += rows_bytes(E); }
  s.corr = (float*)p; p += r256((size_t)E * K0 * 4);
  s.w = (float*)p; p += r256((size_t)E * 8);
  carve_plans(p, E, s.plan);
  return s;
}

}  // namespace upd
}  // namespace dpvo
