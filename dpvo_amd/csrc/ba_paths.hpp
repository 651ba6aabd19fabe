// ba_paths.hpp -- what the three BA translation units share on the host:
// ba.hip (C ABI, dispatch, multi-kernel solver), ba_window.hip (window solver,
// fused start-of-update launches) and ba_large.hip (large graphs).  One problem
// descriptor, the only declaration of every function that crosses between the
// files, and the layout of the marks array.  No device code.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "corr_paths.hpp"  // InsLevels
#include "dpvo_hot.h"

namespace dpvo {

// One BA / reprojection problem as the C ABI receives it.  Calls that do not
// use a field leave it null / 0 (the reprojection launches have no target,
// weight or lmbda and only read poses / patches).
struct BaProblem {
  float* poses;  // written in place by the solvers
  float* patches;
  const float* intrinsics;
  const float* target;
  const float* weight;
  const float* lmbda;
  const int64_t* ii;
  const int64_t* jj;
  const int64_t* kk;
  int E, P, num_poses, num_patches;
  int t0, N;        // free poses [t0, t0 + N)
  const int* t0d;   // device t0 (graph-replayed updates: t0 moves per frame) or null, then t0
};

// Marks array (int64 wall-clock stamps, 100 MHz; instrumentation behind
// dpvo_ba_set_marks, read back by dpvo_ba_phase_marks): [0, 128) phases of
// the solver's first workgroup, then per workgroup g < 256 of the window
// kernel and per workgroup b < 256 of the fused start-of-update launch.
constexpr int kMarkAssembled = 128;  // [+ 256 it + g] block assembled, it < 2
constexpr int kMarkSeen = 640;       // [+ 256 it + g] all partials seen, it < 2
constexpr int kMarkSetup = 1152;     // [+ g] setup done
constexpr int kMarkPre = 1408;       // [+ g] iteration 0 assembled, before its reduction
constexpr int kLaunchMarks = 1664;   // [+ 2b] / [+ 2b + 1] start / end of fused-launch workgroup b
constexpr int kMarkEnd = 2176;       // [+ g] end of workgroup g
constexpr int kMarks = 2432;
static_assert(kMarks == DPVO_BA_MARKS, "dpvo_hot.h must publish the length of the marks array");
static_assert(kMarkEnd + 256 == kMarks && kLaunchMarks + 2 * 256 == kMarkEnd, "marks layout");

// What the window path uses of the caller's workspace.  It borrows the status
// word, the marks and dX from the multi-kernel layout (ba.hip: BaWs) and keeps
// its own scratch behind that layout.
struct BaWindowWs {
  char* scratch;   // ba_window_scratch_bytes(E, N)
  int* status;     // [1] OR of status bits
  int64_t* marks;  // [kMarks] or null (product calls)
  double* dxo;     // [6N] dX of the latest iteration
};

// ---- ba_window.hip: plan kernel + persistent per-block workgroups
bool ba_window_supported(int E, int N, int P);  // false without a device
size_t ba_window_scratch_bytes(int E, int N);
void ba_window_plan_offsets(int E, int64_t* out);  // [5] byte offsets of the plan arrays
void ba_set_status_sink(int* sink);
// edge grouping only (reads ii / jj / kk)
int ba_window_plan(const BaProblem& p, const BaWindowWs& ws, void* stream);
// the iterations on a planned scratch; ba_window_launch plans first
int ba_window_run(const BaProblem& p, int iterations, const BaWindowWs& ws, void* stream);
int ba_window_launch(const BaProblem& p, int iterations, const BaWindowWs& ws, void* stream);
// reprojection + A-CORR edge order + plan in one launch, ...
int ba_window_reproject_plan(const BaProblem& p, int N2, float* coords, int* order,
                             const BaWindowWs& ws, void* stream);
// ... plus the insertion of the new frame (src [C, H, W] NCHW fp32 / fp16, lv
// the L levels as corr_paths.hpp's ins_levels filled them)
int ba_window_reproject_plan_insert(const BaProblem& p, int N2, float* coords, int* order,
                                    const BaWindowWs& ws, const void* src, const InsLevels& lv,
                                    int L, int C, int H, int W, int half, void* stream);

// ---- ba_large.hip: large graphs (global BA, cfg4)
size_t gba_workspace_bytes(int E, int N);
int gba_forward(const BaProblem& p, int PPF, int iterations, void* workspace,
                size_t workspace_bytes, void* stream);
double* gba_dx(void* workspace, int E, int N);
int gba_status_or(const void* workspace, int E, int N, int* acc, void* stream);

}  // namespace dpvo
