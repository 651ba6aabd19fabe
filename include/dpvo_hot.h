/*
 * dpvo_hot.h -- C ABI of the MI355X (gfx950) DPVO hot path.
 *
 * Every entry point takes plain device pointers, sizes and an opaque HIP
 * stream (`void*`, hipStream_t; NULL = legacy default stream), launches
 * hand-written HIP kernels on that stream and returns a dpvo_status.  No
 * entry point allocates device memory, synchronises or copies to the host,
 * so each call is hipGraph-capturable; scratch memory is passed in as a
 * caller-owned workspace sized by the matching *_workspace_bytes().
 *
 * Each function names the reference interface it replaces (paths relative to
 * /root/reference, cuteboyqq/DPVO).  The Python extension modules cuda_corr,
 * cuda_ba and lietorch_backends (dpvo_amd/csrc/ext_*.cpp) bind exactly these.
 *
 * Layouts (row-major, contiguous):
 *   fmap1   [B, N1, C, H, W]    gmap patch features (H = W = p)
 *   fmap2   [B, N2, C, H2, W2]  one pyramid level of frame features
 *   coords  [B, M, 2, H, W]     float32 (x, y) per patch pixel, this level
 *   ii, jj  [M]                 int64 patch / frame index per edge
 *   corr    [B, M, 2R+1, 2R+1, H, W]  axis 2 = x offset, axis 3 = y offset
 *   poses   [*, 7]  float32 (tx, ty, tz, qx, qy, qz, qw)
 *   patches [*, 3, P, P] float32 (x, y, inverse depth)
 */
#ifndef DPVO_HOT_H
#define DPVO_HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DPVO_OK = 0,
  DPVO_ERR_INVALID = 1,     /* bad argument (shape, dtype, null pointer)      */
  DPVO_ERR_LAUNCH = 2,      /* hipLaunchKernel / hipGetLastError failure       */
  DPVO_ERR_UNSUPPORTED = 3, /* configuration outside what this build handles   */
  DPVO_ERR_WORKSPACE = 4    /* workspace smaller than *_workspace_bytes()      */
} dpvo_status;

typedef enum { DPVO_F32 = 0, DPVO_F16 = 1, DPVO_F64 = 2 } dpvo_dtype;

/* Human-readable text for a status code (static storage). */
const char* dpvo_status_string(int status);
/* Build identification, e.g. "dpvo_hot gfx950 <git>". */
const char* dpvo_version(void);

/* ---------------------------------------------------------------- altcorr */

/* A-CORR.  Replaces cuda_corr.forward (dpvo/altcorr/correlation.cpp:57,
   correlation_kernel.cu:232-272 + corr_forward_kernel :82-175).
   out[B,M,2R+1,2R+1,H,W] in fmap dtype; accumulation is always fp32 (f64 for
   DPVO_F64).  Requires H*W <= 16, R <= 7. */
int dpvo_corr_forward(const void* fmap1, const void* fmap2, const float* coords,
                      const int64_t* ii, const int64_t* jj, int B, int M, int C, int H, int W,
                      int N1, int N2, int H2, int W2, int radius, int dtype, void* out,
                      void* stream);

/* A-CORR, all pyramid levels of one DPVO update in one launch (the fused form
   of the two/four per-level calls at dpvo/dpvo.py:462-465).  fmap2[l] is
   [B, N2, C, H2[l], W2[l]]; coords are level-1 coordinates and are divided by
   scale[l] in-kernel (dpvo.py:462-463 passes coords / 1 and coords / 4).
   out is [B, M, 2R+1, 2R+1, H, W, L] float = DPVO's torch.stack(..., -1). */
int dpvo_corr_forward_levels(const void* fmap1, const void* const* fmap2, const int* H2,
                             const int* W2, const float* scale, int L, const float* coords,
                             const int64_t* ii, const int64_t* jj, int B, int M, int C, int H,
                             int W, int N1, int N2, int radius, int dtype, float* out,
                             void* stream);

/* A-CORR, all levels, channels-last pyramid (no reference counterpart: the
   layout is this build's; semantics identical to dpvo_corr_forward_levels).
   fmap2[l] is [B,N2,H2[l],W2[l],C] (a [B,N2,C,H,W] tensor in channels-last
   memory), fp32 or fp16, C == 128, L <= 4, H*W <= 16, (2R+1)^2*H*W <= 512,
   (2R+2)^2 <= 164.  Returns DPVO_ERR_UNSUPPORTED outside that envelope
   (callers fall back to dpvo_corr_forward_levels on NCHW data). */
int dpvo_corr_forward_levels_nhwc(const void* fmap1, const void* const* fmap2, const int* H2,
                                  const int* W2, const float* scale, int L, const float* coords,
                                  const int64_t* ii, const int64_t* jj, int B, int M, int C,
                                  int H, int W, int N1, int N2, int radius, int dtype, float* out,
                                  void* stream);
/* The same with an edge order (B == 1): order[p] = edge processed at position
   p, as written by dpvo_reproject_ordered (edges grouped by target frame).
   Workgroups are mapped to XCDs so that each XCD processes one contiguous
   eighth of that order: a target frame's pyramid levels stay in one XCD's L2.
   Results are identical to the unordered call (order == NULL). */
int dpvo_corr_forward_levels_nhwc_ordered(const void* fmap1, const void* const* fmap2,
                                          const int* H2, const int* W2, const float* scale, int L,
                                          const float* coords, const int64_t* ii,
                                          const int64_t* jj, const int32_t* order, int B, int M,
                                          int C, int H, int W, int N1, int N2, int radius,
                                          int dtype, float* out, void* stream);
/* Which kernel a forward entry would run, without a device: the status the
   entry returns before it launches, and through *path the kernel (NONE:
   rejected, or nothing to do).  entry says which export is meant; the other
   arguments are that export's (dpvo_corr_forward: fmap2 / H2 / W2 arrays of
   one level, scale ignored; order: the ordered channels-last entry only).
   Device pointers are looked at for their alignment only. */
enum { DPVO_CORR_FORWARD = 0, DPVO_CORR_LEVELS = 1, DPVO_CORR_LEVELS_NHWC = 2 };
enum {
  DPVO_CORR_PATH_NONE = 0,
  DPVO_CORR_PATH_NHWC = 1,             /* channels-last levels, matrix cores */
  DPVO_CORR_PATH_NCHW_MMA = 2,         /* NCHW levels, matrix cores */
  DPVO_CORR_PATH_NCHW_MMA_ORDERED = 3, /* the same, edges grouped by target frame */
  DPVO_CORR_PATH_VALU = 4
};
int dpvo_corr_query_path(int entry, const void* fmap1, const void* const* fmap2, const int* H2,
                         const int* W2, const float* scale, int L, const float* coords,
                         const int64_t* ii, const int64_t* jj, const int32_t* order, int B, int M,
                         int C, int H, int W, int N1, int N2, int radius, int dtype,
                         const void* out, int* path);
/* Feature maps [count,C,H,W] -> channels-last [count,H,W,C] (the per-frame
   cost of keeping a channels-last pyramid; dtype F32 or F16). */
int dpvo_feature_to_nhwc(const void* src, void* dst, int count, int C, int H, int W, int dtype,
                         void* stream);

/* Frame insertion of a channels-last pyramid (the ring-buffer writes of
   dpvo.py __call__: fmap -> level 1, avg_pool2d(fmap, s, s) -> level s,
   net.py:411 / dpvo.py:462-463) in one launch.  src: one NCHW level-1 frame
   [C, H, W] fp32; dst[l]: the channels-last slot [H/s, W/s, C] of level l,
   scale[l] in {1, 2, 4, 8}.  Pooling sums row-major in fp32 and divides by
   s^2 (torch avg_pool2d order: bit-identical). */
int dpvo_feature_pyramid_insert(const void* src, void* const* dst, const int* scale, int L, int C,
                                int H, int W, int dtype, void* stream);
/* Ring variant of dpvo_feature_pyramid_insert for graph-replayed frames: dst0[l]
   is slot 0 of level l's ring, slots slot_bytes[l] apart; the slot written is
   *slot_dev % mem, read on the device (replaces the host slot of dpvo.py's
   fmap1_/fmap2_ ring writes). */
int dpvo_feature_pyramid_insert_ring(const void* src, void* const* dst0, const int64_t* slot_bytes,
                                     const int* scale, int L, int C, int H, int W, int mem,
                                     const int32_t* slot_dev, int dtype, void* stream);

/* A-CORR-BWD.  Replaces cuda_corr.backward (correlation.cpp:58,
   correlation_kernel.cu:275-325 + corr_backward_kernel :178-229).
   grad [B,M,2R+1,2R+1,H,W] float32.  fmap1_grad / fmap2_grad are ZEROED by
   this call and then accumulated (fp32 atomics, like the reference). */
int dpvo_corr_backward(const void* fmap1, const void* fmap2, const float* coords,
                       const int64_t* ii, const int64_t* jj, const float* grad, int B, int M,
                       int C, int H, int W, int N1, int N2, int H2, int W2, int radius, int dtype,
                       void* fmap1_grad, void* fmap2_grad, void* stream);

/* A-PATCH.  Replaces cuda_corr.patchify_forward (correlation.cpp:60,
   correlation_kernel.cu:327-346 + patchify_forward_kernel :16-47).
   net [B,C,H,W], coords [B,M,2] float32 -> out [B,M,C,D,D], D = 2R+2.
   clamp=0: zero fill outside the map (CUDA semantics); clamp=1: clamp to the
   border (the fork's runtime patchify_forward_kernel_python,
   correlation_kernel.py:181-224). */
int dpvo_patchify_forward(const void* net, const float* coords, int B, int C, int H, int W, int M,
                          int radius, int clamp, int dtype, void* out, void* stream);

/* A-PATCH-BWD.  Replaces cuda_corr.patchify_backward (correlation.cpp:61,
   correlation_kernel.cu:349-372 + patchify_backward_kernel :49-80).
   net_grad [B,C,H,W] is zeroed by this call, then scatter-added. */
int dpvo_patchify_backward(const void* grad, const float* coords, int B, int C, int H, int W,
                           int M, int radius, int clamp, int dtype, void* net_grad, void* stream);

/* ---------------------------------------------------------------- fastba */

/* Workspace for dpvo_ba_forward / the split BA entry points. */
size_t dpvo_ba_workspace_bytes(int E, int t0, int t1);

/* Instrumentation / testing: which F-BA implementation dpvo_ba_forward uses.
   0 = auto: the window kernel (ba_window.hip: plan kernel + one persistent
   workgroup per share of a lower 6x6 block of S, dense solve in every
   workgroup) for E <= 10240 edges and N <= 16 free poses, the multi-kernel
   path (ba.hip) for E <= 16384 and N <= 20, the large-graph path
   (ba_large.hip) beyond; 2 = the multi-kernel path; 4 = always the
   large-graph path; 5 = same as 0.  1 and 3 (the round-1 single-workgroup
   and per-block kernels) were removed: DPVO_ERR_INVALID.  Process-wide; call
   before sizing the workspace. */
int dpvo_ba_select_path(int mode);

/* Sim3 pose-graph normal equations.  Replaces the host assembly of
   cuda_ba.solve_system (dpvo/fastba/ba.cpp:120-165): J_Ginv_i / J_Ginv_j
   [r, 7, 7] f32, ii / jj [r] int64 (ii != jj, < n), res [r, 7] f32 ->
   dense A [7n, 7n] = J^T J with diag(A) += diag(A)*lm + ep, and
   b [7n] = -J^T res, both fp64 (device memory, zeroed here).  The Cholesky
   solve of the top-left freen*7 block runs in the caller (ba.cpp:103-118). */
int dpvo_pgo_assemble(const float* J_Ginv_i, const float* J_Ginv_j, const int64_t* ii,
                      const int64_t* jj, const float* res, int r, int n, float ep, float lm,
                      double* A, double* b, void* stream);

/* Residual and Jacobians of every pose-graph edge in one launch (replaces the
   PyPose + autograd evaluation of dpvo/loop_closure/optim_utils.py:152-189).
   Ginv [n, 7]: tangent of each world-to-camera Sim3 pose; C [r, 8]: Sim3 data
   (t, q, s) of each edge's measured relative transform; ii / jj [r] int64 in
   [0, n) (the caller validates them; an edge outside the range is skipped).
     res[e] = Log(C[e] Exp(Ginv[ii[e]]) Exp(Ginv[jj[e]])^-1)           [r, 7]
     J_i[e] = d res[e] / d Ginv[ii[e]], J_j[e] = d res[e] / d Ginv[jj[e]]
              [r, 7, 7] = [edge, residual component, pose dof]
   J_i and J_j are both given or both NULL (residual only; the residual is
   bit-identical either way).  Plain derivatives with respect to the 7 tangent
   numbers, exact (forward mode), finite at sigma = 0 and theta = 0.  dtype
   DPVO_F32 / DPVO_F64 is that of every floating tensor; arithmetic is fp64. */
int dpvo_pgo_residual(const void* Ginv, const void* C, const int64_t* ii, const int64_t* jj,
                      int r, int n, int dtype, void* res, void* J_i, void* J_j, void* stream);

/* Structured sparse solve of the same system (the default path of
   cuda_ba.solve_system, replacing Eigen SimplicialCholesky, ba.cpp:99-180).
   Poses touched by a long edge (|i - j| > 1) form a dense "border"; the other
   free poses form chain segments that are block-tridiagonal.
   dpvo_pgo_plan (HOST arrays ii / jj [r]; nf = number of free poses, i.e.
   the reference's freen, or n): call with plan == NULL to get the length in
   int64 words, then again to fill it.  The plan's first 32 words are its
   header (counts, table offsets, workspace offsets in doubles; word 25 = the
   workspace length, 3 = m border poses, 22 / 23 = offsets of the dense border
   matrix [7m, 7m] and its right-hand side, 24 = the [nf, 7] step; the border
   table at word 7 holds (pose, left segment, right segment) triples).
   dpvo_pgo_factor (device plan, host copy of the header `hdr`): zeroes the
   workspace, assembles every 7x7 block (edges summed in ascending order:
   deterministic), factors the segments and folds their Schur terms into the
   border system; *fail (device int) = 1 if a segment pivot is not positive.
   The caller solves the border system (dense SPD) into xB [m, 7];
   dpvo_pgo_back back-substitutes the segments. */
int dpvo_pgo_plan(const int64_t* ii, const int64_t* jj, int r, int nf, int64_t* plan,
                  int64_t plan_cap, int64_t* plan_len);
int dpvo_pgo_factor(const float* J_Ginv_i, const float* J_Ginv_j, const int64_t* ii,
                    const float* res, const int64_t* plan, const int64_t* hdr, float ep, float lm,
                    double* ws, int* fail, void* stream);
int dpvo_pgo_back(const int64_t* plan, const int64_t* hdr, const double* xB, double* ws,
                  void* stream);

/* Loop-closure measurement: RANSAC over 3-point Umeyama models and the refit
   on the winner's inliers (replaces the numba ransac_umeyama /
   umeyama_alignment of dpvo/loop_closure/optim_utils.py:64-150, which run on
   the CPU over points copied off the GPU).  src / dst [N, 3] matched points
   (dtype DPVO_F32 or DPVO_F64; arithmetic is fp64 either way, long_term.py:233
   casts to double), dst ~ s R src + t.  samples [H, 3] int32: the three point
   indices of each hypothesis, in the order the reference's loop would draw
   them (an index outside [0, N) makes its hypothesis degenerate; nothing is
   read out of range).  Two launches:
     score   one wave per hypothesis: counts[h] = #{ |c R x + t - y| <
             threshold } under the sample's Umeyama model, -1 for a degenerate
             sample (fewer than 2 singular values above 2.220446049250313e-16);
     select  stop = first h with counts[h] > early_exit (else H - 1); winner =
             lowest h <= stop with the largest positive count; inlier_mask [N]
             of the winner; Umeyama refit on the inliers, reduced in a fixed
             order (bit-identical from run to run).
   model [21] fp64: R row-major (9), t (3), s (1), then the Sim3 data
   (tx, ty, tz, qx, qy, qz, qw, s) with qw >= 0.  info [4]: number of inliers,
   winning hypothesis (-1: none), stop index, status -- 0 ok; 1 no hypothesis
   with a positive count (identity model, 0 inliers, the reference returns
   None); 2 the refit is degenerate (identity model; inliers and mask kept).
   The workspace holds counts[H] int32 at its start.  NULL pointers, N < 3,
   H < 1 or threshold <= 0: DPVO_ERR_INVALID before any launch. */
size_t dpvo_ransac_umeyama_workspace_bytes(int N, int H);
int dpvo_ransac_umeyama(const void* src, const void* dst, int N, int dtype,
                        const int32_t* samples, int H, double threshold, int early_exit,
                        double* model, int32_t* info, uint8_t* inlier_mask, void* ws,
                        size_t ws_bytes, void* stream);

/* Largest number of free poses (t1 - t0) dpvo_ba_forward handles. */
int dpvo_ba_max_free_poses(void);

/* F-BA.  Replaces cuda_ba.forward (dpvo/fastba/ba.cpp:32-45 -> cuda_ba,
   ba_cuda.cu:433-582; fastba.BA, dpvo/fastba/ba.py:7-8).  Runs `iterations`
   Gauss-Newton/Schur steps and updates poses[t0:t1] and the inverse depth of
   every patch kk[*] IN PLACE.  lmbda is a device pointer to one float.
   eff_impl / PPF select the reference's block-sparse E (block_e.cu); this
   implementation is block-sparse for every call and accepts both values.
   Reductions and the Cholesky solve are fp64, deterministic (no float
   atomics).  A failed factorisation yields dX = 0 and status flag bit 1 in
   ws-reported diagnostics (dpvo_ba_last_status). */
int dpvo_ba_forward(float* poses, float* patches, const float* intrinsics, const float* target,
                    const float* weight, const float* lmbda, const int64_t* ii, const int64_t* jj,
                    const int64_t* kk, int E, int P, int num_poses, int num_patches, int PPF,
                    int t0, int t1, int iterations, int eff_impl, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Split form of dpvo_ba_forward used by the edge-sharded multi-GPU BA
   (SURVEY 8e): setup once per call, then per iteration build the local Schur
   system, all-reduce (S, y) across ranks, and solve+update.
   S_lower: [N(N+1)/2][6][6] double (block (a,b), a >= b, row-major blocks in
   order a*(a+1)/2 + b); y: [6N] double. */
int dpvo_ba_setup(const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int num_patches,
                  int t0, int t1, void* workspace, size_t workspace_bytes, void* stream);
int dpvo_ba_build_schur(const float* poses, const float* patches, const float* intrinsics,
                        const float* target, const float* weight, const float* lmbda,
                        const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int P,
                        int num_poses, int t0, int t1, void* workspace, double* S_lower,
                        double* y, void* stream);
int dpvo_ba_solve_update(float* poses, float* patches, const double* S_lower, const double* y,
                         int E, int P, int num_poses, int t0, int t1, void* workspace,
                         double* dX_out, void* stream);
/* Status word of the last BA call on this workspace, copied to the DEVICE int
   `out`: bit 0 = Cholesky failed in the last solve (dX was set to 0),
   bit 1 = some kk outside [0, num_patches) (clamped). */
int dpvo_ba_last_status(const void* workspace, int E, int t0, int t1, int* out, void* stream);
/* Split F-BA for a caller that knows the edge list before the update (DPVO
   fixes the patch graph before reproject / corr, dpvo.py:775-824).
   dpvo_ba_plan groups the edges by patch -- it reads ii / jj / kk only, so it
   can run on a side stream concurrently with A-CORR -- and
   dpvo_ba_forward_planned runs the iterations on that workspace (same
   workspace size as dpvo_ba_forward; identical results).  Only for shapes
   dpvo_ba_plan_supported() accepts (the window path: E <= 10240, N <= 16,
   P * P <= 64); otherwise call dpvo_ba_forward. */
int dpvo_ba_plan_supported(int E, int t0, int t1, int P);
/* Byte offsets, inside a dpvo_ba_plan workspace, of the plan arrays:
   out[0] epos int32[E] (edge at sorted position p, grouped by patch, ascending
   edge index inside a patch), out[1] poff int32[E+1] (first position of patch
   u), out[2] pmask uint32[E] (free-pose bits of patch u), out[3] pkk int32[E]
   (kk of patch u, ascending), out[4] meta int32[8] (nuniq, fixed-pose minimum,
   status).  For tests and tools; no reference counterpart. */
int dpvo_ba_plan_offsets(int E, int t0, int t1, int64_t* out);
int dpvo_ba_plan(const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int num_patches,
                 int num_poses, int t0, int t1, void* workspace, size_t workspace_bytes,
                 void* stream);
int dpvo_ba_forward_planned(float* poses, float* patches, const float* intrinsics,
                            const float* target, const float* weight, const float* lmbda,
                            const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int P,
                            int num_poses, int num_patches, int t0, int t1, int iterations,
                            void* workspace, size_t workspace_bytes, void* stream);

/* OR the status word of the last dpvo_ba_forward on this workspace (any
   path: window kernels or the large-graph solver) into the DEVICE int `acc`
   (sticky; the caller resets it).  Bits: 1 Cholesky failed (dX = 0, as
   dpvo/ba.py:17-21), 2 kk outside [0, num_patches) (clamped), 4 a patch
   touches more free poses than the large-graph solver handles, 8 too many
   border poses (large graph), 16 a cross-workgroup wait timed out, 32 a
   window graph too large for the per-workgroup LDS plan.  Bits 2..32 mean the step was not the reference's and the extension raises.
   Graph-capturable (one tiny kernel, no host sync). */
int dpvo_ba_status_accumulate(const void* workspace, int E, int t0, int t1, int* acc,
                              void* stream);
/* Register `acc` (device int) as the current device's status sink: the
   window-path kernels OR their status into it directly (no extra launch per
   call); dpvo_ba_status_accumulate is then a no-op for that path. */
int dpvo_ba_set_status_sink(int* acc);
/* Instrumentation (no reference counterpart): the marks the last
   dpvo_ba_forward on this workspace stamped -- wall clock (100 MHz): [0]
   start, [1] setup, then linearize, patch, schur, solve, update per iteration;
   shader clock: [38] start, [39] end; [40..] finer stamps inside the setup
   and the first solve -- copied to the DEVICE array `out`, DPVO_BA_MARKS
   int64 long. */
#define DPVO_BA_MARKS 2432
int dpvo_ba_phase_marks(const void* workspace, int E, int t0, int t1, int64_t* out, void* stream);
/* Instrumentation: start / end wall-clock stamps of every workgroup of the
   last Schur launch, [2 x N(N+1)/2] int64 to DEVICE `out`. */
int dpvo_ba_workgroup_marks(const void* workspace, int E, int t0, int t1, int64_t* out,
                            void* stream);
/* Instrumentation: when `on` is nonzero the BA kernels of later calls on this
   process stamp the phase marks above (off by default: the product calls
   store no marks). */
int dpvo_ba_set_marks(int on);
/* Diagnostics (no reference counterpart; the parity tests' view of the
   reference's dX = chol_solve(S, y), ba_cuda.cu:561-562): the pose step dX
   [6N] (fp64, pose t0 + i at [6 i .. 6 i + 5]) of the LAST iteration of the
   last dpvo_ba_forward / dpvo_ba_forward_planned on this workspace, any
   path, copied to the DEVICE array `out`. */
int dpvo_ba_last_dx(const void* workspace, int E, int t0, int t1, double* out, void* stream);

/* F-BA on large graphs (ba_large.hip): DPVO's global BA (dpvo.py:695-715 ->
   fastba.BA(..., eff_impl=True), block_e.cu:43-300) and the edge-sharded
   multi-GPU form.  dpvo_ba_forward dispatches here by itself;
   the split entry points serve the sharded driver:
     setup   once per call: patch grouping, block-sparse pattern of S and the
             band / border analysis.  Rank ownership: a patch belongs to this
             rank iff own_lo <= kk / PPF < own_hi (its source frame); only
             owned patches (and their edges) are linearised and summed.
     build   per iteration: linearise the owned edges and write this rank's
             part of the packed system [y (6N doubles) | S lower 6x6 blocks
             (nblk x 36 doubles)] at workspace + dpvo_gba_packed_offset().
             (all_reduce(SUM) of the first 6N + 36 nblk doubles goes here.)
     solve_update  damp, solve S dX = y (block cyclic reduction + border
             Schur complement, fp64), retract poses t0..t1-1 and the inverse
             depth of every OWNED patch.
   info copies 8 ints to DEVICE `out`: status (bit 0 factorisation failed ->
   dX = 0, bit 1 kk clamped, bit 2 a patch touches > 24 free poses, bit 3
   more than 64 poses couple further back than 16 poses -> dX = 0), unique
   patches, items, nblk, interior poses, border poses, superblock poses g,
   superblocks.  N <= dpvo_gba_max_free_poses(), E <= 2^22. */
size_t dpvo_gba_workspace_bytes(int E, int t0, int t1);
int dpvo_gba_max_free_poses(void);
size_t dpvo_gba_packed_offset(int E, int t0, int t1);
int dpvo_gba_setup(const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int num_patches,
                   int PPF, int t0, int t1, int own_lo, int own_hi, void* workspace,
                   size_t workspace_bytes, void* stream);
int dpvo_gba_build(const float* poses, const float* patches, const float* intrinsics,
                   const float* target, const float* weight, const float* lmbda, const int64_t* ii,
                   const int64_t* jj, int E, int P, int num_poses, int t0, int t1,
                   void* workspace, void* stream);
int dpvo_gba_solve_update(float* poses, float* patches, int E, int P, int t0, int t1,
                          void* workspace, void* stream);
int dpvo_gba_info(const void* workspace, int E, int t0, int t1, int* out, void* stream);

/* F-REPROJ.  Replaces cuda_ba.reproject (ba.cpp:47-53 -> cuda_reproject,
   ba_cuda.cu:585-616 + reproject :379-429).  coords [E,2,P,P]. */
int dpvo_reproject(const float* poses, const float* patches, const float* intrinsics,
                   const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int P,
                   int num_poses, int num_patches, float* coords, void* stream);

/* dpvo_reproject plus, in the same launch (one extra workgroup), the A-CORR
   edge order: order[0..E) = edges grouped by target frame jj (jj in [0, N2);
   keys outside share the last group).  Feeds
   dpvo_corr_forward_levels_nhwc_ordered. */
int dpvo_reproject_ordered(const float* poses, const float* patches, const float* intrinsics,
                           const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int P,
                           int num_poses, int num_patches, int N2, float* coords, int32_t* order,
                           void* stream);

/* dpvo_reproject_ordered plus dpvo_ba_plan(ii, jj, kk, .., t0, t1, workspace)
   in the same launch: the start of a DPVO update (dpvo.py:775-824 reprojects,
   then runs BA on the same edges), so the edge grouping the window BA needs
   runs beside the reprojection instead of as its own launch.  workspace is
   then passed to dpvo_ba_forward_planned.  Same outputs, bit for bit, as the
   two separate calls; DPVO_ERR_UNSUPPORTED where dpvo_ba_plan_supported is 0. */
int dpvo_reproject_ordered_plan(const float* poses, const float* patches,
                                const float* intrinsics, const int64_t* ii, const int64_t* jj,
                                const int64_t* kk, int E, int P, int num_poses, int num_patches,
                                int N2, float* coords, int32_t* order, int t0, int t1,
                                void* workspace, size_t workspace_bytes, void* stream);
/* dpvo_reproject_ordered_plan plus, in the same launch, the insertion of the
   update's new frame into the channels-last pyramid (dpvo_feature_pyramid_insert's
   arguments: src [C, H, W] NCHW level-1 frame, dst[l] the channels-last slot of
   level l, scale[l] in {1, 2, 4, 8}, dtype F32 / F16).  The insertion tiles run
   on the CUs the reprojection and the single-workgroup plan leave idle (DPVO
   inserts the frame in __call__ just before update(); nothing in this launch
   reads the slot it writes).  Outputs bit-identical to the separate calls. */
int dpvo_reproject_ordered_plan_insert(const float* poses, const float* patches,
                                       const float* intrinsics, const int64_t* ii,
                                       const int64_t* jj, const int64_t* kk, int E, int P,
                                       int num_poses, int num_patches, int N2, float* coords,
                                       int32_t* order, int t0, int t1, void* workspace,
                                       size_t workspace_bytes, const void* src, void* const* dst,
                                       const int* scale, int L, int C, int H, int W, int dtype,
                                       void* stream);
/* Device-scalar variants for graph-replayed DPVO updates (the window start t0
   moves every frame, shapes stay fixed): t0 is read from the int32 device
   scalar *t0_dev, N = t1 - t0 is given.  Same results as the host-t0 calls. */
int dpvo_reproject_ordered_plan_dev(const float* poses, const float* patches,
                                    const float* intrinsics, const int64_t* ii, const int64_t* jj,
                                    const int64_t* kk, int E, int P, int num_poses,
                                    int num_patches, int N2, float* coords, int32_t* order,
                                    const int32_t* t0_dev, int N, void* workspace,
                                    size_t workspace_bytes, void* stream);
int dpvo_ba_forward_planned_dev(float* poses, float* patches, const float* intrinsics,
                                const float* target, const float* weight, const float* lmbda,
                                const int64_t* ii, const int64_t* jj, const int64_t* kk, int E,
                                int P, int num_poses, int num_patches, const int32_t* t0_dev,
                                int N, int iterations, void* workspace, size_t workspace_bytes,
                                void* stream);

/* F-NBR.  Replaces cuda_ba.neighbors (ba.cpp:59-97).  Groups edges by ii,
   stable-sorts each group by jj; ix = previous edge, jx = next edge, -1 at
   the ends.  Single-workgroup LDS sort: E <= dpvo_neighbors_max_edges(). */
int dpvo_neighbors_max_edges(void);
int dpvo_neighbors(const int64_t* ii, const int64_t* jj, int E, int64_t* ix, int64_t* jx,
                   void* stream);

/* ---------------------------------------------------------------- lietorch */

/* L-SE3.  Replaces lietorch_backends.{expm, logm, inv, mul, adj, adjT, act,
   act4, as_matrix, projector, Jinv} (dpvo/lietorch/src/lietorch.cpp:18-283,
   lietorch_gpu.cu:20-601).  group: 1 = SO3, 3 = SE3, 4 = Sim3 (dispatch.h:24-45;
   2 = RxSO3 is DPVO_ERR_UNSUPPORTED).  Sim3: data (t, q, s), N = 8, tangent
   (tau, phi, sigma), K = 7, arithmetic in fp64 for both dtypes, and Jinv and
   the Exp / Log gradients use the exact left Jacobian (the derivative of the
   forward map), not the reference's truncated series (sim3.h:167-191).
   dtype DPVO_F32 / DPVO_F64.  n elements, each row contiguous:
     op 0 exp   : X=a[K]          -> out[N]
     op 1 log   : X[N]            -> out[K]
     op 2 inv   : X[N]            -> out[N]
     op 3 mul   : X[N], Y[N]      -> out[N]
     op 4 adj   : X[N], Y=a[K]    -> out[K]
     op 5 adjT  : X[N], Y=a[K]    -> out[K]
     op 6 act   : X[N], Y=p[3]    -> out[3]
     op 7 act4  : X[N], Y=p[4]    -> out[4]
     op 8 matrix: X[N]            -> out[4x4]
     op 9 proj  : X[N]            -> out[NxN]
     op 10 Jinv : X[N], Y=a[K]    -> out[K]
   Quaternions are normalised on load (so3.h:95-97). */
int dpvo_lie_forward(int group, int op, int dtype, int n, const void* X, const void* Y, void* out,
                     void* stream);

/* Backward of ops 0-7 (lietorch_gpu.cu:32-256); gradient rows of group
   elements are N-strided with the tangent gradient in the first K entries
   (the reference convention).  out0 = dX (or da for exp), out1 = dY/da/dp. */
int dpvo_lie_backward(int group, int op, int dtype, int n, const void* grad, const void* X,
                      const void* Y, void* out0, void* out1, void* stream);

/* PatchGraph edge bookkeeping on the device (dpvo/dpvo.py:480-568,
   dpvo/patchgraph.py:11-63), static MAX_EDGES buffers, counts in the device
   int array `counts`: [0] num_edges, [1] num_edges_inac, [2] error flags
   (1 append overflow -> edges not added; 2 inactive store full -> removed
   edges not stored, like the reference's warning), [3..4] scratch.  No host
   synchronisation.
   dpvo_pg_append replaces append_factors(ii=kk_new, jj=jj_new): edges at
   [num, num + n), ii = ix[kk], net rows zeroed (net may be null).
   dpvo_pg_remove replaces remove_factors(mask, store): mask (uint8, 1 =
   remove, length >= num) or, when mask is null, the DPVO window rule
   ix[kk] < thresh (dpvo.py:684) sparing loop-closure edges with
   jj - ii > 30 and jj > lc_min when lc_min >= 0 (:685-688).  Kept edges are
   compacted in order into the *_b ("back") buffers -- the caller swaps
   them with the active set -- and removed ones appended in order to the
   inactive store when `store`.  pos: int scratch [max_edges]. */
int dpvo_pg_append(const int64_t* ix, const int64_t* kk_new, const int64_t* jj_new, int n,
                   int64_t* ii, int64_t* jj, int64_t* kk, float* net, int DIM, int* counts,
                   int max_edges, void* stream);
int dpvo_pg_remove(const uint8_t* mask, const int64_t* ix, int64_t thresh, int64_t lc_min,
                   int store, int64_t* ii, int64_t* jj, int64_t* kk, float* net, float* weight,
                   float* target, int64_t* ii_b, int64_t* jj_b, int64_t* kk_b, float* net_b,
                   float* weight_b, float* target_b, int64_t* ii_i, int64_t* jj_i, int64_t* kk_i,
                   float* weight_i, float* target_i, int DIM, int* counts, int* pos,
                   int max_edges, void* stream);
/* DPVO.keyframe's window removal (dpvo.py:684-693) with thresholds relative to
   the device frame count n = *n_dev: remove ix[kk] < n + thresh_off, except
   (lc_on) edges with jj - ii > 30 and jj > n + lc_off.  Graph-replayable. */
int dpvo_pg_remove_window_dev(const int64_t* ix, const int32_t* n_dev, int64_t thresh_off,
                              int64_t lc_off, int lc_on, int store, int64_t* ii, int64_t* jj,
                              int64_t* kk, float* net, float* weight, float* target,
                              int64_t* ii_b, int64_t* jj_b, int64_t* kk_b, float* net_b,
                              float* weight_b, float* target_b, int64_t* ii_i, int64_t* jj_i,
                              int64_t* kk_i, float* weight_i, float* target_i, int DIM,
                              int* counts, int* pos, int max_edges, void* stream);
/* append_factors with a device count: n = min(*n_dev, n_cap) edges (e.g. the
   output of dpvo_edges_loop, dpvo.py:986-988).  Graph-replayable. */
int dpvo_pg_append_dev(const int64_t* ix, const int64_t* kk_new, const int64_t* jj_new,
                       const int32_t* n_dev, int n_cap, int64_t* ii, int64_t* jj, int64_t* kk,
                       float* net, int DIM, int* counts, int max_edges, void* stream);
/* DPVO.keyframe's frame-drop removal (dpvo.py:633-641): when kf[0] (the
   device decision of dpvo_kf_motion), remove the active edges with ii == kf[1]
   or jj == kf[1], not stored.  Always compacts into the *_b buffers (a copy
   when nothing is dropped), so the caller swaps unconditionally. */
int dpvo_pg_remove_frame_dev(const int32_t* kf, int64_t* ii, int64_t* jj, int64_t* kk,
                             float* net, float* weight, float* target, int64_t* ii_b,
                             int64_t* jj_b, int64_t* kk_b, float* net_b, float* weight_b,
                             float* target_b, int DIM, int* counts, int* pos, int max_edges,
                             void* stream);

/* --------------------------------------------------------- SPD solve (training) */

/* Batched dense SPD factor + solve: the device side of CholeskySolver
   (dpvo/ba.py:13-38, which calls torch.linalg.cholesky_ex(H) and
   cholesky_solve(b, U); block_solve 67-77 passes it the damped pose system).
   batch items of H [n, n] (row-major; the lower triangle is read, as
   cholesky_ex(upper=False)) and B [n, k]; dtype DPVO_F32 / DPVO_F64.
   factor = 1: L = lower Cholesky factor (zeros above; required when
   n x (n + k) elements exceed 160 KB of LDS: it is then the working copy),
   X = H^-1 B, info[b] = first column whose pivot is not positive (1-based,
   0 = success; LAPACK potrf / cholesky_ex semantics), X = 0 for a failed item.
   factor = 0: H holds a lower factor from a factor = 1 call; X = (H H^T)^-1 B,
   L and info must be null.  One 256-thread workgroup per item.
   Beyond LDS the column scratch alone must fit the default 64 KB less 64 B:
   n <= DPVO_SPD_MAX_N_F64 in fp64 and twice that in fp32; a larger n is
   DPVO_ERR_UNSUPPORTED and launches nothing. */
#define DPVO_SPD_MAX_N_F64 8184
int dpvo_spd_solve(const void* H, const void* B, void* L, void* X, int32_t* info, int batch, int n,
                   int k, int factor, int dtype, void* stream);

/* ------------------------------------------- differentiable BA layer (training) */

/* One Gauss-Newton step of dpvo/ba.py BA (88-297), B = 1, and its adjoint
   (ba_layer.hip).  poses [N, 7], patches [M, 3, p, p], intrinsics [N, 4],
   targets / weights [E, 2] in `dtype` (DPVO_F32 / DPVO_F64; arithmetic and all
   sums are fp64 in a fixed order), ii / jj / kk [E] int64.  n = number of
   poses in the problem (fixedp <= n <= N), the free poses are [fixedp, n);
   with structure_only the step has no pose part.  lmbda_dev (one element of
   `dtype`, device) wins over the host value `lmbda` when not null.  bounds:
   4 host doubles (xmin, ymin, xmax, ymax).  Gates: |r| < 250, Z > 0.2, the
   bounds; an edge with ii / jj outside [0, n) or kk outside [0, M) is closed,
   touches no memory and is counted in the first int32 of the workspace (the
   second holds the factorisation's info: != 0 -> dX = 0).
   Outputs: dX [n - fixedp, 6] (not written with structure_only), dZ [M].  The
   workspace (dpvo_ba_layer_workspace_bytes(E, M, n_free, with_backward),
   n_free = structure_only ? 0 : n - fixedp) carries the linearisation and the
   factor to dpvo_ba_layer_backward, which must get the same buffer, sizes
   and inputs:  gX [n_free, 6], gZ [M] -> g_targets / g_weights [E, 2],
   g_poses [N, 6] (left tangent), g_patches [M, 3] (x, y, d of the centre).
   E <= 0: DPVO_OK, no launch.  n < fixedp, n > N, p even or < 1, a dtype other
   than F32 / F64, null pointers: DPVO_ERR_INVALID; 6 n_free beyond
   DPVO_SPD_MAX_N_F64 (8184: 1364 free poses): DPVO_ERR_UNSUPPORTED; short workspace:
   DPVO_ERR_WORKSPACE (in that order).  8 launches forward, 7 backward. */
size_t dpvo_ba_layer_workspace_bytes(int E, int M, int n_free, int with_backward);
int dpvo_ba_layer_forward(const void* poses, const void* patches, const void* intrinsics,
                          const void* targets, const void* weights, const void* lmbda_dev,
                          double lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk,
                          int E, int M, int p, int N, int n, int fixedp, int structure_only,
                          const double* bounds, double ep, int dtype, void* dX, void* dZ, void* ws,
                          size_t ws_bytes, int with_backward, void* stream);
int dpvo_ba_layer_backward(const void* poses, const void* patches, const void* intrinsics,
                           const void* gX, const void* gZ, int E, int M, int p, int N, int n,
                           int fixedp, int structure_only, int dtype, void* g_targets,
                           void* g_weights, void* g_poses, void* g_patches, void* ws,
                           size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- keyframe */

/* DPVO.keyframe's decision (dpvo.py:586-599, 619-624) on the device.  st =
   {n, m} (device frame counters), i = n - keyframe_index - 1,
   j = n - keyframe_index + 1; motionmag over the active edges with
   projective_ops.flow_mag (projective_ops.py:120-130, beta 0.5).  Writes
   kf = {drop, k = n - keyframe_index} and mag = {motionmag(i,j),
   motionmag(j,i)}.  No host synchronisation: kf predicates
   dpvo_pg_remove_frame_dev and dpvo_kf_shift.
   Limit: a drop moves keyframe_index - 1 frames and dpvo_kf_shift holds at
   most 16 of them, so keyframe_index > 17 returns DPVO_ERR_UNSUPPORTED here,
   before the decision that would predicate such a drop is launched. */
int dpvo_kf_motion(const int64_t* ii, const int64_t* jj, const int64_t* kk, const int32_t* counts,
                   const float* poses, const float* patches, const float* intrinsics, int P,
                   const int32_t* st, int keyframe_index, double keyframe_thresh, int32_t* kf,
                   float* mag, void* stream);
/* The rest of a frame drop (dpvo.py:626-673), predicated on kf[0]: log
   (t1, t0, poses[k] * poses[k-1]^-1) as pg.delta[t1] into delta_log[7 x cap] /
   delta_tstamps[2 x cap] at *delta_count (optional: all three null), shift the
   active edges past k (kk -= M, ii -= 1; jj -= 1), move the per-frame rows
   k+1 .. n-1 of every frame array one row down (ring[a] > 0: row = frame %
   ring[a], the imap/gmap/fmap rings), then n -= 1, m -= M.  A drop whose
   pg.delta record finds the log full ORs 8 into counts[2] (the patch graph's
   error word; the record is not kept).
   Limits: narrays <= 12 (more: DPVO_ERR_UNSUPPORTED); the drop moves
   keyframe_index - 1 <= 16 frames (dpvo_kf_motion refuses a larger index);
   every ring[a] is 0 or > keyframe_index - 1.  Each 4-byte word (or byte) of
   the moved rows is read for all frames and then written, which equals the
   reference's frame-by-frame copy only while the moved rows do not wrap onto
   each other; this entry does not know keyframe_index, the caller checks
   (DevicePatchGraph.keyframe does). */
int dpvo_kf_shift(const int32_t* kf, int M, int32_t* st, int64_t* ii, int64_t* jj, int64_t* kk,
                  int32_t* counts, int max_edges, void* const* frame_arrays,
                  const int64_t* bytes_per_frame, const int32_t* ring, int narrays,
                  const float* poses, const int64_t* tstamps, float* delta_log,
                  int64_t* delta_tstamps, int32_t* delta_count, int delta_cap, void* stream);
/* PatchGraph.edges_loop (dpvo/patchgraph.py:65-91, reduce_edges
   loop_closure/optim_utils.py:24-60) gated like its caller (dpvo.py:984-988:
   only when n - *last_global_ba >= global_opt_freq; *last_global_ba = n when
   edges are found; last_global_ba may be null = no gate).  n = st[0] on the
   device, n_cap >= n sizes the launch.  Writes kk (i M + arange(M)) and jj of
   the accepted loop edges and their count (edges x M) to out_n, ready for
   dpvo_pg_append_dev.  work: dpvo_edges_loop_work_floats() floats.
   Limits: (global_opt_freq - keyframe_index) x min(n_cap - removal_window,
   max_edge_age) <= 16384, n_cap x (global_opt_freq - keyframe_index) <=
   131072, max_num_edges <= 1024 (else DPVO_ERR_UNSUPPORTED).  The target frames
   [n - global_opt_freq, n - keyframe_index) must be frames for every
   n > removal_window: keyframe_index >= 0 and global_opt_freq <=
   removal_window + 1 (else DPVO_ERR_INVALID).  A device n above n_cap takes no loop edges
   and ORs 4 into *errors (optional; the patch graph's counts[2]). */
int dpvo_edges_loop(const float* poses, const float* patches, const float* intrinsics,
                    const int64_t* ix, int P, int M, const int32_t* st, int n_cap,
                    int32_t* last_global_ba, int removal_window, int max_edge_age,
                    int global_opt_freq, int keyframe_index, float backend_thresh,
                    int max_num_edges, int nms, float* work, int64_t* out_kk, int64_t* out_jj,
                    int32_t* out_n, int32_t* errors, void* stream);
size_t dpvo_edges_loop_work_floats(void);

/* ---------------------------------------------------------------- front-end */

/* The head of DPVO.__call__ (dpvo.py:931-965) in one launch of one workgroup,
   no host synchronisation.  Frame row n = *n_dev when n_dev is non-null, else
   the host n; frame counter likewise (int32 device scalars: graph-replayable).
   times [times_cap] (fp64) holds the caller's frame times by frame counter
   (the reference's tlist); times[counter] is written by the caller first.
     tstamps[n]    = counter                                   (:933)
     intrinsics[n] = new_intrinsics / res, fp32 division       (:934)
     poses[n]      only when n > 1 (:943): motion_model 0 = poses[n-1] copied bit
                   for bit (:956-957); 1 = Exp(damping fac Log(P1 P2^-1)) P1 with
                   P1 = poses[n-1], P2 = poses[n-2], fac = (c - b) / (b - a) for
                   a, b, c = times[counter-2 .. counter] (missing entries read
                   as 1, :949); b == a gives fac = 1 (the reference raises).
                   fp64 arithmetic, quaternions normalised on load, rounded to
                   fp32 on store.
     patches rows [n M, (n + 1) M) = new_patches [M, 3, P, P]; with median = 1
                   and n >= 1 their channel 2 is the lower median (sorted rank
                   (count - 1) / 2, what torch.median returns; NaN if any value
                   is NaN) of channel 2 of the patches of frames [max(n-3, 0), n)
                   (:962-965), by a four-pass radix select, not a sort.
   Nothing else is written.  Host n outside [0, N), host counter outside
   [0, times_cap), M / P / N <= 0 or a null pointer: DPVO_ERR_INVALID before any
   launch; device values outside those ranges leave every buffer untouched.
   3 M P P > 2^30: DPVO_ERR_UNSUPPORTED. */
int dpvo_frame_init(float* poses, float* patches, float* intrinsics, int64_t* tstamps,
                    const double* times, int times_cap, const float* new_patches,
                    const float* new_intrinsics, int N, int M, int P, int n, const int32_t* n_dev,
                    int counter, const int32_t* counter_dev, int motion_model, double damping,
                    double res, int median, void* stream);

/* DPVO.terminate's interpolation (dpvo.py:385-417): traj[t] = get_pose(t) for
   t in [0, counter), or its inverse (inverse = 1, what terminate returns), from
   poses [N, 7] / tstamps [N] of the n keyframes (n = *n_dev when non-null) and
   the pg.delta log of dpvo_kf_shift: delta_log [cap, 7], delta_pairs [cap, 2] =
   (t1, t0), *delta_count on the device.  Frame t is a keyframe when
   tstamps[i] == t for some i < n (pose poses[i]; checked first, :386);
   otherwise pose(t) = dP pose(t0) by the last record in log order with t1 == t,
   through chains of any depth.  Records with t0 >= t1 or an index outside
   [0, counter) are ignored.  A frame with neither, or whose chain ends at such
   a frame, gets a NaN row.  root[t] = the row of `poses` frame t hangs on, -1
   when unresolved; info = {unresolved frames, ignored records}.  fp64
   arithmetic, unit quaternions, rounded to fp32 on store.
   2 + ceil(log2(counter)) launches (table build, then pointer jumping; the
   number depends on counter alone), no host synchronisation; counter == 0 is
   a no-op.  workspace: dpvo_trajectory_workspace_bytes(counter). */
size_t dpvo_trajectory_workspace_bytes(int counter);
int dpvo_trajectory(const float* poses, const int64_t* tstamps, int N, int n, const int32_t* n_dev,
                    const float* delta_log, const int64_t* delta_pairs,
                    const int32_t* delta_count, int delta_cap, int counter, int inverse,
                    float* traj, int64_t* root, int32_t* info, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------- image stream and evaluation */

/* The front of a run on a sequence as it sits on disk (dpvo/stream.py:24-39,
   :75-83): undistort, halve and crop one decoded frame in one launch, no host
   synchronisation, no state between calls.
     raw        uint8 [H0, W0, channels] on the device, channels 3 (interleaved,
                as a decoder delivers it) or 1 (grey, replicated into the three
                planes as cv2.imread does)
     calib      ncalib host doubles fx fy cx cy [k1 k2 p1 p2 [k3]] (calib/*.txt)
     scale      1 or 0.5 (0.5 needs even H0 and W0)
     image      uint8 [3, H, W] planar, H = H1 - H1 % 16, W = W1 - W1 % 16 of
                (H1, W1) = (H0, W0) scale, cropped top-left; plane p = channel p,
                or 2 - p with swap_rb.  4-byte aligned.
     intrinsics float32 [4] on the device = (fx, fy, cx, cy) scale
   ncalib 4: no remap (the reference's len(calib) > 4).  ncalib 8 / 9: pixel
   (u, v) of the undistorted H0 x W0 image is, in fp64, in this order, without
   FMA contraction,
     x = (u - cx)/fx;  y = (v - cy)/fy;  r2 = x*x + y*y
     kr = 1 + r2*(k1 + r2*(k2 + r2*k3))
     xd = x*kr + (2*p1*x*y + p2*(r2 + 2*x*x))
     yd = y*kr + (p1*(r2 + 2*y*y) + 2*p2*x*y)
     mx = fx*xd + cx;  my = fy*yd + cy
     qx = floor(mx*32 + 0.5);  qy = floor(my*32 + 0.5)   (clamped to +-2^30, NaN low)
     ix = qx >> 5, ax = qx & 31;  iy = qy >> 5, ay = qy & 31
     val = ((32-ax)(32-ay) S[iy,ix] + ax(32-ay) S[iy,ix+1]
          + (32-ax)ay S[iy+1,ix] + ax ay S[iy+1,ix+1] + 512) >> 10
   with S = 0 outside the source (BORDER_CONSTANT).  At scale 0.5 an output
   pixel is (a + b + c + d + 2) >> 2 over the 2 x 2 block of those rounded
   values (undistort, then INTER_AREA).  OpenCV's camera model with its 1/32
   pixel map quantisation; not claimed bit-equal to cv2.undistort.
   Null pointers, non-positive sizes, channels other than 1 / 3, a misaligned
   image, fx or fy zero or not finite: DPVO_ERR_INVALID; ncalib other than
   4 / 8 / 9, another scale, an odd size at 0.5, a side above 16384 or an empty
   output: DPVO_ERR_UNSUPPORTED; all before any launch.
   dpvo_frame_prepare_shape gives (H, W) with the same size checks. */
int dpvo_frame_prepare_shape(int H0, int W0, double scale, int* H, int* W);
int dpvo_frame_prepare(const uint8_t* raw, int H0, int W0, int channels, const double* calib,
                       int ncalib, double scale, int swap_rb, uint8_t* image, float* intrinsics,
                       void* stream);

/* Absolute trajectory error of an estimated trajectory against a reference
   one (evaluate_euroc.py:109-119 through evo): association by timestamp,
   Sim(3) Umeyama alignment, error statistics.  One launch of one workgroup, no
   host synchronisation; every reduction has a fixed order (run-to-run
   bit-identical).  All pointers but the workspace are device arrays:
     est_xyz [n, 3] (est_dtype DPVO_F32 / DPVO_F64; arithmetic is fp64),
     est_t [n], ref_xyz [m, 3], ref_t [m] fp64; stamps non-decreasing.
   Association: the long side is est if n > m, else ref.  Every stamp of the
   short side takes the long stamp with the smallest |dt| (ties: the lower
   index) and the pair is kept iff |dt| <= max_diff; pairs stay in short-side
   order, a long index may repeat.
   Alignment (align = 1): y ~ c R x + t, x = est, y = ref, by Umeyama's fit on
   the centred moments of the pairs (scale corrected); align = 0: c = 1, R = I,
   t = 0.  Errors e_i = |c R x_i + t - y_i|.
     stats  fp64 [8] = rmse, mean, median (np.median), std (population), min,
            max, sse, count
     model  fp64 [13] = R (row-major), t, c
     pairs  int32 [min(n, m), 2] = (est index, ref index), unused rows -1
     status int32 [1]: bit 0 fewer than 3 pairs, bit 1 degenerate covariance,
            bit 2 unsorted (or NaN) stamps: nothing is associated, count 0.
   On any set bit stats[0..6] are NaN, count is still written and model is the
   identity.  Null pointers, n or m < 1, max_diff negative or NaN, align other
   than 0 / 1: DPVO_ERR_INVALID; another est_dtype, n or m above 65536:
   DPVO_ERR_UNSUPPORTED; short workspace: DPVO_ERR_WORKSPACE (in that order). */
size_t dpvo_trajectory_ate_workspace_bytes(int n, int m);
int dpvo_trajectory_ate(const void* est_xyz, int est_dtype, const double* est_t, int n,
                        const double* ref_xyz, const double* ref_t, int m, double max_diff,
                        int align, double* stats, double* model, int32_t* pairs, int32_t* status,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------ training data readers */

/* The device half of dpvo/data_readers (base.py, rgbd_utils.py,
   augmentation.py).  Every entry checks its arguments on the host before any
   launch (null or misaligned pointers, non-positive sizes: DPVO_ERR_INVALID;
   sizes past the stated capacity: DPVO_ERR_UNSUPPORTED; invalid first), runs on
   `stream` without host synchronisation, and sums in a fixed order: two calls
   give identical bits.  All arrays are device arrays, 4-byte aligned. */

/* rgbd_utils.compute_distance_matrix_flow (rgbd_utils.py:122-160), one launch.
   The reference calls pops.induced_flow, which does not exist; the flow is
   defined through projective_ops.transform(.., valid=True) on P = 1 patches.
     poses      float32 [N, 7] world-from-camera (tx ty tz qx qy qz qw), as the
                dataset stores them
     disps      float32 [N, h, w];  intrinsics float32 [N, 4] (fx fy cx cy)
     D          float32 [N, N]
   Inputs are fp32, all arithmetic is fp64, D is rounded to fp32 once.  With
   G = inv(pose) and G_ab = G_b * inv(G_a) (quaternion product and action as
   lietorch's, no renormalisation), the direction a -> b gives for every grid
   point (x, y) of frame a
     X0 = ((x - cx_a)/fx_a, (y - cy_a)/fy_a, 1);  d = disps[a, y, x]
     X1 = R(G_ab) X0 + t(G_ab) d;  Z = X1.z
     u = fx_b (X1.x / max(Z, 0.1)) + cx_b;  v = fy_b (X1.y / max(Z, 0.1)) + cy_b
     mag = min(|(u - x, v - y)|, 100)      (a NaN flow counts as 100)
     val = Z > 0.2                         (false for a NaN Z)
   For i <= j the points of i -> j are summed first, then those of j -> i
   (each lane of one wave takes points lane, lane + 64, .. in order, the 64
   lanes are added in an xor tree); with n = 2 h w and k = sum val
     D[i, j] = D[j, i] = (float)k / (float)n < 0.7f ? +inf : sum(mag val) / k
   so D is symmetric bit for bit; the diagonal is computed like any entry.
   Capacity: N <= 8192, h w <= 65536. */
int dpvo_frame_flow_distance(const float* poses, const float* disps, const float* intrinsics, int N,
                             int h, int w, float* D, void* stream);

/* base.py:77-80 as CSR: row i holds the columns j, ascending, with
   d = f * D[i, j] < max_flow (one fp32 product, as numpy's) and dist = d.
   dpvo_frame_graph_count: rowptr int32 [N + 1] (a count per row, then the
   project's workgroup scan; two launches), rowptr[N] = nnz.  The caller reads
   nnz, allocates col int32 [nnz] and dist float32 [nnz] and calls
   dpvo_frame_graph_fill with the same D, f and max_flow (one launch; nothing
   is written at or past nnz).  f must be positive and finite, max_flow not
   NaN.  Capacity: N <= 8192. */
int dpvo_frame_graph_count(const float* D, int N, float f, float max_flow, int32_t* rowptr,
                           void* stream);
int dpvo_frame_graph_fill(const float* D, int N, float f, float max_flow, const int32_t* rowptr,
                          int32_t* col, float* dist, int nnz, void* stream);

/* The random draws of augmentation.py, made by the caller and passed by value:
   the device work is a function of them alone. */
typedef struct dpvo_augment_params {
  int do_color;      /* 0: no colour map at all (the image values pass through) */
  int order[4];      /* a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue */
  float brightness, contrast, saturation;  /* factors, >= 0 (the reference draws [0.6, 1.4]) */
  float hue;         /* shift in turns (the reference draws +-0.2 / 3.14) */
  int gray, invert;  /* 0 / 1 */
  double scale;      /* 1, or the resize factor (the reference draws 2^U(0, 0.5)) */
  int swap_rb;       /* 0: plane 0 is red; 1: plane 2 is red (cv2.imread's order) */
} dpvo_augment_params;

/* RGBDAugmentor.__call__ (augmentation.py:24-66) with the draws in `params`.
     images [N, 3, H, W] float32 in 0..255, disps [N, H, W], intrinsics [N, 4]
     -> images_out [N, 3, ch, cw], disps_out [N, ch, cw], intrinsics_out [N, 4]
   Colour (do_color), per pixel in fp32 without FMA contraction, (r, g, b) by
   swap_rb, gray(r, g, b) = 0.299 r + 0.587 g + 0.114 b, clamp = to [0, 1]:
     x = x / 255; then the four operations in `order`, each clamped:
       brightness  x = clamp(x b)
       contrast    x = clamp(c x + (1 - c) m), m = (float)(S / (N H W)) with S the
                   fp64 sum of gray over all N frames as they stand when
                   contrast's turn comes (a launch of its own: 256 workgroups,
                   thread t of them takes pixels t, t + 65536, ..; xor tree in
                   the wave, waves ascending, workgroups by the same tree)
       saturation  x = clamp(s x + (1 - s) gray)
       hue         maxc, minc, cr = maxc - minc; cr == 0: h = s = 0, else
                   s = cr / maxc, (rc, gc, bc) = (maxc - (r, g, b)) / cr,
                   h = maxc == r ? bc - gc : maxc == g ? 2 + rc - bc : 4 + gc - rc,
                   h = fmod(h / 6 + 1, 1);  h = h + hue;  h = h - floor(h);
                   h6 = 6 h, i = (int)floor(h6) % 6, f = h6 - floor(h6), v = maxc,
                   p = v (1 - s), q = v (1 - f s), t = v (1 - (1 - f) s),
                   (r, g, b) = (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q) by i;
                   clamped
     gray: r = g = b = gray(r, g, b);  invert: x = 1 - x;  x = x 255
   The reference round-trips through PIL and quantises to uint8 between the
   operations; this stays in fp32 and does not quantise.
   Spatial: ht1 = (int)(scale H), wd1 = (int)(scale W), y0 = (ht1 - ch) / 2,
   x0 = (wd1 - cw) / 2; only the crop window [y0, y0 + ch) x [x0, x0 + cw) of
   the resized frame is computed.  scale == 1: no resampling, the window is
   copied (with do_color = 0 bit for bit).  Otherwise, in fp32, for output pixel
   (oy, ox) of the resized frame, sh = (float)H / ht1 (and sw likewise):
     image   F.interpolate(mode='bicubic', align_corners=False): ry = sh (oy + 0.5)
             - 0.5, iy = floor(ry), t = ry - iy, taps iy - 1 .. iy + 2 clamped to
             [0, H - 1], weights of the cubic convolution with A = -0.75; rows
             first, then the four row values; not clamped
     depth   nearest: row min((int)floor(oy sh), H - 1)
   intrinsics_out = (float)scale K - (0, 0, x0, y0), two fp32 roundings.
   Colour then resampling goes through a scratch image in the workspace.
   DPVO_ERR_INVALID also for: flags outside 0 / 1, an order that is not a
   permutation, non-finite or negative factors, a non-finite hue, a scale that
   is not finite and positive, and a crop that does not fit: ch > ht1 - 1 or
   cw > wd1 - 1 when the frame is resized (augmentation.py:29-31 keeps the
   resized frame larger than the crop), ch > H or cw > W at scale 1.
   Capacity: H, W <= 16384, scale H and scale W <= 65536, 3 N H W < 2^31.
   A short workspace: DPVO_ERR_WORKSPACE (8-byte aligned; 2048 bytes suffice
   unless colour is followed by resampling, which needs the scratch image too). */
size_t dpvo_rgbd_augment_workspace_bytes(int N, int H, int W);
int dpvo_rgbd_augment(const float* images, const float* disps, const float* intrinsics, int N, int H,
                      int W, int crop_h, int crop_w, const dpvo_augment_params* params,
                      float* images_out, float* disps_out, float* intrinsics_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* base.py:171-173: s = 0.7 torch.quantile(disps, 0.98) over all n elements,
   disps_out = disps / s, poses_out = poses with columns 0..2 times s (poses
   float32 [nposes, 7]).  Two launches.  In fp32 as torch computes it:
   pos = 0.98f (n - 1), lo = floor(pos), hi = ceil(pos), w = pos - lo; a and b
   the values of sorted ranks lo and hi (exact, by the four-pass radix select
   that dpvo_frame_init's median uses, one workgroup, once per rank);
   q = w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w) (torch's lerp); s = 0.7f q.
   scale float32 [3] on the device = (s, a, b); any NaN among disps makes all
   three NaN.  The outputs must not overlap the inputs.
   Capacity: n <= 2^30, nposes <= 2^24. */
int dpvo_normalize_depth(const float* disps, int n, const float* poses, int nposes, float* disps_out,
                         float* poses_out, float* scale, void* stream);

/* ------------------------------------------------------------------ tracker */

/* The four small kernels of the tracker's frame path (dpvo_amd/dpvo.py), one
   launch each on `stream`, no host synchronisation, argument checks before
   the launch.  Counts given as int32 device scalars (non-null *_dev) replace
   the host value, as in dpvo_frame_init. */

/* Patchifier.forward after the encoders (dpvo/net.py:388-399) plus the ring
   writes of DPVO.__call__ (dpvo.py:937-938, 965-969), frame n = *n_dev or n.
   For patch m with integer-valued centre (x, y) = coords[m] (clamped to
   [P/2, w-1-P/2] x [P/2, h-1-P/2]) and ring row r = (n % pmem) M + m:
     gmap_ring[r] [C, P, P]  = the P x P window of fmap [C, h, w] at the centre
     imap_ring[r] [DIM]      = imap [DIM, h, w] at the centre
                               (rings DPVO_F32 or DPVO_F16, round to nearest even)
     patches_out[m] [3, P, P] = (x + dx, y + dy, 1)
     colors[n, m, k] (uint8)  = (image[2-k] + 0.5) * 127.5 truncated, image
                               [3, H, W] normalised fp32 read at pixel
                               (res x + res/2, res y + res/2); two fp32
                               roundings, no contraction (B, G, R order)
   Exact copies: every output is bit-exact.  No other row is written.  One
   wave per patch.  Null pointers, sizes <= 0, P even or larger than the map,
   host n outside [0, N): DPVO_ERR_INVALID; another ring dtype or a map of 2^31
   elements or more: DPVO_ERR_UNSUPPORTED; a device n outside [0, N) writes
   nothing. */
int dpvo_frame_sample(const float* fmap, const float* imap, const float* image,
                      const float* coords, void* gmap_ring, void* imap_ring, int ring_dtype,
                      float* patches_out, uint8_t* colors, int h, int w, int H, int W, int C,
                      int DIM, int M, int P, int res, int pmem, int N, int n,
                      const int32_t* n_dev, void* stream);

/* torch.quantile(delta.norm(dim=-1).float(), 0.5) (dpvo.py:584): delta [M, 2]
   (DPVO_F32, or DPVO_F16 widened first), out one fp32 device scalar.  Norms
   sqrt(fma(y, y, x x)) in fp32 (torch's accumulation); rank select in LDS by one
   workgroup; even M: b - (b - a) 0.5 over the two middle values (torch.lerp at
   weight 0.5), odd M the middle value; NaN if any norm is NaN.  Null pointers,
   M <= 0 or another dtype: DPVO_ERR_INVALID; M > 1024: DPVO_ERR_UNSUPPORTED. */
int dpvo_probe_median(const void* delta, int dtype, int M, float* out, void* stream);

/* dpvo.py:805-810 for edges e < E (E = *E_dev clamped to [0, cap], or the host
   E <= cap; cap = rows of the buffers): target[e] = coords[e, :, P/2, P/2] +
   (float)delta[e] (one fp32 add), weight[e] = (float)w[e].  coords [E, 2, P, P]
   fp32; delta / w [E, 2] DPVO_F32 or DPVO_F16; target / weight [cap, 2] fp32.
   Rows >= E are not written.  Host E == 0 (or cap == 0): DPVO_OK, no launch.
   E < 0, E > cap, cap < 0, P even, another dtype, null pointers:
   DPVO_ERR_INVALID. */
int dpvo_update_targets(const float* coords, const void* delta, const void* w, int dtype,
                        float* target, float* weight, int P, int E, const int32_t* E_dev,
                        int cap, void* stream);

/* The centre pixel of pops.point_cloud (dpvo.py:834-836) for patches k < m
   (m = *m_dev clamped to [0, cap], or the host m <= cap; cap = rows of points
   and of patches): points[k] = X.xyz / X.w with X = poses[ix[k]]^-1 *
   ((x - cx) / fx, (y - cy) / fy, 1, d), (x, y, d) the centre of patch k and
   the intrinsics of frame ix[k] (clamped to [0, N)).  fp64 arithmetic, the
   quaternion normalised, rounded to fp32 on store; d == 0 divides.  Rows >= m
   are not written.  Host m == 0 (or cap == 0): DPVO_OK, no launch.  m < 0,
   m > cap, cap < 0, N <= 0, P even, null pointers: DPVO_ERR_INVALID. */
int dpvo_map_points(const float* poses, const float* patches, const float* intrinsics,
                    const int64_t* ix, float* points, int N, int P, int m, const int32_t* m_dev,
                    int cap, void* stream);

/* ------------------------------------------------- long-term loop closure */

/* Mutual nearest neighbours of two descriptor sets with a ratio test (the
   matcher between the detector and dpvo_ransac_umeyama; it stands where the
   reference runs LightGlue, long_term.py:82-88, 228-229).  desc0 [N0, D],
   desc1 [N1, D], contiguous, DPVO_F32 or DPVO_F16 (widened exactly), rows
   aligned to four elements; 1 <= N0, N1 <= 4096, D % 4 == 0, 4 <= D <= 256.
   Rows i < n0 / j < n1 are valid (n = *n_dev where n_dev is not null, else the
   host n; clamped to [0, N]); the others are never read.  All in fp32:
     sim[i, j] = sum_d a[i, d] b[j, d]        an fma chain, d ascending
     d2[i, j]  = max((|a_i|^2 + |b_j|^2) - 2 sim[i, j], 0)
   Every row takes its best column (smaller d2, then the lower index) and the
   second-best d2 (+inf with one valid column), every column likewise; (i, j)
   is a match when each is the other's best, d2 <= ratio2 * second on both
   sides (one fp32 product) and d2 <= max_dist2.
     partner0 [N0] / partner1 [N1] (int64)  the matched column / row, or -1
     matches [min(N0, N1), 2] (int64)       the pairs by ascending i, then -1
     dist2 [min(N0, N1)]                    d2 of each pair, then -1
     count                                  the number of pairs
   Two launches (64 x 64 tiles on v_mfma_f32_32x32x2_f32 reduced to top-2
   triples, then one workgroup that merges, tests and compacts), no host sync,
   no atomics: two runs are bit-equal.  Null pointers, N < 1, D < 4, D % 4 != 0,
   another dtype, a host n outside [0, N], a negative or NaN ratio2 /
   max_dist2, misaligned rows: DPVO_ERR_INVALID; N > 4096 or D > 256:
   DPVO_ERR_UNSUPPORTED; short workspace: DPVO_ERR_WORKSPACE (in that order).
   dpvo_match_workspace_bytes is 0 outside 1 <= N <= 4096. */
size_t dpvo_match_workspace_bytes(int N0, int N1);
int dpvo_match_descriptors(const void* desc0, const void* desc1, int dtype, int N0, int N1, int D,
                           int n0, const int32_t* n0_dev, int n1, const int32_t* n1_dev,
                           float ratio2, float max_dist2, int64_t* partner0, int64_t* partner1,
                           int64_t* matches, float* dist2, int32_t* count, void* workspace,
                           size_t workspace_bytes, void* stream);

/* The 3-D keypoints of frame i from its tracks over the frames i-1, i, i+1
   (long_term.py:90-136 joined with the depth filter of :213-217).  poses [3, 7]
   and intrinsics [3, 4] (at image resolution) of the three frames; disps: M
   inverse depths `disp_stride` floats apart (the centre pixels of frame i's
   patches); kps0 [N0, 2], kps1 [N1, 2], kps2 [N2, 2] in image pixels; m10 /
   m12 [N1]: the partner of keypoint n of frame i in kps0 / kps2, or -1.  A
   keypoint with both partners in range is a track: its inverse depth starts at
   the lower median of disps (torch.median) and takes `iterations` steps
   dZ = u / (C + lmbda) of the structure-only BA over its two observations,
   weight 1, linearised, gated and clamped as dpvo_ba_forward does (fp32 edge
   math, fp64 sums).  Then
     points [N1, 3]  ((u - cx) / fx, (v - cy) / fy, 1) / d, intrinsics of frame i
     disp [N1]       d (0 where the keypoint is no track, as are its points)
     keep [N1]       track, both reprojection residuals < max_residual and
                     points.z < max_depth
     sel [N1]        the kept indices in ascending order, then -1 (int64)
     count           their number
   One launch of one workgroup, no host sync.  Null pointers, M / N0 / N1 / N2 /
   disp_stride < 1, iterations < 0, a negative or NaN lmbda: DPVO_ERR_INVALID;
   M > 1024 or N1 > 4096: DPVO_ERR_UNSUPPORTED. */
int dpvo_triangulate_tracks(const float* poses, const float* intrinsics, const float* disps,
                            int disp_stride, int M, const float* kps0, int N0, const float* kps1,
                            int N1, const float* kps2, int N2, const int64_t* m10,
                            const int64_t* m12, float max_depth, float max_residual,
                            int iterations, float lmbda, float* points, float* disp,
                            uint8_t* keep, int64_t* sel, int32_t* count, void* stream);

/* --------------------------------------------------------- update operator */

/* DPVO's update operator (dpvo/net.py:175-339 `Update`, with
   blocks.py:15-29 GatedResidual and net.py:671-714 SoftAggONNX / blocks.py:31-48
   SoftAgg), as fused kernels on the matrix cores: the inference forward, and
   further down the training forward and the backward.  dim must be 384.

     t  = corr MLP(corr)                       net.py:201-208
     x  = LN(net + inp + t)                    net.py:283-284
     x += c1(m_ix * x[ix]); x += c2(m_jx * x[jx])          net.py:305-306 (265-266)
     x += h_kk(sum_group softmax_group(g_kk(x)) f_kk(x))[group]   net.py:319
     x += h_ij(...)                                         net.py:320
     x  = gru(x); d = d(x); w = w(x)           net.py:322-326

   ix / jx and the group ids are inputs, so one operator serves the original
   DPVO (fastba.neighbors, -1 = missing and masked; groups kk and
   ii * 12345 + jj) and the fork's live Update (neighbors_tensor, always in
   range; groups kk and ii).  An index outside [0, E) is a missing neighbour.
   The group softmax subtracts the per-(group, channel) maximum
   (torch_scatter.scatter_softmax); there is no +-50 clamp and no ii * 1e-10
   term on d and w (net.py:692, 331-337).

   Weights are DPVO_F32 (exact fp32 products, v_mfma_f32_16x16x4_f32) or
   DPVO_F16 (v_mfma_f32_16x16x32_f16: activations rounded to fp16 only as
   matrix operands, fp32 accumulation); everything between the linears is
   fp32.  Group sums run in ascending edge order: results are deterministic. */

/* Bytes of the packed weight blob; 0 for K0 < 1 or a wdtype other than
   DPVO_F32 / DPVO_F16.  K0 = corr_dim = 2 * 49 * p * p (net.py:202). */
size_t dpvo_update_packed_bytes(int K0, int wdtype);

/* HOST function: packs the 50 parameter tensors of Update (fp32, PyTorch
   layout, host pointers, in state_dict order: c1.0.weight, c1.0.bias,
   c1.2.*, c2.0.*, c2.2.*, norm.*, agg_kk.f.*, .g.*, .h.*, agg_ij.f.*, .g.*,
   .h.*, gru.0.*, gru.1.gate.0.*, gru.1.res.0.*, gru.1.res.2.*, gru.2.*,
   gru.3.gate.0.*, gru.3.res.0.*, gru.3.res.2.*, corr.0.*, corr.2.*, corr.3.*,
   corr.5.*, d.1.*, w.1.*) into a host blob of dpvo_update_packed_bytes()
   bytes (layout: csrc/update_op.hip).  fp16 weights are rounded to nearest
   even; the first layer's K tail (K0 up to a multiple of 128) is zero.  Pack
   once at load and upload the blob.  dim != 384 or a bad wdtype:
   DPVO_ERR_UNSUPPORTED; ntensors != 50, null pointers, K0 < 1:
   DPVO_ERR_INVALID; blob_size too small: DPVO_ERR_WORKSPACE. */
int dpvo_update_pack_weights(const float* const* tensors, int ntensors, int dim, int K0,
                             int wdtype, void* blob, size_t blob_size);

/* Bytes of the caller-owned device workspace of one E (scratch rows f, g, the
   second x buffer, the group rows, and the group plan); 0 for E < 1 or K0 < 1. */
size_t dpvo_update_workspace_bytes(int E, int K0);

/* Group plan of the two aggregations (replaces torch.unique(ix,
   return_inverse=True), blocks.py:41, and the [H, H] equality mask of
   net.py:695-702), built on the device without a host sync: per edge the
   dense group index (groups numbered by their smallest member edge), member
   lists in ascending edge order, and the group count, all kept in the
   workspace.  gk, gij: int64 [E] group ids (any values).  Valid until the ids
   change; dpvo_update_forward of the same E and workspace reads it. */
int dpvo_update_plan(const int64_t* gk, const int64_t* gij, int E, void* workspace,
                     size_t workspace_size, void* stream);

/* The operator (replaces Update.forward, net.py:221-339).  blob: device copy
   of the packed weights of (K0, wdtype).  net, inp [E, 384], corr [E, K0],
   net_out [E, 384] in iodtype (DPVO_F32, or DPVO_F16 with DPVO_F16 weights);
   ix, jx int64 [E]; d, w fp32 [E, 2].  net_out may alias net.  No allocation,
   nine plain launches on `stream` (capturable).  E <= 0: DPVO_OK without a
   launch; dim != 384 or an unsupported dtype pair: DPVO_ERR_UNSUPPORTED; null
   pointers, K0 < 1: DPVO_ERR_INVALID; short workspace: DPVO_ERR_WORKSPACE;
   all checked before any launch. */
int dpvo_update_forward(const void* blob, int wdtype, const void* net, const void* inp,
                        const void* corr, const int64_t* ix, const int64_t* jx, int E, int dim,
                        int K0, int iodtype, void* workspace, size_t workspace_size,
                        void* net_out, float* d, float* w, void* stream);

/* --- the update operator's training surface (csrc/update_op.hip,
   csrc/update_bwd.hip) ---
   fp32 weights and fp32 I/O only.  Exact fp32 products
   (v_mfma_f32_16x16x4_f32); every sum over edges or over the members of a group
   runs in a fixed order that depends on E and the indices only (fixed chunks
   folded in fp64, ascending edge order inside a group), no float atomics: two
   calls on the same state are bit-identical.  Plain launches on `stream`, no
   allocation, no host synchronisation.  Status rules of all entry points, all
   checked before any launch: dim != 384 or a dtype other than DPVO_F32 (the
   device pack also takes DPVO_F16): DPVO_ERR_UNSUPPORTED; K0 < 1:
   DPVO_ERR_INVALID; then E <= 0: DPVO_OK without a launch; null required
   pointers: DPVO_ERR_INVALID; short buffers: DPVO_ERR_WORKSPACE. */

/* DEVICE pack: the blob of dpvo_update_pack_weights, byte for byte (header and
   zero padding included), written by one launch from `params`, a host array
   of the 50 device fp32 tensors in state_dict order.  For the step after an
   optimiser update: no host round trip.  wdtype DPVO_F32 or DPVO_F16. */
int dpvo_update_pack_weights_device(const float* const* params, int dim, int K0, int wdtype,
                                    void* blob, size_t blob_size, void* stream);

/* Bytes of the `saved` buffer of dpvo_update_forward_train (layout:
   csrc/update_layout.hpp; 25 fp32 planes [E, 384], corr, w and the two group
   plans: 38456 + 4 K0 bytes per edge); 0 for E < 1 or K0 < 1. */
size_t dpvo_update_saved_bytes(int E, int K0);

/* dpvo_update_forward (after dpvo_update_plan on the same workspace) with
   DPVO_F32 weights and I/O: the same nine launches with the same arithmetic,
   so net_out, d and w are bit-identical to the inference call at every E, and
   one more launch that copies the two group plans.  Everything the backward
   needs is kept in the caller-owned `saved`; the workspace may be reused
   (with another E, too) before the backward runs. */
int dpvo_update_forward_train(const void* blob, int wdtype, const void* net, const void* inp,
                              const void* corr, const int64_t* ix, const int64_t* jx, int E,
                              int dim, int K0, int iodtype, void* workspace,
                              size_t workspace_size, void* saved, size_t saved_size,
                              void* net_out, float* d, float* w, void* stream);

/* One launch: the six ReLU masks the training forward used, uint8
   [6, E, 384] (1 where the ReLU passed), in the order corr.0, the ReLU after
   corr.3, c1.0, c2.0, gru.1.res.0, gru.3.res.0.  The seventh, the heads'
   relu(x), is net_out > 0. */
int dpvo_update_saved_relu_masks(const void* saved, size_t saved_size, int E, int K0,
                                 uint8_t* masks, void* stream);

/* Bytes of the backward's device workspace; 0 for E < 1 or K0 < 1. */
size_t dpvo_update_backward_workspace_bytes(int E, int K0);

/* The backward.  params: host array of the 50 device fp32 parameter tensors
   (PyTorch layout, state_dict order; the values the forward's blob was packed
   from).  saved: as filled by dpvo_update_forward_train with the same (E, K0);
   ix, jx: as given to it.  Cotangents g_net_out [E, 384], g_d, g_w [E, 2]:
   each may be null, which means zero (bit-identical to a buffer of zeros).
   Outputs g_net, g_inp [E, 384], g_corr [E, K0]: each may be null (not wanted,
   not computed; the other outputs' bits do not change).  grads: host array of
   50 device fp32 tensors shaped like params, every element overwritten; or
   null when no parameter gradient is wanted.  agg_kk.g.bias and
   agg_ij.g.bias have an analytically zero gradient (the group softmax is
   shift-invariant per channel): what is written is what the arithmetic
   gives, rounding noise.  A null entry of params or grads: DPVO_ERR_INVALID;
   E above 65535 * 64: DPVO_ERR_UNSUPPORTED.  3 + 141 launches with every
   gradient wanted. */
int dpvo_update_backward(const float* const* params, int dim, int K0, const void* saved,
                         size_t saved_size, const int64_t* ix, const int64_t* jx, int E,
                         const float* g_net_out, const float* g_d, const float* g_w, float* g_net,
                         float* g_inp, float* g_corr, float* const* grads, void* workspace,
                         size_t workspace_size, void* stream);

/* ---------------------------------------------------------------------------
   The feature encoders (replace BasicEncoder4, dpvo/extractor.py:200-264: the
   fnet / inet of net.py's Patchifier): the inference forward, and further
   down the training forward and the backward.

     x = relu(norm(conv1(img)))                 7x7 stride 2,  3 -> 32
     x = layer1(x)                              two residual blocks, 32 -> 32
     x = layer2(x)                              32 -> 64 stride 2 (skip: 1x1
                                                stride-2 conv + norm), 64 -> 64
     out = conv2(x) / 4                         1x1, 64 -> out_dim
     block: y = relu(norm(conv3x3(x))); y = relu(norm(conv3x3(y)));
            out = relu(skip(x) + y)

   norm is the identity (DPVO_ENCODER_NORM_NONE, inet) or InstanceNorm2d with
   its defaults (DPVO_ENCODER_NORM_INSTANCE, fnet: per image and channel over
   the plane, biased variance, eps 1e-5, no affine).  H x W -> H1 x W1 -> h x w
   with H1 = (H - 1) / 2 + 1, h = (H1 - 1) / 2 + 1.  The / 4 of Patchifier
   (net.py:361-362) is part of the operator.

   Weights are DPVO_F32 (exact fp32 products, v_mfma_f32_16x16x4_f32) or
   DPVO_F16 (v_mfma_f32_16x16x32_f16: activations rounded to fp16 only as
   matrix operands, fp32 accumulation); bias, statistics (combined in fp64 in
   a fixed order), normalisation, ReLU, residual adds and the / 4 are fp32.
   No float atomics: results are deterministic. */
enum { DPVO_ENCODER_NORM_NONE = 0, DPVO_ENCODER_NORM_INSTANCE = 1 };
enum { DPVO_ENCODER_NCHW = 0, DPVO_ENCODER_NHWC = 1 };

/* Bytes of the packed weight blob; 0 for an out_dim that is not a multiple of
   64 in [64, 1024] or a wdtype other than DPVO_F32 / DPVO_F16. */
size_t dpvo_encoder_packed_bytes(int out_dim, int wdtype);

/* HOST function: packs the 22 parameter tensors of BasicEncoder4 (fp32,
   PyTorch layout [Cout, Cin, kh, kw], host pointers, in state_dict order:
   conv1.weight, conv1.bias, layer1.0.conv1.*, layer1.0.conv2.*,
   layer1.1.conv1.*, layer1.1.conv2.*, layer2.0.conv1.*, layer2.0.conv2.*,
   layer2.0.downsample.0.*, layer2.1.conv1.*, layer2.1.conv2.*, conv2.*) into
   a host blob of dpvo_encoder_packed_bytes() bytes (layout:
   csrc/encoder.hip).  fp16 weights are rounded to nearest even.  Pack once at
   load and upload the blob.  ntensors != 22 or null pointers:
   DPVO_ERR_INVALID; a bad out_dim, norm or wdtype: DPVO_ERR_UNSUPPORTED;
   blob_size too small: DPVO_ERR_WORKSPACE. */
int dpvo_encoder_pack_weights(const float* const* tensors, int ntensors, int out_dim, int norm,
                              int wdtype, void* blob, size_t blob_size);

/* Bytes of the caller-owned device workspace (the intermediate channels-last
   fp32 planes and the norm statistics); 0 for non-positive sizes, a bad
   out_dim or sizes outside the kernels' index range. */
size_t dpvo_encoder_workspace_bytes(int n_images, int H, int W, int out_dim);

/* The encoder.  blob: device copy of the packed weights of (out_dim, norm,
   wdtype).  images: fp32 [n_images, 3, H, W] contiguous, already scaled
   (2 (img / 255) - 0.5, dpvo.py).  out: fp32 [n_images, out_dim, h, w], stored
   NCHW-contiguous (DPVO_ENCODER_NCHW) or as channels-last memory
   [n_images, h, w, out_dim] (DPVO_ENCODER_NHWC); the two hold the same values
   bit for bit.  Any H, W, n_images >= 1.  No allocation; 11 (none) or 25
   (instance) plain launches on `stream` (capturable).  Null pointers,
   non-positive sizes, an unknown out_layout: DPVO_ERR_INVALID; a bad wdtype,
   norm or out_dim, or sizes outside the index range: DPVO_ERR_UNSUPPORTED;
   short workspace: DPVO_ERR_WORKSPACE; all checked before any launch. */
int dpvo_encoder_forward(const void* blob, int wdtype, int norm, int out_dim, const float* images,
                         int n_images, int H, int W, float* out, int out_layout, void* workspace,
                         size_t workspace_bytes, void* stream);

/* --- the encoders' training surface (csrc/encoder.hip, csrc/encoder_bwd.hip) ---
   The gradients of the 22 parameters; the image gradient is not provided.
   Exact fp32 (DPVO_F32 weights are what the backward differentiates; an fp16
   pack has no gradient here), fixed-order fp64 sums wherever a sum spans
   workgroups, no float atomics: two calls on the same state are bit-identical. */

/* DEVICE pack: the blob of dpvo_encoder_pack_weights, byte for byte (header
   and zero padding included), written by one launch on `stream` from `params`,
   a host array of 22 device pointers (fp32, PyTorch layout, state_dict
   order).  For the step after an optimiser update: no host round trip.  Null
   pointers (a null entry included): DPVO_ERR_INVALID; a bad out_dim, norm or
   wdtype: DPVO_ERR_UNSUPPORTED; blob_bytes too small: DPVO_ERR_WORKSPACE; all
   before the launch. */
int dpvo_encoder_pack_weights_device(const float* const* params, int out_dim, int norm, int wdtype,
                                     void* blob, size_t blob_bytes, void* stream);

/* Bytes of the `saved` buffer of dpvo_encoder_forward_train (every plane the
   backward needs; layout: csrc/encoder_layout.hpp); 0 where
   dpvo_encoder_workspace_bytes returns 0 or for a bad norm. */
size_t dpvo_encoder_saved_bytes(int n_images, int H, int W, int out_dim, int norm);

/* dpvo_encoder_forward with every intermediate plane kept in the caller-owned
   `saved` instead of a ping-pong workspace: the same kernels and the same
   arithmetic, so `out` is bit-identical to dpvo_encoder_forward in both
   layouts.  Status rules as dpvo_encoder_forward (short `saved`:
   DPVO_ERR_WORKSPACE). */
int dpvo_encoder_forward_train(const void* blob, int wdtype, int norm, int out_dim,
                               const float* images, int n_images, int H, int W, float* out,
                               int out_layout, void* saved, size_t saved_bytes, void* stream);

/* Bytes of the backward's device workspace; 0 where
   dpvo_encoder_workspace_bytes returns 0. */
size_t dpvo_encoder_backward_workspace_bytes(int n_images, int H, int W, int out_dim);

/* The backward.  params: host array of the 22 device fp32 parameter tensors
   (the masters, PyTorch layout, state_dict order; the values the forward's
   blob was packed from).  images, saved: as given to / filled by
   dpvo_encoder_forward_train with the same (norm, out_dim, n_images, H, W).
   grad_out: the cotangent of `out`, fp32 [n_images, out_dim, h, w], stored
   NCHW-contiguous or channels-last (grad_layout).  grads: host array of 22
   device fp32 tensors shaped like params, every element overwritten.  With
   DPVO_ENCODER_NORM_INSTANCE the bias of convs 0..9 cancels in the mean
   subtraction: its gradient is identically zero and exact zeros are written.
   66 (instance) or 56 (none) launches.  Null pointers (a null entry of params
   or grads included), non-positive sizes, an unknown grad_layout:
   DPVO_ERR_INVALID; a bad norm or out_dim, or sizes outside the index range:
   DPVO_ERR_UNSUPPORTED; short workspace: DPVO_ERR_WORKSPACE; all checked
   before any launch. */
int dpvo_encoder_backward(int norm, int out_dim, const float* const* params, const float* images,
                          int n_images, int H, int W, const void* saved, const float* grad_out,
                          int grad_layout, float* const* grads, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
   The training step's reprojection and losses (csrc/train.hip).  fp32 in and
   out, fp64 arithmetic and fixed-order fp64 sums inside, no floating-point
   atomics (two calls give identical bits), plain launches on `stream`, no
   allocation, no host synchronisation.  Status rules of all seven entries,
   decided before any launch, in this order: an unsupported shape (P other
   than 1 or 3, E P P >= 2^30, n > 32): DPVO_ERR_UNSUPPORTED; nothing to do
   (E <= 0, n < 2, no gradient wanted): DPVO_OK without a launch; a null
   required pointer (or N, M < 1): DPVO_ERR_INVALID; a short workspace:
   DPVO_ERR_WORKSPACE. */

/* projective_ops.transform (projective_ops.py:53-113) for SE3 and the whole
   P x P patch.  poses [N, 7] (quaternions normalised on load), patches
   [M, 3, P, P], intrinsics [N, 4] (row ii lifts, row jj projects), ii / jj /
   kk [E] int64.  X1 = (G_j G_i^-1) ((x - cx) / fx, (y - cy) / fy, 1, d),
   d' = 1 / max(Z, 0.1), coords [E, P, P, 2] = (fx d' X + cx, fy d' Y + cy),
   valid [E, P, P] = Z > 0.2 as float; coords_corr (may be null): the same
   coords as [E, 2, P, P], the layout A-CORR takes.  An edge with ii / jj
   outside [0, N) or kk outside [0, M) reads nothing, gets NaN coords and
   valid = 0, and contributes no gradient.  One launch. */
int dpvo_transform_forward(const float* poses, const float* patches, const float* intrinsics,
                           const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int P,
                           int N, int M, float* coords, float* valid, float* coords_corr,
                           void* stream);

/* E (12 + 3 P P) doubles; 0 for E <= 0 or an unsupported P. */
size_t dpvo_transform_workspace_bytes(int E, int P);

/* g_coords [E, P, P, 2] -> g_poses [N, 6] (left tangent; every row written)
   and g_patches [M, 3, P, P]; either may be null (not wanted, not formed).
   Nothing passes through d' where Z < 0.1; intrinsics get no gradient.  A
   pose's (patch's) sum over its edges runs in ascending edge order per thread
   (lane) of its workgroup (wave) and then through a fixed tree.  1 + 1 + 1
   launches. */
int dpvo_transform_backward(const float* poses, const float* patches, const float* intrinsics,
                            const int64_t* ii, const int64_t* jj, const int64_t* kk, int E, int P,
                            int N, int M, const float* g_coords, float* g_poses, float* g_patches,
                            void* workspace, size_t workspace_bytes, void* stream);

/* train.py:87-88.  coords, coords_gt [E, P, P, 2], valid [E] (of the patch
   centre).  emin [E]: min over the P P points of |coords - coords_gt| (ties:
   the lowest point index -> argmin [E]); loss [1]: the mean of emin over the
   edges with valid > 0.5, count [1] their number.  With no valid edge the
   loss is 0 (the reference's empty mean is NaN).  One workgroup, one launch. */
int dpvo_flow_loss_forward(const float* coords, const float* coords_gt, const float* valid, int E,
                           int P, float* loss, int32_t* count, float* emin, int32_t* argmin,
                           void* stream);

/* g_coords [E, P, P, 2] = g_loss[0] (x - y) / |x - y| / count at each valid
   edge's argmin (0 for an exactly-zero difference), 0 everywhere else. */
int dpvo_flow_loss_backward(const float* coords, const float* coords_gt, const float* valid,
                            const int32_t* count, const int32_t* argmin, const float* g_loss, int E,
                            int P, float* g_coords, void* stream);

/* train.py:90-113 for 2 <= n <= 32 poses G, Ps [n, 7].  A_i = inv(G_i) with
   its translation times s, B_i = inv(Ps_i), s = min(VarA / trace(D), 10) of
   kabsch_umeyama(t_gt, t_est) (IEEE: a zero trace gives 10), e_ij =
   Log((A_i^-1 A_j) (B_i^-1 B_j)^-1) for i != j.  out [3] = {mean |e[:3]|,
   mean |e[3:]|, s}; tr, ro [n (n - 1)]: the pairs in meshgrid 'ij' order
   with the diagonal removed.  One workgroup, one launch. */
int dpvo_pose_loss_forward(const float* G, const float* Ps, int n, float* out, float* tr,
                           float* ro, void* stream);

/* g_out [2] (cotangents of the two means) -> g_G [n, 6], the left-tangent
   gradient of G; s is a constant; Log through the exact J_l^-1. */
int dpvo_pose_loss_backward(const float* G, const float* Ps, int n, const float* g_out,
                            float* g_G, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DPVO_HOT_H */
