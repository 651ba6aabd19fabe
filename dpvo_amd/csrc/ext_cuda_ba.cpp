// ext_cuda_ba.cpp -- the `cuda_ba` extension module (drop-in for
// dpvo/fastba/ba.cpp:183-189), bound to the C ABI in dpvo_hot.h.
#include <map>
#include <mutex>
#include <string>

#include "ext_common.hpp"

using namespace dpvo_ext;

static torch::Tensor f32_contig(const torch::Tensor& t, const char* name) {
  check_device(t, name);
  // packed_accessor32<float> in the reference (ba_cuda.cu:496-501) rejects
  // other dtypes with a RuntimeError; keep that behaviour.
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32, got ",
              t.scalar_type());
  return t.contiguous();
}

// ---------------------------------------------------------------------------
// BA status surfacing.  Every forward ORs its status word into a sticky
// device int (one tiny kernel: graph-capturable, no sync) and, outside graph
// capture, copies it asynchronously to pinned host memory.  The next forward
// (or check_status()) reads a completed copy and raises RuntimeError when a
// fatal bit is set: 2 kk out of range, 4 / 8 large-graph structure limits,
// 16 cross-workgroup timeout (a dX = 0 step that the reference would not take).
// Bit 1 (Cholesky failed -> zero step, dpvo/ba.py:17-21) is recorded, not
// raised (the reference ignores `info`, ba_cuda.cu:547).  Errors therefore
// surface at most one call late, like an asynchronous HIP error.
// ---------------------------------------------------------------------------
namespace {
constexpr int kFatalBits = 2 | 4 | 8 | 16 | 32;
struct StatusSlot {
  torch::Tensor acc;     // device int32 [1], sticky OR of all statuses
  int* host = nullptr;   // pinned copy
  hipEvent_t ev = nullptr;
  bool pending = false;
  int last = 0;          // last status seen on the host (all bits)
};
std::mutex g_st_mu;
std::map<int, StatusSlot> g_st;

std::string describe_status(int s) {
  std::string m;
  if (s & 1) m += " [1: Cholesky failed, zero step]";
  if (s & 2) m += " [2: kk outside [0, num_patches)]";
  if (s & 4) m += " [4: a patch touches more free poses than the large-graph solver handles]";
  if (s & 8) m += " [8: too many border poses for the large-graph solver]";
  if (s & 16) m += " [16: cross-workgroup wait timed out]";
  if (s & 32) m += " [32: window graph exceeds the per-workgroup LDS capacity]";
  return m;
}

// consume a finished copy; raise on fatal bits (and reset the accumulator)
void consume(StatusSlot& sl, bool wait, void* stream) {
  if (!sl.pending) return;
  if (wait) {
    (void)hipEventSynchronize(sl.ev);
  } else if (hipEventQuery(sl.ev) != hipSuccess) {
    return;
  }
  sl.pending = false;
  sl.last = *sl.host;
  if (sl.last & kFatalBits) {
    const int s = sl.last;
    (void)hipMemsetAsync(sl.acc.data_ptr<int>(), 0, sizeof(int), (hipStream_t)stream);
    *sl.host = 0;
    TORCH_CHECK(false, "cuda_ba.forward: bundle adjustment reported status ", s,
                describe_status(s), "; the poses/patches of that call did not take the "
                "reference's step");
  }
}

StatusSlot& slot_for(const torch::Tensor& like) {
  const int dev = like.get_device();
  auto& sl = g_st[dev];
  if (!sl.acc.defined() && !is_capturing()) {
    sl.acc = torch::zeros({1}, like.options().dtype(torch::kInt32));
    TORCH_CHECK(hipHostMalloc((void**)&sl.host, sizeof(int), hipHostMallocDefault) == hipSuccess,
                "cuda_ba: pinned status buffer");
    *sl.host = 0;
    TORCH_CHECK(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) == hipSuccess,
                "cuda_ba: status event");
    check_status(dpvo_ba_set_status_sink(sl.acc.data_ptr<int>()), "cuda_ba: status sink");
  }
  return sl;
}

void track_status(const torch::Tensor& ws, const torch::Tensor& like, int E, int t0, int t1) {
  std::lock_guard<std::mutex> lk(g_st_mu);
  auto& sl = slot_for(like);
  if (!sl.acc.defined()) return;  // first call happened inside a capture: untracked
  void* st = current_stream();
  check_status(dpvo_ba_status_accumulate(ws.data_ptr(), E, t0, t1, sl.acc.data_ptr<int>(), st),
               "cuda_ba.forward(status)");
  if (is_capturing() || sl.pending) return;
  TORCH_CHECK(hipMemcpyAsync(sl.host, sl.acc.data_ptr<int>(), sizeof(int), hipMemcpyDeviceToHost,
                             (hipStream_t)st) == hipSuccess, "cuda_ba: status copy");
  TORCH_CHECK(hipEventRecord(sl.ev, (hipStream_t)st) == hipSuccess, "cuda_ba: status event");
  sl.pending = true;
}

// before a launch: creates the device's slot (registering its status sink, so
// the window kernels of this very call report into it) and raises a finished
// earlier call's fatal status
void poll_status(const torch::Tensor& like) {
  if (is_capturing()) return;
  std::lock_guard<std::mutex> lk(g_st_mu);
  auto& sl = slot_for(like);
  consume(sl, false, current_stream());
}
}  // namespace

// cuda_ba.check_status(device): synchronise on the status of every forward
// issued so far on that device; raise on a fatal bit; return the OR of all
// bits seen (bit 1 included) and reset the accumulator.
int ba_check_status(torch::Tensor like) {
  TORCH_CHECK(!is_capturing(), "cuda_ba.check_status: not allowed during graph capture");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(like.device());
  std::lock_guard<std::mutex> lk(g_st_mu);
  auto it = g_st.find(like.get_device());
  if (it == g_st.end() || !it->second.acc.defined()) return 0;
  auto& sl = it->second;
  void* st = current_stream();
  consume(sl, true, st);  // may raise
  TORCH_CHECK(hipMemcpyAsync(sl.host, sl.acc.data_ptr<int>(), sizeof(int), hipMemcpyDeviceToHost,
                             (hipStream_t)st) == hipSuccess, "cuda_ba: status copy");
  TORCH_CHECK(hipEventRecord(sl.ev, (hipStream_t)st) == hipSuccess, "cuda_ba: status event");
  sl.pending = true;
  consume(sl, true, st);  // may raise
  const int all = sl.last;
  (void)hipMemsetAsync(sl.acc.data_ptr<int>(), 0, sizeof(int), (hipStream_t)st);
  *sl.host = 0;
  return all;
}

// ---------------------------------------------------------------------------
// Input validation shared by the BA and reprojection entries.  Both helpers
// normalise the caller's tensors in place (which keeps their storage alive)
// and hand back raw pointers; a tensor that is already contiguous is kept as
// it is: no copy, no allocation, no device query.
// ---------------------------------------------------------------------------
struct EdgeIn {
  float* poses;
  float* patches;
  const float* intrinsics;
  const int64_t* ii;
  const int64_t* jj;
  const int64_t* kk;
  int P, E, num_poses, num_patches;
};

// The edge inputs of every entry: GPU tensors, float32 / int64, made
// contiguous, ii / jj / kk of one length (the kernels read jj[e] and kk[e] for
// every e < ii.numel()).  Non-contiguous poses / patches are copied, which
// suits the reprojections; the in-place entries call ba_inputs first.
static EdgeIn edge_inputs(torch::Tensor& poses, torch::Tensor& patches, torch::Tensor& intrinsics,
                          torch::Tensor& ii, torch::Tensor& jj, torch::Tensor& kk) {
  poses = f32_contig(poses, "poses");
  patches = f32_contig(patches, "patches");
  intrinsics = f32_contig(intrinsics, "intrinsics");
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  EdgeIn e;
  e.P = patches.size(-1);
  e.E = ii.numel();
  TORCH_CHECK(jj.numel() == e.E && kk.numel() == e.E, "ii, jj, kk must have equal length");
  e.num_poses = poses.numel() / 7;
  e.num_patches = patches.numel() / (3 * e.P * e.P);
  e.poses = poses.data_ptr<float>();
  e.patches = patches.data_ptr<float>();
  e.intrinsics = intrinsics.data_ptr<float>();
  e.ii = ii.data_ptr<int64_t>();
  e.jj = jj.data_ptr<int64_t>();
  e.kk = kk.data_ptr<int64_t>();
  return e;
}

struct BaIn {
  const float* target;
  const float* weight;
  const float* lmbda;
};

// What the in-place BA entries need beyond the edges: poses / patches that the
// kernels can update where they are, and the residual inputs.  The sizes of
// target / weight against E stay with each entry.
static BaIn ba_inputs(const torch::Tensor& poses, const torch::Tensor& patches,
                      torch::Tensor& target, torch::Tensor& weight, torch::Tensor& lmbda) {
  check_device(poses, "poses");
  check_device(patches, "patches");
  TORCH_CHECK(poses.scalar_type() == torch::kFloat32 && patches.scalar_type() == torch::kFloat32,
              "poses / patches must be float32");
  // poses.view({-1,7}) / patches.view({-1,3,P,P}) must alias the caller's
  // storage for the in-place update to land (ba_cuda.cu:458-459)
  TORCH_CHECK(poses.is_contiguous() && patches.is_contiguous(),
              "poses and patches must be contiguous (updated in place)");
  target = f32_contig(target, "target");
  weight = f32_contig(weight, "weight");
  lmbda = f32_contig(lmbda, "lmbda");
  return {target.data_ptr<float>(), weight.data_ptr<float>(), lmbda.data_ptr<float>()};
}

// ba.cpp:32-45 -> cuda_ba (ba_cuda.cu:433-582).  Mutates poses / patches.
static torch::Tensor ba_forward_ws(torch::Tensor poses, torch::Tensor patches,
                                      torch::Tensor intrinsics, torch::Tensor target,
                                      torch::Tensor weight, torch::Tensor lmbda, torch::Tensor ii,
                                      torch::Tensor jj, torch::Tensor kk, int PPF, int t0, int t1,
                                      int iterations, bool eff_impl) {
  const BaIn b = ba_inputs(poses, patches, target, weight, lmbda);
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(target.numel() >= 2 * e.E && weight.numel() >= 2 * e.E,
              "target/weight must be [.., E, 2]");
  if (e.E == 0 || iterations <= 0) return torch::Tensor();
  TORCH_CHECK(t1 - t0 <= dpvo_ba_max_free_poses(), "cuda_ba.forward: t1 - t0 = ", t1 - t0,
              " free poses exceeds this build's limit (", dpvo_ba_max_free_poses(), ")");
  poll_status(poses);  // a previous call's fatal status raises here
  const size_t wsb = dpvo_ba_workspace_bytes(e.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, poses.options().dtype(torch::kUInt8));
  check_status(dpvo_ba_forward(e.poses, e.patches, e.intrinsics, b.target, b.weight, b.lmbda, e.ii,
                               e.jj, e.kk, e.E, e.P, e.num_poses, e.num_patches, PPF, t0, t1,
                               iterations, eff_impl ? 1 : 0, ws.data_ptr(), wsb,
                               current_stream()),
               "cuda_ba.forward");
  track_status(ws, poses, e.E, t0, t1);
  return ws;
}

std::vector<torch::Tensor> ba_forward(torch::Tensor poses, torch::Tensor patches,
                                      torch::Tensor intrinsics, torch::Tensor target,
                                      torch::Tensor weight, torch::Tensor lmbda, torch::Tensor ii,
                                      torch::Tensor jj, torch::Tensor kk, int PPF, int t0, int t1,
                                      int iterations, bool eff_impl) {
  ba_forward_ws(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, PPF, t0, t1,
                iterations, eff_impl);
  return {};
}

// Split call (dpvo_ba_plan / dpvo_ba_forward_planned): plan(...) -> workspace,
// reads ii / jj / kk only (may run on a side stream concurrently with A-CORR);
// forward_planned(ws, ...) runs the iterations.  Same results as forward().
bool ba_plan_supported(int E, int t0, int t1, int P) { return dpvo_ba_plan_supported(E, t0, t1, P); }

torch::Tensor ba_plan(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int64_t num_patches,
                      int64_t num_poses, int t0, int t1) {
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ii.device());
  const int E = ii.numel();
  TORCH_CHECK(jj.numel() == E && kk.numel() == E, "ii, jj, kk must have equal length");
  const size_t wsb = dpvo_ba_workspace_bytes(E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, ii.options().dtype(torch::kUInt8));
  check_status(dpvo_ba_plan(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(),
                            E, (int)num_patches, (int)num_poses, t0, t1, ws.data_ptr(), wsb,
                            current_stream()),
               "cuda_ba.plan");
  return ws;
}

std::vector<int64_t> ba_plan_offsets(int64_t E, int t0, int t1) {
  std::vector<int64_t> o(5);
  check_status(dpvo_ba_plan_offsets((int)E, t0, t1, o.data()), "cuda_ba.plan_offsets");
  return o;
}

void ba_forward_planned(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
                        torch::Tensor intrinsics, torch::Tensor target, torch::Tensor weight,
                        torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                        int t0, int t1, int iterations) {
  const BaIn b = ba_inputs(poses, patches, target, weight, lmbda);
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(target.numel() >= 2 * e.E && weight.numel() >= 2 * e.E,
              "target/weight must be [.., E, 2]");
  if (e.E == 0 || iterations <= 0) return;
  poll_status(poses);
  check_status(dpvo_ba_forward_planned(e.poses, e.patches, e.intrinsics, b.target, b.weight,
                                       b.lmbda, e.ii, e.jj, e.kk, e.E, e.P, e.num_poses,
                                       e.num_patches, t0, t1, iterations, ws.data_ptr(),
                                       ws.numel(), current_stream()),
               "cuda_ba.forward_planned");
  track_status(ws, poses, e.E, t0, t1);
}

// Same call; returns the DPVO_BA_MARKS phase marks (100 MHz ticks: [0, 128) phases; window kernel
// [128 + 256 it + g] / [640 + 256 it + g] per-workgroup assembled / partials seen, [1152 + g]
// setup done, [1408 + g] iteration 0 assembled before its reduction) followed by the
// multi-kernel path's per-workgroup marks.
torch::Tensor ba_forward_marks(torch::Tensor poses, torch::Tensor patches,
                               torch::Tensor intrinsics, torch::Tensor target, torch::Tensor weight,
                               torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj,
                               torch::Tensor kk, int PPF, int t0, int t1, int iterations,
                               bool eff_impl) {
  check_status(dpvo_ba_set_marks(1), "cuda_ba.forward_marks");
  torch::Tensor ws;
  try {
    ws = ba_forward_ws(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, PPF, t0, t1,
                       iterations, eff_impl);
  } catch (...) {
    dpvo_ba_set_marks(0);
    throw;
  }
  check_status(dpvo_ba_set_marks(0), "cuda_ba.forward_marks");
  auto out = torch::zeros({DPVO_BA_MARKS}, poses.options().dtype(torch::kInt64));
  if (!ws.defined()) return out;
  check_status(dpvo_ba_phase_marks(ws.data_ptr(), ii.numel(), t0, t1, out.data_ptr<int64_t>(),
                                   current_stream()),
               "cuda_ba.forward_marks");
  const int N = t1 - t0, E = ii.numel();
  const int64_t grid = N * (N + 1) / 2;
  auto wg = torch::zeros({2 * grid}, out.options());
  check_status(dpvo_ba_workgroup_marks(ws.data_ptr(), E, t0, t1, wg.data_ptr<int64_t>(),
                                       current_stream()),
               "cuda_ba.forward_marks");
  return torch::cat({out, wg});
}

// The marks a workspace holds (after launches made with set_marks(true)).
torch::Tensor ba_workspace_marks(torch::Tensor ws, int64_t E, int t0, int t1) {
  check_device(ws, "ws");
  TORCH_CHECK(E >= 0 && t1 > t0, "cuda_ba.workspace_marks: bad E / window");
  TORCH_CHECK((size_t)ws.nbytes() >= dpvo_ba_workspace_bytes((int)E, t0, t1),
              "cuda_ba.workspace_marks: ws is not a BA workspace planned for (E, t0, t1)");
  auto out = torch::zeros({DPVO_BA_MARKS}, ws.options().dtype(torch::kInt64));
  check_status(dpvo_ba_phase_marks(ws.data_ptr(), (int)E, t0, t1, out.data_ptr<int64_t>(),
                                   current_stream()),
               "cuda_ba.workspace_marks");
  return out;
}

// Same call; returns the pose step dX [N, 6] (fp64) of the last iteration
// (ba_cuda.cu:561-562) -- the parity tests' view of the solve.
torch::Tensor ba_forward_dx(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                            torch::Tensor target, torch::Tensor weight, torch::Tensor lmbda,
                            torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int PPF, int t0,
                            int t1, int iterations, bool eff_impl) {
  auto ws = ba_forward_ws(poses, patches, intrinsics, target, weight, lmbda, ii, jj, kk, PPF, t0,
                          t1, iterations, eff_impl);
  const int N = t1 > t0 ? t1 - t0 : 0;
  auto out = torch::zeros({N, 6}, poses.options().dtype(torch::kFloat64));
  if (!ws.defined() || N == 0) return out;
  check_status(dpvo_ba_last_dx(ws.data_ptr(), ii.numel(), t0, t1, out.data_ptr<double>(),
                               current_stream()),
               "cuda_ba.forward_dx");
  return out;
}

// dX [N, 6] of the last iteration of forward_planned(_dev) on workspace ws
torch::Tensor ba_last_dx(torch::Tensor ws, int64_t E, int t0, int t1) {
  const int N = t1 > t0 ? t1 - t0 : 0;
  auto out = torch::zeros({N, 6}, ws.options().dtype(torch::kFloat64));
  if (N == 0) return out;
  check_status(dpvo_ba_last_dx(ws.data_ptr(), (int)E, t0, t1, out.data_ptr<double>(),
                               current_stream()),
               "cuda_ba.last_dx");
  return out;
}

// ba.cpp:47-53 -> cuda_reproject (ba_cuda.cu:585-616)
torch::Tensor ba_reproject(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                           torch::Tensor ii, torch::Tensor jj, torch::Tensor kk) {
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  check_status(dpvo_reproject(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P,
                              e.num_poses, e.num_patches, coords.data_ptr<float>(),
                              current_stream()),
               "cuda_ba.reproject");
  return coords.view({1, e.E, 2, e.P, e.P});
}

// reproject + the A-CORR edge order (edges grouped by target frame) in one launch
std::vector<torch::Tensor> ba_reproject_ordered(torch::Tensor poses, torch::Tensor patches,
                                                torch::Tensor intrinsics, torch::Tensor ii,
                                                torch::Tensor jj, torch::Tensor kk, int N2) {
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  auto order = torch::empty({e.E}, poses.options().dtype(torch::kInt32));
  check_status(dpvo_reproject_ordered(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P,
                                      e.num_poses, e.num_patches, N2, coords.data_ptr<float>(),
                                      order.data_ptr<int32_t>(), current_stream()),
               "cuda_ba.reproject_ordered");
  return {coords.view({1, e.E, 2, e.P, e.P}), order};
}

// reproject + edge order + BA plan (workspace for forward_planned) in one launch
std::vector<torch::Tensor> ba_reproject_ordered_plan(torch::Tensor poses, torch::Tensor patches,
                                                     torch::Tensor intrinsics, torch::Tensor ii,
                                                     torch::Tensor jj, torch::Tensor kk, int N2,
                                                     int t0, int t1) {
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  auto order = torch::empty({e.E}, poses.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_ba_workspace_bytes(e.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, poses.options().dtype(torch::kUInt8));
  check_status(dpvo_reproject_ordered_plan(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E,
                                           e.P, e.num_poses, e.num_patches, N2,
                                           coords.data_ptr<float>(), order.data_ptr<int32_t>(), t0,
                                           t1, ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.reproject_ordered_plan");
  return {coords.view({1, e.E, 2, e.P, e.P}), order, ws};
}

// ... plus the new frame's pyramid insertion in the same launch (src [C, H, W]
// NCHW, dst[l] the channels-last [C, H/s, W/s] slot view of level l)
std::vector<torch::Tensor> ba_reproject_ordered_plan_insert(
    torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics, torch::Tensor ii,
    torch::Tensor jj, torch::Tensor kk, int N2, int t0, int t1, torch::Tensor src,
    std::vector<torch::Tensor> dst, std::vector<int64_t> scales) {
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  check_device(src, "src");
  TORCH_CHECK(src.dim() == 3, "src must be [C, H, W]");
  TORCH_CHECK(src.scalar_type() == torch::kFloat32 || src.scalar_type() == torch::kFloat16,
              "src must be float32 or float16");
  TORCH_CHECK(dst.size() == scales.size() && !dst.empty(), "one scale per destination level");
  src = src.contiguous();
  const int C = src.size(0), H = src.size(1), W = src.size(2);
  std::vector<void*> ptrs;
  std::vector<int> sc;
  for (size_t l = 0; l < dst.size(); l++) {
    const torch::Tensor& d = dst[l];
    check_device(d, "dst");
    const int s = (int)scales[l];
    TORCH_CHECK(d.scalar_type() == src.scalar_type() && d.dim() == 3 && d.size(0) == C && s > 0 &&
                    d.size(1) == H / s && d.size(2) == W / s,
                "dst level ", l, " must be [C, H/s, W/s] of src's dtype");
    TORCH_CHECK(d.stride(0) == 1 && d.stride(2) == C && d.stride(1) == (int64_t)C * d.size(2),
                "dst level ", l, " must be channels-last");
    ptrs.push_back(d.data_ptr());
    sc.push_back(s);
  }
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  auto order = torch::empty({e.E}, poses.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_ba_workspace_bytes(e.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, poses.options().dtype(torch::kUInt8));
  check_status(dpvo_reproject_ordered_plan_insert(
                   e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P, e.num_poses,
                   e.num_patches, N2, coords.data_ptr<float>(), order.data_ptr<int32_t>(), t0, t1,
                   ws.data_ptr(), wsb, src.data_ptr(), ptrs.data(), sc.data(), (int)ptrs.size(), C,
                   H, W, dtype_code(src), current_stream()),
               "cuda_ba.reproject_ordered_plan_insert");
  return {coords.view({1, e.E, 2, e.P, e.P}), order, ws};
}

// Device-t0 variants (graph-replayed DPVO updates: the window start moves
// every frame while shapes stay fixed): t0_dev is an int32 device scalar, N =
// t1 - t0 the (fixed) number of free poses.
static const int32_t* dev_scalar(const torch::Tensor& t, const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kInt32 && t.numel() >= 1 && t.is_contiguous(), name,
              " must be a contiguous int32 device tensor");
  return t.data_ptr<int32_t>();
}

std::vector<torch::Tensor> ba_reproject_ordered_plan_dev(torch::Tensor poses, torch::Tensor patches,
                                                         torch::Tensor intrinsics, torch::Tensor ii,
                                                         torch::Tensor jj, torch::Tensor kk, int N2,
                                                         torch::Tensor t0_dev, int N) {
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  auto order = torch::empty({e.E}, poses.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_ba_workspace_bytes(e.E, 0, N);
  auto ws = torch::empty({(int64_t)wsb}, poses.options().dtype(torch::kUInt8));
  check_status(dpvo_reproject_ordered_plan_dev(
                   e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P, e.num_poses,
                   e.num_patches, N2, coords.data_ptr<float>(), order.data_ptr<int32_t>(),
                   dev_scalar(t0_dev, "t0_dev"), N, ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.reproject_ordered_plan_dev");
  return {coords.view({1, e.E, 2, e.P, e.P}), order, ws};
}

void ba_forward_planned_dev(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
                            torch::Tensor intrinsics, torch::Tensor target, torch::Tensor weight,
                            torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj,
                            torch::Tensor kk, torch::Tensor t0_dev, int N, int iterations) {
  const BaIn b = ba_inputs(poses, patches, target, weight, lmbda);
  const EdgeIn e = edge_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  // exactly 2 E here, where forward / forward_planned accept longer buffers
  TORCH_CHECK(target.numel() == 2 * (int64_t)e.E && weight.numel() == 2 * (int64_t)e.E,
              "target / weight must hold 2 E values");
  // runs under graph capture: no status poll before, no status copy after
  check_status(dpvo_ba_forward_planned_dev(e.poses, e.patches, e.intrinsics, b.target, b.weight,
                                           b.lmbda, e.ii, e.jj, e.kk, e.E, e.P, e.num_poses,
                                           e.num_patches, dev_scalar(t0_dev, "t0_dev"), N,
                                           iterations, ws.data_ptr(), ws.numel(),
                                           current_stream()),
               "cuda_ba.forward_planned_dev");
}

// ba.cpp:59-97 (host loop in the reference; here one O(E^2) LDS-tiled kernel)
std::vector<torch::Tensor> ba_neighbors(torch::Tensor ii, torch::Tensor jj) {
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ii.device());
  const int E = ii.numel();
  auto ix = torch::empty({E}, ii.options());
  auto jx = torch::empty({E}, ii.options());
  check_status(dpvo_neighbors(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), E,
                              ix.data_ptr<int64_t>(), jx.data_ptr<int64_t>(), current_stream()),
               "cuda_ba.neighbors");
  return {ix, jx};
}

// ba.cpp:120-180: Sim3 pose-graph solve of the loop-closure backend
// (optim_utils.py:229).  Like the reference it accepts tensors on any device
// and returns delta on res.device() (ba.cpp:123-129, 170): host inputs (the
// loop-closure worker runs perform_updates on CPU tensors, long_term.py:258)
// are copied to the current HIP device, solved there, and copied back.
// Assembly of A = J^T J (+ damping) and b = -J^T res on the device (pgo.hip,
// fp64 like the reference's Eigen system); the SPD solve of the top-left
// freen*7 block by the device Cholesky in fp64; delta returned as f32 [n, 7]
// with the rows of fixed poses zero (ba.cpp:103-118).  A factorisation that
// fails (NaN / not positive definite) raises RuntimeError instead of
// returning garbage (the reference leaves Eigen's info unchecked).
std::vector<torch::Tensor> ba_solve_system(torch::Tensor J_Ginv_i, torch::Tensor J_Ginv_j,
                                           torch::Tensor ii, torch::Tensor jj, torch::Tensor res,
                                           double ep, double lm, int freen) {
  const torch::Device out_dev = res.device();
  torch::Device dev = out_dev;
  if (!res.is_cuda()) {
    TORCH_CHECK(torch::cuda::is_available(),
                "cuda_ba.solve_system: no HIP device (the MI355X build has no CPU path)");
    dev = torch::Device(torch::kCUDA, c10::hip::current_device());
  }
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
  J_Ginv_i = J_Ginv_i.to(dev);
  J_Ginv_j = J_Ginv_j.to(dev);
  ii = ii.to(dev);
  jj = jj.to(dev);
  res = res.to(dev);
  J_Ginv_i = f32_contig(J_Ginv_i, "J_Ginv_i");
  J_Ginv_j = f32_contig(J_Ginv_j, "J_Ginv_j");
  res = f32_contig(res, "res");
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  const int64_t r = res.size(0);
  TORCH_CHECK(r > 0 && res.numel() == 7 * r, "res must be [r, 7] with r > 0");
  TORCH_CHECK(J_Ginv_i.numel() == 49 * r && J_Ginv_j.numel() == 49 * r,
              "J_Ginv_i / J_Ginv_j must be [r, 7, 7]");
  TORCH_CHECK(ii.numel() == r && jj.numel() == r, "ii / jj must be [r]");
  // The structure (which poses a long edge touches) is host logic, as in the
  // reference (ba.cpp:141-158 builds the triplets on the host): one copy of
  // the indices to the host, which also does the reference's checks.
  const auto iih = ii.cpu(), jjh = jj.cpu();
  const int64_t* ip = iih.data_ptr<int64_t>();
  const int64_t* jp = jjh.data_ptr<int64_t>();
  int64_t n = 0;
  for (int64_t x = 0; x < r; x++) {
    // the reference calls exit(1) on a self edge (ba.cpp:150-151); raise instead
    TORCH_CHECK(ip[x] != jp[x], "cuda_ba.solve_system: edge with ii == jj");
    TORCH_CHECK(ip[x] >= 0 && jp[x] >= 0, "cuda_ba.solve_system: negative pose index");
    n = std::max(n, std::max(ip[x], jp[x]) + 1);
  }
  int64_t nf = freen;  // solve(A, b, freen*7): < 0 (or past the end) -> whole system
  if (nf < 0 || nf > n) nf = n;
  auto delta = torch::zeros({n, 7}, res.options().dtype(torch::kFloat64));
  if (nf > 0) {
    TORCH_CHECK(nf < (1LL << 30), "cuda_ba.solve_system: too many poses");
    int64_t len = 0;
    check_status(dpvo_pgo_plan(ip, jp, (int)r, (int)nf, nullptr, 0, &len), "cuda_ba.solve_system");
    auto planh = torch::empty({len}, torch::kInt64);
    check_status(dpvo_pgo_plan(ip, jp, (int)r, (int)nf, planh.data_ptr<int64_t>(), len, &len),
                 "cuda_ba.solve_system");
    const int64_t* hdr = planh.data_ptr<int64_t>();
    const int64_t m = hdr[3], ws_n = hdr[25], hS = hdr[22], hBB = hdr[23], hDelta = hdr[24];
    auto plan = planh.to(dev, /*non_blocking=*/false);
    auto ws = torch::empty({ws_n}, res.options().dtype(torch::kFloat64));
    auto fail = torch::zeros({1}, res.options().dtype(torch::kInt32));
    check_status(dpvo_pgo_factor(J_Ginv_i.data_ptr<float>(), J_Ginv_j.data_ptr<float>(),
                                 ii.data_ptr<int64_t>(), res.data_ptr<float>(),
                                 plan.data_ptr<int64_t>(), hdr, (float)ep, (float)lm,
                                 ws.data_ptr<double>(), fail.data_ptr<int>(), current_stream()),
                 "cuda_ba.solve_system");
    torch::Tensor xB, info = torch::zeros({1}, res.options().dtype(torch::kInt32));
    if (m > 0) {  // dense SPD solve of the border system (7 m unknowns)
      auto S = ws.narrow(0, hS, 49 * m * m).view({7 * m, 7 * m});
      auto bB = ws.narrow(0, hBB, 7 * m);
      auto chol = at::linalg_cholesky_ex(S);
      info = std::get<1>(chol).to(torch::kInt32).view({1});
      xB = at::cholesky_solve(bB.unsqueeze(1), std::get<0>(chol)).squeeze(1).contiguous();
    }
    check_status(dpvo_pgo_back(plan.data_ptr<int64_t>(), hdr,
                               m > 0 ? xB.data_ptr<double>() : nullptr, ws.data_ptr<double>(),
                               current_stream()),
                 "cuda_ba.solve_system");
    delta.narrow(0, 0, nf).copy_(ws.narrow(0, hDelta, 7 * nf).view({nf, 7}));
    if (m > 0) {
      auto bidx = planh.narrow(0, hdr[7], 3 * m).view({m, 3}).select(1, 0).contiguous().to(dev);
      delta.index_copy_(0, bidx, xB.view({m, 7}));
    }
    // one device->host sync for both failure reports
    const auto st = torch::cat({fail, info}).cpu();
    const int* sv = st.data_ptr<int>();
    TORCH_CHECK(sv[0] == 0 && sv[1] == 0,
                "cuda_ba.solve_system: the damped pose-graph system is not positive definite "
                "(segment pivot failure ", sv[0], ", border Cholesky info ", sv[1],
                "); check for NaN residuals/Jacobians or unconstrained poses with ep = 0");
  }
  return {delta.to(torch::kFloat32).to(out_dev)};
}

// Residual (and Jacobians) of every pose-graph edge in one launch: the device
// form of optim_utils.py:152-189 (_residual + batch_jacobian), whose outputs
// are solve_system's inputs.  Everything is validated on the host before the
// launch; the index range check costs one reduction and one sync (the LM loop
// of dpvo_amd/loop_closure.py syncs every iteration anyway).
std::vector<torch::Tensor> ba_pgo_residual(torch::Tensor Ginv, torch::Tensor C, torch::Tensor ii,
                                           torch::Tensor jj, bool jacobian) {
  check_device(Ginv, "Ginv");
  check_device(C, "C");
  TORCH_CHECK(Ginv.scalar_type() == torch::kFloat32 || Ginv.scalar_type() == torch::kFloat64,
              "cuda_ba.pgo_residual: Ginv must be float32 or float64");
  TORCH_CHECK(C.scalar_type() == Ginv.scalar_type(),
              "cuda_ba.pgo_residual: Ginv and C must have the same dtype");
  TORCH_CHECK(Ginv.dim() == 2 && Ginv.size(1) == 7, "cuda_ba.pgo_residual: Ginv must be [n, 7]");
  TORCH_CHECK(C.dim() == 2 && C.size(1) == 8, "cuda_ba.pgo_residual: C must be [r, 8]");
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  const int64_t n = Ginv.size(0), r = C.size(0);
  TORCH_CHECK(ii.dim() == 1 && jj.dim() == 1 && ii.numel() == r && jj.numel() == r,
              "cuda_ba.pgo_residual: ii / jj must be [r]");
  TORCH_CHECK(Ginv.device() == C.device() && ii.device() == C.device() &&
                  jj.device() == C.device(),
              "cuda_ba.pgo_residual: tensors on different devices");
  TORCH_CHECK(r <= (1 << 26) && n < (1LL << 31), "cuda_ba.pgo_residual: graph too large");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(Ginv.device());
  Ginv = Ginv.contiguous();
  C = C.contiguous();
  auto res = torch::empty({r, 7}, Ginv.options());
  torch::Tensor Ji, Jj;
  if (jacobian) {
    Ji = torch::empty({r, 7, 7}, Ginv.options());
    Jj = torch::empty({r, 7, 7}, Ginv.options());
  }
  if (r > 0) {
    const auto mm = at::aminmax(torch::cat({ii, jj}));
    const auto mmh = torch::stack({std::get<0>(mm), std::get<1>(mm)}).cpu();
    const int64_t lo = mmh.data_ptr<int64_t>()[0], hi = mmh.data_ptr<int64_t>()[1];
    TORCH_CHECK(lo >= 0 && hi < n, "cuda_ba.pgo_residual: pose index out of range [0, ", n,
                "): min ", lo, ", max ", hi);
    check_status(dpvo_pgo_residual(Ginv.data_ptr(), C.data_ptr(), ii.data_ptr<int64_t>(),
                                   jj.data_ptr<int64_t>(), (int)r, (int)n, dtype_code(Ginv),
                                   res.data_ptr(), jacobian ? Ji.data_ptr() : nullptr,
                                   jacobian ? Jj.data_ptr() : nullptr, current_stream()),
                 "cuda_ba.pgo_residual");
  }
  if (jacobian) return {res, Ji, Jj};
  return {res};
}

// RANSAC-Umeyama estimate of a loop measurement (optim_utils.py:64-150) in two
// launches: [model f64[21], info i32[4], mask bool[N]] of dpvo_ransac_umeyama
// (+ counts i32[H], the score of every hypothesis, with return_counts).
// check_samples: the range check of `samples` costs one aminmax and one host
// read, as pgo_residual's; without it (the caller drew the samples itself, or
// the stream is being captured) the call makes no sync, and a sample outside
// [0, N) only makes its hypothesis degenerate.
std::vector<torch::Tensor> ba_ransac_umeyama(torch::Tensor src, torch::Tensor dst,
                                             torch::Tensor samples, double threshold,
                                             int64_t early_exit, bool check_samples,
                                             bool return_counts) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda() && samples.is_cuda(),
              "cuda_ba.ransac_umeyama: src, dst and samples must be GPU (HIP) tensors; the "
              "MI355X build has no CPU path");
  TORCH_CHECK(src.scalar_type() == torch::kFloat32 || src.scalar_type() == torch::kFloat64,
              "cuda_ba.ransac_umeyama: src must be float32 or float64");
  TORCH_CHECK(dst.scalar_type() == src.scalar_type(),
              "cuda_ba.ransac_umeyama: src and dst must have the same dtype");
  TORCH_CHECK(src.dim() == 2 && src.size(1) == 3 && dst.dim() == 2 && dst.size(1) == 3 &&
                  src.size(0) == dst.size(0),
              "cuda_ba.ransac_umeyama: src and dst must both be [N, 3]");
  TORCH_CHECK(samples.scalar_type() == torch::kInt32 || samples.scalar_type() == torch::kInt64,
              "cuda_ba.ransac_umeyama: samples must be int32 or int64");
  TORCH_CHECK(samples.dim() == 2 && samples.size(1) == 3 && samples.size(0) >= 1,
              "cuda_ba.ransac_umeyama: samples must be [H, 3] with H >= 1");
  TORCH_CHECK(src.device() == dst.device() && src.device() == samples.device(),
              "cuda_ba.ransac_umeyama: tensors on different devices");
  const int64_t N = src.size(0), H = samples.size(0);
  TORCH_CHECK(N >= 3, "cuda_ba.ransac_umeyama: needs N >= 3 points, got ", N);
  TORCH_CHECK(N <= (1 << 28) && H <= (1 << 24), "cuda_ba.ransac_umeyama: problem too large");
  TORCH_CHECK(threshold > 0.0, "cuda_ba.ransac_umeyama: threshold must be positive");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(src.device());
  if (check_samples && !is_capturing()) {
    const auto mm = at::aminmax(samples);
    const auto mmh = torch::stack({std::get<0>(mm), std::get<1>(mm)}).to(torch::kInt64).cpu();
    const int64_t lo = mmh.data_ptr<int64_t>()[0], hi = mmh.data_ptr<int64_t>()[1];
    TORCH_CHECK(lo >= 0 && hi < N, "cuda_ba.ransac_umeyama: sample index out of range [0, ", N,
                "): min ", lo, ", max ", hi);
  }
  src = src.contiguous();
  dst = dst.contiguous();
  samples = samples.to(torch::kInt32).contiguous();
  const auto i32 = src.options().dtype(torch::kInt32);
  auto model = torch::empty({21}, src.options().dtype(torch::kFloat64));
  auto info = torch::empty({4}, i32);
  auto mask = torch::empty({N}, src.options().dtype(torch::kBool));
  const size_t wsb = dpvo_ransac_umeyama_workspace_bytes((int)N, (int)H);
  auto ws = torch::empty({(int64_t)(wsb / sizeof(int32_t))}, i32);
  early_exit = std::min<int64_t>(std::max<int64_t>(early_exit, INT32_MIN), INT32_MAX);
  check_status(dpvo_ransac_umeyama(src.data_ptr(), dst.data_ptr(), (int)N, dtype_code(src),
                                   samples.data_ptr<int32_t>(), (int)H, threshold,
                                   (int)early_exit, model.data_ptr<double>(),
                                   info.data_ptr<int32_t>(),
                                   reinterpret_cast<uint8_t*>(mask.data_ptr<bool>()),
                                   ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.ransac_umeyama");
  if (return_counts) return {model, info, mask, ws.narrow(0, 0, H)};
  return {model, info, mask};
}

// Split F-BA for the edge-sharded multi-GPU path.
torch::Tensor ba_setup(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int num_patches,
                       int t0, int t1) {
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ii.device());
  const int E = ii.numel();
  const size_t wsb = dpvo_ba_workspace_bytes(E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, ii.options().dtype(torch::kUInt8));
  check_status(dpvo_ba_setup(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(),
                             kk.data_ptr<int64_t>(), E, num_patches, t0, t1, ws.data_ptr(), wsb,
                             current_stream()),
               "cuda_ba.setup");
  return ws;
}

std::vector<torch::Tensor> ba_build_schur(torch::Tensor ws, torch::Tensor poses,
                                          torch::Tensor patches, torch::Tensor intrinsics,
                                          torch::Tensor target, torch::Tensor weight,
                                          torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj,
                                          torch::Tensor kk, int t0, int t1) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.is_contiguous() && patches.is_contiguous(), "poses/patches contiguous");
  intrinsics = f32_contig(intrinsics, "intrinsics");
  target = f32_contig(target, "target");
  weight = f32_contig(weight, "weight");
  lmbda = f32_contig(lmbda, "lmbda");
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  const int N = t1 - t0, E = ii.numel(), P = patches.size(-1);
  auto S = torch::zeros({N * (N + 1) / 2, 6, 6}, poses.options().dtype(torch::kFloat64));
  auto y = torch::zeros({6 * N}, poses.options().dtype(torch::kFloat64));
  check_status(dpvo_ba_build_schur(poses.data_ptr<float>(), patches.data_ptr<float>(),
                                   intrinsics.data_ptr<float>(), target.data_ptr<float>(),
                                   weight.data_ptr<float>(), lmbda.data_ptr<float>(),
                                   ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(),
                                   kk.data_ptr<int64_t>(), E, P, poses.numel() / 7, t0, t1,
                                   ws.data_ptr(), S.data_ptr<double>(), y.data_ptr<double>(),
                                   current_stream()),
               "cuda_ba.build_schur");
  return {S, y};
}

torch::Tensor ba_solve_update(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
                              torch::Tensor S, torch::Tensor y, int E, int t0, int t1) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.is_contiguous() && patches.is_contiguous(), "poses/patches contiguous");
  S = S.contiguous();
  y = y.contiguous();
  TORCH_CHECK(S.scalar_type() == torch::kFloat64 && y.scalar_type() == torch::kFloat64,
              "S / y must be float64");
  const int N = t1 - t0, P = patches.size(-1);
  auto dX = torch::zeros({N > 0 ? N : 0, 6}, poses.options().dtype(torch::kFloat64));
  check_status(dpvo_ba_solve_update(poses.data_ptr<float>(), patches.data_ptr<float>(),
                                    S.data_ptr<double>(), y.data_ptr<double>(), E, P,
                                    poses.numel() / 7, t0, t1, ws.data_ptr(),
                                    N > 0 ? dX.data_ptr<double>() : nullptr, current_stream()),
               "cuda_ba.solve_update");
  return dX;
}

torch::Tensor ba_last_status(torch::Tensor ws, int E, int t0, int t1) {
  auto out = torch::zeros({1}, ws.options().dtype(torch::kInt32));
  check_status(dpvo_ba_last_status(ws.data_ptr(), E, t0, t1, out.data_ptr<int>(),
                                   current_stream()),
               "cuda_ba.last_status");
  return out;
}

// Large-graph F-BA split for the edge-sharded driver (dpvo_amd/fastba/sharded.py):
// setup -> [build -> all_reduce(packed) -> solve_update] x iterations.
torch::Tensor gba_setup(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int num_patches,
                        int PPF, int t0, int t1, int own_lo, int own_hi) {
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ii.device());
  const int E = ii.numel();
  TORCH_CHECK(E > 0, "gba_setup: empty graph");
  const size_t wsb = dpvo_gba_workspace_bytes(E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, ii.options().dtype(torch::kUInt8));
  check_status(dpvo_gba_setup(ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(),
                              kk.data_ptr<int64_t>(), E, num_patches, PPF, t0, t1, own_lo, own_hi,
                              ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.gba_setup");
  return ws;
}

void gba_build(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
               torch::Tensor intrinsics, torch::Tensor target, torch::Tensor weight,
               torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj, int t0, int t1) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.is_contiguous() && patches.is_contiguous(), "poses/patches contiguous");
  poses = f32_contig(poses, "poses");
  patches = f32_contig(patches, "patches");
  intrinsics = f32_contig(intrinsics, "intrinsics");
  target = f32_contig(target, "target");
  weight = f32_contig(weight, "weight");
  lmbda = f32_contig(lmbda, "lmbda");
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  const int E = ii.numel(), P = patches.size(-1);
  TORCH_CHECK(ws.numel() >= (int64_t)dpvo_gba_workspace_bytes(E, t0, t1), "workspace too small");
  check_status(dpvo_gba_build(poses.data_ptr<float>(), patches.data_ptr<float>(),
                              intrinsics.data_ptr<float>(), target.data_ptr<float>(),
                              weight.data_ptr<float>(), lmbda.data_ptr<float>(),
                              ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(), E, P,
                              poses.numel() / 7, t0, t1, ws.data_ptr(), current_stream()),
               "cuda_ba.gba_build");
}

// the packed [y (6N) | S blocks (nblk x 36)] fp64 system inside the workspace
torch::Tensor gba_packed(torch::Tensor ws, int E, int t0, int t1, int64_t nblk) {
  const int64_t N = t1 > t0 ? t1 - t0 : 0;
  const int64_t off = (int64_t)dpvo_gba_packed_offset(E, t0, t1);
  const int64_t n = 6 * N + 36 * nblk;
  TORCH_CHECK(off % 8 == 0 && off + 8 * n <= ws.numel(), "gba_packed: bad extent");
  return ws.narrow(0, off, 8 * n).view(torch::kFloat64);
}

void gba_solve_update(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches, int E, int t0,
                      int t1) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.is_contiguous() && patches.is_contiguous(), "poses/patches contiguous");
  check_status(dpvo_gba_solve_update(poses.data_ptr<float>(), patches.data_ptr<float>(), E,
                                     patches.size(-1), t0, t1, ws.data_ptr(), current_stream()),
               "cuda_ba.gba_solve_update");
}

torch::Tensor gba_info(torch::Tensor ws, int E, int t0, int t1) {
  auto out = torch::zeros({8}, ws.options().dtype(torch::kInt32));
  check_status(dpvo_gba_info(ws.data_ptr(), E, t0, t1, out.data_ptr<int>(), current_stream()),
               "cuda_ba.gba_info");
  return out;
}

// PatchGraph bookkeeping on the device (dpvo.py:480-568): no host sync.
static float* opt_f32(const torch::Tensor& t) {
  return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr;
}

void pg_append(torch::Tensor ix, torch::Tensor kk_new, torch::Tensor jj_new, torch::Tensor ii,
               torch::Tensor jj, torch::Tensor kk, torch::Tensor net, torch::Tensor counts) {
  ix = idx64(ix, "ix");
  kk_new = idx64(kk_new, "kk");
  jj_new = idx64(jj_new, "jj");
  TORCH_CHECK(ii.is_contiguous() && jj.is_contiguous() && kk.is_contiguous() &&
              counts.is_contiguous() && counts.scalar_type() == torch::kInt32,
              "pg buffers must be contiguous, counts int32");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ii.device());
  const int max_edges = ii.numel();
  const int DIM = net.defined() && net.numel() ? (int)(net.numel() / max_edges) : 0;
  check_status(dpvo_pg_append(ix.data_ptr<int64_t>(), kk_new.data_ptr<int64_t>(),
                              jj_new.data_ptr<int64_t>(), kk_new.numel(), ii.data_ptr<int64_t>(),
                              jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), opt_f32(net), DIM,
                              counts.data_ptr<int>(), max_edges, current_stream()),
               "cuda_ba.pg_append");
}

void pg_remove(c10::optional<torch::Tensor> mask, c10::optional<torch::Tensor> ix, int64_t thresh,
               int64_t lc_min, bool store, std::vector<torch::Tensor> act,
               std::vector<torch::Tensor> back, std::vector<torch::Tensor> inac,
               torch::Tensor counts, torch::Tensor pos) {
  TORCH_CHECK(act.size() == 6 && back.size() == 6 && inac.size() == 5,
              "act/back: [ii, jj, kk, net, weight, target]; inac: [ii, jj, kk, weight, target]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(counts.device());
  const int max_edges = act[0].numel();
  const int DIM = act[3].defined() && act[3].numel() ? (int)(act[3].numel() / max_edges) : 0;
  const uint8_t* mp = nullptr;
  torch::Tensor m8;
  if (mask && mask->defined()) {
    m8 = mask->to(torch::kUInt8).contiguous();
    check_device(m8, "mask");
    mp = m8.data_ptr<uint8_t>();
  }
  const int64_t* ixp = (ix && ix->defined()) ? idx64(*ix, "ix").data_ptr<int64_t>() : nullptr;
  auto L = [](const torch::Tensor& t) { return t.data_ptr<int64_t>(); };
  check_status(dpvo_pg_remove(mp, ixp, thresh, lc_min, store ? 1 : 0, L(act[0]), L(act[1]),
                              L(act[2]), opt_f32(act[3]), act[4].data_ptr<float>(),
                              act[5].data_ptr<float>(), L(back[0]), L(back[1]), L(back[2]),
                              opt_f32(back[3]), back[4].data_ptr<float>(), back[5].data_ptr<float>(),
                              L(inac[0]), L(inac[1]), L(inac[2]), inac[3].data_ptr<float>(),
                              inac[4].data_ptr<float>(), DIM, counts.data_ptr<int>(),
                              pos.data_ptr<int>(), max_edges, current_stream()),
               "cuda_ba.pg_remove");
}

void pg_remove_window_dev(torch::Tensor ix, torch::Tensor n_dev, int64_t thresh_off,
                         int64_t lc_off, bool lc_on, bool store, std::vector<torch::Tensor> act,
                         std::vector<torch::Tensor> back, std::vector<torch::Tensor> inac,
                         torch::Tensor counts, torch::Tensor pos) {
  TORCH_CHECK(act.size() == 6 && back.size() == 6 && inac.size() == 5,
              "act/back: [ii, jj, kk, net, weight, target]; inac: [ii, jj, kk, weight, target]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(counts.device());
  const int max_edges = act[0].numel();
  const int DIM = act[3].defined() && act[3].numel() ? (int)(act[3].numel() / max_edges) : 0;
  ix = idx64(ix, "ix");
  auto L = [](const torch::Tensor& t) { return t.data_ptr<int64_t>(); };
  check_status(dpvo_pg_remove_window_dev(
                   ix.data_ptr<int64_t>(), dev_scalar(n_dev, "n_dev"), thresh_off, lc_off,
                   lc_on ? 1 : 0, store ? 1 : 0, L(act[0]), L(act[1]), L(act[2]), opt_f32(act[3]),
                   act[4].data_ptr<float>(), act[5].data_ptr<float>(), L(back[0]), L(back[1]),
                   L(back[2]), opt_f32(back[3]), back[4].data_ptr<float>(),
                   back[5].data_ptr<float>(), L(inac[0]), L(inac[1]), L(inac[2]),
                   inac[3].data_ptr<float>(), inac[4].data_ptr<float>(), DIM,
                   counts.data_ptr<int>(), pos.data_ptr<int>(), max_edges, current_stream()),
               "cuda_ba.pg_remove_window_dev");
}

void pg_append_dev(torch::Tensor ix, torch::Tensor kk_new, torch::Tensor jj_new,
                   torch::Tensor n_dev, torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                   torch::Tensor net, torch::Tensor counts) {
  ix = idx64(ix, "ix");
  kk_new = idx64(kk_new, "kk");
  jj_new = idx64(jj_new, "jj");
  TORCH_CHECK(kk_new.numel() == jj_new.numel(), "kk / jj sizes differ");
  TORCH_CHECK(ii.is_contiguous() && jj.is_contiguous() && kk.is_contiguous() &&
              counts.is_contiguous() && counts.scalar_type() == torch::kInt32,
              "pg buffers must be contiguous, counts int32");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ii.device());
  const int max_edges = ii.numel();
  const int DIM = net.defined() && net.numel() ? (int)(net.numel() / max_edges) : 0;
  check_status(dpvo_pg_append_dev(ix.data_ptr<int64_t>(), kk_new.data_ptr<int64_t>(),
                                  jj_new.data_ptr<int64_t>(), dev_scalar(n_dev, "n_dev"),
                                  (int)kk_new.numel(), ii.data_ptr<int64_t>(),
                                  jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), opt_f32(net),
                                  DIM, counts.data_ptr<int>(), max_edges, current_stream()),
               "cuda_ba.pg_append_dev");
}

void pg_remove_frame_dev(torch::Tensor kf, std::vector<torch::Tensor> act,
                         std::vector<torch::Tensor> back, torch::Tensor counts, torch::Tensor pos) {
  TORCH_CHECK(act.size() == 6 && back.size() == 6, "act/back: [ii, jj, kk, net, weight, target]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(counts.device());
  const int max_edges = act[0].numel();
  const int DIM = act[3].defined() && act[3].numel() ? (int)(act[3].numel() / max_edges) : 0;
  auto L = [](const torch::Tensor& t) { return t.data_ptr<int64_t>(); };
  check_status(dpvo_pg_remove_frame_dev(
                   dev_scalar(kf, "kf"), L(act[0]), L(act[1]), L(act[2]), opt_f32(act[3]),
                   act[4].data_ptr<float>(), act[5].data_ptr<float>(), L(back[0]), L(back[1]),
                   L(back[2]), opt_f32(back[3]), back[4].data_ptr<float>(),
                   back[5].data_ptr<float>(), DIM, counts.data_ptr<int>(), pos.data_ptr<int>(),
                   max_edges, current_stream()),
               "cuda_ba.pg_remove_frame_dev");
}

// DPVO.keyframe decision (dpvo.py:586-624): kf = {drop, k}, mag = both motionmags
void kf_motion(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, torch::Tensor counts,
               torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
               torch::Tensor st, int64_t keyframe_index, double keyframe_thresh, torch::Tensor kf,
               torch::Tensor mag) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.scalar_type() == torch::kFloat32 && patches.scalar_type() == torch::kFloat32 &&
                  intrinsics.scalar_type() == torch::kFloat32 && poses.is_contiguous() &&
                  patches.is_contiguous() && intrinsics.is_contiguous(),
              "poses / patches / intrinsics: contiguous float32");
  TORCH_CHECK(mag.scalar_type() == torch::kFloat32 && mag.numel() >= 2 && kf.numel() >= 2,
              "kf int32[2], mag float32[2]");
  auto L = [](const torch::Tensor& t) { return t.data_ptr<int64_t>(); };
  check_status(dpvo_kf_motion(L(idx64(ii, "ii")), L(idx64(jj, "jj")), L(idx64(kk, "kk")),
                              dev_scalar(counts, "counts"), poses.data_ptr<float>(),
                              patches.data_ptr<float>(), intrinsics.data_ptr<float>(),
                              (int)patches.size(-1), dev_scalar(st, "st"), (int)keyframe_index,
                              keyframe_thresh, const_cast<int32_t*>(dev_scalar(kf, "kf")),
                              mag.data_ptr<float>(), current_stream()),
               "cuda_ba.kf_motion");
}

// the rest of the frame drop (dpvo.py:626-673); frames: per-frame arrays whose
// leading dim is the frame (ring 0) or a ring slot (ring > 0)
void kf_shift(torch::Tensor kf, int64_t M, torch::Tensor st, torch::Tensor ii, torch::Tensor jj,
              torch::Tensor kk, torch::Tensor counts, std::vector<torch::Tensor> frames,
              std::vector<int64_t> rings, c10::optional<torch::Tensor> poses,
              c10::optional<torch::Tensor> tstamps, c10::optional<torch::Tensor> delta_log,
              c10::optional<torch::Tensor> delta_tstamps, c10::optional<torch::Tensor> delta_count) {
  TORCH_CHECK(frames.size() == rings.size(), "one ring size per frame array");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(counts.device());
  std::vector<void*> ptrs;
  std::vector<int64_t> bytes;
  std::vector<int32_t> ring;
  for (size_t a = 0; a < frames.size(); a++) {
    check_device(frames[a], "frame array");
    TORCH_CHECK(frames[a].is_contiguous() && frames[a].dim() >= 1, "frame arrays contiguous");
    ptrs.push_back(frames[a].data_ptr());
    bytes.push_back(frames[a].numel() / frames[a].size(0) * frames[a].element_size());
    ring.push_back((int32_t)rings[a]);
  }
  auto L = [](const torch::Tensor& t) { return t.data_ptr<int64_t>(); };
  const bool log = delta_log && delta_log->defined();
  float* dl = nullptr;
  int64_t* dt = nullptr;
  int32_t* dc = nullptr;
  const float* pp = nullptr;
  const int64_t* ts = nullptr;
  int cap = 0;
  if (log) {
    TORCH_CHECK(poses && tstamps && delta_tstamps && delta_count, "delta log needs all buffers");
    // the kernel ORs its delta-log overflow bit into counts[2] (keyframe.hip
    // kf_delta_kernel): counts must hold the error word too
    TORCH_CHECK(counts.numel() >= 3, "kf_shift with a delta log: counts needs >= 3 int32 words "
                                     "(n, m, errors)");
    dl = delta_log->data_ptr<float>();
    dt = delta_tstamps->data_ptr<int64_t>();
    dc = const_cast<int32_t*>(dev_scalar(*delta_count, "delta_count"));
    pp = poses->data_ptr<float>();
    ts = tstamps->data_ptr<int64_t>();
    cap = (int)(delta_log->numel() / 7);
  }
  check_status(dpvo_kf_shift(dev_scalar(kf, "kf"), (int)M, const_cast<int32_t*>(dev_scalar(st, "st")),
                             L(ii), L(jj), L(kk), const_cast<int32_t*>(dev_scalar(counts, "counts")),
                             (int)ii.numel(),
                             ptrs.data(), bytes.data(), ring.data(), (int)ptrs.size(), pp, ts, dl,
                             dt, dc, cap, current_stream()),
               "cuda_ba.kf_shift");
}

// CholeskySolver's device solve (dpvo/ba.py:13-38 -> torch.linalg.cholesky_ex +
// cholesky_solve): batched over the leading dims, fp32 / fp64
static void spd_shapes(const torch::Tensor& H, const torch::Tensor& B, int64_t& batch, int& n,
                       int& k) {
  check_device(H, "H");
  check_device(B, "B");
  TORCH_CHECK(H.dim() >= 2 && H.size(-1) == H.size(-2), "H must be [..., n, n]");
  TORCH_CHECK(B.dim() == H.dim() && B.size(-2) == H.size(-1), "B must be [..., n, k]");
  TORCH_CHECK(H.scalar_type() == B.scalar_type() &&
                  (H.scalar_type() == torch::kFloat32 || H.scalar_type() == torch::kFloat64),
              "H / B: float32 or float64, one dtype");
  for (int64_t d = 0; d + 2 < H.dim(); d++)
    TORCH_CHECK(H.size(d) == B.size(d), "H / B batch dims differ");
  n = (int)H.size(-1);
  k = (int)B.size(-1);
  batch = n ? H.numel() / ((int64_t)n * n) : 0;
}

std::vector<torch::Tensor> spd_solve(torch::Tensor H, torch::Tensor B) {
  int64_t batch;
  int n, k;
  spd_shapes(H, B, batch, n, k);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(H.device());
  H = H.contiguous();
  B = B.contiguous();
  auto L = torch::empty_like(H);
  auto X = torch::empty_like(B);
  std::vector<int64_t> bs(H.sizes().begin(), H.sizes().end() - 2);
  auto info = torch::zeros(bs, H.options().dtype(torch::kInt32));
  check_status(dpvo_spd_solve(H.data_ptr(), B.data_ptr(), L.data_ptr(), X.data_ptr(),
                              info.data_ptr<int32_t>(), (int)batch, n, k, 1, dtype_code(H),
                              current_stream()),
               "cuda_ba.spd_solve");
  return {X, L, info};
}

torch::Tensor spd_solve_factored(torch::Tensor L, torch::Tensor B) {
  int64_t batch;
  int n, k;
  spd_shapes(L, B, batch, n, k);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(L.device());
  L = L.contiguous();
  B = B.contiguous();
  auto X = torch::empty_like(B);
  check_status(dpvo_spd_solve(L.data_ptr(), B.data_ptr(), nullptr, X.data_ptr(), nullptr,
                              (int)batch, n, k, 0, dtype_code(L), current_stream()),
               "cuda_ba.spd_solve_factored");
  return X;
}

// The differentiable BA layer (dpvo/ba.py BA, 88-297): one Gauss-Newton step
// and its adjoint (ba_layer.hip).  No host synchronisation in either call.
struct LayerIn {
  int E, M, p, N, dtype;
};

static LayerIn layer_inputs(torch::Tensor& poses, torch::Tensor& patches, torch::Tensor& intrinsics,
                            torch::Tensor& ii, torch::Tensor& jj, torch::Tensor& kk) {
  check_device(poses, "poses");
  check_device(patches, "patches");
  check_device(intrinsics, "intrinsics");
  const auto dt = poses.scalar_type();
  TORCH_CHECK(dt == torch::kFloat32 || dt == torch::kFloat64,
              "cuda_ba.ba_layer: float32 or float64 tensors");
  TORCH_CHECK(patches.scalar_type() == dt && intrinsics.scalar_type() == dt,
              "cuda_ba.ba_layer: poses, patches and intrinsics must have one dtype");
  TORCH_CHECK(poses.dim() >= 2 && poses.size(-1) == 7, "poses must be [.., N, 7]");
  TORCH_CHECK(patches.dim() >= 4 && patches.size(-3) == 3 && patches.size(-1) == patches.size(-2),
              "patches must be [.., M, 3, p, p]");
  poses = poses.contiguous();
  patches = patches.contiguous();
  intrinsics = intrinsics.contiguous();
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  LayerIn l;
  l.E = ii.numel();
  TORCH_CHECK(jj.numel() == l.E && kk.numel() == l.E, "ii, jj, kk must have equal length");
  l.p = patches.size(-1);
  l.N = poses.numel() / 7;
  l.M = patches.numel() / (3 * (int64_t)l.p * l.p);
  TORCH_CHECK(intrinsics.numel() == 4 * (int64_t)l.N, "intrinsics must be [.., N, 4]");
  l.dtype = dtype_code(poses);
  return l;
}

std::vector<torch::Tensor> ba_layer_forward(torch::Tensor poses, torch::Tensor patches,
                                            torch::Tensor intrinsics, torch::Tensor targets,
                                            torch::Tensor weights,
                                            c10::optional<torch::Tensor> lmbda_dev, double lmbda,
                                            torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                                            int64_t n, int64_t fixedp, bool structure_only,
                                            std::vector<double> bounds, double ep,
                                            bool with_backward) {
  const LayerIn l = layer_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  check_device(targets, "targets");
  check_device(weights, "weights");
  TORCH_CHECK(targets.scalar_type() == poses.scalar_type() &&
                  weights.scalar_type() == poses.scalar_type(),
              "cuda_ba.ba_layer_forward: targets / weights must have the dtype of poses");
  TORCH_CHECK(targets.numel() == 2 * (int64_t)l.E && weights.numel() == 2 * (int64_t)l.E,
              "targets / weights must be [.., E, 2]");
  TORCH_CHECK(bounds.size() == 4, "bounds must hold 4 values");
  TORCH_CHECK(fixedp >= 0 && n >= fixedp && n <= l.N, "cuda_ba.ba_layer_forward: need 0 <= fixedp <= "
              "n <= N, got fixedp ", fixedp, ", n ", n, ", N ", l.N);
  targets = targets.contiguous();
  weights = weights.contiguous();
  const void* lm = nullptr;
  torch::Tensor lmt;
  if (lmbda_dev && lmbda_dev->defined()) {
    check_device(*lmbda_dev, "lmbda");
    TORCH_CHECK(lmbda_dev->numel() == 1, "lmbda must be a float or a 1-element tensor");
    lmt = lmbda_dev->to(poses.scalar_type()).contiguous();
    lm = lmt.data_ptr();
  }
  const int nf = structure_only ? 0 : (int)(n - fixedp);
  const bool none = l.E == 0;  // nothing launched: the outputs are the zero step
  auto dX = none ? torch::zeros({nf, 6}, poses.options()) : torch::empty({nf, 6}, poses.options());
  auto dZ = none ? torch::zeros({l.M}, poses.options()) : torch::empty({l.M}, poses.options());
  const size_t wsb = dpvo_ba_layer_workspace_bytes(l.E, l.M, nf, with_backward ? 1 : 0);
  auto ws = torch::empty({(int64_t)std::max<size_t>(wsb, 32)}, poses.options().dtype(torch::kUInt8));
  if (l.E == 0) {
    ws.zero_();
    return {dX, dZ, ws};
  }
  check_status(dpvo_ba_layer_forward(poses.data_ptr(), patches.data_ptr(), intrinsics.data_ptr(),
                                     targets.data_ptr(), weights.data_ptr(), lm, lmbda,
                                     ii.data_ptr<int64_t>(), jj.data_ptr<int64_t>(),
                                     kk.data_ptr<int64_t>(), l.E, l.M, l.p, l.N, (int)n, (int)fixedp,
                                     structure_only ? 1 : 0, bounds.data(), ep, l.dtype,
                                     dX.data_ptr(), dZ.data_ptr(), ws.data_ptr(), wsb,
                                     with_backward ? 1 : 0, current_stream()),
               "cuda_ba.ba_layer_forward");
  return {dX, dZ, ws};
}

// -> [g_targets [E, 2], g_weights [E, 2], g_poses [N, 6], g_patches [M, 3]]
std::vector<torch::Tensor> ba_layer_backward(torch::Tensor ws, torch::Tensor poses,
                                             torch::Tensor patches, torch::Tensor intrinsics,
                                             torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                                             torch::Tensor gX, torch::Tensor gZ, int64_t n,
                                             int64_t fixedp, bool structure_only) {
  const LayerIn l = layer_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  check_device(ws, "ws");
  check_device(gX, "gX");
  check_device(gZ, "gZ");
  const int nf = structure_only ? 0 : (int)(n - fixedp);
  TORCH_CHECK(gX.scalar_type() == poses.scalar_type() && gZ.scalar_type() == poses.scalar_type(),
              "cuda_ba.ba_layer_backward: gX / gZ must have the dtype of poses");
  TORCH_CHECK(gX.numel() == 6 * (int64_t)nf && gZ.numel() == l.M,
              "cuda_ba.ba_layer_backward: gX must be [n_free, 6] and gZ [M]");
  gX = gX.contiguous();
  gZ = gZ.contiguous();
  const auto mk = [&](int64_t r, int64_t c) {  // every row is written by the kernels
    return l.E == 0 ? torch::zeros({r, c}, poses.options()) : torch::empty({r, c}, poses.options());
  };
  auto gT = mk(l.E, 2), gW = mk(l.E, 2), gP = mk(l.N, 6), gK = mk(l.M, 3);
  if (l.E == 0) return {gT, gW, gP, gK};
  check_status(dpvo_ba_layer_backward(poses.data_ptr(), patches.data_ptr(), intrinsics.data_ptr(),
                                      gX.data_ptr(), gZ.data_ptr(), l.E, l.M, l.p, l.N, (int)n,
                                      (int)fixedp, structure_only ? 1 : 0, l.dtype, gT.data_ptr(),
                                      gW.data_ptr(), gP.data_ptr(), gK.data_ptr(), ws.data_ptr(),
                                      (size_t)ws.numel(), current_stream()),
               "cuda_ba.ba_layer_backward");
  return {gT, gW, gP, gK};
}

// The training step's reprojection and losses (train.hip): fp32 tensors, no
// host synchronisation in any call.
static torch::Tensor f32c(torch::Tensor t, const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, "cuda_ba: ", name, " must be float32");
  return t.contiguous();
}

struct TransformIn {
  int E, M, P, N;
};

static TransformIn transform_inputs(torch::Tensor& poses, torch::Tensor& patches,
                                    torch::Tensor& intrinsics, torch::Tensor& ii,
                                    torch::Tensor& jj, torch::Tensor& kk) {
  poses = f32c(poses, "poses");
  patches = f32c(patches, "patches");
  intrinsics = f32c(intrinsics, "intrinsics");
  TORCH_CHECK(poses.dim() >= 2 && poses.size(-1) == 7, "poses must be [.., N, 7]");
  TORCH_CHECK(patches.dim() >= 4 && patches.size(-3) == 3 && patches.size(-1) == patches.size(-2),
              "patches must be [.., M, 3, P, P]");
  ii = idx64(ii, "ii");
  jj = idx64(jj, "jj");
  kk = idx64(kk, "kk");
  TransformIn t;
  t.E = ii.numel();
  TORCH_CHECK(jj.numel() == t.E && kk.numel() == t.E, "ii, jj, kk must have equal length");
  t.P = patches.size(-1);
  t.N = poses.numel() / 7;
  t.M = patches.numel() / (3 * (int64_t)t.P * t.P);
  TORCH_CHECK(intrinsics.numel() == 4 * (int64_t)t.N, "intrinsics must be [.., N, 4]");
  return t;
}

// -> [coords [E, P, P, 2], valid [E, P, P]] (+ coords_corr [E, 2, P, P])
std::vector<torch::Tensor> transform_forward(torch::Tensor poses, torch::Tensor patches,
                                             torch::Tensor intrinsics, torch::Tensor ii,
                                             torch::Tensor jj, torch::Tensor kk, bool with_corr) {
  const TransformIn t = transform_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto coords = torch::empty({t.E, t.P, t.P, 2}, poses.options());
  auto valid = torch::empty({t.E, t.P, t.P}, poses.options());
  torch::Tensor corr;
  if (with_corr) corr = torch::empty({t.E, 2, t.P, t.P}, poses.options());
  check_status(dpvo_transform_forward(poses.data_ptr<float>(), patches.data_ptr<float>(),
                                      intrinsics.data_ptr<float>(), ii.data_ptr<int64_t>(),
                                      jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), t.E, t.P, t.N,
                                      t.M, coords.data_ptr<float>(), valid.data_ptr<float>(),
                                      with_corr ? corr.data_ptr<float>() : nullptr,
                                      current_stream()),
               "cuda_ba.transform_forward");
  if (with_corr) return {coords, valid, corr};
  return {coords, valid};
}

// -> [g_poses [N, 6] or undefined, g_patches [M, 3, P, P] or undefined]
std::vector<c10::optional<torch::Tensor>> transform_backward(
    torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics, torch::Tensor ii,
    torch::Tensor jj, torch::Tensor kk, torch::Tensor g_coords, bool want_poses,
    bool want_patches) {
  const TransformIn t = transform_inputs(poses, patches, intrinsics, ii, jj, kk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  g_coords = f32c(g_coords, "g_coords");
  TORCH_CHECK(g_coords.numel() == 2 * (int64_t)t.E * t.P * t.P, "g_coords must be [E, P, P, 2]");
  const auto mk = [&](std::vector<int64_t> s) {  // every row is written by the kernels
    return t.E == 0 ? torch::zeros(s, poses.options()) : torch::empty(s, poses.options());
  };
  c10::optional<torch::Tensor> gP, gK;
  if (want_poses) gP = mk({t.N, 6});
  if (want_patches) gK = mk({t.M, 3, t.P, t.P});
  const size_t wsb = dpvo_transform_workspace_bytes(t.E, t.P);
  auto ws = torch::empty({(int64_t)std::max<size_t>(wsb, 8)}, poses.options().dtype(torch::kUInt8));
  check_status(dpvo_transform_backward(poses.data_ptr<float>(), patches.data_ptr<float>(),
                                       intrinsics.data_ptr<float>(), ii.data_ptr<int64_t>(),
                                       jj.data_ptr<int64_t>(), kk.data_ptr<int64_t>(), t.E, t.P,
                                       t.N, t.M, g_coords.data_ptr<float>(),
                                       gP ? gP->data_ptr<float>() : nullptr,
                                       gK ? gK->data_ptr<float>() : nullptr, ws.data_ptr(), wsb,
                                       current_stream()),
               "cuda_ba.transform_backward");
  return {gP, gK};
}

// -> [loss [1], count [1] int32, emin [E], argmin [E] int32]
std::vector<torch::Tensor> flow_loss_forward(torch::Tensor coords, torch::Tensor coords_gt,
                                             torch::Tensor valid) {
  coords = f32c(coords, "coords");
  coords_gt = f32c(coords_gt, "coords_gt");
  valid = f32c(valid, "valid");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(coords.device());
  TORCH_CHECK(coords.dim() >= 4 && coords.size(-1) == 2 && coords.size(-2) == coords.size(-3),
              "coords must be [.., E, P, P, 2]");
  const int P = coords.size(-2);
  const int64_t E = coords.numel() / (2 * (int64_t)P * P);
  TORCH_CHECK(coords_gt.numel() == coords.numel() && valid.numel() == E,
              "coords_gt must match coords and valid must be [E]");
  const auto i32 = coords.options().dtype(torch::kInt32);
  auto loss = torch::zeros({1}, coords.options());
  auto count = torch::zeros({1}, i32);
  auto emin = torch::empty({E}, coords.options());
  auto amin = torch::empty({E}, i32);
  check_status(dpvo_flow_loss_forward(coords.data_ptr<float>(), coords_gt.data_ptr<float>(),
                                      valid.data_ptr<float>(), (int)E, P, loss.data_ptr<float>(),
                                      count.data_ptr<int32_t>(), emin.data_ptr<float>(),
                                      amin.data_ptr<int32_t>(), current_stream()),
               "cuda_ba.flow_loss_forward");
  return {loss, count, emin, amin};
}

torch::Tensor flow_loss_backward(torch::Tensor coords, torch::Tensor coords_gt, torch::Tensor valid,
                                 torch::Tensor count, torch::Tensor argmin, torch::Tensor g_loss) {
  coords = f32c(coords, "coords");
  coords_gt = f32c(coords_gt, "coords_gt");
  valid = f32c(valid, "valid");
  g_loss = f32c(g_loss, "g_loss");
  check_device(count, "count");
  check_device(argmin, "argmin");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(coords.device());
  const int P = coords.size(-2);
  const int64_t E = coords.numel() / (2 * (int64_t)P * P);
  TORCH_CHECK(count.scalar_type() == torch::kInt32 && argmin.scalar_type() == torch::kInt32 &&
                  count.numel() == 1 && argmin.numel() == E && g_loss.numel() == 1 &&
                  valid.numel() == E && coords_gt.numel() == coords.numel(),
              "cuda_ba.flow_loss_backward: buffers of another forward call");
  auto g = torch::empty_like(coords);
  check_status(dpvo_flow_loss_backward(coords.data_ptr<float>(), coords_gt.data_ptr<float>(),
                                       valid.data_ptr<float>(), count.data_ptr<int32_t>(),
                                       argmin.contiguous().data_ptr<int32_t>(),
                                       g_loss.data_ptr<float>(), (int)E, P, g.data_ptr<float>(),
                                       current_stream()),
               "cuda_ba.flow_loss_backward");
  return g;
}

// -> [out [3] = (mean tr, mean ro, s), tr [n (n - 1)], ro [n (n - 1)]]
std::vector<torch::Tensor> pose_loss_forward(torch::Tensor G, torch::Tensor Ps) {
  G = f32c(G, "G");
  Ps = f32c(Ps, "Ps");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(G.device());
  TORCH_CHECK(G.dim() >= 2 && G.size(-1) == 7 && Ps.numel() == G.numel(),
              "G and Ps must be [.., n, 7]");
  const int64_t n = G.numel() / 7;
  const int64_t np = n > 1 ? n * (n - 1) : 0;
  auto out = torch::zeros({3}, G.options());  // n < 2: zeros, nothing launched
  auto tr = torch::empty({np}, G.options()), ro = torch::empty({np}, G.options());
  check_status(dpvo_pose_loss_forward(G.data_ptr<float>(), Ps.data_ptr<float>(), (int)n,
                                      out.data_ptr<float>(), tr.data_ptr<float>(),
                                      ro.data_ptr<float>(), current_stream()),
               "cuda_ba.pose_loss_forward");
  return {out, tr, ro};
}

torch::Tensor pose_loss_backward(torch::Tensor G, torch::Tensor Ps, torch::Tensor g_out) {
  G = f32c(G, "G");
  Ps = f32c(Ps, "Ps");
  g_out = f32c(g_out, "g_out");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(G.device());
  TORCH_CHECK(G.size(-1) == 7 && Ps.numel() == G.numel() && g_out.numel() == 2,
              "G and Ps must be [.., n, 7], g_out [2]");
  const int64_t n = G.numel() / 7;
  auto gG = n < 2 ? torch::zeros({n, 6}, G.options()) : torch::empty({n, 6}, G.options());
  check_status(dpvo_pose_loss_backward(G.data_ptr<float>(), Ps.data_ptr<float>(), (int)n,
                                       g_out.data_ptr<float>(), gG.data_ptr<float>(),
                                       current_stream()),
               "cuda_ba.pose_loss_backward");
  return gG;
}

// PatchGraph.edges_loop (patchgraph.py:65-91) gated as dpvo.py:984-988
void edges_loop(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                torch::Tensor ix, int64_t M, torch::Tensor st, int64_t n_cap,
                c10::optional<torch::Tensor> last_global_ba, int64_t removal_window,
                int64_t max_edge_age, int64_t global_opt_freq, int64_t keyframe_index,
                double backend_thresh, int64_t max_num_edges, int64_t nms, torch::Tensor work,
                torch::Tensor out_kk, torch::Tensor out_jj, torch::Tensor out_n,
                c10::optional<torch::Tensor> errors) {
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  int32_t* err = (errors && errors->defined())
                     ? const_cast<int32_t*>(dev_scalar(*errors, "errors"))
                     : nullptr;
  TORCH_CHECK(work.scalar_type() == torch::kFloat32 &&
                  work.numel() >= (int64_t)dpvo_edges_loop_work_floats(),
              "work: float32[edges_loop_work_floats()]");
  TORCH_CHECK(M > 0 && patches.numel() % (M * 3 * patches.size(-1) * patches.size(-1)) == 0,
              "patches: [N * M, 3, P, P]");
  TORCH_CHECK(out_kk.numel() >= max_num_edges * M && out_jj.numel() >= max_num_edges * M,
              "out_kk / out_jj: max_num_edges x M");
  int32_t* lb = (last_global_ba && last_global_ba->defined())
                    ? const_cast<int32_t*>(dev_scalar(*last_global_ba, "last_global_ba"))
                    : nullptr;
  check_status(dpvo_edges_loop(poses.data_ptr<float>(), patches.data_ptr<float>(),
                               intrinsics.data_ptr<float>(), idx64(ix, "ix").data_ptr<int64_t>(),
                               (int)patches.size(-1), (int)M, dev_scalar(st, "st"), (int)n_cap, lb,
                               (int)removal_window, (int)max_edge_age, (int)global_opt_freq,
                               (int)keyframe_index, (float)backend_thresh, (int)max_num_edges,
                               (int)nms, work.data_ptr<float>(), out_kk.data_ptr<int64_t>(),
                               out_jj.data_ptr<int64_t>(),
                               const_cast<int32_t*>(dev_scalar(out_n, "out_n")), err,
                               current_stream()),
               "cuda_ba.edges_loop");
}

// The head of DPVO.__call__ (dpvo.py:931-965): tstamps / intrinsics / pose /
// patches of frame row n, in place, one launch.  n / counter: the host value,
// or the int32 device scalar when given.
void frame_init(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                torch::Tensor tstamps, torch::Tensor times, torch::Tensor new_patches,
                torch::Tensor new_intrinsics, int64_t M, int64_t n,
                c10::optional<torch::Tensor> n_dev, int64_t counter,
                c10::optional<torch::Tensor> counter_dev, int64_t motion_model, double damping,
                double res, bool median) {
  check_device(poses, "poses");
  check_device(patches, "patches");
  check_device(intrinsics, "intrinsics");
  check_device(tstamps, "tstamps");
  check_device(times, "times");
  TORCH_CHECK(poses.scalar_type() == torch::kFloat32 && patches.scalar_type() == torch::kFloat32 &&
                  intrinsics.scalar_type() == torch::kFloat32,
              "poses / patches / intrinsics must be float32");
  TORCH_CHECK(tstamps.scalar_type() == torch::kInt64, "tstamps must be int64 (long)");
  TORCH_CHECK(times.scalar_type() == torch::kFloat64, "times must be float64");
  TORCH_CHECK(poses.is_contiguous() && patches.is_contiguous() && intrinsics.is_contiguous() &&
                  tstamps.is_contiguous() && times.is_contiguous(),
              "the per-frame buffers and times must be contiguous (written / read in place)");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) > 0, "poses: [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(patches.dim() == 4 && patches.size(1) == 3 && patches.size(2) == patches.size(3),
              "patches: [N * M, 3, P, P]");
  const int64_t P = patches.size(-1);
  TORCH_CHECK(M > 0 && patches.size(0) == N * M, "patches: [N * M, 3, P, P] with N = ", N,
              " frames of M = ", M);
  TORCH_CHECK(intrinsics.numel() == 4 * N, "intrinsics: [N, 4]");
  TORCH_CHECK(tstamps.numel() >= N, "tstamps: [N]");
  TORCH_CHECK(times.dim() == 1 && times.numel() > 0 && times.numel() < (1LL << 31), "times: [cap]");
  new_patches = f32_contig(new_patches, "new_patches");
  new_intrinsics = f32_contig(new_intrinsics, "new_intrinsics");
  TORCH_CHECK(new_patches.numel() == M * 3 * P * P, "new_patches: [M, 3, P, P]");
  TORCH_CHECK(new_intrinsics.numel() == 4, "new_intrinsics: [4]");
  TORCH_CHECK(N * M * 3 * P * P < (1LL << 40) && N < (1LL << 31) && M < (1LL << 31), "too large");
  const int32_t* nd = (n_dev && n_dev->defined()) ? dev_scalar(*n_dev, "n") : nullptr;
  const int32_t* cd =
      (counter_dev && counter_dev->defined()) ? dev_scalar(*counter_dev, "counter") : nullptr;
  TORCH_CHECK(nd || (n >= 0 && n < N), "frame_init: n = ", n, " outside [0, ", N, ")");
  TORCH_CHECK(cd || (counter >= 0 && counter < times.numel()), "frame_init: counter = ", counter,
              " outside times [0, ", times.numel(), ")");
  check_status(dpvo_frame_init(poses.data_ptr<float>(), patches.data_ptr<float>(),
                               intrinsics.data_ptr<float>(), tstamps.data_ptr<int64_t>(),
                               times.data_ptr<double>(), (int)times.numel(),
                               new_patches.data_ptr<float>(), new_intrinsics.data_ptr<float>(),
                               (int)N, (int)M, (int)P, nd ? 0 : (int)n, nd, cd ? 0 : (int)counter,
                               cd, (int)motion_model, damping, res, median ? 1 : 0,
                               current_stream()),
               "cuda_ba.frame_init");
}

// DPVO.terminate's interpolation (dpvo.py:385-417) -> [traj [counter, 7],
// root [counter] int64, info int32[2] = {unresolved frames, ignored records}]
std::vector<torch::Tensor> trajectory(torch::Tensor poses, torch::Tensor tstamps, int64_t n,
                                      c10::optional<torch::Tensor> n_dev, torch::Tensor delta_log,
                                      torch::Tensor delta_pairs, torch::Tensor delta_count,
                                      int64_t counter, bool inverse) {
  poses = f32_contig(poses, "poses");
  tstamps = idx64(tstamps, "tstamps");
  delta_log = f32_contig(delta_log, "delta log");
  delta_pairs = idx64(delta_pairs, "delta pairs");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) > 0, "poses: [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(tstamps.numel() >= N && N < (1LL << 31), "tstamps: [N]");
  TORCH_CHECK(delta_log.numel() % 7 == 0, "delta log: [cap, 7]");
  const int64_t cap = delta_log.numel() / 7;
  TORCH_CHECK(delta_pairs.numel() == 2 * cap && cap < (1LL << 31), "delta pairs: [cap, 2]");
  TORCH_CHECK(counter >= 0 && counter < (1LL << 30), "trajectory: counter = ", counter);
  const int32_t* nd = (n_dev && n_dev->defined()) ? dev_scalar(*n_dev, "n") : nullptr;
  TORCH_CHECK(nd || (n >= 0 && n <= N), "trajectory: n = ", n, " outside [0, ", N, "]");
  const int32_t* dc = dev_scalar(delta_count, "delta count");
  auto traj = torch::empty({counter, 7}, poses.options());
  auto root = torch::empty({counter}, tstamps.options());
  auto info = torch::zeros({2}, poses.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_trajectory_workspace_bytes((int)counter);
  auto ws = torch::empty({(int64_t)(wsb / sizeof(double))}, poses.options().dtype(torch::kFloat64));
  check_status(dpvo_trajectory(poses.data_ptr<float>(), tstamps.data_ptr<int64_t>(), (int)N,
                               nd ? 0 : (int)n, nd, delta_log.data_ptr<float>(),
                               delta_pairs.data_ptr<int64_t>(), dc, (int)cap, (int)counter,
                               inverse ? 1 : 0, traj.data_ptr<float>(), root.data_ptr<int64_t>(),
                               info.data_ptr<int32_t>(), ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.trajectory");
  return {traj, root, info};
}

// ---- stream.hip / evaluate.hip: frame in, score out ------------------------------
// Undistort, halve and crop a decoded frame (dpvo/stream.py:24-39, :75-83), one
// launch -> [image uint8 [3, H, W], intrinsics float32 [4]].  raw: uint8
// [H0, W0, 3] or [H0, W0]; calib: the 4, 8 or 9 numbers of calib/*.txt.
std::vector<torch::Tensor> frame_prepare(torch::Tensor raw, std::vector<double> calib,
                                         double scale, bool swap_rb,
                                         c10::optional<torch::Tensor> out) {
  check_device(raw, "raw");
  TORCH_CHECK(raw.scalar_type() == torch::kUInt8, "frame_prepare: raw must be uint8, got ",
              raw.scalar_type());
  TORCH_CHECK(raw.dim() == 2 || (raw.dim() == 3 && raw.size(2) == 3),
              "frame_prepare: raw must be [H0, W0, 3] or [H0, W0]");
  TORCH_CHECK(raw.size(0) > 0 && raw.size(1) > 0 && raw.size(0) < (1LL << 31) &&
                  raw.size(1) < (1LL << 31),
              "frame_prepare: empty or oversized frame");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(raw.device());
  raw = raw.contiguous();
  const int H0 = (int)raw.size(0), W0 = (int)raw.size(1);
  int H = 0, W = 0;
  // the count is checked first here only to give dpvo_frame_prepare's own answer for it
  if (calib.size() == 4 || calib.size() == 8 || calib.size() == 9)
    check_status(dpvo_frame_prepare_shape(H0, W0, scale, &H, &W), "cuda_ba.frame_prepare");
  else
    check_status(DPVO_ERR_UNSUPPORTED, "cuda_ba.frame_prepare (4, 8 or 9 calibration numbers)");
  torch::Tensor image;
  if (out && out->defined()) {
    image = *out;
    check_device(image, "out");
    TORCH_CHECK(image.scalar_type() == torch::kUInt8 && image.is_contiguous() &&
                    image.dim() == 3 && image.size(0) == 3 && image.size(1) == H &&
                    image.size(2) == W && image.device() == raw.device(),
                "frame_prepare: out must be a contiguous uint8 [3, ", H, ", ", W,
                "] tensor on raw's device");
  } else {
    image = torch::empty({3, H, W}, raw.options());
  }
  auto intr = torch::empty({4}, raw.options().dtype(torch::kFloat32));
  check_status(dpvo_frame_prepare(raw.data_ptr<uint8_t>(), H0, W0, raw.dim() == 2 ? 1 : 3,
                                  calib.data(), (int)calib.size(), scale, swap_rb ? 1 : 0,
                                  image.data_ptr<uint8_t>(), intr.data_ptr<float>(),
                                  current_stream()),
               "cuda_ba.frame_prepare");
  return {image, intr};
}

// ATE of an estimated trajectory against a reference one (evaluate_euroc.py:109-119
// through evo), one launch -> [stats f64[8], model f64[13], pairs i32[min(n, m), 2],
// status i32[1]]
std::vector<torch::Tensor> trajectory_ate(torch::Tensor est_xyz, torch::Tensor est_t,
                                          torch::Tensor ref_xyz, torch::Tensor ref_t,
                                          double max_diff, bool align) {
  check_device(est_xyz, "est_xyz");
  check_device(est_t, "est_t");
  check_device(ref_xyz, "ref_xyz");
  check_device(ref_t, "ref_t");
  TORCH_CHECK(est_xyz.scalar_type() == torch::kFloat32 || est_xyz.scalar_type() == torch::kFloat64,
              "trajectory_ate: est_xyz must be float32 or float64");
  TORCH_CHECK(est_t.scalar_type() == torch::kFloat64 && ref_xyz.scalar_type() == torch::kFloat64 &&
                  ref_t.scalar_type() == torch::kFloat64,
              "trajectory_ate: est_t, ref_xyz and ref_t must be float64");
  TORCH_CHECK(est_xyz.dim() == 2 && est_xyz.size(1) == 3 && est_t.dim() == 1 &&
                  est_t.size(0) == est_xyz.size(0),
              "trajectory_ate: est_xyz [n, 3], est_t [n]");
  TORCH_CHECK(ref_xyz.dim() == 2 && ref_xyz.size(1) == 3 && ref_t.dim() == 1 &&
                  ref_t.size(0) == ref_xyz.size(0),
              "trajectory_ate: ref_xyz [m, 3], ref_t [m]");
  TORCH_CHECK(est_xyz.device() == est_t.device() && est_xyz.device() == ref_xyz.device() &&
                  est_xyz.device() == ref_t.device(),
              "trajectory_ate: tensors on different devices");
  const int64_t n = est_xyz.size(0), m = ref_xyz.size(0);
  TORCH_CHECK(n >= 1 && m >= 1, "trajectory_ate: empty trajectory");
  TORCH_CHECK(n < (1LL << 31) && m < (1LL << 31), "trajectory_ate: trajectory too long");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(est_xyz.device());
  est_xyz = est_xyz.contiguous();
  est_t = est_t.contiguous();
  ref_xyz = ref_xyz.contiguous();
  ref_t = ref_t.contiguous();
  const auto f64 = ref_xyz.options();
  const auto i32 = ref_xyz.options().dtype(torch::kInt32);
  auto stats = torch::empty({8}, f64);
  auto model = torch::empty({13}, f64);
  auto pairs = torch::empty({std::min(n, m), 2}, i32);
  auto status = torch::empty({1}, i32);
  const size_t wsb = dpvo_trajectory_ate_workspace_bytes((int)n, (int)m);
  auto ws = torch::empty({(int64_t)(wsb / sizeof(double))}, f64);
  check_status(dpvo_trajectory_ate(est_xyz.data_ptr(), dtype_code(est_xyz),
                                   est_t.data_ptr<double>(), (int)n, ref_xyz.data_ptr<double>(),
                                   ref_t.data_ptr<double>(), (int)m, max_diff, align ? 1 : 0,
                                   stats.data_ptr<double>(), model.data_ptr<double>(),
                                   pairs.data_ptr<int32_t>(), status.data_ptr<int32_t>(),
                                   ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.trajectory_ate");
  return {stats, model, pairs, status};
}

// ---- dataset.hip: the device half of the training data readers -------------------
static torch::Tensor data_f32(const torch::Tensor& t, const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32, got ", t.scalar_type());
  return t.contiguous();
}

// rgbd_utils.compute_distance_matrix_flow: poses [N, 7] (world-from-camera), disps
// [N, h, w], intrinsics [N, 4] -> D float32 [N, N], one launch
torch::Tensor frame_flow_distance(torch::Tensor poses, torch::Tensor disps,
                                  torch::Tensor intrinsics) {
  poses = data_f32(poses, "poses");
  disps = data_f32(disps, "disps");
  intrinsics = data_f32(intrinsics, "intrinsics");
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) >= 1,
              "frame_flow_distance: poses must be [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(disps.dim() == 3 && disps.size(0) == N && disps.size(1) >= 1 && disps.size(2) >= 1,
              "frame_flow_distance: disps must be [N, h, w]");
  TORCH_CHECK(intrinsics.dim() == 2 && intrinsics.size(0) == N && intrinsics.size(1) == 4,
              "frame_flow_distance: intrinsics must be [N, 4]");
  TORCH_CHECK(poses.device() == disps.device() && poses.device() == intrinsics.device(),
              "frame_flow_distance: tensors on different devices");
  TORCH_CHECK(N < (1LL << 31) && disps.size(1) < (1LL << 31) && disps.size(2) < (1LL << 31),
              "frame_flow_distance: too large");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto D = torch::empty({N, N}, poses.options());
  check_status(dpvo_frame_flow_distance(poses.data_ptr<float>(), disps.data_ptr<float>(),
                                        intrinsics.data_ptr<float>(), (int)N, (int)disps.size(1),
                                        (int)disps.size(2), D.data_ptr<float>(), current_stream()),
               "cuda_ba.frame_flow_distance");
  return D;
}

// base.py:77-80 as CSR -> [rowptr i32 [N + 1], col i32 [nnz], dist f32 [nnz]].
// One host read (nnz) sizes the outputs: a build step, not a per-frame call.
std::vector<torch::Tensor> frame_graph(torch::Tensor D, double f, double max_flow) {
  D = data_f32(D, "D");
  TORCH_CHECK(D.dim() == 2 && D.size(0) == D.size(1) && D.size(0) >= 1 && D.size(0) < (1LL << 31),
              "frame_graph: D must be [N, N]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(D.device());
  const int N = (int)D.size(0);
  const auto i32 = D.options().dtype(torch::kInt32);
  auto rowptr = torch::empty({(int64_t)N + 1}, i32);
  check_status(dpvo_frame_graph_count(D.data_ptr<float>(), N, (float)f, (float)max_flow,
                                      rowptr.data_ptr<int32_t>(), current_stream()),
               "cuda_ba.frame_graph (count)");
  const int nnz = rowptr[N].item<int32_t>();
  auto col = torch::empty({(int64_t)nnz}, i32);
  auto dist = torch::empty({(int64_t)nnz}, D.options());
  check_status(dpvo_frame_graph_fill(D.data_ptr<float>(), N, (float)f, (float)max_flow,
                                     rowptr.data_ptr<int32_t>(), nnz ? col.data_ptr<int32_t>() : nullptr,
                                     nnz ? dist.data_ptr<float>() : nullptr, nnz, current_stream()),
               "cuda_ba.frame_graph (fill)");
  return {rowptr, col, dist};
}

// augmentation.py with the random draws given -> [images [N, 3, ch, cw], disps
// [N, ch, cw], intrinsics [N, 4]]
std::vector<torch::Tensor> rgbd_augment(torch::Tensor images, torch::Tensor disps,
                                        torch::Tensor intrinsics, int64_t crop_h, int64_t crop_w,
                                        bool do_color, std::vector<int64_t> order, double brightness,
                                        double contrast, double saturation, double hue, bool gray,
                                        bool invert, double scale, bool swap_rb) {
  images = data_f32(images, "images");
  disps = data_f32(disps, "disps");
  intrinsics = data_f32(intrinsics, "intrinsics");
  TORCH_CHECK(images.dim() == 4 && images.size(1) == 3 && images.size(0) >= 1,
              "rgbd_augment: images must be [N, 3, H, W]");
  const int64_t N = images.size(0), H = images.size(2), W = images.size(3);
  TORCH_CHECK(disps.dim() == 3 && disps.size(0) == N && disps.size(1) == H && disps.size(2) == W,
              "rgbd_augment: disps must be [N, H, W]");
  TORCH_CHECK(intrinsics.dim() == 2 && intrinsics.size(0) == N && intrinsics.size(1) == 4,
              "rgbd_augment: intrinsics must be [N, 4]");
  TORCH_CHECK(images.device() == disps.device() && images.device() == intrinsics.device(),
              "rgbd_augment: tensors on different devices");
  TORCH_CHECK(order.size() == 4, "rgbd_augment: order must hold four operations");
  TORCH_CHECK(N < (1LL << 31) && H >= 1 && W >= 1 && H < (1LL << 31) && W < (1LL << 31) &&
                  crop_h >= 1 && crop_w >= 1 && crop_h < (1LL << 31) && crop_w < (1LL << 31),
              "rgbd_augment: empty or oversized");
  dpvo_augment_params p;
  p.do_color = do_color ? 1 : 0;
  for (int k = 0; k < 4; k++)
    p.order[k] = (order[k] >= 0 && order[k] <= 3) ? (int)order[k] : -1;
  p.brightness = (float)brightness;
  p.contrast = (float)contrast;
  p.saturation = (float)saturation;
  p.hue = (float)hue;
  p.gray = gray ? 1 : 0;
  p.invert = invert ? 1 : 0;
  p.scale = scale;
  p.swap_rb = swap_rb ? 1 : 0;
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(images.device());
  auto images_out = torch::empty({N, 3, crop_h, crop_w}, images.options());
  auto disps_out = torch::empty({N, crop_h, crop_w}, images.options());
  auto intr_out = torch::empty({N, 4}, images.options());
  const size_t wsb = dpvo_rgbd_augment_workspace_bytes((int)N, (int)H, (int)W);
  // the scratch image is touched only by colour followed by resampling
  const size_t need = (do_color && scale != 1.0) ? wsb : 8 * 256;
  auto ws = torch::empty({(int64_t)((need + 7) / sizeof(double))},
                         images.options().dtype(torch::kFloat64));
  check_status(dpvo_rgbd_augment(images.data_ptr<float>(), disps.data_ptr<float>(),
                                 intrinsics.data_ptr<float>(), (int)N, (int)H, (int)W, (int)crop_h,
                                 (int)crop_w, &p, images_out.data_ptr<float>(),
                                 disps_out.data_ptr<float>(), intr_out.data_ptr<float>(),
                                 ws.data_ptr(), need, current_stream()),
               "cuda_ba.rgbd_augment");
  return {images_out, disps_out, intr_out};
}

// base.py:171-173 -> [disps / s, poses with the translation times s, (s, lo, hi) f32 [3]]
std::vector<torch::Tensor> normalize_depth(torch::Tensor disps, torch::Tensor poses) {
  disps = data_f32(disps, "disps");
  poses = data_f32(poses, "poses");
  TORCH_CHECK(disps.numel() >= 1 && disps.numel() < (1LL << 31), "normalize_depth: disps is empty or too large");
  TORCH_CHECK(poses.dim() >= 1 && poses.size(-1) == 7 && poses.numel() >= 7 &&
                  poses.numel() < (1LL << 31),
              "normalize_depth: poses must be [.., 7]");
  TORCH_CHECK(disps.device() == poses.device(), "normalize_depth: tensors on different devices");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(disps.device());
  auto disps_out = torch::empty_like(disps);
  auto poses_out = torch::empty_like(poses);
  auto s = torch::empty({3}, disps.options());
  check_status(dpvo_normalize_depth(disps.data_ptr<float>(), (int)disps.numel(),
                                    poses.data_ptr<float>(), (int)(poses.numel() / 7),
                                    disps_out.data_ptr<float>(), poses_out.data_ptr<float>(),
                                    s.data_ptr<float>(), current_stream()),
               "cuda_ba.normalize_depth");
  return {disps_out, poses_out, s};
}

// ---- tracker.hip: the small kernels of the tracker's frame path ----------------
static int ring_dtype(const torch::Tensor& t, const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 || t.scalar_type() == torch::kFloat16, name,
              " must be float32 or float16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous (written / read in place)");
  return dtype_code(t);
}

// Patchifier's gathers and DPVO.__call__'s ring writes of frame n, one launch.
void frame_sample(torch::Tensor fmap, torch::Tensor imap, torch::Tensor image,
                  torch::Tensor coords, torch::Tensor gmap_ring, torch::Tensor imap_ring,
                  torch::Tensor patches_out, torch::Tensor colors, int64_t res, int64_t n,
                  c10::optional<torch::Tensor> n_dev) {
  fmap = f32_contig(fmap, "fmap");
  imap = f32_contig(imap, "imap");
  image = f32_contig(image, "image");
  coords = f32_contig(coords, "coords");
  const int gd = ring_dtype(gmap_ring, "gmap ring");
  TORCH_CHECK(ring_dtype(imap_ring, "imap ring") == gd, "the two rings must share one dtype");
  check_device(patches_out, "patches_out");
  check_device(colors, "colors");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(fmap.device());
  TORCH_CHECK(fmap.dim() == 3 && imap.dim() == 3 && image.dim() == 3 && image.size(0) == 3,
              "fmap [C, h, w], imap [DIM, h, w], image [3, H, W]");
  const int64_t C = fmap.size(0), h = fmap.size(1), w = fmap.size(2), DIM = imap.size(0);
  TORCH_CHECK(imap.size(1) == h && imap.size(2) == w, "fmap and imap differ in size");
  TORCH_CHECK(coords.dim() == 2 && coords.size(1) == 2 && coords.size(0) > 0, "coords: [M, 2]");
  const int64_t M = coords.size(0);
  TORCH_CHECK(gmap_ring.dim() >= 3 && gmap_ring.size(-1) == gmap_ring.size(-2), "gmap ring: [.., C, P, P]");
  const int64_t P = gmap_ring.size(-1);
  TORCH_CHECK(gmap_ring.numel() % (M * C * P * P) == 0 && gmap_ring.numel() > 0,
              "gmap ring: [pmem, M, C, P, P]");
  const int64_t pmem = gmap_ring.numel() / (M * C * P * P);
  TORCH_CHECK(imap_ring.numel() == pmem * M * DIM, "imap ring: [pmem, M, DIM]");
  TORCH_CHECK(patches_out.scalar_type() == torch::kFloat32 && patches_out.is_contiguous() &&
                  patches_out.numel() == M * 3 * P * P,
              "patches_out: contiguous float32 [M, 3, P, P]");
  TORCH_CHECK(colors.scalar_type() == torch::kUInt8 && colors.is_contiguous() &&
                  colors.numel() % (3 * M) == 0 && colors.numel() > 0,
              "colors: contiguous uint8 [N, M, 3]");
  const int64_t N = colors.numel() / (3 * M);
  TORCH_CHECK(N < (1LL << 31) && M < (1LL << 31) && pmem < (1LL << 31), "too large");
  TORCH_CHECK(res > 0 && image.size(1) >= res * h && image.size(2) >= res * w,
              "image must cover res x the feature map");
  const int32_t* nd = (n_dev && n_dev->defined()) ? dev_scalar(*n_dev, "n") : nullptr;
  TORCH_CHECK(nd || (n >= 0 && n < N), "frame_sample: n = ", n, " outside [0, ", N, ")");
  check_status(dpvo_frame_sample(fmap.data_ptr<float>(), imap.data_ptr<float>(),
                                 image.data_ptr<float>(), coords.data_ptr<float>(),
                                 gmap_ring.data_ptr(), imap_ring.data_ptr(), gd,
                                 patches_out.data_ptr<float>(), colors.data_ptr<uint8_t>(), (int)h,
                                 (int)w, (int)image.size(1), (int)image.size(2), (int)C, (int)DIM,
                                 (int)M, (int)P, (int)res, (int)pmem, (int)N, nd ? 0 : (int)n, nd,
                                 current_stream()),
               "cuda_ba.frame_sample");
}

// torch.quantile(delta.norm(dim=-1).float(), 0.5) -> fp32 device scalar
torch::Tensor probe_median(torch::Tensor delta) {
  check_device(delta, "delta");
  TORCH_CHECK(delta.scalar_type() == torch::kFloat32 || delta.scalar_type() == torch::kFloat16,
              "delta must be float32 or float16");
  delta = delta.contiguous();
  TORCH_CHECK(delta.numel() > 0 && delta.size(-1) == 2, "delta: [M, 2]");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(delta.device());
  const int64_t M = delta.numel() / 2;
  TORCH_CHECK(M < (1LL << 31), "too large");
  auto out = torch::empty({}, delta.options().dtype(torch::kFloat32));
  check_status(dpvo_probe_median(delta.data_ptr(), dtype_code(delta), (int)M,
                                 out.data_ptr<float>(), current_stream()),
               "cuda_ba.probe_median");
  return out;
}

// dpvo.py:805-810 into the patch graph's target / weight rows [0, E)
void update_targets(torch::Tensor coords, torch::Tensor delta, torch::Tensor w,
                    torch::Tensor target, torch::Tensor weight, int64_t E,
                    c10::optional<torch::Tensor> E_dev) {
  coords = f32_contig(coords, "coords");
  check_device(delta, "delta");
  check_device(w, "w");
  check_device(target, "target");
  check_device(weight, "weight");
  TORCH_CHECK((delta.scalar_type() == torch::kFloat32 || delta.scalar_type() == torch::kFloat16) &&
                  w.scalar_type() == delta.scalar_type(),
              "delta / w must both be float32 or both float16");
  delta = delta.contiguous();
  w = w.contiguous();
  TORCH_CHECK(target.scalar_type() == torch::kFloat32 && weight.scalar_type() == torch::kFloat32 &&
                  target.is_contiguous() && weight.is_contiguous(),
              "target / weight must be contiguous float32 (written in place)");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(coords.device());
  TORCH_CHECK(coords.dim() >= 3 && coords.size(-1) == coords.size(-2), "coords: [.., E, 2, P, P]");
  const int64_t P = coords.size(-1);
  const int64_t cap = std::min({coords.numel() / (2 * P * P), delta.numel() / 2, w.numel() / 2,
                                target.numel() / 2, weight.numel() / 2});
  TORCH_CHECK(cap < (1LL << 30), "too large");
  const int32_t* ed = (E_dev && E_dev->defined()) ? dev_scalar(*E_dev, "E") : nullptr;
  TORCH_CHECK(ed || (E >= 0 && E <= cap), "update_targets: E = ", E, " outside [0, ", cap, "]");
  check_status(dpvo_update_targets(coords.data_ptr<float>(), delta.data_ptr(), w.data_ptr(),
                                   dtype_code(delta), target.data_ptr<float>(),
                                   weight.data_ptr<float>(), (int)P, ed ? 0 : (int)E, ed, (int)cap,
                                   current_stream()),
               "cuda_ba.update_targets");
}

// dpvo.py:834-836, the centre pixel only, into points rows [0, m)
void map_points(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                torch::Tensor ix, torch::Tensor points, int64_t m,
                c10::optional<torch::Tensor> m_dev) {
  poses = f32_contig(poses, "poses");
  patches = f32_contig(patches, "patches");
  intrinsics = f32_contig(intrinsics, "intrinsics");
  ix = idx64(ix, "ix");
  check_device(points, "points");
  TORCH_CHECK(points.scalar_type() == torch::kFloat32 && points.is_contiguous() &&
                  points.dim() == 2 && points.size(1) == 3,
              "points: contiguous float32 [*, 3] (written in place)");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) > 0, "poses: [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(intrinsics.numel() == 4 * N, "intrinsics: [N, 4]");
  TORCH_CHECK(patches.dim() == 4 && patches.size(1) == 3 && patches.size(2) == patches.size(3),
              "patches: [*, 3, P, P]");
  const int64_t cap = std::min({patches.size(0), points.size(0), ix.numel()});
  TORCH_CHECK(cap < (1LL << 31) && N < (1LL << 31), "too large");
  const int32_t* md = (m_dev && m_dev->defined()) ? dev_scalar(*m_dev, "m") : nullptr;
  TORCH_CHECK(md || (m >= 0 && m <= cap), "map_points: m = ", m, " outside [0, ", cap, "]");
  check_status(dpvo_map_points(poses.data_ptr<float>(), patches.data_ptr<float>(),
                               intrinsics.data_ptr<float>(), ix.data_ptr<int64_t>(),
                               points.data_ptr<float>(), (int)N, (int)patches.size(-1),
                               md ? 0 : (int)m, md, (int)cap, current_stream()),
               "cuda_ba.map_points");
}

// ---- match.hip / triangulate.hip: the front half of the long-term loop closure ---
// -> [partner0 [N0], partner1 [N1], matches [min(N0, N1), 2] (int64), dist2, count (int32 [1])]
std::vector<torch::Tensor> match_descriptors(torch::Tensor desc0, torch::Tensor desc1,
                                             double ratio, double max_dist, int64_t n0,
                                             c10::optional<torch::Tensor> n0_dev, int64_t n1,
                                             c10::optional<torch::Tensor> n1_dev) {
  check_device(desc0, "desc0");
  check_device(desc1, "desc1");
  TORCH_CHECK((desc0.scalar_type() == torch::kFloat32 || desc0.scalar_type() == torch::kFloat16) &&
                  desc1.scalar_type() == desc0.scalar_type(),
              "match_descriptors: desc0 / desc1 must both be float32 or both float16");
  TORCH_CHECK(desc0.dim() == 2 && desc1.dim() == 2 && desc0.size(1) == desc1.size(1),
              "match_descriptors: desc0 [N0, D], desc1 [N1, D]");
  TORCH_CHECK(desc0.device() == desc1.device(), "match_descriptors: tensors on different devices");
  const int64_t N0 = desc0.size(0), N1 = desc1.size(0), D = desc0.size(1);
  TORCH_CHECK(N0 >= 1 && N1 >= 1 && N0 <= 4096 && N1 <= 4096,
              "match_descriptors: 1 <= N0, N1 <= 4096, got ", N0, " and ", N1);
  TORCH_CHECK(D >= 4 && D <= 256 && D % 4 == 0,
              "match_descriptors: D must be a multiple of 4 in [4, 256], got ", D);
  TORCH_CHECK(ratio >= 0.0 && max_dist >= 0.0, "match_descriptors: ratio and max_dist must be >= 0");
  // rows are read four elements at a time: a view at an odd offset is copied
  auto aligned = [](torch::Tensor t) {
    t = t.contiguous();
    const uintptr_t al = t.scalar_type() == torch::kFloat16 ? 7 : 15;
    return ((uintptr_t)t.data_ptr() & al) ? t.clone() : t;
  };
  desc0 = aligned(desc0);
  desc1 = aligned(desc1);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(desc0.device());
  const int32_t* d0 = (n0_dev && n0_dev->defined()) ? dev_scalar(*n0_dev, "n0") : nullptr;
  const int32_t* d1 = (n1_dev && n1_dev->defined()) ? dev_scalar(*n1_dev, "n1") : nullptr;
  // a host limit is clamped to the rows present, as a device one is
  n0 = std::min(std::max(n0, (int64_t)0), N0);
  n1 = std::min(std::max(n1, (int64_t)0), N1);
  const auto i64 = desc0.options().dtype(torch::kInt64);
  const int64_t K = std::min(N0, N1);
  auto partner0 = torch::empty({N0}, i64), partner1 = torch::empty({N1}, i64);
  auto matches = torch::empty({K, 2}, i64);
  auto dist2 = torch::empty({K}, desc0.options().dtype(torch::kFloat32));
  auto count = torch::empty({1}, desc0.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_match_workspace_bytes((int)N0, (int)N1);
  auto ws = torch::empty({(int64_t)wsb}, desc0.options().dtype(torch::kUInt8));
  const float r2 = (float)(ratio * ratio), md2 = (float)(max_dist * max_dist);
  check_status(dpvo_match_descriptors(desc0.data_ptr(), desc1.data_ptr(), dtype_code(desc0),
                                      (int)N0, (int)N1, (int)D, d0 ? 0 : (int)n0, d0,
                                      d1 ? 0 : (int)n1, d1, r2, md2, partner0.data_ptr<int64_t>(),
                                      partner1.data_ptr<int64_t>(), matches.data_ptr<int64_t>(),
                                      dist2.data_ptr<float>(), count.data_ptr<int32_t>(),
                                      ws.data_ptr(), wsb, current_stream()),
               "cuda_ba.match_descriptors");
  return {partner0, partner1, matches, dist2, count};
}

// -> [points [N1, 3], disp [N1], keep [N1] (bool), sel [N1] (int64), count (int32 [1])]
std::vector<torch::Tensor> triangulate_tracks(torch::Tensor poses, torch::Tensor intrinsics,
                                              torch::Tensor disps, torch::Tensor kps0,
                                              torch::Tensor kps1, torch::Tensor kps2,
                                              torch::Tensor m10, torch::Tensor m12,
                                              double max_depth, double max_residual,
                                              int64_t iterations, double lmbda) {
  poses = f32_contig(poses, "poses");
  intrinsics = f32_contig(intrinsics, "intrinsics");
  kps0 = f32_contig(kps0, "kps0");
  kps1 = f32_contig(kps1, "kps1");
  kps2 = f32_contig(kps2, "kps2");
  m10 = idx64(m10, "m10");
  m12 = idx64(m12, "m12");
  check_device(disps, "disps");
  TORCH_CHECK(disps.scalar_type() == torch::kFloat32 && disps.dim() == 1 && disps.numel() >= 1,
              "triangulate_tracks: disps must be float32 [M]");
  if (disps.stride(0) < 1) disps = disps.contiguous();
  TORCH_CHECK(poses.numel() == 21 && intrinsics.numel() == 12,
              "triangulate_tracks: poses [3, 7] and intrinsics [3, 4] of frames i-1, i, i+1");
  for (const auto* k : {&kps0, &kps1, &kps2})
    TORCH_CHECK(k->dim() == 2 && k->size(1) == 2 && k->size(0) >= 1,
                "triangulate_tracks: keypoints must be [N, 2] with N >= 1");
  const int64_t M = disps.numel(), N0 = kps0.size(0), N1 = kps1.size(0), N2 = kps2.size(0);
  TORCH_CHECK(m10.numel() == N1 && m12.numel() == N1, "triangulate_tracks: m10 / m12 must be [N1]");
  TORCH_CHECK(M <= 1024, "triangulate_tracks: M <= 1024, got ", M);
  TORCH_CHECK(N1 <= 4096 && N0 < (1LL << 31) && N2 < (1LL << 31) && disps.stride(0) < (1LL << 31),
              "triangulate_tracks: N1 <= 4096, got ", N1);
  TORCH_CHECK(iterations >= 0 && lmbda >= 0.0, "triangulate_tracks: iterations, lmbda >= 0");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(poses.device());
  auto points = torch::empty({N1, 3}, poses.options());
  auto disp = torch::empty({N1}, poses.options());
  auto keep = torch::empty({N1}, poses.options().dtype(torch::kBool));
  auto sel = torch::empty({N1}, poses.options().dtype(torch::kInt64));
  auto count = torch::empty({1}, poses.options().dtype(torch::kInt32));
  check_status(dpvo_triangulate_tracks(
                   poses.data_ptr<float>(), intrinsics.data_ptr<float>(), disps.data_ptr<float>(),
                   (int)disps.stride(0), (int)M, kps0.data_ptr<float>(), (int)N0,
                   kps1.data_ptr<float>(), (int)N1, kps2.data_ptr<float>(), (int)N2,
                   m10.data_ptr<int64_t>(), m12.data_ptr<int64_t>(), (float)max_depth,
                   (float)max_residual, (int)iterations, (float)lmbda, points.data_ptr<float>(),
                   disp.data_ptr<float>(), reinterpret_cast<uint8_t*>(keep.data_ptr<bool>()),
                   sel.data_ptr<int64_t>(), count.data_ptr<int32_t>(), current_stream()),
               "cuda_ba.triangulate_tracks");
  return {points, disp, keep, sel, count};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("match_descriptors", &match_descriptors,
        "mutual nearest neighbours of two descriptor sets with a ratio test, two launches -> "
        "[partner0, partner1, matches, dist2, count]",
        py::arg("desc0"), py::arg("desc1"), py::arg("ratio"), py::arg("max_dist"), py::arg("n0"),
        py::arg("n0_dev"), py::arg("n1"), py::arg("n1_dev"));
  m.def("triangulate_tracks", &triangulate_tracks,
        "3-D keypoints of frame i from its tracks over i-1, i, i+1 (long_term.py:90-136), one "
        "launch -> [points, disp, keep, sel, count]",
        py::arg("poses"), py::arg("intrinsics"), py::arg("disps"), py::arg("kps0"),
        py::arg("kps1"), py::arg("kps2"), py::arg("m10"), py::arg("m12"), py::arg("max_depth"),
        py::arg("max_residual"), py::arg("iterations"), py::arg("lmbda"));
  m.def("forward", &ba_forward, "BA forward operator");
  m.def("neighbors", &ba_neighbors, "temporal neighboor indicies");
  m.def("reproject", &ba_reproject, "temporal neighboor indicies");
  m.def("solve_system", &ba_solve_system, "Sim3 pose-graph solve (ba.cpp:120-180)");
  m.def("pgo_residual", &ba_pgo_residual, "Sim3 pose-graph residual and Jacobians, one launch",
        py::arg("Ginv"), py::arg("C"), py::arg("ii"), py::arg("jj"), py::arg("jacobian") = false);
  m.def("ransac_umeyama", &ba_ransac_umeyama,
        "RANSAC-Umeyama Sim3 estimate from matched points, two launches", py::arg("src"),
        py::arg("dst"), py::arg("samples"), py::arg("threshold"), py::arg("early_exit"),
        py::arg("check_samples") = true, py::arg("return_counts") = false);
  // additions: split BA for the sharded multi-GPU path
  m.def("setup", &ba_setup, "BA graph setup -> workspace");
  m.def("build_schur", &ba_build_schur, "linearize + Schur complement (S_lower, y)");
  m.def("solve_update", &ba_solve_update, "Cholesky solve + pose/patch retraction");
  m.def("last_status", &ba_last_status, "status word of the last BA on a workspace");
  m.def("max_free_poses", &dpvo_ba_max_free_poses);
  m.def("pg_append", &pg_append, "PatchGraph.append_factors on the device (dpvo.py:480-521)");
  m.def("pg_remove", &pg_remove, "PatchGraph.remove_factors on the device (dpvo.py:523-568)");
  m.def("plan_supported", &ba_plan_supported, "window path available for (E, t0, t1, P)");
  m.def("plan", &ba_plan, "group the edges by patch (reads ii/jj/kk only) -> workspace");
  m.def("plan_offsets", &ba_plan_offsets,
        "byte offsets of epos, poff, pmask, pkk, meta inside a plan workspace");
  m.def("forward_planned", &ba_forward_planned, "BA iterations on a planned workspace");
  m.def("check_status", &ba_check_status,
        "sync on the BA status of every forward so far on the device of `like`; raises "
        "RuntimeError on fatal bits (2 bad kk, 4/8 large-graph limits, 16 timeout); returns "
        "the OR of all bits (1 = a Cholesky failure gave a zero step) and resets it");
  m.def("gba_setup", &gba_setup, "large-graph BA setup (ownership own_lo <= kk/PPF < own_hi)");
  m.def("gba_build", &gba_build, "large-graph BA: linearise owned patches -> packed (y, S)");
  m.def("gba_packed", &gba_packed, "view of the packed fp64 [y | S blocks] system");
  m.def("gba_solve_update", &gba_solve_update, "large-graph BA: solve + retraction");
  m.def("gba_info", &gba_info, "status, nuniq, nitems, nblk, nI, nB, g, nsb (device int32[8])");
  m.def("forward_marks", &ba_forward_marks, "forward + per-phase wall-clock marks");
  m.def("set_marks", [](bool on) { check_status(dpvo_ba_set_marks(on ? 1 : 0), "set_marks"); },
        "stamp wall-clock marks into the BA workspace (instrumentation)");
  m.def("workspace_marks", &ba_workspace_marks,
        "the DPVO_BA_MARKS marks of a workspace ([1664 + 2b] / [1665 + 2b]: fused launch workgroup b)");
  m.def("forward_dx", &ba_forward_dx, "forward; returns the last iteration's dX [N, 6] (fp64)");
  m.def("last_dx", &ba_last_dx, "dX [N, 6] of the last iteration of a planned forward on ws");
  m.def("reproject_ordered_plan", &ba_reproject_ordered_plan,
        "reproject + A-CORR edge order + BA plan (workspace for forward_planned), one launch");
  m.def("reproject_ordered_plan_dev", &ba_reproject_ordered_plan_dev,
        "reproject_ordered_plan with the window start t0 read from an int32 device scalar");
  m.def("forward_planned_dev", &ba_forward_planned_dev,
        "forward_planned with t0 read from an int32 device scalar (graph replay)");
  m.def("pg_remove_window_dev", &pg_remove_window_dev,
        "DPVO.keyframe window removal with thresholds relative to a device frame count");
  m.def("pg_append_dev", &pg_append_dev, "append_factors with a device edge count");
  m.def("pg_remove_frame_dev", &pg_remove_frame_dev,
        "DPVO.keyframe frame-drop removal predicated on the device decision kf");
  m.def("kf_motion", &kf_motion, "DPVO.keyframe motion magnitude + decision (dpvo.py:586-624)");
  m.def("kf_shift", &kf_shift, "DPVO.keyframe frame drop: delta log, edge / frame shift, counters",
        py::arg("kf"), py::arg("M"), py::arg("st"), py::arg("ii"), py::arg("jj"), py::arg("kk"),
        py::arg("counts"), py::arg("frames"), py::arg("rings"), py::arg("poses") = py::none(),
        py::arg("tstamps") = py::none(), py::arg("delta_log") = py::none(),
        py::arg("delta_tstamps") = py::none(), py::arg("delta_count") = py::none());
  m.def("edges_loop", &edges_loop, "PatchGraph.edges_loop (patchgraph.py:65-91), device count");
  m.def("edges_loop_work_floats", []() { return (int64_t)dpvo_edges_loop_work_floats(); });
  m.def("frame_init", &frame_init,
        "the head of DPVO.__call__ (dpvo.py:931-965): tstamps, intrinsics / RES, motion-model "
        "pose and median-depth patches of frame row n, one launch",
        py::arg("poses"), py::arg("patches"), py::arg("intrinsics"), py::arg("tstamps"),
        py::arg("times"), py::arg("new_patches"), py::arg("new_intrinsics"), py::arg("M"),
        py::arg("n"), py::arg("n_dev"), py::arg("counter"), py::arg("counter_dev"),
        py::arg("motion_model"), py::arg("damping"), py::arg("res"), py::arg("median"));
  m.def("trajectory", &trajectory,
        "DPVO.terminate's interpolation (dpvo.py:385-417) -> [traj, root, info]",
        py::arg("poses"), py::arg("tstamps"), py::arg("n"), py::arg("n_dev"),
        py::arg("delta_log"), py::arg("delta_pairs"), py::arg("delta_count"), py::arg("counter"),
        py::arg("inverse"));
  m.def("frame_prepare", &frame_prepare,
        "undistort, halve and crop a decoded frame (dpvo/stream.py), one launch -> "
        "[image uint8 [3, H, W], intrinsics float32 [4]]",
        py::arg("raw"), py::arg("calib"), py::arg("scale") = 1.0, py::arg("swap_rb") = false,
        py::arg("out") = py::none());
  m.def("frame_flow_distance", &frame_flow_distance,
        "mean clamped flow magnitude between every pair of frames (rgbd_utils.py:122-160), one "
        "launch -> D float32 [N, N]",
        py::arg("poses"), py::arg("disps"), py::arg("intrinsics"));
  m.def("frame_graph", &frame_graph,
        "the entries f D < max_flow as CSR (base.py:77-80) -> [rowptr i32 [N + 1], col i32 [nnz], "
        "dist f32 [nnz]]",
        py::arg("D"), py::arg("f") = 16.0, py::arg("max_flow") = 256.0);
  m.def("rgbd_augment", &rgbd_augment,
        "RGBDAugmentor.__call__ (augmentation.py) with the random draws given -> [images, disps, "
        "intrinsics] of the crop",
        py::arg("images"), py::arg("disps"), py::arg("intrinsics"), py::arg("crop_h"),
        py::arg("crop_w"), py::arg("do_color"), py::arg("order"), py::arg("brightness"),
        py::arg("contrast"), py::arg("saturation"), py::arg("hue"), py::arg("gray"),
        py::arg("invert"), py::arg("scale"), py::arg("swap_rb"));
  m.def("normalize_depth", &normalize_depth,
        "s = 0.7 quantile(disps, 0.98) (base.py:171-173) -> [disps / s, poses with t s, "
        "(s, lo, hi) f32 [3]]",
        py::arg("disps"), py::arg("poses"));
  m.def("trajectory_ate", &trajectory_ate,
        "association, Sim(3) alignment and error statistics of two trajectories, one launch -> "
        "[stats f64[8], model f64[13], pairs i32[min(n, m), 2], status i32[1]]",
        py::arg("est_xyz"), py::arg("est_t"), py::arg("ref_xyz"), py::arg("ref_t"),
        py::arg("max_diff") = 0.01, py::arg("align") = true);
  m.def("frame_sample", &frame_sample,
        "Patchifier's gathers (net.py:388-399) and the ring / colour writes of DPVO.__call__ "
        "(dpvo.py:937-938, 965-969) of frame n, one launch",
        py::arg("fmap"), py::arg("imap"), py::arg("image"), py::arg("coords"),
        py::arg("gmap_ring"), py::arg("imap_ring"), py::arg("patches_out"), py::arg("colors"),
        py::arg("res"), py::arg("n"), py::arg("n_dev"));
  m.def("probe_median", &probe_median,
        "torch.quantile(delta.norm(dim=-1).float(), 0.5) (dpvo.py:584) -> fp32 device scalar",
        py::arg("delta"));
  m.def("update_targets", &update_targets,
        "target = coords[..., P/2, P/2] + delta, weight = w for edges < E (dpvo.py:805-810)",
        py::arg("coords"), py::arg("delta"), py::arg("w"), py::arg("target"), py::arg("weight"),
        py::arg("E"), py::arg("E_dev"));
  m.def("map_points", &map_points,
        "centre-pixel point cloud of the first m patches (dpvo.py:834-836)", py::arg("poses"),
        py::arg("patches"), py::arg("intrinsics"), py::arg("ix"), py::arg("points"), py::arg("m"),
        py::arg("m_dev"));
  m.def("reproject_ordered_plan_insert", &ba_reproject_ordered_plan_insert,
        "reproject + edge order + BA plan + the new frame's pyramid insertion, one launch");
  m.def("reproject_ordered", &ba_reproject_ordered,
        "reproject + edge order by target frame (for cuda_corr.forward_levels(order=))");
  m.def("select_path", [](int mode) { check_status(dpvo_ba_select_path(mode), "select_path"); },
        "F-BA implementation: 0 auto, 2 multi-kernel, 4 large-graph, 5 window");
  m.def("spd_solve", &spd_solve,
        "batched SPD factor + solve (CholeskySolver, dpvo/ba.py:13-38): H [..., n, n] (lower "
        "triangle read), B [..., n, k] -> [X, L (lower factor), info (first failed column, 0 = ok)]");
  m.def("spd_solve_factored", &spd_solve_factored,
        "X = (L L^T)^-1 B for a lower factor L from spd_solve (the backward's cholesky_solve)");
  m.def("ba_layer_forward", &ba_layer_forward,
        "one Gauss-Newton step of dpvo/ba.py BA: (poses, patches, intrinsics, targets, weights, "
        "lmbda tensor or None, lmbda float, ii, jj, kk, n, fixedp, structure_only, bounds, ep, "
        "with_backward) -> [dX [n_free, 6], dZ [M], workspace (int32 words: out-of-range edges, "
        "factorisation info)]");
  m.def("transform_forward", &transform_forward,
        "projective_ops.transform, one launch: (poses, patches, intrinsics, ii, jj, kk, with_corr) "
        "-> [coords [E,P,P,2], valid [E,P,P] (, coords [E,2,P,P])]");
  m.def("transform_backward", &transform_backward,
        "adjoint of transform_forward: (.., g_coords, want_poses, want_patches) -> "
        "[g_poses [N,6] | None, g_patches [M,3,P,P] | None]");
  m.def("flow_loss_forward", &flow_loss_forward,
        "train.py:87-88: (coords, coords_gt, valid [E]) -> [loss, count, emin, argmin]");
  m.def("flow_loss_backward", &flow_loss_backward,
        "(coords, coords_gt, valid, count, argmin, g_loss) -> g_coords");
  m.def("pose_loss_forward", &pose_loss_forward,
        "train.py:90-113: (G, Ps [n,7]) -> [(mean tr, mean ro, s), tr, ro]");
  m.def("pose_loss_backward", &pose_loss_backward, "(G, Ps, g_out [2]) -> g_G [n,6]");
  m.def("ba_layer_backward", &ba_layer_backward,
        "adjoint of ba_layer_forward on its workspace: (ws, poses, patches, intrinsics, ii, jj, kk, "
        "gX, gZ, n, fixedp, structure_only) -> [g_targets, g_weights, g_poses [N, 6], g_patches [M, 3]]");
  m.attr("native_library") = dpvo_version();
}
