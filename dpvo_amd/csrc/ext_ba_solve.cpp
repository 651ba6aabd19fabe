// ext_ba_solve.cpp -- cuda_ba, part 1: bundle adjustment and reprojection
// (drop-in for dpvo/fastba/ba.cpp:183-189), the BA status, the split and
// large-graph BA of the sharded path, the SPD solves, and the pose-graph
// entries of the loop closure (solve_system, pgo_residual, ransac_umeyama).
#include <map>
#include <mutex>
#include <string>

#include "ext_common.hpp"

using namespace dpvo_ext;

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

void track_status(void* ws, const torch::Tensor& like, int E, int t0, int t1) {
  std::lock_guard<std::mutex> lk(g_st_mu);
  auto& sl = slot_for(like);
  if (!sl.acc.defined()) return;  // first call happened inside a capture: untracked
  void* st = current_stream();
  check_status(dpvo_ba_status_accumulate(ws, E, t0, t1, sl.acc.data_ptr<int>(), st),
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

// cuda_ba.check_status(device): synchronise on the status of every forward
// issued so far on that device; raise on a fatal bit; return the OR of all
// bits seen (bit 1 included) and reset the accumulator.
int ba_check_status(torch::Tensor like) {
  Entry("cuda_ba.check_status").on_gpu(like, "like");
  TORCH_CHECK(!is_capturing(), "cuda_ba.check_status: not allowed during graph capture");
  const DeviceGuard guard(like.device());
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
// The BA entries: Entry::edges for the edge sextuple, and on top of it what
// the in-place entries need: poses / patches that the kernels can update where
// they are (poses.view({-1,7}) / patches.view({-1,3,P,P}) must alias the
// caller's storage for the update to land, ba_cuda.cu:458-459), and the
// residual inputs.  The sizes of target / weight against E stay with each entry.
// ---------------------------------------------------------------------------
struct BaIn {
  const float *target, *weight, *lmbda;
};

BaIn ba_inputs(const Entry& a, const torch::Tensor& poses, const torch::Tensor& patches,
               torch::Tensor& target, torch::Tensor& weight, torch::Tensor& lmbda) {
  a.buf<float>(poses, "poses");
  a.buf<float>(patches, "patches");
  return {a.in<float>(target, "target"), a.in<float>(weight, "weight"),
          a.in<float>(lmbda, "lmbda")};
}

// ba.cpp:32-45 -> cuda_ba (ba_cuda.cu:433-582).  Mutates poses / patches.
torch::Tensor ba_forward_ws(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                            torch::Tensor target, torch::Tensor weight, torch::Tensor lmbda,
                            torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int PPF, int t0,
                            int t1, int iterations, bool eff_impl) {
  const Entry a("cuda_ba.forward");
  const BaIn b = ba_inputs(a, poses, patches, target, weight, lmbda);
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  const DeviceGuard guard(poses.device());
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
               a.fn());
  track_status(ws.data_ptr(), poses, e.E, t0, t1);
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

// ii / jj / kk alone, for the setup entries
struct Idx {
  const int64_t *ii, *jj, *kk;
  int E;
};

Idx index_inputs(const Entry& a, torch::Tensor& ii, torch::Tensor& jj, torch::Tensor& kk) {
  const Idx x = {a.in<int64_t>(ii, "ii"), a.in<int64_t>(jj, "jj"), a.in<int64_t>(kk, "kk"),
                 (int)ii.numel()};
  a.one_length(ii, jj, kk);
  return x;
}

torch::Tensor ba_plan(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int64_t num_patches,
                      int64_t num_poses, int t0, int t1) {
  const Entry a("cuda_ba.plan");
  const Idx x = index_inputs(a, ii, jj, kk);
  const DeviceGuard guard(ii.device());
  const size_t wsb = dpvo_ba_workspace_bytes(x.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, ii.options().dtype(torch::kUInt8));
  check_status(dpvo_ba_plan(x.ii, x.jj, x.kk, x.E, (int)num_patches, (int)num_poses, t0, t1,
                            ws.data_ptr(), wsb, current_stream()),
               a.fn());
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
  const Entry a("cuda_ba.forward_planned");
  const BaIn b = ba_inputs(a, poses, patches, target, weight, lmbda);
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  void* wsp = a.bytes(ws, "ws", poses.device());
  const DeviceGuard guard(poses.device());
  TORCH_CHECK(target.numel() >= 2 * e.E && weight.numel() >= 2 * e.E,
              "target/weight must be [.., E, 2]");
  if (e.E == 0 || iterations <= 0) return;
  poll_status(poses);
  check_status(dpvo_ba_forward_planned(e.poses, e.patches, e.intrinsics, b.target, b.weight,
                                       b.lmbda, e.ii, e.jj, e.kk, e.E, e.P, e.num_poses,
                                       e.num_patches, t0, t1, iterations, wsp, ws.numel(),
                                       current_stream()),
               a.fn());
  track_status(wsp, poses, e.E, t0, t1);
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
  const Entry a("cuda_ba.workspace_marks");
  TORCH_CHECK(E >= 0 && t1 > t0, "cuda_ba.workspace_marks: bad E / window");
  void* wsp = a.bytes(ws, "ws", ws.device(), dpvo_ba_workspace_bytes((int)E, t0, t1));
  const DeviceGuard guard(ws.device());
  auto out = torch::zeros({DPVO_BA_MARKS}, ws.options().dtype(torch::kInt64));
  check_status(dpvo_ba_phase_marks(wsp, (int)E, t0, t1, out.data_ptr<int64_t>(), current_stream()),
               a.fn());
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
  const Entry a("cuda_ba.last_dx");
  void* wsp = a.bytes(ws, "ws", ws.device());
  const DeviceGuard guard(ws.device());
  const int N = t1 > t0 ? t1 - t0 : 0;
  auto out = torch::zeros({N, 6}, ws.options().dtype(torch::kFloat64));
  if (N == 0) return out;
  check_status(dpvo_ba_last_dx(wsp, (int)E, t0, t1, out.data_ptr<double>(), current_stream()),
               a.fn());
  return out;
}

// ba.cpp:47-53 -> cuda_reproject (ba_cuda.cu:585-616)
torch::Tensor ba_reproject(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                           torch::Tensor ii, torch::Tensor jj, torch::Tensor kk) {
  const Entry a("cuda_ba.reproject");
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  const DeviceGuard guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  check_status(dpvo_reproject(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P,
                              e.num_poses, e.num_patches, coords.data_ptr<float>(),
                              current_stream()),
               a.fn());
  return coords.view({1, e.E, 2, e.P, e.P});
}

// reproject + the A-CORR edge order (edges grouped by target frame) in one launch
std::vector<torch::Tensor> ba_reproject_ordered(torch::Tensor poses, torch::Tensor patches,
                                                torch::Tensor intrinsics, torch::Tensor ii,
                                                torch::Tensor jj, torch::Tensor kk, int N2) {
  const Entry a("cuda_ba.reproject_ordered");
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  const DeviceGuard guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  auto order = torch::empty({e.E}, poses.options().dtype(torch::kInt32));
  check_status(dpvo_reproject_ordered(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P,
                                      e.num_poses, e.num_patches, N2, coords.data_ptr<float>(),
                                      order.data_ptr<int32_t>(), current_stream()),
               a.fn());
  return {coords.view({1, e.E, 2, e.P, e.P}), order};
}

// reproject + edge order + BA plan (workspace for forward_planned) in one
// launch; t0_dev: the window start as an int32 device scalar (graph-replayed
// DPVO updates: it moves every frame while shapes stay fixed), t1 - t0 = N the
// (fixed) number of free poses; src / dst / scales: the new frame's pyramid
// insertion in the same launch (src [C, H, W] NCHW, dst[l] the channels-last
// [C, H/s, W/s] slot view of level l)
std::vector<torch::Tensor> reproject_plan(const char* fn, torch::Tensor poses,
                                          torch::Tensor patches, torch::Tensor intrinsics,
                                          torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                                          int N2, int t0, int t1, const torch::Tensor* t0_dev,
                                          torch::Tensor* src, const std::vector<torch::Tensor>* dst,
                                          const std::vector<int64_t>* scales) {
  const Entry a(fn);
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  const int32_t* t0p = t0_dev ? a.buf<int32_t>(*t0_dev, "t0_dev", 1) : nullptr;
  Pyramid p;
  if (src) p = a.pyramid(*src, *dst, *scales, "dst");
  const DeviceGuard guard(poses.device());
  auto coords = torch::empty({e.E, 2, e.P, e.P}, poses.options());
  auto order = torch::empty({e.E}, poses.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_ba_workspace_bytes(e.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, poses.options().dtype(torch::kUInt8));
  float* cp = coords.data_ptr<float>();
  int32_t* op = order.data_ptr<int32_t>();
  int st;
  if (t0p)
    st = dpvo_reproject_ordered_plan_dev(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E,
                                         e.P, e.num_poses, e.num_patches, N2, cp, op, t0p, t1 - t0,
                                         ws.data_ptr(), wsb, current_stream());
  else if (src)
    st = dpvo_reproject_ordered_plan_insert(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E,
                                            e.P, e.num_poses, e.num_patches, N2, cp, op, t0, t1,
                                            ws.data_ptr(), wsb, p.src, p.dst.data(),
                                            p.scales.data(), (int)p.dst.size(), p.C, p.H, p.W,
                                            p.dtype, current_stream());
  else
    st = dpvo_reproject_ordered_plan(e.poses, e.patches, e.intrinsics, e.ii, e.jj, e.kk, e.E, e.P,
                                     e.num_poses, e.num_patches, N2, cp, op, t0, t1, ws.data_ptr(),
                                     wsb, current_stream());
  check_status(st, fn);
  return {coords.view({1, e.E, 2, e.P, e.P}), order, ws};
}

std::vector<torch::Tensor> ba_reproject_ordered_plan(torch::Tensor poses, torch::Tensor patches,
                                                     torch::Tensor intrinsics, torch::Tensor ii,
                                                     torch::Tensor jj, torch::Tensor kk, int N2,
                                                     int t0, int t1) {
  return reproject_plan("cuda_ba.reproject_ordered_plan", poses, patches, intrinsics, ii, jj, kk,
                        N2, t0, t1, nullptr, nullptr, nullptr, nullptr);
}

std::vector<torch::Tensor> ba_reproject_ordered_plan_insert(
    torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics, torch::Tensor ii,
    torch::Tensor jj, torch::Tensor kk, int N2, int t0, int t1, torch::Tensor src,
    std::vector<torch::Tensor> dst, std::vector<int64_t> scales) {
  return reproject_plan("cuda_ba.reproject_ordered_plan_insert", poses, patches, intrinsics, ii, jj,
                        kk, N2, t0, t1, nullptr, &src, &dst, &scales);
}

std::vector<torch::Tensor> ba_reproject_ordered_plan_dev(torch::Tensor poses, torch::Tensor patches,
                                                         torch::Tensor intrinsics, torch::Tensor ii,
                                                         torch::Tensor jj, torch::Tensor kk, int N2,
                                                         torch::Tensor t0_dev, int N) {
  return reproject_plan("cuda_ba.reproject_ordered_plan_dev", poses, patches, intrinsics, ii, jj,
                        kk, N2, 0, N, &t0_dev, nullptr, nullptr, nullptr);
}

void ba_forward_planned_dev(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
                            torch::Tensor intrinsics, torch::Tensor target, torch::Tensor weight,
                            torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj,
                            torch::Tensor kk, torch::Tensor t0_dev, int N, int iterations) {
  const Entry a("cuda_ba.forward_planned_dev");
  const BaIn b = ba_inputs(a, poses, patches, target, weight, lmbda);
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  const int32_t* t0p = a.buf<int32_t>(t0_dev, "t0_dev", 1);
  void* wsp = a.bytes(ws, "ws", poses.device());
  const DeviceGuard guard(poses.device());
  // exactly 2 E here, where forward / forward_planned accept longer buffers
  TORCH_CHECK(target.numel() == 2 * (int64_t)e.E && weight.numel() == 2 * (int64_t)e.E,
              "target / weight must hold 2 E values");
  // runs under graph capture: no status poll before, no status copy after
  check_status(dpvo_ba_forward_planned_dev(e.poses, e.patches, e.intrinsics, b.target, b.weight,
                                           b.lmbda, e.ii, e.jj, e.kk, e.E, e.P, e.num_poses,
                                           e.num_patches, t0p, N, iterations, wsp, ws.numel(),
                                           current_stream()),
               a.fn());
}

// ba.cpp:59-97 (host loop in the reference; here one O(E^2) LDS-tiled kernel)
std::vector<torch::Tensor> ba_neighbors(torch::Tensor ii, torch::Tensor jj) {
  const Entry a("cuda_ba.neighbors");
  const int64_t* ip = a.in<int64_t>(ii, "ii");
  const int64_t* jp = a.in<int64_t>(jj, "jj");
  const DeviceGuard guard(ii.device());
  const int E = ii.numel();
  auto ix = torch::empty({E}, ii.options());
  auto jx = torch::empty({E}, ii.options());
  check_status(dpvo_neighbors(ip, jp, E, ix.data_ptr<int64_t>(), jx.data_ptr<int64_t>(),
                              current_stream()),
               a.fn());
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
  const Entry a("cuda_ba.solve_system");
  const torch::Device out_dev = res.device();
  torch::Device dev = out_dev;
  if (!res.is_cuda()) {
    TORCH_CHECK(torch::cuda::is_available(),
                "cuda_ba.solve_system: no HIP device (the MI355X build has no CPU path)");
    dev = torch::Device(torch::kCUDA, c10::hip::current_device());
  }
  const DeviceGuard guard(dev);
  J_Ginv_i = J_Ginv_i.to(dev);
  J_Ginv_j = J_Ginv_j.to(dev);
  ii = ii.to(dev);
  jj = jj.to(dev);
  res = res.to(dev);
  const float* Jip = a.in<float>(J_Ginv_i, "J_Ginv_i");
  const float* Jjp = a.in<float>(J_Ginv_j, "J_Ginv_j");
  const float* rp = a.in<float>(res, "res");
  const int64_t* iip = a.in<int64_t>(ii, "ii");
  a.in<int64_t>(jj, "jj");
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
    check_status(dpvo_pgo_plan(ip, jp, (int)r, (int)nf, nullptr, 0, &len), a.fn());
    auto planh = torch::empty({len}, torch::kInt64);
    check_status(dpvo_pgo_plan(ip, jp, (int)r, (int)nf, planh.data_ptr<int64_t>(), len, &len),
                 a.fn());
    const int64_t* hdr = planh.data_ptr<int64_t>();
    const int64_t m = hdr[3], ws_n = hdr[25], hS = hdr[22], hBB = hdr[23], hDelta = hdr[24];
    auto plan = planh.to(dev, /*non_blocking=*/false);
    auto ws = torch::empty({ws_n}, res.options().dtype(torch::kFloat64));
    auto fail = torch::zeros({1}, res.options().dtype(torch::kInt32));
    check_status(dpvo_pgo_factor(Jip, Jjp, iip, rp, plan.data_ptr<int64_t>(), hdr, (float)ep,
                                 (float)lm, ws.data_ptr<double>(), fail.data_ptr<int>(),
                                 current_stream()),
                 a.fn());
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
                 a.fn());
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

// lowest and highest value of an index tensor: one reduction, one host read
std::pair<int64_t, int64_t> index_range(const torch::Tensor& idx) {
  const auto mm = at::aminmax(idx);
  const auto mmh = torch::stack({std::get<0>(mm), std::get<1>(mm)}).to(torch::kInt64).cpu();
  return {mmh.data_ptr<int64_t>()[0], mmh.data_ptr<int64_t>()[1]};
}

// Residual (and Jacobians) of every pose-graph edge in one launch: the device
// form of optim_utils.py:152-189 (_residual + batch_jacobian), whose outputs
// are solve_system's inputs.  Everything is validated on the host before the
// launch; the index range check costs one reduction and one sync (the LM loop
// of dpvo_amd/loop_closure.py syncs every iteration anyway).
std::vector<torch::Tensor> ba_pgo_residual(torch::Tensor Ginv, torch::Tensor C, torch::Tensor ii,
                                           torch::Tensor jj, bool jacobian) {
  const Entry a("cuda_ba.pgo_residual");
  a.on_gpu(Ginv, "Ginv");
  a.on_gpu(C, "C");
  TORCH_CHECK(C.scalar_type() == Ginv.scalar_type(),
              "cuda_ba.pgo_residual: Ginv and C must have the same dtype");
  TORCH_CHECK(Ginv.dim() == 2 && Ginv.size(1) == 7, "cuda_ba.pgo_residual: Ginv must be [n, 7]");
  TORCH_CHECK(C.dim() == 2 && C.size(1) == 8, "cuda_ba.pgo_residual: C must be [r, 8]");
  const int64_t n = Ginv.size(0), r = C.size(0);
  TORCH_CHECK(ii.dim() == 1 && jj.dim() == 1 && ii.numel() == r && jj.numel() == r,
              "cuda_ba.pgo_residual: ii / jj must be [r]");
  TORCH_CHECK(r <= (1 << 26) && n < (1LL << 31), "cuda_ba.pgo_residual: graph too large");
  int dt;
  const void* Gp = a.in(Ginv, "Ginv", kF32 | kF64, &dt);
  const void* Cp = a.in(C, "C", kF32 | kF64);
  const int64_t* ip = a.in<int64_t>(ii, "ii");
  const int64_t* jp = a.in<int64_t>(jj, "jj");
  a.same_device({C, Ginv, ii, jj});
  const DeviceGuard guard(Ginv.device());
  auto res = torch::empty({r, 7}, Ginv.options());
  torch::Tensor Ji, Jj;
  if (jacobian) {
    Ji = torch::empty({r, 7, 7}, Ginv.options());
    Jj = torch::empty({r, 7, 7}, Ginv.options());
  }
  if (r > 0) {
    const auto range = index_range(torch::cat({ii, jj}));
    TORCH_CHECK(range.first >= 0 && range.second < n, "cuda_ba.pgo_residual: pose index out of "
                "range [0, ", n, "): min ", range.first, ", max ", range.second);
    check_status(dpvo_pgo_residual(Gp, Cp, ip, jp, (int)r, (int)n, dt, res.data_ptr(),
                                   jacobian ? Ji.data_ptr() : nullptr,
                                   jacobian ? Jj.data_ptr() : nullptr, current_stream()),
                 a.fn());
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
  const Entry a("cuda_ba.ransac_umeyama");
  a.on_gpu(src, "src");
  a.on_gpu(dst, "dst");
  a.on_gpu(samples, "samples");
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
  a.same_device({src, dst, samples});
  const int64_t N = src.size(0), H = samples.size(0);
  TORCH_CHECK(N >= 3, "cuda_ba.ransac_umeyama: needs N >= 3 points, got ", N);
  TORCH_CHECK(N <= (1 << 28) && H <= (1 << 24), "cuda_ba.ransac_umeyama: problem too large");
  TORCH_CHECK(threshold > 0.0, "cuda_ba.ransac_umeyama: threshold must be positive");
  const DeviceGuard guard(src.device());
  if (check_samples && !is_capturing()) {
    const auto range = index_range(samples);
    TORCH_CHECK(range.first >= 0 && range.second < N, "cuda_ba.ransac_umeyama: sample index out "
                "of range [0, ", N, "): min ", range.first, ", max ", range.second);
  }
  int dt;
  const void* sp = a.in(src, "src", kF32 | kF64, &dt);
  const void* dp = a.in(dst, "dst", kF32 | kF64);
  samples = samples.to(torch::kInt32);
  const int32_t* smp = a.in<int32_t>(samples, "samples");
  const auto i32 = src.options().dtype(torch::kInt32);
  auto model = torch::empty({21}, src.options().dtype(torch::kFloat64));
  auto info = torch::empty({4}, i32);
  auto mask = torch::empty({N}, src.options().dtype(torch::kBool));
  const size_t wsb = dpvo_ransac_umeyama_workspace_bytes((int)N, (int)H);
  auto ws = torch::empty({(int64_t)(wsb / sizeof(int32_t))}, i32);
  early_exit = std::min<int64_t>(std::max<int64_t>(early_exit, INT32_MIN), INT32_MAX);
  check_status(dpvo_ransac_umeyama(sp, dp, (int)N, dt, smp, (int)H, threshold, (int)early_exit,
                                   model.data_ptr<double>(), info.data_ptr<int32_t>(),
                                   reinterpret_cast<uint8_t*>(mask.data_ptr<bool>()),
                                   ws.data_ptr(), wsb, current_stream()),
               a.fn());
  if (return_counts) return {model, info, mask, ws.narrow(0, 0, H)};
  return {model, info, mask};
}

// Split F-BA for the edge-sharded multi-GPU path.
torch::Tensor ba_setup(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int num_patches,
                       int t0, int t1) {
  const Entry a("cuda_ba.setup");
  const Idx x = index_inputs(a, ii, jj, kk);
  const DeviceGuard guard(ii.device());
  const size_t wsb = dpvo_ba_workspace_bytes(x.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, ii.options().dtype(torch::kUInt8));
  check_status(dpvo_ba_setup(x.ii, x.jj, x.kk, x.E, num_patches, t0, t1, ws.data_ptr(), wsb,
                             current_stream()),
               a.fn());
  return ws;
}

std::vector<torch::Tensor> ba_build_schur(torch::Tensor ws, torch::Tensor poses,
                                          torch::Tensor patches, torch::Tensor intrinsics,
                                          torch::Tensor target, torch::Tensor weight,
                                          torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj,
                                          torch::Tensor kk, int t0, int t1) {
  const Entry a("cuda_ba.build_schur");
  const BaIn b = ba_inputs(a, poses, patches, target, weight, lmbda);
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  void* wsp = a.bytes(ws, "ws", poses.device());
  const DeviceGuard guard(poses.device());
  const int N = t1 - t0;
  auto S = torch::zeros({N * (N + 1) / 2, 6, 6}, poses.options().dtype(torch::kFloat64));
  auto y = torch::zeros({6 * N}, poses.options().dtype(torch::kFloat64));
  check_status(dpvo_ba_build_schur(e.poses, e.patches, e.intrinsics, b.target, b.weight, b.lmbda,
                                   e.ii, e.jj, e.kk, e.E, e.P, e.num_poses, t0, t1, wsp,
                                   S.data_ptr<double>(), y.data_ptr<double>(), current_stream()),
               a.fn());
  return {S, y};
}

torch::Tensor ba_solve_update(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
                              torch::Tensor S, torch::Tensor y, int E, int t0, int t1) {
  const Entry a("cuda_ba.solve_update");
  float* pp = a.buf<float>(poses, "poses");
  float* tp = a.buf<float>(patches, "patches");
  const double* Sp = a.in<double>(S, "S");
  const double* yp = a.in<double>(y, "y");
  void* wsp = a.bytes(ws, "ws", poses.device());
  const DeviceGuard guard(poses.device());
  const int N = t1 - t0, P = patches.size(-1);
  auto dX = torch::zeros({N > 0 ? N : 0, 6}, poses.options().dtype(torch::kFloat64));
  check_status(dpvo_ba_solve_update(pp, tp, Sp, yp, E, P, poses.numel() / 7, t0, t1, wsp,
                                    N > 0 ? dX.data_ptr<double>() : nullptr, current_stream()),
               a.fn());
  return dX;
}

torch::Tensor ba_last_status(torch::Tensor ws, int E, int t0, int t1) {
  const Entry a("cuda_ba.last_status");
  void* wsp = a.bytes(ws, "ws", ws.device());
  const DeviceGuard guard(ws.device());
  auto out = torch::zeros({1}, ws.options().dtype(torch::kInt32));
  check_status(dpvo_ba_last_status(wsp, E, t0, t1, out.data_ptr<int>(), current_stream()), a.fn());
  return out;
}

// Large-graph F-BA split for the edge-sharded driver (dpvo_amd/fastba/sharded.py):
// setup -> [build -> all_reduce(packed) -> solve_update] x iterations.
torch::Tensor gba_setup(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, int num_patches,
                        int PPF, int t0, int t1, int own_lo, int own_hi) {
  const Entry a("cuda_ba.gba_setup");
  const Idx x = index_inputs(a, ii, jj, kk);
  const DeviceGuard guard(ii.device());
  TORCH_CHECK(x.E > 0, "gba_setup: empty graph");
  const size_t wsb = dpvo_gba_workspace_bytes(x.E, t0, t1);
  auto ws = torch::empty({(int64_t)wsb}, ii.options().dtype(torch::kUInt8));
  check_status(dpvo_gba_setup(x.ii, x.jj, x.kk, x.E, num_patches, PPF, t0, t1, own_lo, own_hi,
                              ws.data_ptr(), wsb, current_stream()),
               a.fn());
  return ws;
}

void gba_build(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches,
               torch::Tensor intrinsics, torch::Tensor target, torch::Tensor weight,
               torch::Tensor lmbda, torch::Tensor ii, torch::Tensor jj, int t0, int t1) {
  const Entry a("cuda_ba.gba_build");
  const BaIn b = ba_inputs(a, poses, patches, target, weight, lmbda);
  torch::Tensor kk = jj;  // the build reads ii / jj only
  const Edges<float> e = a.edges(poses, patches, intrinsics, ii, jj, kk);
  void* wsp = a.bytes(ws, "ws", poses.device(), dpvo_gba_workspace_bytes(e.E, t0, t1));
  const DeviceGuard guard(poses.device());
  check_status(dpvo_gba_build(e.poses, e.patches, e.intrinsics, b.target, b.weight, b.lmbda, e.ii,
                              e.jj, e.E, e.P, e.num_poses, t0, t1, wsp, current_stream()),
               a.fn());
}

// the packed [y (6N) | S blocks (nblk x 36)] fp64 system inside the workspace
torch::Tensor gba_packed(torch::Tensor ws, int E, int t0, int t1, int64_t nblk) {
  Entry("cuda_ba.gba_packed").on_gpu(ws, "ws");
  const int64_t N = t1 > t0 ? t1 - t0 : 0;
  const int64_t off = (int64_t)dpvo_gba_packed_offset(E, t0, t1);
  const int64_t n = 6 * N + 36 * nblk;
  TORCH_CHECK(off % 8 == 0 && off + 8 * n <= ws.numel(), "gba_packed: bad extent");
  return ws.narrow(0, off, 8 * n).view(torch::kFloat64);
}

void gba_solve_update(torch::Tensor ws, torch::Tensor poses, torch::Tensor patches, int E, int t0,
                      int t1) {
  const Entry a("cuda_ba.gba_solve_update");
  float* pp = a.buf<float>(poses, "poses");
  float* tp = a.buf<float>(patches, "patches");
  void* wsp = a.bytes(ws, "ws", poses.device());
  const DeviceGuard guard(poses.device());
  check_status(dpvo_gba_solve_update(pp, tp, E, patches.size(-1), t0, t1, wsp, current_stream()),
               a.fn());
}

torch::Tensor gba_info(torch::Tensor ws, int E, int t0, int t1) {
  const Entry a("cuda_ba.gba_info");
  void* wsp = a.bytes(ws, "ws", ws.device());
  const DeviceGuard guard(ws.device());
  auto out = torch::zeros({8}, ws.options().dtype(torch::kInt32));
  check_status(dpvo_gba_info(wsp, E, t0, t1, out.data_ptr<int>(), current_stream()), a.fn());
  return out;
}

// CholeskySolver's device solve (dpvo/ba.py:13-38 -> torch.linalg.cholesky_ex +
// cholesky_solve): batched over the leading dims, fp32 / fp64
struct Spd {
  const void *H, *B;
  int64_t batch;
  int n, k, dtype;
};

Spd spd_inputs(const Entry& a, torch::Tensor& H, torch::Tensor& B) {
  Spd s;
  s.H = a.in(H, "H", kF32 | kF64, &s.dtype);
  s.B = a.in(B, "B", s.dtype == DPVO_F32 ? kF32 : kF64);
  TORCH_CHECK(H.dim() >= 2 && H.size(-1) == H.size(-2), "H must be [..., n, n]");
  TORCH_CHECK(B.dim() == H.dim() && B.size(-2) == H.size(-1), "B must be [..., n, k]");
  for (int64_t d = 0; d + 2 < H.dim(); d++)
    TORCH_CHECK(H.size(d) == B.size(d), "H / B batch dims differ");
  s.n = (int)H.size(-1);
  s.k = (int)B.size(-1);
  s.batch = s.n ? H.numel() / ((int64_t)s.n * s.n) : 0;
  return s;
}

std::vector<torch::Tensor> spd_solve(torch::Tensor H, torch::Tensor B) {
  const Entry a("cuda_ba.spd_solve");
  const Spd s = spd_inputs(a, H, B);
  const DeviceGuard guard(H.device());
  auto L = torch::empty_like(H);
  auto X = torch::empty_like(B);
  std::vector<int64_t> bs(H.sizes().begin(), H.sizes().end() - 2);
  auto info = torch::zeros(bs, H.options().dtype(torch::kInt32));
  check_status(dpvo_spd_solve(s.H, s.B, L.data_ptr(), X.data_ptr(), info.data_ptr<int32_t>(),
                              (int)s.batch, s.n, s.k, 1, s.dtype, current_stream()),
               a.fn());
  return {X, L, info};
}

torch::Tensor spd_solve_factored(torch::Tensor L, torch::Tensor B) {
  const Entry a("cuda_ba.spd_solve_factored");
  const Spd s = spd_inputs(a, L, B);
  const DeviceGuard guard(L.device());
  auto X = torch::empty_like(B);
  check_status(dpvo_spd_solve(s.H, s.B, nullptr, X.data_ptr(), nullptr, (int)s.batch, s.n, s.k, 0,
                              s.dtype, current_stream()),
               a.fn());
  return X;
}

}  // namespace

void bind_solve(py::module_& m) {
  m.def("forward", &ba_forward, "BA forward operator");
  m.def("neighbors", &ba_neighbors, "temporal neighboor indicies");
  m.def("reproject", &ba_reproject,
        "reprojection of every edge's patch into its target frame -> coords [1, E, 2, P, P]");
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
}
