// ext_update.cpp -- the `dpvo_update` extension module: DPVO's update operator
// (dpvo/net.py:175-339) bound to the dpvo_update_* C ABI of dpvo_hot.h.  The
// reference has no extension for it (it is PyTorch there); dpvo_amd/net.py is
// the nn.Module on top.
#include <climits>
#include <vector>

#include "ext_common.hpp"

using namespace dpvo_ext;

static int64_t packed_bytes(int64_t K0, int64_t wdtype) {
  const int wd = Entry("dpvo_update.packed_bytes").wdtype_code(wdtype);
  return (int64_t)dpvo_update_packed_bytes((int)K0, wd);
}

// element counts of Update's 50 parameter tensors in state_dict order
static std::function<int64_t(size_t)> param_numel(int64_t K0) {
  return [K0](size_t i) -> int64_t {
    return (i % 2 == 0 && i != 8 && i != 22 && i != 30 && i != 42)
               ? (i == 38 ? 384 * K0 : (i >= 46 ? 2 * 384 : 384 * 384))
               : (i == 47 || i == 49 ? 2 : 384);
  };
}

// 50 CPU float32 tensors in state_dict order -> packed host blob (uint8)
static torch::Tensor pack_weights(std::vector<torch::Tensor> tensors, int64_t K0, int64_t wdtype) {
  const Entry a("dpvo_update.pack_weights");
  TORCH_CHECK(K0 >= 1 && K0 <= INT_MAX, "dpvo_update.pack_weights: bad corr_dim ", K0);
  const auto ptrs = a.host_params(tensors, 50, param_numel(K0));
  const int wd = a.wdtype_code(wdtype);
  const size_t bytes = dpvo_update_packed_bytes((int)K0, wd);
  auto blob = torch::empty({(int64_t)bytes}, torch::dtype(torch::kUInt8));
  check_status(dpvo_update_pack_weights(ptrs.data(), 50, 384, (int)K0, wd, blob.data_ptr(), bytes),
               "dpvo_update_pack_weights");
  return blob;
}

static int64_t workspace_bytes(int64_t E, int64_t K0) {
  return (int64_t)dpvo_update_workspace_bytes((int)E, (int)K0);
}

static void plan(torch::Tensor gk, torch::Tensor gij, torch::Tensor workspace) {
  const Entry a("dpvo_update.plan");
  const int64_t* kp = a.in<int64_t>(gk, "gk");
  const int64_t* jp = a.in<int64_t>(gij, "gij");
  TORCH_CHECK(gk.dim() == 1 && gij.dim() == 1 && gk.numel() == gij.numel(),
              "dpvo_update.plan: gk and gij must be 1-D of one length");
  a.same_device({gk, gij});
  TORCH_CHECK(gk.numel() <= INT_MAX, "dpvo_update.plan: too many edges");
  void* ws = a.bytes(workspace, "workspace", gk.device());
  const DeviceGuard guard(gk.device());
  check_status(dpvo_update_plan(kp, jp, (int)gk.numel(), ws, (size_t)workspace.numel(),
                                current_stream()),
               "dpvo_update_plan");
}

// t: contiguous [E, cols] of dtype `accept` on like's device
static void* rows(const Entry& a, const torch::Tensor& t, const torch::Tensor& like, int64_t E,
                  int64_t cols, unsigned accept, const char* name) {
  void* p = a.buf(t, name, accept);
  TORCH_CHECK(t.device() == like.device() && t.numel() == E * cols, a.fn(), ": ", name,
              " must be [E, ", cols, "] on the inputs' device");
  return p;
}

static void forward(torch::Tensor blob, int64_t wdtype, torch::Tensor net, torch::Tensor inp,
                    torch::Tensor corr, torch::Tensor ix, torch::Tensor jx, torch::Tensor workspace,
                    torch::Tensor net_out, torch::Tensor d, torch::Tensor w) {
  const Entry a("dpvo_update.forward");
  const int wd = a.wdtype_code(wdtype);
  int io;
  const void* np = a.buf(net, "net", kF32 | kF16, &io);
  TORCH_CHECK(io == DPVO_F32 || wd == DPVO_F16,
              "dpvo_update.forward: net/inp/corr are float32, or float16 with float16 weights");
  TORCH_CHECK(net.dim() == 2 && net.size(1) == 384, "dpvo_update.forward: net must be [E, 384]");
  const int64_t E = net.size(0);
  TORCH_CHECK(E <= INT_MAX, "dpvo_update.forward: too many edges");
  a.on_gpu(corr, "corr");
  TORCH_CHECK(corr.dim() == 2 && corr.size(0) == E && corr.size(1) >= 1,
              "dpvo_update.forward: corr must be [E, corr_dim]");
  const int64_t K0 = corr.size(1);
  const unsigned same = io == DPVO_F32 ? kF32 : kF16;
  const void* ip = rows(a, inp, net, E, 384, same, "inp");
  const void* cp = rows(a, corr, net, E, K0, same, "corr");
  void* op = rows(a, net_out, net, E, 384, same, "net_out");
  float* dp = (float*)rows(a, d, net, E, 2, kF32, "d");
  float* wp = (float*)rows(a, w, net, E, 2, kF32, "w");
  const int64_t* ixp = a.in<int64_t>(ix, "ix");
  const int64_t* jxp = a.in<int64_t>(jx, "jx");
  TORCH_CHECK(ix.numel() == E && jx.numel() == E, "dpvo_update.forward: ix, jx must have E elements");
  a.same_device({net, ix, jx});
  const void* bp = a.bytes(blob, "blob (packed for this corr_dim and weight dtype)", net.device(),
                           dpvo_update_packed_bytes((int)K0, wd), true);
  void* ws = a.bytes(workspace, "workspace", net.device());
  const DeviceGuard guard(net.device());
  check_status(dpvo_update_forward(bp, wd, np, ip, cp, ixp, jxp, (int)E, 384, (int)K0, io, ws,
                                   (size_t)workspace.numel(), op, dp, wp, current_stream()),
               "dpvo_update_forward");
}

// --- the training surface ------------------------------------------------------------
static void pack_weights_device(std::vector<torch::Tensor> params, int64_t K0, int64_t wdtype,
                                torch::Tensor blob) {
  const Entry a("dpvo_update.pack_weights_device");
  TORCH_CHECK(K0 >= 1 && K0 <= INT_MAX, "dpvo_update.pack_weights_device: bad corr_dim ", K0);
  void* bp = a.bytes(blob, "blob", blob.device());
  const auto ptrs = a.device_params(params, 50, param_numel(K0), blob.device(), "params");
  const DeviceGuard guard(blob.device());
  check_status(dpvo_update_pack_weights_device(ptrs.data(), 384, (int)K0, a.wdtype_code(wdtype),
                                               bp, (size_t)blob.numel(), current_stream()),
               "dpvo_update_pack_weights_device");
}

static int64_t saved_bytes(int64_t E, int64_t K0) {
  return (int64_t)dpvo_update_saved_bytes((int)E, (int)K0);
}

static int64_t backward_workspace_bytes(int64_t E, int64_t K0) {
  return (int64_t)dpvo_update_backward_workspace_bytes((int)E, (int)K0);
}

static void forward_train(torch::Tensor blob, torch::Tensor net, torch::Tensor inp,
                          torch::Tensor corr, torch::Tensor ix, torch::Tensor jx,
                          torch::Tensor workspace, torch::Tensor saved, torch::Tensor net_out,
                          torch::Tensor d, torch::Tensor w) {
  const Entry a("dpvo_update.forward_train");
  const void* np = a.buf<float>(net, "net");
  TORCH_CHECK(net.dim() == 2 && net.size(1) == 384,
              "dpvo_update.forward_train: net must be contiguous [E, 384]");
  const int64_t E = net.size(0);
  TORCH_CHECK(E <= INT_MAX, "dpvo_update.forward_train: too many edges");
  a.on_gpu(corr, "corr");
  TORCH_CHECK(corr.dim() == 2 && corr.size(0) == E && corr.size(1) >= 1,
              "dpvo_update.forward_train: corr must be [E, corr_dim]");
  const int64_t K0 = corr.size(1);
  const void* ip = rows(a, inp, net, E, 384, kF32, "inp");
  const void* cp = rows(a, corr, net, E, K0, kF32, "corr");
  void* op = rows(a, net_out, net, E, 384, kF32, "net_out");
  float* dp = (float*)rows(a, d, net, E, 2, kF32, "d");
  float* wp = (float*)rows(a, w, net, E, 2, kF32, "w");
  const int64_t* ixp = a.in<int64_t>(ix, "ix");
  const int64_t* jxp = a.in<int64_t>(jx, "jx");
  TORCH_CHECK(ix.numel() == E && jx.numel() == E,
              "dpvo_update.forward_train: ix, jx must have E elements");
  a.same_device({net, ix, jx});
  const void* bp = a.bytes(blob, "blob (packed as float32 for this corr_dim)", net.device(),
                           dpvo_update_packed_bytes((int)K0, DPVO_F32), true);
  void* ws = a.bytes(workspace, "workspace", net.device());
  void* sv = a.bytes(saved, "saved", net.device());
  const DeviceGuard guard(net.device());
  check_status(dpvo_update_forward_train(bp, DPVO_F32, np, ip, cp, ixp, jxp, (int)E, 384, (int)K0,
                                         DPVO_F32, ws, (size_t)workspace.numel(), sv,
                                         (size_t)saved.numel(), op, dp, wp, current_stream()),
               "dpvo_update_forward_train");
}

// uint8 [6, E, 384]
static torch::Tensor relu_masks(torch::Tensor saved, int64_t E, int64_t K0) {
  const Entry a("dpvo_update.relu_masks");
  const void* sv = a.bytes(saved, "saved", saved.device());
  TORCH_CHECK(E >= 0 && E <= INT_MAX && K0 >= 1 && K0 <= INT_MAX, "dpvo_update.relu_masks: bad sizes");
  const DeviceGuard guard(saved.device());
  auto out = torch::empty({6, E, 384}, torch::dtype(torch::kUInt8).device(saved.device()));
  check_status(dpvo_update_saved_relu_masks(sv, (size_t)saved.numel(), (int)E, (int)K0,
                                            out.data_ptr<uint8_t>(), current_stream()),
               "dpvo_update_saved_relu_masks");
  return out;
}

// cotangents and input gradients are optional (None); grads: 50 tensors or an
// empty list (no parameter gradient wanted)
static void backward(std::vector<torch::Tensor> params, torch::Tensor saved, torch::Tensor ix,
                     torch::Tensor jx, int64_t K0, c10::optional<torch::Tensor> g_net_out,
                     c10::optional<torch::Tensor> g_d, c10::optional<torch::Tensor> g_w,
                     c10::optional<torch::Tensor> g_net, c10::optional<torch::Tensor> g_inp,
                     c10::optional<torch::Tensor> g_corr, std::vector<torch::Tensor> grads,
                     torch::Tensor workspace) {
  const Entry a("dpvo_update.backward");
  const int64_t* ixp = a.in<int64_t>(ix, "ix");
  const int64_t* jxp = a.in<int64_t>(jx, "jx");
  const int64_t E = ix.numel();
  TORCH_CHECK(jx.numel() == E && jx.device() == ix.device() && E <= INT_MAX,
              "dpvo_update.backward: ix, jx must have E elements on one device");
  TORCH_CHECK(K0 >= 1 && K0 <= INT_MAX, "dpvo_update.backward: bad corr_dim ", K0);
  const auto pp = a.device_params(params, 50, param_numel(K0), ix.device(), "params");
  std::vector<float*> gp;
  if (!grads.empty()) gp = a.device_params(grads, 50, param_numel(K0), ix.device(), "grads");
  const void* sv = a.bytes(saved, "saved", ix.device());
  void* ws = a.bytes(workspace, "workspace", ix.device());
  auto opt = [&](const c10::optional<torch::Tensor>& t, int64_t cols, const char* name) -> float* {
    return t.has_value() ? (float*)rows(a, *t, ix, E, cols, kF32, name) : nullptr;
  };
  float* gno = opt(g_net_out, 384, "g_net_out");
  float* gd = opt(g_d, 2, "g_d");
  float* gw = opt(g_w, 2, "g_w");
  float* gn = opt(g_net, 384, "g_net");
  float* gi = opt(g_inp, 384, "g_inp");
  float* gc = opt(g_corr, K0, "g_corr");
  const DeviceGuard guard(ix.device());
  check_status(dpvo_update_backward(pp.data(), 384, (int)K0, sv, (size_t)saved.numel(), ixp, jxp,
                                    (int)E, gno, gd, gw, gn, gi, gc,
                                    gp.empty() ? nullptr : gp.data(), ws,
                                    (size_t)workspace.numel(), current_stream()),
               "dpvo_update_backward");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.attr("F32") = (int)DPVO_F32;
  m.attr("F16") = (int)DPVO_F16;
  m.def("packed_bytes", &packed_bytes, "bytes of the packed weight blob");
  m.def("pack_weights", &pack_weights, "pack Update's 50 parameter tensors (host)");
  m.def("workspace_bytes", &workspace_bytes, "bytes of the device workspace");
  m.def("plan", &plan, "group plan of the two aggregations");
  m.def("forward", &forward, "update operator forward");
  m.def("pack_weights_device", &pack_weights_device, "pack the 50 device parameter tensors");
  m.def("saved_bytes", &saved_bytes, "bytes of forward_train's saved buffer");
  m.def("forward_train", &forward_train, "forward that keeps what the backward needs");
  m.def("relu_masks", &relu_masks, "the six ReLU masks of a training forward, uint8 [6, E, 384]");
  m.def("backward_workspace_bytes", &backward_workspace_bytes, "bytes of the backward's workspace");
  m.def("backward", &backward, "update operator backward");
}
