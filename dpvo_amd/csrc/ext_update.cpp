// ext_update.cpp -- the `dpvo_update` extension module: DPVO's update operator
// (dpvo/net.py:175-339) bound to the dpvo_update_* C ABI of dpvo_hot.h.  The
// reference has no extension for it (it is PyTorch there); dpvo_amd/net.py is
// the nn.Module on top.
#include <climits>
#include <vector>

#include "ext_common.hpp"

using namespace dpvo_ext;

static int wdtype_code(int64_t code) {
  TORCH_CHECK(code == DPVO_F32 || code == DPVO_F16, "dpvo_update: weights are float32 or float16");
  return (int)code;
}

static int64_t packed_bytes(int64_t K0, int64_t wdtype) {
  return (int64_t)dpvo_update_packed_bytes((int)K0, wdtype_code(wdtype));
}

// 50 CPU float32 tensors in state_dict order -> packed host blob (uint8)
static torch::Tensor pack_weights(std::vector<torch::Tensor> tensors, int64_t K0, int64_t wdtype) {
  TORCH_CHECK(tensors.size() == 50, "dpvo_update.pack_weights: expected the 50 parameter tensors of "
                                    "Update, got ", tensors.size());
  TORCH_CHECK(K0 >= 1 && K0 <= INT_MAX, "dpvo_update.pack_weights: bad corr_dim ", K0);
  std::vector<const float*> ptrs;
  for (size_t i = 0; i < tensors.size(); i++) {
    auto& t = tensors[i];
    TORCH_CHECK(!t.is_cuda(), "dpvo_update.pack_weights: tensor ", i, " must be a CPU tensor");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "dpvo_update.pack_weights: tensor ", i,
                " must be float32");
    t = t.contiguous();
    const int64_t want = (i % 2 == 0 && i != 8 && i != 22 && i != 30 && i != 42)
                             ? (i == 38 ? 384 * K0 : (i >= 46 ? 2 * 384 : 384 * 384))
                             : (i == 47 || i == 49 ? 2 : 384);
    TORCH_CHECK(t.numel() == want, "dpvo_update.pack_weights: tensor ", i, " has ", t.numel(),
                " elements, expected ", want);
    ptrs.push_back(t.data_ptr<float>());
  }
  const int wd = wdtype_code(wdtype);
  const size_t bytes = dpvo_update_packed_bytes((int)K0, wd);
  auto blob = torch::empty({(int64_t)bytes}, torch::dtype(torch::kUInt8));
  check_status(dpvo_update_pack_weights(ptrs.data(), 50, 384, (int)K0, wd, blob.data_ptr(), bytes),
               "dpvo_update_pack_weights");
  return blob;
}

static int64_t workspace_bytes(int64_t E, int64_t K0) {
  return (int64_t)dpvo_update_workspace_bytes((int)E, (int)K0);
}

static void check_ws(const torch::Tensor& ws, const torch::Tensor& like) {
  check_device(ws, "workspace");
  TORCH_CHECK(ws.device() == like.device(), "dpvo_update: workspace is on another device");
  TORCH_CHECK(ws.scalar_type() == torch::kUInt8 && ws.is_contiguous(),
              "dpvo_update: workspace must be a contiguous uint8 tensor");
}

static void plan(torch::Tensor gk, torch::Tensor gij, torch::Tensor workspace) {
  gk = idx64(gk, "gk");
  gij = idx64(gij, "gij");
  TORCH_CHECK(gk.dim() == 1 && gij.dim() == 1 && gk.numel() == gij.numel(),
              "dpvo_update.plan: gk and gij must be 1-D of one length");
  TORCH_CHECK(gij.device() == gk.device(), "dpvo_update.plan: gij is not on gk's device");
  TORCH_CHECK(gk.numel() <= INT_MAX, "dpvo_update.plan: too many edges");
  check_ws(workspace, gk);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(gk.device());
  check_status(dpvo_update_plan(gk.data_ptr<int64_t>(), gij.data_ptr<int64_t>(), (int)gk.numel(),
                                workspace.data_ptr(), (size_t)workspace.numel(), current_stream()),
               "dpvo_update_plan");
}

static void forward(torch::Tensor blob, int64_t wdtype, torch::Tensor net, torch::Tensor inp,
                    torch::Tensor corr, torch::Tensor ix, torch::Tensor jx, torch::Tensor workspace,
                    torch::Tensor net_out, torch::Tensor d, torch::Tensor w) {
  check_device(net, "net");
  const int wd = wdtype_code(wdtype);
  const int io = dtype_code(net);
  TORCH_CHECK(io == DPVO_F32 || (io == DPVO_F16 && wd == DPVO_F16),
              "dpvo_update.forward: net/inp/corr are float32, or float16 with float16 weights");
  TORCH_CHECK(net.dim() == 2 && net.size(1) == 384, "dpvo_update.forward: net must be [E, 384]");
  const int64_t E = net.size(0);
  TORCH_CHECK(E <= INT_MAX, "dpvo_update.forward: too many edges");
  TORCH_CHECK(corr.dim() == 2 && corr.size(0) == E && corr.size(1) >= 1,
              "dpvo_update.forward: corr must be [E, corr_dim]");
  const int64_t K0 = corr.size(1);
  const torch::Tensor* same[] = {&inp, &corr, &net_out};
  const char* names[] = {"inp", "corr", "net_out"};
  for (int i = 0; i < 3; i++) {
    check_device(*same[i], names[i]);
    TORCH_CHECK(same[i]->device() == net.device(), "dpvo_update.forward: ", names[i],
                " is not on net's device");
    TORCH_CHECK(same[i]->scalar_type() == net.scalar_type(), "dpvo_update.forward: ", names[i],
                " dtype differs from net's");
    TORCH_CHECK(same[i]->is_contiguous(), "dpvo_update.forward: ", names[i], " must be contiguous");
  }
  TORCH_CHECK(net.is_contiguous(), "dpvo_update.forward: net must be contiguous");
  TORCH_CHECK(inp.sizes() == net.sizes() && net_out.sizes() == net.sizes(),
              "dpvo_update.forward: inp and net_out must have net's shape");
  ix = idx64(ix, "ix");
  jx = idx64(jx, "jx");
  TORCH_CHECK(ix.numel() == E && jx.numel() == E, "dpvo_update.forward: ix, jx must have E elements");
  TORCH_CHECK(ix.device() == net.device() && jx.device() == net.device(),
              "dpvo_update.forward: ix / jx are not on net's device");
  const torch::Tensor* outs[] = {&d, &w};
  for (auto* o : outs) {
    check_device(*o, "d / w");
    TORCH_CHECK(o->device() == net.device() && o->scalar_type() == torch::kFloat32 &&
                    o->is_contiguous() && o->numel() == 2 * E,
                "dpvo_update.forward: d and w must be contiguous float32 [E, 2] on net's device");
  }
  check_device(blob, "blob");
  TORCH_CHECK(blob.device() == net.device() && blob.scalar_type() == torch::kUInt8 &&
                  blob.is_contiguous(),
              "dpvo_update.forward: blob must be a contiguous uint8 tensor on net's device");
  TORCH_CHECK((size_t)blob.numel() == dpvo_update_packed_bytes((int)K0, wd),
              "dpvo_update.forward: blob was not packed for corr_dim ", K0, " and this weight dtype");
  check_ws(workspace, net);
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(net.device());
  check_status(dpvo_update_forward(blob.data_ptr(), wd, net.data_ptr(), inp.data_ptr(),
                                   corr.data_ptr(), ix.data_ptr<int64_t>(), jx.data_ptr<int64_t>(),
                                   (int)E, 384, (int)K0, io, workspace.data_ptr(),
                                   (size_t)workspace.numel(), net_out.data_ptr(),
                                   d.data_ptr<float>(), w.data_ptr<float>(), current_stream()),
               "dpvo_update_forward");
}

// --- the training surface ------------------------------------------------------------
static int64_t param_numel(size_t i, int64_t K0) {
  return (i % 2 == 0 && i != 8 && i != 22 && i != 30 && i != 42)
             ? (i == 38 ? 384 * K0 : (i >= 46 ? 2 * 384 : 384 * 384))
             : (i == 47 || i == 49 ? 2 : 384);
}

// 50 contiguous float32 device tensors of Update's shapes -> their data pointers
static std::vector<float*> device_params(const std::vector<torch::Tensor>& ts, int64_t K0,
                                         const torch::Device& dev, const char* what) {
  TORCH_CHECK(ts.size() == 50, "dpvo_update: ", what, ": expected 50 tensors, got ", ts.size());
  std::vector<float*> ptrs;
  for (size_t i = 0; i < ts.size(); i++) {
    const auto& t = ts[i];
    check_device(t, what);
    TORCH_CHECK(t.device() == dev, "dpvo_update: ", what, " ", i, " is on another device");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous(), "dpvo_update: ", what, " ",
                i, " must be contiguous float32");
    TORCH_CHECK(t.numel() == param_numel(i, K0), "dpvo_update: ", what, " ", i, " has ", t.numel(),
                " elements, expected ", param_numel(i, K0));
    ptrs.push_back(t.data_ptr<float>());
  }
  return ptrs;
}

static void check_bytes(const torch::Tensor& t, const torch::Tensor& like, const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.device() == like.device() && t.scalar_type() == torch::kUInt8 && t.is_contiguous(),
              "dpvo_update: ", name, " must be a contiguous uint8 tensor on the inputs' device");
}

static void check_rows(const torch::Tensor& t, const torch::Tensor& like, int64_t E, int64_t cols,
                       const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.device() == like.device() && t.scalar_type() == torch::kFloat32 &&
                  t.is_contiguous() && t.numel() == E * cols,
              "dpvo_update: ", name, " must be contiguous float32 [E, ", cols,
              "] on the inputs' device");
}

static void pack_weights_device(std::vector<torch::Tensor> params, int64_t K0, int64_t wdtype,
                                torch::Tensor blob) {
  TORCH_CHECK(K0 >= 1 && K0 <= INT_MAX, "dpvo_update.pack_weights_device: bad corr_dim ", K0);
  check_device(blob, "blob");
  const auto ptrs = device_params(params, K0, blob.device(), "params");
  TORCH_CHECK(blob.scalar_type() == torch::kUInt8 && blob.is_contiguous(),
              "dpvo_update.pack_weights_device: blob must be a contiguous uint8 tensor");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(blob.device());
  check_status(dpvo_update_pack_weights_device(ptrs.data(), 384, (int)K0, wdtype_code(wdtype),
                                               blob.data_ptr(), (size_t)blob.numel(),
                                               current_stream()),
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
  check_device(net, "net");
  TORCH_CHECK(net.scalar_type() == torch::kFloat32, "dpvo_update.forward_train: float32 only");
  TORCH_CHECK(net.dim() == 2 && net.size(1) == 384 && net.is_contiguous(),
              "dpvo_update.forward_train: net must be contiguous [E, 384]");
  const int64_t E = net.size(0);
  TORCH_CHECK(E <= INT_MAX, "dpvo_update.forward_train: too many edges");
  TORCH_CHECK(corr.dim() == 2 && corr.size(0) == E && corr.size(1) >= 1,
              "dpvo_update.forward_train: corr must be [E, corr_dim]");
  const int64_t K0 = corr.size(1);
  check_rows(inp, net, E, 384, "inp");
  check_rows(corr, net, E, K0, "corr");
  check_rows(net_out, net, E, 384, "net_out");
  check_rows(d, net, E, 2, "d");
  check_rows(w, net, E, 2, "w");
  ix = idx64(ix, "ix");
  jx = idx64(jx, "jx");
  TORCH_CHECK(ix.numel() == E && jx.numel() == E && ix.device() == net.device() &&
                  jx.device() == net.device(),
              "dpvo_update.forward_train: ix, jx must have E elements on net's device");
  check_bytes(blob, net, "blob");
  TORCH_CHECK((size_t)blob.numel() == dpvo_update_packed_bytes((int)K0, DPVO_F32),
              "dpvo_update.forward_train: blob was not packed as float32 for corr_dim ", K0);
  check_ws(workspace, net);
  check_bytes(saved, net, "saved");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(net.device());
  check_status(dpvo_update_forward_train(
                   blob.data_ptr(), DPVO_F32, net.data_ptr(), inp.data_ptr(), corr.data_ptr(),
                   ix.data_ptr<int64_t>(), jx.data_ptr<int64_t>(), (int)E, 384, (int)K0, DPVO_F32,
                   workspace.data_ptr(), (size_t)workspace.numel(), saved.data_ptr(),
                   (size_t)saved.numel(), net_out.data_ptr(), d.data_ptr<float>(),
                   w.data_ptr<float>(), current_stream()),
               "dpvo_update_forward_train");
}

// uint8 [6, E, 384]
static torch::Tensor relu_masks(torch::Tensor saved, int64_t E, int64_t K0) {
  check_device(saved, "saved");
  TORCH_CHECK(saved.scalar_type() == torch::kUInt8 && saved.is_contiguous(),
              "dpvo_update.relu_masks: saved must be a contiguous uint8 tensor");
  TORCH_CHECK(E >= 0 && E <= INT_MAX && K0 >= 1 && K0 <= INT_MAX, "dpvo_update.relu_masks: bad sizes");
  auto out = torch::empty({6, E, 384}, torch::dtype(torch::kUInt8).device(saved.device()));
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(saved.device());
  check_status(dpvo_update_saved_relu_masks(saved.data_ptr(), (size_t)saved.numel(), (int)E, (int)K0,
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
  ix = idx64(ix, "ix");
  jx = idx64(jx, "jx");
  const int64_t E = ix.numel();
  TORCH_CHECK(jx.numel() == E && jx.device() == ix.device() && E <= INT_MAX,
              "dpvo_update.backward: ix, jx must have E elements on one device");
  TORCH_CHECK(K0 >= 1 && K0 <= INT_MAX, "dpvo_update.backward: bad corr_dim ", K0);
  const auto pp = device_params(params, K0, ix.device(), "params");
  std::vector<float*> gp;
  if (!grads.empty()) gp = device_params(grads, K0, ix.device(), "grads");
  check_bytes(saved, ix, "saved");
  check_bytes(workspace, ix, "workspace");
  auto opt = [&](const c10::optional<torch::Tensor>& t, int64_t cols, const char* name) -> float* {
    if (!t.has_value()) return nullptr;
    check_rows(*t, ix, E, cols, name);
    return t->data_ptr<float>();
  };
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ix.device());
  check_status(dpvo_update_backward(
                   pp.data(), 384, (int)K0, saved.data_ptr(), (size_t)saved.numel(),
                   ix.data_ptr<int64_t>(), jx.data_ptr<int64_t>(), (int)E,
                   opt(g_net_out, 384, "g_net_out"), opt(g_d, 2, "g_d"), opt(g_w, 2, "g_w"),
                   opt(g_net, 384, "g_net"), opt(g_inp, 384, "g_inp"), opt(g_corr, K0, "g_corr"),
                   gp.empty() ? nullptr : gp.data(), workspace.data_ptr(),
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
