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

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.attr("F32") = (int)DPVO_F32;
  m.attr("F16") = (int)DPVO_F16;
  m.def("packed_bytes", &packed_bytes, "bytes of the packed weight blob");
  m.def("pack_weights", &pack_weights, "pack Update's 50 parameter tensors (host)");
  m.def("workspace_bytes", &workspace_bytes, "bytes of the device workspace");
  m.def("plan", &plan, "group plan of the two aggregations");
  m.def("forward", &forward, "update operator forward");
}
