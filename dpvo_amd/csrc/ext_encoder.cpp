// ext_encoder.cpp -- the `dpvo_encoder` extension module: DPVO's feature
// encoders (dpvo/extractor.py:200-264, BasicEncoder4) bound to the
// dpvo_encoder_* C ABI of dpvo_hot.h.  The reference has no extension for them
// (they are PyTorch there); dpvo_amd/extractor.py is the nn.Module on top.
#include <climits>
#include <vector>

#include "ext_common.hpp"

using namespace dpvo_ext;

static int wdtype_code(int64_t code) {
  TORCH_CHECK(code == DPVO_F32 || code == DPVO_F16, "dpvo_encoder: weights are float32 or float16");
  return (int)code;
}

static int norm_code(int64_t code) {
  TORCH_CHECK(code == DPVO_ENCODER_NORM_NONE || code == DPVO_ENCODER_NORM_INSTANCE,
              "dpvo_encoder: norm is NORM_NONE or NORM_INSTANCE");
  return (int)code;
}

static int out_dim_code(int64_t out_dim, int wd) {
  TORCH_CHECK(out_dim >= 1 && out_dim <= INT_MAX && dpvo_encoder_packed_bytes((int)out_dim, wd) > 0,
              "dpvo_encoder: output dim ", out_dim, " is not a multiple of 64 in [64, 1024]");
  return (int)out_dim;
}

static int64_t packed_bytes(int64_t out_dim, int64_t wdtype) {
  return (int64_t)dpvo_encoder_packed_bytes((int)out_dim, wdtype_code(wdtype));
}

static int64_t down(int64_t n) { return (n - 1) / 2 + 1; }

// 22 CPU float32 tensors in state_dict order -> packed host blob (uint8)
static torch::Tensor pack_weights(std::vector<torch::Tensor> tensors, int64_t out_dim, int64_t norm,
                                  int64_t wdtype) {
  TORCH_CHECK(tensors.size() == 22, "dpvo_encoder.pack_weights: expected the 22 parameter tensors "
                                    "of BasicEncoder4, got ", tensors.size());
  const int wd = wdtype_code(wdtype);
  const int od = out_dim_code(out_dim, wd);
  // (cout, cin, k) of the eleven convolutions in state_dict order
  const int64_t shape[11][3] = {{32, 3, 7},  {32, 32, 3}, {32, 32, 3}, {32, 32, 3},
                                {32, 32, 3}, {64, 32, 3}, {64, 64, 3}, {64, 32, 1},
                                {64, 64, 3}, {64, 64, 3}, {od, 64, 1}};
  std::vector<const float*> ptrs;
  for (size_t i = 0; i < tensors.size(); i++) {
    auto& t = tensors[i];
    TORCH_CHECK(!t.is_cuda(), "dpvo_encoder.pack_weights: tensor ", i, " must be a CPU tensor");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "dpvo_encoder.pack_weights: tensor ", i,
                " must be float32");
    t = t.contiguous();
    const int64_t* s = shape[i / 2];
    const int64_t want = i % 2 ? s[0] : s[0] * s[1] * s[2] * s[2];
    TORCH_CHECK(t.numel() == want, "dpvo_encoder.pack_weights: tensor ", i, " has ", t.numel(),
                " elements, expected ", want);
    ptrs.push_back(t.data_ptr<float>());
  }
  const size_t bytes = dpvo_encoder_packed_bytes(od, wd);
  auto blob = torch::empty({(int64_t)bytes}, torch::dtype(torch::kUInt8));
  check_status(dpvo_encoder_pack_weights(ptrs.data(), 22, od, norm_code(norm), wd, blob.data_ptr(),
                                         bytes),
               "dpvo_encoder_pack_weights");
  return blob;
}

static int64_t workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t out_dim) {
  TORCH_CHECK(n <= INT_MAX && H <= INT_MAX && W <= INT_MAX && out_dim <= INT_MAX,
              "dpvo_encoder.workspace_bytes: size out of range");
  return (int64_t)dpvo_encoder_workspace_bytes((int)n, (int)H, (int)W, (int)out_dim);
}

// images [n, 3, H, W] float32 contiguous -> out [n, out_dim, h, w] float32,
// contiguous or channels-last (torch.channels_last strides)
static void forward(torch::Tensor blob, int64_t wdtype, int64_t norm, torch::Tensor images,
                    torch::Tensor out, torch::Tensor workspace) {
  check_device(images, "images");
  const int wd = wdtype_code(wdtype);
  TORCH_CHECK(images.scalar_type() == torch::kFloat32 && images.dim() == 4 && images.size(1) == 3 &&
                  images.is_contiguous(),
              "dpvo_encoder.forward: images must be contiguous float32 [n, 3, H, W]");
  const int64_t n = images.size(0), H = images.size(2), W = images.size(3);
  TORCH_CHECK(n >= 1 && H >= 1 && W >= 1 && n <= INT_MAX && H <= INT_MAX && W <= INT_MAX,
              "dpvo_encoder.forward: empty or oversized images");
  check_device(out, "out");
  TORCH_CHECK(out.device() == images.device() && out.scalar_type() == torch::kFloat32 &&
                  out.dim() == 4 && out.size(0) == n && out.size(2) == down(down(H)) &&
                  out.size(3) == down(down(W)),
              "dpvo_encoder.forward: out must be float32 [n, out_dim, h, w] on the images' device");
  const int od = out_dim_code(out.size(1), wd);
  int layout;
  if (out.is_contiguous()) layout = DPVO_ENCODER_NCHW;
  else if (out.is_contiguous(at::MemoryFormat::ChannelsLast)) layout = DPVO_ENCODER_NHWC;
  else TORCH_CHECK(false, "dpvo_encoder.forward: out must be contiguous or channels-last");
  check_device(blob, "blob");
  TORCH_CHECK(blob.device() == images.device() && blob.scalar_type() == torch::kUInt8 &&
                  blob.is_contiguous(),
              "dpvo_encoder.forward: blob must be a contiguous uint8 tensor on the images' device");
  TORCH_CHECK((size_t)blob.numel() == dpvo_encoder_packed_bytes(od, wd),
              "dpvo_encoder.forward: blob was not packed for output dim ", od,
              " and this weight dtype");
  check_device(workspace, "workspace");
  TORCH_CHECK(workspace.device() == images.device() && workspace.scalar_type() == torch::kUInt8 &&
                  workspace.is_contiguous(),
              "dpvo_encoder.forward: workspace must be a contiguous uint8 tensor on the images' "
              "device");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(images.device());
  check_status(dpvo_encoder_forward(blob.data_ptr(), wd, norm_code(norm), od,
                                    images.data_ptr<float>(), (int)n, (int)H, (int)W,
                                    out.data_ptr<float>(), layout, workspace.data_ptr(),
                                    (size_t)workspace.numel(), current_stream()),
               "dpvo_encoder_forward");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.attr("F32") = (int)DPVO_F32;
  m.attr("F16") = (int)DPVO_F16;
  m.attr("NORM_NONE") = (int)DPVO_ENCODER_NORM_NONE;
  m.attr("NORM_INSTANCE") = (int)DPVO_ENCODER_NORM_INSTANCE;
  m.def("packed_bytes", &packed_bytes, "bytes of the packed weight blob");
  m.def("pack_weights", &pack_weights, "pack BasicEncoder4's 22 parameter tensors (host)");
  m.def("workspace_bytes", &workspace_bytes, "bytes of the device workspace");
  m.def("forward", &forward, "encoder forward");
}
