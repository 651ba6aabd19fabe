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

// (cout, cin, k) of the eleven convolutions in state_dict order
static void conv_dims(int od, int64_t shape[11][3]) {
  const int64_t s[11][3] = {{32, 3, 7},  {32, 32, 3}, {32, 32, 3}, {32, 32, 3},
                            {32, 32, 3}, {64, 32, 3}, {64, 64, 3}, {64, 32, 1},
                            {64, 64, 3}, {64, 64, 3}, {od, 64, 1}};
  for (int i = 0; i < 11; i++)
    for (int j = 0; j < 3; j++) shape[i][j] = s[i][j];
}

// 22 device float32 tensors in state_dict order, contiguous, of the encoder's sizes
static std::vector<const float*> device_params(const std::vector<torch::Tensor>& tensors, int od,
                                               const torch::Device& dev, const char* fn,
                                               const char* what) {
  TORCH_CHECK(tensors.size() == 22, "dpvo_encoder.", fn, ": expected 22 ", what, " tensors, got ",
              tensors.size());
  int64_t shape[11][3];
  conv_dims(od, shape);
  std::vector<const float*> ptrs;
  for (size_t i = 0; i < tensors.size(); i++) {
    const auto& t = tensors[i];
    check_device(t, what);
    const int64_t* s = shape[i / 2];
    const int64_t want = i % 2 ? s[0] : s[0] * s[1] * s[2] * s[2];
    TORCH_CHECK(t.device() == dev && t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
                    t.numel() == want,
                "dpvo_encoder.", fn, ": ", what, " tensor ", i, " must be contiguous float32 with ",
                want, " elements on the images' device");
    ptrs.push_back(t.data_ptr<float>());
  }
  return ptrs;
}

static void check_bytes(const torch::Tensor& t, const torch::Device& dev, const char* fn,
                        const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.device() == dev && t.scalar_type() == torch::kUInt8 && t.is_contiguous(),
              "dpvo_encoder.", fn, ": ", name, " must be a contiguous uint8 tensor on the images' "
              "device");
}

static void check_images(const torch::Tensor& images, const char* fn) {
  check_device(images, "images");
  TORCH_CHECK(images.scalar_type() == torch::kFloat32 && images.dim() == 4 && images.size(1) == 3 &&
                  images.is_contiguous(),
              "dpvo_encoder.", fn, ": images must be contiguous float32 [n, 3, H, W]");
  TORCH_CHECK(images.size(0) >= 1 && images.size(2) >= 1 && images.size(3) >= 1 &&
                  images.size(0) <= INT_MAX && images.size(2) <= INT_MAX && images.size(3) <= INT_MAX,
              "dpvo_encoder.", fn, ": empty or oversized images");
}

// t [n, C, h, w] float32 on the images' device -> its layout code
static int check_map(const torch::Tensor& t, const torch::Tensor& images, const char* fn,
                     const char* name) {
  check_device(t, name);
  TORCH_CHECK(t.device() == images.device() && t.scalar_type() == torch::kFloat32 && t.dim() == 4 &&
                  t.size(0) == images.size(0) && t.size(2) == down(down(images.size(2))) &&
                  t.size(3) == down(down(images.size(3))),
              "dpvo_encoder.", fn, ": ", name, " must be float32 [n, out_dim, h, w] on the images' "
              "device");
  if (t.is_contiguous()) return DPVO_ENCODER_NCHW;
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), "dpvo_encoder.", fn, ": ", name,
              " must be contiguous or channels-last");
  return DPVO_ENCODER_NHWC;
}

// 22 device float32 tensors -> the packed device blob (uint8), one launch
static void pack_weights_device(std::vector<torch::Tensor> params, int64_t out_dim, int64_t norm,
                                int64_t wdtype, torch::Tensor blob) {
  const int wd = wdtype_code(wdtype);
  const int od = out_dim_code(out_dim, wd);
  check_device(blob, "blob");
  const auto ptrs = device_params(params, od, blob.device(), "pack_weights_device", "parameter");
  check_bytes(blob, blob.device(), "pack_weights_device", "blob");
  TORCH_CHECK((size_t)blob.numel() == dpvo_encoder_packed_bytes(od, wd),
              "dpvo_encoder.pack_weights_device: blob must have packed_bytes(out_dim, wdtype) bytes");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(blob.device());
  check_status(dpvo_encoder_pack_weights_device(ptrs.data(), od, norm_code(norm), wd,
                                                blob.data_ptr(), (size_t)blob.numel(),
                                                current_stream()),
               "dpvo_encoder_pack_weights_device");
}

static int64_t saved_bytes(int64_t n, int64_t H, int64_t W, int64_t out_dim, int64_t norm) {
  TORCH_CHECK(n <= INT_MAX && H <= INT_MAX && W <= INT_MAX && out_dim <= INT_MAX,
              "dpvo_encoder.saved_bytes: size out of range");
  return (int64_t)dpvo_encoder_saved_bytes((int)n, (int)H, (int)W, (int)out_dim, norm_code(norm));
}

static int64_t backward_workspace_bytes(int64_t n, int64_t H, int64_t W, int64_t out_dim) {
  TORCH_CHECK(n <= INT_MAX && H <= INT_MAX && W <= INT_MAX && out_dim <= INT_MAX,
              "dpvo_encoder.backward_workspace_bytes: size out of range");
  return (int64_t)dpvo_encoder_backward_workspace_bytes((int)n, (int)H, (int)W, (int)out_dim);
}

// forward with every plane the backward needs kept in `saved`
static void forward_train(torch::Tensor blob, int64_t wdtype, int64_t norm, torch::Tensor images,
                          torch::Tensor out, torch::Tensor saved) {
  check_images(images, "forward_train");
  const int wd = wdtype_code(wdtype);
  const int nc = norm_code(norm);
  const int64_t n = images.size(0), H = images.size(2), W = images.size(3);
  const int layout = check_map(out, images, "forward_train", "out");
  const int od = out_dim_code(out.size(1), wd);
  check_bytes(blob, images.device(), "forward_train", "blob");
  TORCH_CHECK((size_t)blob.numel() == dpvo_encoder_packed_bytes(od, wd),
              "dpvo_encoder.forward_train: blob was not packed for output dim ", od,
              " and this weight dtype");
  check_bytes(saved, images.device(), "forward_train", "saved");
  const size_t need = dpvo_encoder_saved_bytes((int)n, (int)H, (int)W, od, nc);
  TORCH_CHECK(need > 0 && (size_t)saved.numel() >= need,
              "dpvo_encoder.forward_train: saved must have saved_bytes(n, H, W, out_dim, norm) bytes");
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(images.device());
  check_status(dpvo_encoder_forward_train(blob.data_ptr(), wd, nc, od, images.data_ptr<float>(),
                                          (int)n, (int)H, (int)W, out.data_ptr<float>(), layout,
                                          saved.data_ptr(), (size_t)saved.numel(), current_stream()),
               "dpvo_encoder_forward_train");
}

// the 22 parameter gradients (overwritten) from `saved` and the cotangent of out
static void backward(int64_t norm, std::vector<torch::Tensor> params, torch::Tensor images,
                     torch::Tensor saved, torch::Tensor grad_out, std::vector<torch::Tensor> grads,
                     torch::Tensor workspace) {
  check_images(images, "backward");
  const int nc = norm_code(norm);
  const int64_t n = images.size(0), H = images.size(2), W = images.size(3);
  const int layout = check_map(grad_out, images, "backward", "grad_out");
  const int od = out_dim_code(grad_out.size(1), DPVO_F32);
  const auto pp = device_params(params, od, images.device(), "backward", "parameter");
  const auto gp = device_params(grads, od, images.device(), "backward", "gradient");
  check_bytes(saved, images.device(), "backward", "saved");
  const size_t sneed = dpvo_encoder_saved_bytes((int)n, (int)H, (int)W, od, nc);
  TORCH_CHECK(sneed > 0 && (size_t)saved.numel() >= sneed,
              "dpvo_encoder.backward: saved must have saved_bytes(n, H, W, out_dim, norm) bytes");
  check_bytes(workspace, images.device(), "backward", "workspace");
  const size_t wneed = dpvo_encoder_backward_workspace_bytes((int)n, (int)H, (int)W, od);
  TORCH_CHECK(wneed > 0 && (size_t)workspace.numel() >= wneed,
              "dpvo_encoder.backward: workspace must have backward_workspace_bytes(n, H, W, "
              "out_dim) bytes");
  std::vector<float*> gw;
  for (const float* g : gp) gw.push_back(const_cast<float*>(g));
  const c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(images.device());
  check_status(dpvo_encoder_backward(nc, od, pp.data(), images.data_ptr<float>(), (int)n, (int)H,
                                     (int)W, saved.data_ptr(), grad_out.data_ptr<float>(), layout,
                                     gw.data(), workspace.data_ptr(), (size_t)workspace.numel(),
                                     current_stream()),
               "dpvo_encoder_backward");
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
  m.def("pack_weights_device", &pack_weights_device,
        "pack BasicEncoder4's 22 device parameter tensors into a device blob");
  m.def("saved_bytes", &saved_bytes, "bytes of forward_train's saved buffer");
  m.def("forward_train", &forward_train, "encoder forward that keeps what the backward needs");
  m.def("backward_workspace_bytes", &backward_workspace_bytes, "bytes of the backward's workspace");
  m.def("backward", &backward, "gradients of the 22 parameters");
}
