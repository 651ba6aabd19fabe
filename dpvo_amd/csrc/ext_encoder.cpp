// ext_encoder.cpp -- the `dpvo_encoder` extension module: DPVO's feature
// encoders (dpvo/extractor.py:200-264, BasicEncoder4) bound to the
// dpvo_encoder_* C ABI of dpvo_hot.h.  The reference has no extension for them
// (they are PyTorch there); dpvo_amd/extractor.py is the nn.Module on top.
#include <climits>
#include <vector>

#include "ext_common.hpp"

using namespace dpvo_ext;

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
  const int wd = Entry("dpvo_encoder.packed_bytes").wdtype_code(wdtype);
  return (int64_t)dpvo_encoder_packed_bytes((int)out_dim, wd);
}

static int64_t down(int64_t n) { return (n - 1) / 2 + 1; }

// element counts of BasicEncoder4's 22 parameter tensors in state_dict order:
// weight and bias of the eleven convolutions (cout, cin, k)
static std::function<int64_t(size_t)> param_numel(int od) {
  return [od](size_t i) -> int64_t {
    const int64_t shape[11][3] = {{32, 3, 7},  {32, 32, 3}, {32, 32, 3}, {32, 32, 3},
                                  {32, 32, 3}, {64, 32, 3}, {64, 64, 3}, {64, 32, 1},
                                  {64, 64, 3}, {64, 64, 3}, {od, 64, 1}};
    const int64_t* s = shape[i / 2];
    return i % 2 ? s[0] : s[0] * s[1] * s[2] * s[2];
  };
}

// 22 CPU float32 tensors in state_dict order -> packed host blob (uint8)
static torch::Tensor pack_weights(std::vector<torch::Tensor> tensors, int64_t out_dim, int64_t norm,
                                  int64_t wdtype) {
  const Entry a("dpvo_encoder.pack_weights");
  const int wd = a.wdtype_code(wdtype);
  const int od = out_dim_code(out_dim, wd);
  const auto ptrs = a.host_params(tensors, 22, param_numel(od));
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

// images: contiguous float32 [n, 3, H, W]
static const float* check_images(const Entry& a, const torch::Tensor& images) {
  const float* p = a.buf<float>(images, "images");
  TORCH_CHECK(images.dim() == 4 && images.size(1) == 3, a.fn(),
              ": images must be contiguous float32 [n, 3, H, W]");
  TORCH_CHECK(images.size(0) >= 1 && images.size(2) >= 1 && images.size(3) >= 1 &&
                  images.size(0) <= INT_MAX && images.size(2) <= INT_MAX && images.size(3) <= INT_MAX,
              a.fn(), ": empty or oversized images");
  return p;
}

// t [n, C, h, w] float32 on the images' device, contiguous or channels-last
// (torch.channels_last strides) -> its pointer and layout code
static float* check_map(const Entry& a, const torch::Tensor& t, const torch::Tensor& images,
                        const char* name, int* layout) {
  const float* p = a.view<float>(t, name);
  TORCH_CHECK(t.device() == images.device() && t.dim() == 4 && t.size(0) == images.size(0) &&
                  t.size(2) == down(down(images.size(2))) && t.size(3) == down(down(images.size(3))),
              a.fn(), ": ", name, " must be float32 [n, out_dim, h, w] on the images' device");
  *layout = t.is_contiguous() ? DPVO_ENCODER_NCHW : DPVO_ENCODER_NHWC;
  TORCH_CHECK(t.is_contiguous() || t.is_contiguous(at::MemoryFormat::ChannelsLast), a.fn(), ": ",
              name, " must be contiguous or channels-last");
  return const_cast<float*>(p);
}

// images [n, 3, H, W] float32 contiguous -> out [n, out_dim, h, w] float32
static void forward(torch::Tensor blob, int64_t wdtype, int64_t norm, torch::Tensor images,
                    torch::Tensor out, torch::Tensor workspace) {
  const Entry a("dpvo_encoder.forward");
  const int wd = a.wdtype_code(wdtype);
  const float* ip = check_images(a, images);
  const int64_t n = images.size(0), H = images.size(2), W = images.size(3);
  int layout;
  float* op = check_map(a, out, images, "out", &layout);
  const int od = out_dim_code(out.size(1), wd);
  const void* bp = a.bytes(blob, "blob (packed for this output dim and weight dtype)",
                           images.device(), dpvo_encoder_packed_bytes(od, wd), true);
  void* ws = a.bytes(workspace, "workspace", images.device());
  const DeviceGuard guard(images.device());
  check_status(dpvo_encoder_forward(bp, wd, norm_code(norm), od, ip, (int)n, (int)H, (int)W, op,
                                    layout, ws, (size_t)workspace.numel(), current_stream()),
               "dpvo_encoder_forward");
}

// 22 device float32 tensors -> the packed device blob (uint8), one launch
static void pack_weights_device(std::vector<torch::Tensor> params, int64_t out_dim, int64_t norm,
                                int64_t wdtype, torch::Tensor blob) {
  const Entry a("dpvo_encoder.pack_weights_device");
  const int wd = a.wdtype_code(wdtype);
  const int od = out_dim_code(out_dim, wd);
  void* bp = a.bytes(blob, "blob (packed_bytes(out_dim, wdtype) long)", blob.device(),
                     dpvo_encoder_packed_bytes(od, wd), true);
  const auto ptrs = a.device_params(params, 22, param_numel(od), blob.device(), "parameter");
  const DeviceGuard guard(blob.device());
  check_status(dpvo_encoder_pack_weights_device(ptrs.data(), od, norm_code(norm), wd, bp,
                                                (size_t)blob.numel(), current_stream()),
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
  const Entry a("dpvo_encoder.forward_train");
  const float* ip = check_images(a, images);
  const int wd = a.wdtype_code(wdtype);
  const int nc = norm_code(norm);
  const int64_t n = images.size(0), H = images.size(2), W = images.size(3);
  int layout;
  float* op = check_map(a, out, images, "out", &layout);
  const int od = out_dim_code(out.size(1), wd);
  const void* bp = a.bytes(blob, "blob (packed for this output dim and weight dtype)",
                           images.device(), dpvo_encoder_packed_bytes(od, wd), true);
  const size_t need = dpvo_encoder_saved_bytes((int)n, (int)H, (int)W, od, nc);
  TORCH_CHECK(need > 0, "dpvo_encoder.forward_train: unsupported sizes");
  void* sv = a.bytes(saved, "saved (saved_bytes(n, H, W, out_dim, norm) long)", images.device(),
                     need);
  const DeviceGuard guard(images.device());
  check_status(dpvo_encoder_forward_train(bp, wd, nc, od, ip, (int)n, (int)H, (int)W, op, layout,
                                          sv, (size_t)saved.numel(), current_stream()),
               "dpvo_encoder_forward_train");
}

// the 22 parameter gradients (overwritten) from `saved` and the cotangent of out
static void backward(int64_t norm, std::vector<torch::Tensor> params, torch::Tensor images,
                     torch::Tensor saved, torch::Tensor grad_out, std::vector<torch::Tensor> grads,
                     torch::Tensor workspace) {
  const Entry a("dpvo_encoder.backward");
  const float* ip = check_images(a, images);
  const int nc = norm_code(norm);
  const int64_t n = images.size(0), H = images.size(2), W = images.size(3);
  int layout;
  const float* gop = check_map(a, grad_out, images, "grad_out", &layout);
  const int od = out_dim_code(grad_out.size(1), DPVO_F32);
  const auto pp = a.device_params(params, 22, param_numel(od), images.device(), "parameter");
  const auto gp = a.device_params(grads, 22, param_numel(od), images.device(), "gradient");
  const size_t sneed = dpvo_encoder_saved_bytes((int)n, (int)H, (int)W, od, nc);
  const size_t wneed = dpvo_encoder_backward_workspace_bytes((int)n, (int)H, (int)W, od);
  TORCH_CHECK(sneed > 0 && wneed > 0, "dpvo_encoder.backward: unsupported sizes");
  const void* sv = a.bytes(saved, "saved (saved_bytes(n, H, W, out_dim, norm) long)",
                           images.device(), sneed);
  void* ws = a.bytes(workspace, "workspace (backward_workspace_bytes(n, H, W, out_dim) long)",
                     images.device(), wneed);
  const DeviceGuard guard(images.device());
  check_status(dpvo_encoder_backward(nc, od, pp.data(), ip, (int)n, (int)H, (int)W, sv, gop, layout,
                                     gp.data(), ws, (size_t)workspace.numel(), current_stream()),
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
