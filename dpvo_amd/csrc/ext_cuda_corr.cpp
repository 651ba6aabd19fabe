// ext_cuda_corr.cpp -- the `cuda_corr` extension module (drop-in for
// dpvo/altcorr/correlation.cpp:57-63), bound to the C ABI in dpvo_hot.h.
#include "ext_common.hpp"

using namespace dpvo_ext;

namespace {

// forward (`single`: one level, result in the fmap dtype) and forward_levels:
// one input check, then channels-last first, NCHW otherwise.  A pyramid whose
// levels are all channels-last ([B,N,C,H,W] views of [B,N,H,W,C] memory,
// INTEGRATION.md) takes the matrix-core entry (the edge order is honoured
// there only) instead of a transposing .contiguous() copy of the whole ring;
// outside its envelope, or with a level in another layout, contiguous NCHW
// levels (already-contiguous ones pass through) take the NCHW entry.
// fmap2 [L] (made contiguous in place off the channels-last path), scales [L] or null = 1
torch::Tensor corr_impl(torch::Tensor fmap1, torch::Tensor* fmap2, int L, torch::Tensor coords,
                        torch::Tensor ii, torch::Tensor jj, int radius, const double* scales,
                        const c10::optional<torch::Tensor>& order, bool single, const char* what) {
  const Entry a(what);
  a.on_gpu(fmap1, "fmap1");
  a.on_gpu(coords, "coords");
  TORCH_CHECK(L >= 1 && L <= 8, "one scale per pyramid level (1..8 levels)");
  TORCH_CHECK(fmap1.dim() == 5 && coords.dim() == 5 && coords.size(2) == 2 &&
                  coords.scalar_type() == torch::kFloat32,
              "corr: expected fmap1 [B,N1,C,H,W], fmap2 [B,N2,C,H2,W2], coords [B,M,2,H,W] float32");
  int dt;
  const void* f1 = a.in(fmap1, "fmap1", kF32 | kF16 | kF64, &dt);
  const float* co = a.in<float>(coords, "coords");
  const int64_t* ip = a.in<int64_t>(ii, "ii");
  const int64_t* jp = a.in<int64_t>(jj, "jj");
  const int B = coords.size(0), M = coords.size(1), H = coords.size(3), W = coords.size(4);
  TORCH_CHECK(ii.numel() >= M && jj.numel() >= M, "ii/jj shorter than coords.size(1)");
  TORCH_CHECK(fmap1.size(3) == H && fmap1.size(4) == W, "fmap1 patch size != coords size");
  const void* ptrs[8];
  int H2[8], W2[8];
  float sc[8];
  bool nhwc = true;
  for (int l = 0; l < L; l++) {
    const torch::Tensor& f = fmap2[l];
    ptrs[l] = a.view(f, "fmap2", kF32 | kF16 | kF64);
    TORCH_CHECK(f.dim() == 5 && f.scalar_type() == fmap1.scalar_type(),
                "fmap2 levels must be [B,N,C,H,W] of fmap1's dtype");
    nhwc = nhwc && f.permute({0, 1, 3, 4, 2}).is_contiguous() && f.size(2) > 1;
    H2[l] = f.size(3);
    W2[l] = f.size(4);
    sc[l] = scales ? (float)scales[l] : 1.0f;
  }
  const int Dp = 2 * radius + 1, C = fmap1.size(2), N1 = fmap1.size(1), N2 = fmap2[0].size(1);
  const int32_t* ord = nullptr;
  if (nhwc && order.has_value() && order->defined()) {
    ord = a.buf<int32_t>(*order, "order");
    TORCH_CHECK(order->numel() == M && B == 1, "order: contiguous int32 [E] (B == 1)");
  }
  const DeviceGuard guard(fmap1.device());
  torch::Tensor out;
  if (nhwc || !single)
    out = torch::empty({B, M, Dp, Dp, H, W, L}, fmap1.options().dtype(torch::kFloat32));
  if (nhwc) {
    const int st = dpvo_corr_forward_levels_nhwc_ordered(f1, ptrs, H2, W2, sc, L, co, ip, jp, ord, B,
                                                         M, C, H, W, N1, N2, radius, dt,
                                                         out.data_ptr<float>(), current_stream());
    if (st != DPVO_ERR_UNSUPPORTED) {
      check_status(st, what);
      // forward: fp32 accumulation, returned in the fmap dtype as the reference does
      return single ? out.view({B, M, Dp, Dp, H, W}).to(fmap1.scalar_type()) : out;
    }
  }
  for (int l = 0; l < L; l++) ptrs[l] = a.in(fmap2[l], "fmap2", kF32 | kF16 | kF64);
  if (single) {
    out = torch::empty({B, M, Dp, Dp, H, W}, fmap1.options());
    check_status(dpvo_corr_forward(f1, ptrs[0], co, ip, jp, B, M, C, H, W, N1, N2, H2[0], W2[0],
                                   radius, dt, out.data_ptr(), current_stream()),
                 what);
  } else {
    check_status(dpvo_corr_forward_levels(f1, ptrs, H2, W2, sc, L, co, ip, jp, B, M, C, H, W, N1,
                                          N2, radius, dt, out.data_ptr<float>(), current_stream()),
                 what);
  }
  return out;
}

// The two frame insertions of a channels-last pyramid (Entry::pyramid);
// slot_dev: the ring variant
void insert_impl(const char* fn, torch::Tensor src, const std::vector<torch::Tensor>& d,
                 const std::vector<int64_t>& scales, const char* name,
                 const torch::Tensor* slot_dev, int mem, const std::vector<int64_t>& slot_bytes) {
  const Entry a(fn);
  const Pyramid p = a.pyramid(src, d, scales, name);
  const int32_t* slot = slot_dev ? a.buf<int32_t>(*slot_dev, "slot_dev", 1) : nullptr;
  const DeviceGuard guard(src.device());
  const int L = p.dst.size();
  if (slot)
    check_status(dpvo_feature_pyramid_insert_ring(p.src, p.dst.data(), slot_bytes.data(),
                                                  p.scales.data(), L, p.C, p.H, p.W, mem, slot,
                                                  p.dtype, current_stream()),
                 fn);
  else
    check_status(dpvo_feature_pyramid_insert(p.src, p.dst.data(), p.scales.data(), L, p.C, p.H, p.W,
                                             p.dtype, current_stream()),
                 fn);
}

}  // namespace

// correlation.cpp:32-38 -> correlation_kernel.cu:232-272
std::vector<torch::Tensor> corr_forward(torch::Tensor fmap1, torch::Tensor fmap2,
                                        torch::Tensor coords, torch::Tensor ii, torch::Tensor jj,
                                        int radius) {
  return {corr_impl(fmap1, &fmap2, 1, coords, ii, jj, radius, nullptr, c10::nullopt, true,
                    "cuda_corr.forward")};
}

// Fused multi-level form (dpvo/dpvo.py:462-465): returns [B, M, Dp, Dp, H, W, L]
// float32 = torch.stack([corr(level l) for l], -1).
torch::Tensor corr_forward_levels(torch::Tensor fmap1, std::vector<torch::Tensor> fmap2,
                                  torch::Tensor coords, torch::Tensor ii, torch::Tensor jj,
                                  int radius, std::vector<double> scales,
                                  c10::optional<torch::Tensor> order) {
  TORCH_CHECK(fmap2.size() == scales.size(), "one scale per pyramid level (1..8 levels)");
  return corr_impl(fmap1, fmap2.data(), fmap2.size(), coords, ii, jj, radius, scales.data(), order,
                   false, "cuda_corr.forward_levels");
}

// src [..., C, H, W] contiguous -> dst: same shape, channels-last memory
// (dst.permute(..., H, W, C) contiguous), e.g. one frame of a pyramid level.
void feature_to_nhwc(torch::Tensor src, torch::Tensor dst) {
  const Entry a("cuda_corr.feature_to_nhwc");
  a.on_gpu(src, "src");
  a.on_gpu(dst, "dst");
  TORCH_CHECK(src.dim() >= 3 && src.sizes() == dst.sizes(), "src / dst shapes differ");
  TORCH_CHECK(src.scalar_type() == dst.scalar_type(), "src / dst dtypes differ");
  const int d = src.dim();
  int dt;
  const void* sp = a.in(src, "src", kF32 | kF16 | kF64, &dt);
  // dst is written through its channels-last view, which is the contiguous one
  torch::Tensor dv = dst.movedim(d - 3, d - 1);
  void* dp = a.buf(dv, "dst (channels-last)", kF32 | kF16 | kF64);
  const DeviceGuard guard(src.device());
  const int C = src.size(d - 3), H = src.size(d - 2), W = src.size(d - 1);
  const int count = src.numel() / ((int64_t)C * H * W);
  check_status(dpvo_feature_to_nhwc(sp, dp, count, C, H, W, dt, current_stream()), a.fn());
}

void feature_pyramid_insert(torch::Tensor src, std::vector<torch::Tensor> dst,
                            std::vector<int64_t> scales) {
  insert_impl("cuda_corr.feature_pyramid_insert", src, dst, scales, "dst", nullptr, 0, {});
}

// ring variant: slot = *slot_dev % mem read on the device (graph-replayed
// frames); rings[l] is the whole [B, mem, C, H/s, W/s] channels-last ring
void feature_pyramid_insert_ring(torch::Tensor src, std::vector<torch::Tensor> rings,
                                 std::vector<int64_t> scales, torch::Tensor slot_dev) {
  TORCH_CHECK(!rings.empty(), "one scale per ring level");
  const int mem = rings[0].dim() == 5 ? rings[0].size(1) : 0;
  std::vector<torch::Tensor> slot0;  // slot 0 of every ring
  std::vector<int64_t> slot_bytes;
  for (const torch::Tensor& r : rings) {
    TORCH_CHECK(r.dim() == 5 && r.size(1) == mem, "rings must be [B, mem, C, h, w]");
    slot0.push_back(r[0][0]);
    slot_bytes.push_back(r.stride(1) * (int64_t)r.element_size());
  }
  insert_impl("cuda_corr.feature_pyramid_insert_ring", src, slot0, scales, "ring", &slot_dev, mem,
              slot_bytes);
}

// correlation.cpp:40-48 -> correlation_kernel.cu:275-325
std::vector<torch::Tensor> corr_backward(torch::Tensor fmap1, torch::Tensor fmap2,
                                         torch::Tensor coords, torch::Tensor ii, torch::Tensor jj,
                                         torch::Tensor corr_grad, int radius) {
  const Entry a("cuda_corr.backward");
  a.on_gpu(fmap1, "fmap1");
  a.on_gpu(fmap2, "fmap2");
  a.on_gpu(coords, "coords");
  a.on_gpu(corr_grad, "corr_grad");
  const int64_t* ip = a.in<int64_t>(ii, "ii");
  const int64_t* jp = a.in<int64_t>(jj, "jj");
  const DeviceGuard guard(fmap1.device());
  const auto dtype = fmap1.scalar_type();
  // the atomic accumulation runs in fp32 for every input dtype
  auto f1 = fmap1.to(torch::kFloat32), f2 = fmap2.to(torch::kFloat32);
  auto g = corr_grad.to(torch::kFloat32);
  coords = coords.to(torch::kFloat32);
  const float* f1p = a.in<float>(f1, "fmap1");
  const float* f2p = a.in<float>(f2, "fmap2");
  const float* co = a.in<float>(coords, "coords");
  const float* gp = a.in<float>(g, "corr_grad");
  const int B = coords.size(0), M = coords.size(1), H = coords.size(3), W = coords.size(4);
  auto g1 = torch::empty_like(f1);
  auto g2 = torch::empty_like(f2);
  check_status(dpvo_corr_backward(f1p, f2p, co, ip, jp, gp, B, M, f1.size(2), H, W, f1.size(1),
                                  f2.size(1), f2.size(3), f2.size(4), radius, DPVO_F32,
                                  g1.data_ptr(), g2.data_ptr(), current_stream()),
               "cuda_corr.backward");
  return {g1.to(dtype), g2.to(dtype)};
}

// correlation.cpp:50-53 -> correlation_kernel.cu:327-346 (zero fill); CLAMP: the
// fork's runtime patchify (clamp at the border), correlation_kernel.py:181-224
template <bool CLAMP>
std::vector<torch::Tensor> patchify_forward(torch::Tensor net, torch::Tensor coords, int radius) {
  const Entry a("cuda_corr.patchify_forward");
  a.on_gpu(coords, "coords");
  int dt;
  const void* np = a.in(net, "net", kF32 | kF16 | kF64, &dt);
  TORCH_CHECK(net.dim() == 4 && coords.dim() == 3 && coords.size(2) == 2,
              "patchify: expected net [B,C,H,W], coords [B,M,2]");
  const DeviceGuard guard(net.device());
  coords = coords.to(torch::kFloat32);
  const float* co = a.in<float>(coords, "coords");
  const int B = coords.size(0), M = coords.size(1), C = net.size(1), D = 2 * radius + 2;
  auto out = torch::empty({B, M, C, D, D}, net.options());
  check_status(dpvo_patchify_forward(np, co, B, C, net.size(2), net.size(3), M, radius,
                                     CLAMP ? 1 : 0, dt, out.data_ptr(), current_stream()),
               a.fn());
  return {out};
}

// correlation.cpp:55-58 -> correlation_kernel.cu:349-372
template <bool CLAMP>
std::vector<torch::Tensor> patchify_backward(torch::Tensor net, torch::Tensor coords,
                                             torch::Tensor gradient, int radius) {
  const Entry a("cuda_corr.patchify_backward");
  a.on_gpu(net, "net");
  a.on_gpu(coords, "coords");
  a.on_gpu(gradient, "gradient");
  TORCH_CHECK(net.dim() == 4 && coords.dim() == 3 && coords.size(2) == 2,
              "patchify: expected net [B,C,H,W], coords [B,M,2]");
  const DeviceGuard guard(net.device());
  coords = coords.to(torch::kFloat32);
  auto g = gradient.to(torch::kFloat32);
  const float* co = a.in<float>(coords, "coords");
  const float* gp = a.in<float>(g, "gradient");
  const int B = coords.size(0), M = coords.size(1), C = net.size(1);
  auto out = torch::empty({net.size(0), C, net.size(2), net.size(3)},
                          net.options().dtype(torch::kFloat32));
  check_status(dpvo_patchify_backward(gp, co, B, C, net.size(2), net.size(3), M, radius,
                                      CLAMP ? 1 : 0, DPVO_F32, out.data_ptr(), current_stream()),
               a.fn());
  return {out.to(net.scalar_type())};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("forward", &corr_forward, "CORR forward");
  m.def("backward", &corr_backward, "CORR backward");
  m.def("patchify_forward", &patchify_forward<false>, "PATCHIFY forward");
  m.def("patchify_backward", &patchify_backward<false>, "PATCHIFY backward");
  // additions (not in the reference surface)
  m.def("forward_levels", &corr_forward_levels, "CORR forward, all pyramid levels in one launch",
        py::arg("fmap1"), py::arg("fmap2"), py::arg("coords"), py::arg("ii"), py::arg("jj"),
        py::arg("radius"), py::arg("scales"), py::arg("order") = py::none());
  m.def("feature_pyramid_insert_ring", &feature_pyramid_insert_ring,
        "feature_pyramid_insert into ring slot *slot_dev % mem (device scalar, graph replay)");
  m.def("feature_pyramid_insert", &feature_pyramid_insert,
        "NCHW level-1 frame -> channels-last pyramid slot (all levels, one launch)");
  m.def("feature_to_nhwc", &feature_to_nhwc, "[..., C, H, W] -> channels-last copy into dst");
  m.def("patchify_forward_clamped", &patchify_forward<true>, "PATCHIFY forward, border clamp");
  m.def("patchify_backward_clamped", &patchify_backward<true>, "PATCHIFY backward, border clamp");
  m.attr("native_library") = dpvo_version();
}
