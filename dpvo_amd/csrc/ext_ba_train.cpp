// ext_ba_train.cpp -- cuda_ba, part 3: the training side.  The differentiable
// BA layer (ba_layer.hip), the training step's reprojection and losses
// (train.hip) and the device half of the training data readers (dataset.hip).
#include "ext_common.hpp"

using namespace dpvo_ext;

namespace {

// The differentiable BA layer (dpvo/ba.py BA, 88-297): one Gauss-Newton step
// and its adjoint, float32 or float64.  No host synchronisation in either call.
std::vector<torch::Tensor> ba_layer_forward(torch::Tensor poses, torch::Tensor patches,
                                            torch::Tensor intrinsics, torch::Tensor targets,
                                            torch::Tensor weights,
                                            c10::optional<torch::Tensor> lmbda_dev, double lmbda,
                                            torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                                            int64_t n, int64_t fixedp, bool structure_only,
                                            std::vector<double> bounds, double ep,
                                            bool with_backward) {
  const Entry a("cuda_ba.ba_layer_forward");
  const Edges<void> l = a.edges(poses, patches, intrinsics, ii, jj, kk, kF32 | kF64, true);
  const unsigned same = l.dtype == DPVO_F32 ? kF32 : kF64;
  const void* tp = a.in(targets, "targets", same);
  const void* wp = a.in(weights, "weights", same);
  TORCH_CHECK(targets.numel() == 2 * (int64_t)l.E && weights.numel() == 2 * (int64_t)l.E,
              "targets / weights must be [.., E, 2]");
  TORCH_CHECK(bounds.size() == 4, "bounds must hold 4 values");
  TORCH_CHECK(fixedp >= 0 && n >= fixedp && n <= l.num_poses, "cuda_ba.ba_layer_forward: need 0 <= "
              "fixedp <= n <= N, got fixedp ", fixedp, ", n ", n, ", N ", l.num_poses);
  const bool has_lm = lmbda_dev && lmbda_dev->defined();
  if (has_lm) {
    a.on_gpu(*lmbda_dev, "lmbda");
    TORCH_CHECK(lmbda_dev->numel() == 1, "lmbda must be a float or a 1-element tensor");
  }
  const DeviceGuard guard(poses.device());
  torch::Tensor lmt;
  const void* lm = nullptr;
  if (has_lm) {
    lmt = lmbda_dev->to(poses.scalar_type());
    lm = a.in(lmt, "lmbda", same);
  }
  const int nf = structure_only ? 0 : (int)(n - fixedp), M = l.num_patches;
  const bool none = l.E == 0;  // nothing launched: the outputs are the zero step
  auto dX = none ? torch::zeros({nf, 6}, poses.options()) : torch::empty({nf, 6}, poses.options());
  auto dZ = none ? torch::zeros({M}, poses.options()) : torch::empty({M}, poses.options());
  const size_t wsb = dpvo_ba_layer_workspace_bytes(l.E, M, nf, with_backward ? 1 : 0);
  auto ws = torch::empty({(int64_t)std::max<size_t>(wsb, 32)}, poses.options().dtype(torch::kUInt8));
  if (none) {
    ws.zero_();
    return {dX, dZ, ws};
  }
  check_status(dpvo_ba_layer_forward(l.poses, l.patches, l.intrinsics, tp, wp, lm, lmbda, l.ii,
                                     l.jj, l.kk, l.E, M, l.P, l.num_poses, (int)n, (int)fixedp,
                                     structure_only ? 1 : 0, bounds.data(), ep, l.dtype,
                                     dX.data_ptr(), dZ.data_ptr(), ws.data_ptr(), wsb,
                                     with_backward ? 1 : 0, current_stream()),
               a.fn());
  return {dX, dZ, ws};
}

// -> [g_targets [E, 2], g_weights [E, 2], g_poses [N, 6], g_patches [M, 3]]
std::vector<torch::Tensor> ba_layer_backward(torch::Tensor ws, torch::Tensor poses,
                                             torch::Tensor patches, torch::Tensor intrinsics,
                                             torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                                             torch::Tensor gX, torch::Tensor gZ, int64_t n,
                                             int64_t fixedp, bool structure_only) {
  const Entry a("cuda_ba.ba_layer_backward");
  const Edges<void> l = a.edges(poses, patches, intrinsics, ii, jj, kk, kF32 | kF64, true);
  const unsigned same = l.dtype == DPVO_F32 ? kF32 : kF64;
  const int nf = structure_only ? 0 : (int)(n - fixedp), M = l.num_patches, N = l.num_poses;
  const void* gXp = a.in(gX, "gX", same);
  const void* gZp = a.in(gZ, "gZ", same);
  TORCH_CHECK(gX.numel() == 6 * (int64_t)nf && gZ.numel() == M,
              "cuda_ba.ba_layer_backward: gX must be [n_free, 6] and gZ [M]");
  void* wsp = a.bytes(ws, "ws", poses.device());
  const DeviceGuard guard(poses.device());
  const auto mk = [&](int64_t r, int64_t c) {  // every row is written by the kernels
    return l.E == 0 ? torch::zeros({r, c}, poses.options()) : torch::empty({r, c}, poses.options());
  };
  auto gT = mk(l.E, 2), gW = mk(l.E, 2), gP = mk(N, 6), gK = mk(M, 3);
  if (l.E == 0) return {gT, gW, gP, gK};
  check_status(dpvo_ba_layer_backward(l.poses, l.patches, l.intrinsics, gXp, gZp, l.E, M, l.P, N,
                                      (int)n, (int)fixedp, structure_only ? 1 : 0, l.dtype,
                                      gT.data_ptr(), gW.data_ptr(), gP.data_ptr(), gK.data_ptr(),
                                      wsp, (size_t)ws.numel(), current_stream()),
               a.fn());
  return {gT, gW, gP, gK};
}

// The training step's reprojection and losses (train.hip): fp32 tensors, no
// host synchronisation in any call.
// -> [coords [E, P, P, 2], valid [E, P, P]] (+ coords_corr [E, 2, P, P])
std::vector<torch::Tensor> transform_forward(torch::Tensor poses, torch::Tensor patches,
                                             torch::Tensor intrinsics, torch::Tensor ii,
                                             torch::Tensor jj, torch::Tensor kk, bool with_corr) {
  const Entry a("cuda_ba.transform_forward");
  const Edges<float> t = a.edges(poses, patches, intrinsics, ii, jj, kk, true);
  const DeviceGuard guard(poses.device());
  auto coords = torch::empty({t.E, t.P, t.P, 2}, poses.options());
  auto valid = torch::empty({t.E, t.P, t.P}, poses.options());
  torch::Tensor corr;
  if (with_corr) corr = torch::empty({t.E, 2, t.P, t.P}, poses.options());
  check_status(dpvo_transform_forward(t.poses, t.patches, t.intrinsics, t.ii, t.jj, t.kk, t.E, t.P,
                                      t.num_poses, t.num_patches, coords.data_ptr<float>(),
                                      valid.data_ptr<float>(),
                                      with_corr ? corr.data_ptr<float>() : nullptr,
                                      current_stream()),
               a.fn());
  if (with_corr) return {coords, valid, corr};
  return {coords, valid};
}

// -> [g_poses [N, 6] or undefined, g_patches [M, 3, P, P] or undefined]
std::vector<c10::optional<torch::Tensor>> transform_backward(
    torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics, torch::Tensor ii,
    torch::Tensor jj, torch::Tensor kk, torch::Tensor g_coords, bool want_poses,
    bool want_patches) {
  const Entry a("cuda_ba.transform_backward");
  const Edges<float> t = a.edges(poses, patches, intrinsics, ii, jj, kk, true);
  const float* gc = a.in<float>(g_coords, "g_coords");
  TORCH_CHECK(g_coords.numel() == 2 * (int64_t)t.E * t.P * t.P, "g_coords must be [E, P, P, 2]");
  const DeviceGuard guard(poses.device());
  const auto mk = [&](std::vector<int64_t> s) {  // every row is written by the kernels
    return t.E == 0 ? torch::zeros(s, poses.options()) : torch::empty(s, poses.options());
  };
  c10::optional<torch::Tensor> gP, gK;
  if (want_poses) gP = mk({t.num_poses, 6});
  if (want_patches) gK = mk({t.num_patches, 3, t.P, t.P});
  const size_t wsb = dpvo_transform_workspace_bytes(t.E, t.P);
  auto ws = torch::empty({(int64_t)std::max<size_t>(wsb, 8)}, poses.options().dtype(torch::kUInt8));
  check_status(dpvo_transform_backward(t.poses, t.patches, t.intrinsics, t.ii, t.jj, t.kk, t.E, t.P,
                                       t.num_poses, t.num_patches, gc,
                                       gP ? gP->data_ptr<float>() : nullptr,
                                       gK ? gK->data_ptr<float>() : nullptr, ws.data_ptr(), wsb,
                                       current_stream()),
               a.fn());
  return {gP, gK};
}

// -> [loss [1], count [1] int32, emin [E], argmin [E] int32]
std::vector<torch::Tensor> flow_loss_forward(torch::Tensor coords, torch::Tensor coords_gt,
                                             torch::Tensor valid) {
  const Entry a("cuda_ba.flow_loss_forward");
  const float* cp = a.in<float>(coords, "coords");
  const float* gp = a.in<float>(coords_gt, "coords_gt");
  const float* vp = a.in<float>(valid, "valid");
  const DeviceGuard guard(coords.device());
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
  check_status(dpvo_flow_loss_forward(cp, gp, vp, (int)E, P, loss.data_ptr<float>(),
                                      count.data_ptr<int32_t>(), emin.data_ptr<float>(),
                                      amin.data_ptr<int32_t>(), current_stream()),
               a.fn());
  return {loss, count, emin, amin};
}

torch::Tensor flow_loss_backward(torch::Tensor coords, torch::Tensor coords_gt, torch::Tensor valid,
                                 torch::Tensor count, torch::Tensor argmin, torch::Tensor g_loss) {
  const Entry a("cuda_ba.flow_loss_backward");
  const float* cp = a.in<float>(coords, "coords");
  const float* gp = a.in<float>(coords_gt, "coords_gt");
  const float* vp = a.in<float>(valid, "valid");
  const float* lp = a.in<float>(g_loss, "g_loss");
  TORCH_CHECK(coords.dim() >= 2, "cuda_ba.flow_loss_backward: coords must be [.., E, P, P, 2]");
  const int P = coords.size(-2);
  const int64_t E = coords.numel() / (2 * (int64_t)P * P);
  TORCH_CHECK(count.numel() == 1 && argmin.numel() == E && g_loss.numel() == 1 &&
                  valid.numel() == E && coords_gt.numel() == coords.numel(),
              "cuda_ba.flow_loss_backward: buffers of another forward call");
  const int32_t* np = a.buf<int32_t>(count, "count");
  const int32_t* ap = a.in<int32_t>(argmin, "argmin");
  const DeviceGuard guard(coords.device());
  auto g = torch::empty_like(coords);
  check_status(dpvo_flow_loss_backward(cp, gp, vp, np, ap, lp, (int)E, P, g.data_ptr<float>(),
                                       current_stream()),
               a.fn());
  return g;
}

// -> [out [3] = (mean tr, mean ro, s), tr [n (n - 1)], ro [n (n - 1)]]
std::vector<torch::Tensor> pose_loss_forward(torch::Tensor G, torch::Tensor Ps) {
  const Entry a("cuda_ba.pose_loss_forward");
  const float* Gp = a.in<float>(G, "G");
  const float* Pp = a.in<float>(Ps, "Ps");
  const DeviceGuard guard(G.device());
  TORCH_CHECK(G.dim() >= 2 && G.size(-1) == 7 && Ps.numel() == G.numel(),
              "G and Ps must be [.., n, 7]");
  const int64_t n = G.numel() / 7;
  const int64_t np = n > 1 ? n * (n - 1) : 0;
  auto out = torch::zeros({3}, G.options());  // n < 2: zeros, nothing launched
  auto tr = torch::empty({np}, G.options()), ro = torch::empty({np}, G.options());
  check_status(dpvo_pose_loss_forward(Gp, Pp, (int)n, out.data_ptr<float>(), tr.data_ptr<float>(),
                                      ro.data_ptr<float>(), current_stream()),
               a.fn());
  return {out, tr, ro};
}

torch::Tensor pose_loss_backward(torch::Tensor G, torch::Tensor Ps, torch::Tensor g_out) {
  const Entry a("cuda_ba.pose_loss_backward");
  const float* Gp = a.in<float>(G, "G");
  const float* Pp = a.in<float>(Ps, "Ps");
  const float* gp = a.in<float>(g_out, "g_out");
  const DeviceGuard guard(G.device());
  TORCH_CHECK(G.dim() >= 1 && G.size(-1) == 7 && Ps.numel() == G.numel() && g_out.numel() == 2,
              "G and Ps must be [.., n, 7], g_out [2]");
  const int64_t n = G.numel() / 7;
  auto gG = n < 2 ? torch::zeros({n, 6}, G.options()) : torch::empty({n, 6}, G.options());
  check_status(dpvo_pose_loss_backward(Gp, Pp, (int)n, gp, gG.data_ptr<float>(), current_stream()),
               a.fn());
  return gG;
}

// ---- dataset.hip: the device half of the training data readers -------------------
// rgbd_utils.compute_distance_matrix_flow: poses [N, 7] (world-from-camera), disps
// [N, h, w], intrinsics [N, 4] -> D float32 [N, N], one launch
torch::Tensor frame_flow_distance(torch::Tensor poses, torch::Tensor disps,
                                  torch::Tensor intrinsics) {
  const Entry a("cuda_ba.frame_flow_distance");
  const float* pp = a.in<float>(poses, "poses");
  const float* dp = a.in<float>(disps, "disps");
  const float* ip = a.in<float>(intrinsics, "intrinsics");
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) >= 1,
              "frame_flow_distance: poses must be [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(disps.dim() == 3 && disps.size(0) == N && disps.size(1) >= 1 && disps.size(2) >= 1,
              "frame_flow_distance: disps must be [N, h, w]");
  TORCH_CHECK(intrinsics.dim() == 2 && intrinsics.size(0) == N && intrinsics.size(1) == 4,
              "frame_flow_distance: intrinsics must be [N, 4]");
  a.same_device({poses, disps, intrinsics});
  TORCH_CHECK(N < (1LL << 31) && disps.size(1) < (1LL << 31) && disps.size(2) < (1LL << 31),
              "frame_flow_distance: too large");
  const DeviceGuard guard(poses.device());
  auto D = torch::empty({N, N}, poses.options());
  check_status(dpvo_frame_flow_distance(pp, dp, ip, (int)N, (int)disps.size(1), (int)disps.size(2),
                                        D.data_ptr<float>(), current_stream()),
               a.fn());
  return D;
}

// base.py:77-80 as CSR -> [rowptr i32 [N + 1], col i32 [nnz], dist f32 [nnz]].
// One host read (nnz) sizes the outputs: a build step, not a per-frame call.
std::vector<torch::Tensor> frame_graph(torch::Tensor D, double f, double max_flow) {
  const Entry a("cuda_ba.frame_graph");
  const float* Dp = a.in<float>(D, "D");
  TORCH_CHECK(D.dim() == 2 && D.size(0) == D.size(1) && D.size(0) >= 1 && D.size(0) < (1LL << 31),
              "frame_graph: D must be [N, N]");
  const DeviceGuard guard(D.device());
  const int N = (int)D.size(0);
  const auto i32 = D.options().dtype(torch::kInt32);
  auto rowptr = torch::empty({(int64_t)N + 1}, i32);
  check_status(dpvo_frame_graph_count(Dp, N, (float)f, (float)max_flow, rowptr.data_ptr<int32_t>(),
                                      current_stream()),
               "cuda_ba.frame_graph (count)");
  const int nnz = rowptr[N].item<int32_t>();
  auto col = torch::empty({(int64_t)nnz}, i32);
  auto dist = torch::empty({(int64_t)nnz}, D.options());
  check_status(dpvo_frame_graph_fill(Dp, N, (float)f, (float)max_flow, rowptr.data_ptr<int32_t>(),
                                     nnz ? col.data_ptr<int32_t>() : nullptr,
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
  const Entry a("cuda_ba.rgbd_augment");
  const float* mp = a.in<float>(images, "images");
  const float* dp = a.in<float>(disps, "disps");
  const float* ip = a.in<float>(intrinsics, "intrinsics");
  TORCH_CHECK(images.dim() == 4 && images.size(1) == 3 && images.size(0) >= 1,
              "rgbd_augment: images must be [N, 3, H, W]");
  const int64_t N = images.size(0), H = images.size(2), W = images.size(3);
  TORCH_CHECK(disps.dim() == 3 && disps.size(0) == N && disps.size(1) == H && disps.size(2) == W,
              "rgbd_augment: disps must be [N, H, W]");
  TORCH_CHECK(intrinsics.dim() == 2 && intrinsics.size(0) == N && intrinsics.size(1) == 4,
              "rgbd_augment: intrinsics must be [N, 4]");
  a.same_device({images, disps, intrinsics});
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
  const DeviceGuard guard(images.device());
  auto images_out = torch::empty({N, 3, crop_h, crop_w}, images.options());
  auto disps_out = torch::empty({N, crop_h, crop_w}, images.options());
  auto intr_out = torch::empty({N, 4}, images.options());
  const size_t wsb = dpvo_rgbd_augment_workspace_bytes((int)N, (int)H, (int)W);
  // the scratch image is touched only by colour followed by resampling
  const size_t need = (do_color && scale != 1.0) ? wsb : 8 * 256;
  auto ws = torch::empty({(int64_t)((need + 7) / sizeof(double))},
                         images.options().dtype(torch::kFloat64));
  check_status(dpvo_rgbd_augment(mp, dp, ip, (int)N, (int)H, (int)W, (int)crop_h, (int)crop_w, &p,
                                 images_out.data_ptr<float>(), disps_out.data_ptr<float>(),
                                 intr_out.data_ptr<float>(), ws.data_ptr(), need, current_stream()),
               a.fn());
  return {images_out, disps_out, intr_out};
}

// base.py:171-173 -> [disps / s, poses with the translation times s, (s, lo, hi) f32 [3]]
std::vector<torch::Tensor> normalize_depth(torch::Tensor disps, torch::Tensor poses) {
  const Entry a("cuda_ba.normalize_depth");
  const float* dp = a.in<float>(disps, "disps");
  const float* pp = a.in<float>(poses, "poses");
  TORCH_CHECK(disps.numel() >= 1 && disps.numel() < (1LL << 31),
              "normalize_depth: disps is empty or too large");
  TORCH_CHECK(poses.dim() >= 1 && poses.size(-1) == 7 && poses.numel() >= 7 &&
                  poses.numel() < (1LL << 31),
              "normalize_depth: poses must be [.., 7]");
  a.same_device({disps, poses});
  const DeviceGuard guard(disps.device());
  auto disps_out = torch::empty_like(disps);
  auto poses_out = torch::empty_like(poses);
  auto s = torch::empty({3}, disps.options());
  check_status(dpvo_normalize_depth(dp, (int)disps.numel(), pp, (int)(poses.numel() / 7),
                                    disps_out.data_ptr<float>(), poses_out.data_ptr<float>(),
                                    s.data_ptr<float>(), current_stream()),
               a.fn());
  return {disps_out, poses_out, s};
}

}  // namespace

void bind_train(py::module_& m) {
  m.def("ba_layer_forward", &ba_layer_forward,
        "one Gauss-Newton step of dpvo/ba.py BA: (poses, patches, intrinsics, targets, weights, "
        "lmbda tensor or None, lmbda float, ii, jj, kk, n, fixedp, structure_only, bounds, ep, "
        "with_backward) -> [dX [n_free, 6], dZ [M], workspace (int32 words: out-of-range edges, "
        "factorisation info)]");
  m.def("ba_layer_backward", &ba_layer_backward,
        "adjoint of ba_layer_forward on its workspace: (ws, poses, patches, intrinsics, ii, jj, kk, "
        "gX, gZ, n, fixedp, structure_only) -> [g_targets, g_weights, g_poses [N, 6], g_patches [M, 3]]");
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
}
