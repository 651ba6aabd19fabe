// ext_ba_tracker.cpp -- cuda_ba, part 4: the tracker's frame path.  The front
// end and trajectory read-out (frontend.hip), the small per-frame kernels
// (tracker.hip), the image stream and ATE evaluation (stream.hip,
// evaluate.hip), and the front half of the long-term loop closure (match.hip,
// triangulate.hip).
#include "ext_common.hpp"

using namespace dpvo_ext;

namespace {

// The head of DPVO.__call__ (dpvo.py:931-965): tstamps / intrinsics / pose /
// patches of frame row n, in place, one launch.  n / counter: the host value,
// or the int32 device scalar when given.
void frame_init(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                torch::Tensor tstamps, torch::Tensor times, torch::Tensor new_patches,
                torch::Tensor new_intrinsics, int64_t M, int64_t n,
                c10::optional<torch::Tensor> n_dev, int64_t counter,
                c10::optional<torch::Tensor> counter_dev, int64_t motion_model, double damping,
                double res, bool median) {
  const Entry a("cuda_ba.frame_init");
  float* pp = a.buf<float>(poses, "poses");
  float* tp = a.buf<float>(patches, "patches");
  float* ip = a.buf<float>(intrinsics, "intrinsics");
  int64_t* sp = a.buf<int64_t>(tstamps, "tstamps");
  const double* mp = a.buf<double>(times, "times");
  const float* np = a.in<float>(new_patches, "new_patches");
  const float* ni = a.in<float>(new_intrinsics, "new_intrinsics");
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
  TORCH_CHECK(new_patches.numel() == M * 3 * P * P, "new_patches: [M, 3, P, P]");
  TORCH_CHECK(new_intrinsics.numel() == 4, "new_intrinsics: [4]");
  TORCH_CHECK(N * M * 3 * P * P < (1LL << 40) && N < (1LL << 31) && M < (1LL << 31), "too large");
  const Count nc = a.count(n, n_dev, "n", 0, N - 1);
  const Count cc = a.count(counter, counter_dev, "counter", 0, times.numel() - 1);
  const DeviceGuard guard(poses.device());
  check_status(dpvo_frame_init(pp, tp, ip, sp, mp, (int)times.numel(), np, ni, (int)N, (int)M,
                               (int)P, nc.host, nc.dev, cc.host, cc.dev, (int)motion_model, damping,
                               res, median ? 1 : 0, current_stream()),
               a.fn());
}

// DPVO.terminate's interpolation (dpvo.py:385-417) -> [traj [counter, 7],
// root [counter] int64, info int32[2] = {unresolved frames, ignored records}]
std::vector<torch::Tensor> trajectory(torch::Tensor poses, torch::Tensor tstamps, int64_t n,
                                      c10::optional<torch::Tensor> n_dev, torch::Tensor delta_log,
                                      torch::Tensor delta_pairs, torch::Tensor delta_count,
                                      int64_t counter, bool inverse) {
  const Entry a("cuda_ba.trajectory");
  const float* pp = a.in<float>(poses, "poses");
  const int64_t* tp = a.in<int64_t>(tstamps, "tstamps");
  const float* lp = a.in<float>(delta_log, "delta log");
  const int64_t* dp = a.in<int64_t>(delta_pairs, "delta pairs");
  const int32_t* dc = a.buf<int32_t>(delta_count, "delta count", 1);
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) > 0, "poses: [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(tstamps.numel() >= N && N < (1LL << 31), "tstamps: [N]");
  TORCH_CHECK(delta_log.numel() % 7 == 0, "delta log: [cap, 7]");
  const int64_t cap = delta_log.numel() / 7;
  TORCH_CHECK(delta_pairs.numel() == 2 * cap && cap < (1LL << 31), "delta pairs: [cap, 2]");
  TORCH_CHECK(counter >= 0 && counter < (1LL << 30), "trajectory: counter = ", counter);
  const Count nc = a.count(n, n_dev, "n", 0, N);
  const DeviceGuard guard(poses.device());
  auto traj = torch::empty({counter, 7}, poses.options());
  auto root = torch::empty({counter}, tstamps.options());
  auto info = torch::zeros({2}, poses.options().dtype(torch::kInt32));
  const size_t wsb = dpvo_trajectory_workspace_bytes((int)counter);
  auto ws = torch::empty({(int64_t)(wsb / sizeof(double))}, poses.options().dtype(torch::kFloat64));
  check_status(dpvo_trajectory(pp, tp, (int)N, nc.host, nc.dev, lp, dp, dc, (int)cap, (int)counter,
                               inverse ? 1 : 0, traj.data_ptr<float>(), root.data_ptr<int64_t>(),
                               info.data_ptr<int32_t>(), ws.data_ptr(), wsb, current_stream()),
               a.fn());
  return {traj, root, info};
}

// ---- stream.hip / evaluate.hip: frame in, score out ------------------------------
// Undistort, halve and crop a decoded frame (dpvo/stream.py:24-39, :75-83), one
// launch -> [image uint8 [3, H, W], intrinsics float32 [4]].  raw: uint8
// [H0, W0, 3] or [H0, W0]; calib: the 4, 8 or 9 numbers of calib/*.txt.
std::vector<torch::Tensor> frame_prepare(torch::Tensor raw, std::vector<double> calib,
                                         double scale, bool swap_rb,
                                         c10::optional<torch::Tensor> out) {
  const Entry a("cuda_ba.frame_prepare");
  const uint8_t* rp = a.in<uint8_t>(raw, "raw");
  TORCH_CHECK(raw.dim() == 2 || (raw.dim() == 3 && raw.size(2) == 3),
              "frame_prepare: raw must be [H0, W0, 3] or [H0, W0]");
  TORCH_CHECK(raw.size(0) > 0 && raw.size(1) > 0 && raw.size(0) < (1LL << 31) &&
                  raw.size(1) < (1LL << 31),
              "frame_prepare: empty or oversized frame");
  const DeviceGuard guard(raw.device());
  const int H0 = (int)raw.size(0), W0 = (int)raw.size(1);
  int H = 0, W = 0;
  // the count is checked first here only to give dpvo_frame_prepare's own answer for it
  if (calib.size() == 4 || calib.size() == 8 || calib.size() == 9)
    check_status(dpvo_frame_prepare_shape(H0, W0, scale, &H, &W), a.fn());
  else
    check_status(DPVO_ERR_UNSUPPORTED, "cuda_ba.frame_prepare (4, 8 or 9 calibration numbers)");
  torch::Tensor image;
  uint8_t* op;
  if (out && out->defined()) {
    image = *out;
    op = a.buf<uint8_t>(image, "out");
    TORCH_CHECK(image.dim() == 3 && image.size(0) == 3 && image.size(1) == H &&
                    image.size(2) == W && image.device() == raw.device(),
                "frame_prepare: out must be a contiguous uint8 [3, ", H, ", ", W,
                "] tensor on raw's device");
  } else {
    image = torch::empty({3, H, W}, raw.options());
    op = image.data_ptr<uint8_t>();
  }
  auto intr = torch::empty({4}, raw.options().dtype(torch::kFloat32));
  check_status(dpvo_frame_prepare(rp, H0, W0, raw.dim() == 2 ? 1 : 3, calib.data(),
                                  (int)calib.size(), scale, swap_rb ? 1 : 0, op,
                                  intr.data_ptr<float>(), current_stream()),
               a.fn());
  return {image, intr};
}

// ATE of an estimated trajectory against a reference one (evaluate_euroc.py:109-119
// through evo), one launch -> [stats f64[8], model f64[13], pairs i32[min(n, m), 2],
// status i32[1]]
std::vector<torch::Tensor> trajectory_ate(torch::Tensor est_xyz, torch::Tensor est_t,
                                          torch::Tensor ref_xyz, torch::Tensor ref_t,
                                          double max_diff, bool align) {
  const Entry a("cuda_ba.trajectory_ate");
  int dt;
  const void* ex = a.in(est_xyz, "est_xyz", kF32 | kF64, &dt);
  const double* et = a.in<double>(est_t, "est_t");
  const double* rx = a.in<double>(ref_xyz, "ref_xyz");
  const double* rt = a.in<double>(ref_t, "ref_t");
  TORCH_CHECK(est_xyz.dim() == 2 && est_xyz.size(1) == 3 && est_t.dim() == 1 &&
                  est_t.size(0) == est_xyz.size(0),
              "trajectory_ate: est_xyz [n, 3], est_t [n]");
  TORCH_CHECK(ref_xyz.dim() == 2 && ref_xyz.size(1) == 3 && ref_t.dim() == 1 &&
                  ref_t.size(0) == ref_xyz.size(0),
              "trajectory_ate: ref_xyz [m, 3], ref_t [m]");
  a.same_device({est_xyz, est_t, ref_xyz, ref_t});
  const int64_t n = est_xyz.size(0), m = ref_xyz.size(0);
  TORCH_CHECK(n >= 1 && m >= 1, "trajectory_ate: empty trajectory");
  TORCH_CHECK(n < (1LL << 31) && m < (1LL << 31), "trajectory_ate: trajectory too long");
  const DeviceGuard guard(est_xyz.device());
  const auto f64 = ref_xyz.options();
  const auto i32 = ref_xyz.options().dtype(torch::kInt32);
  auto stats = torch::empty({8}, f64);
  auto model = torch::empty({13}, f64);
  auto pairs = torch::empty({std::min(n, m), 2}, i32);
  auto status = torch::empty({1}, i32);
  const size_t wsb = dpvo_trajectory_ate_workspace_bytes((int)n, (int)m);
  auto ws = torch::empty({(int64_t)(wsb / sizeof(double))}, f64);
  check_status(dpvo_trajectory_ate(ex, dt, et, (int)n, rx, rt, (int)m, max_diff, align ? 1 : 0,
                                   stats.data_ptr<double>(), model.data_ptr<double>(),
                                   pairs.data_ptr<int32_t>(), status.data_ptr<int32_t>(),
                                   ws.data_ptr(), wsb, current_stream()),
               a.fn());
  return {stats, model, pairs, status};
}

// ---- tracker.hip: the small kernels of the tracker's frame path ----------------
// Patchifier's gathers and DPVO.__call__'s ring writes of frame n, one launch.
void frame_sample(torch::Tensor fmap, torch::Tensor imap, torch::Tensor image,
                  torch::Tensor coords, torch::Tensor gmap_ring, torch::Tensor imap_ring,
                  torch::Tensor patches_out, torch::Tensor colors, int64_t res, int64_t n,
                  c10::optional<torch::Tensor> n_dev) {
  const Entry a("cuda_ba.frame_sample");
  const float* fp = a.in<float>(fmap, "fmap");
  const float* ip = a.in<float>(imap, "imap");
  const float* gp = a.in<float>(image, "image");
  const float* cp = a.in<float>(coords, "coords");
  int gd, id;
  void* gr = a.buf(gmap_ring, "gmap ring", kF32 | kF16, &gd);
  void* ir = a.buf(imap_ring, "imap ring", kF32 | kF16, &id);
  TORCH_CHECK(id == gd, "the two rings must share one dtype");
  float* po = a.buf<float>(patches_out, "patches_out");
  uint8_t* co = a.buf<uint8_t>(colors, "colors");
  TORCH_CHECK(fmap.dim() == 3 && imap.dim() == 3 && image.dim() == 3 && image.size(0) == 3,
              "fmap [C, h, w], imap [DIM, h, w], image [3, H, W]");
  const int64_t C = fmap.size(0), h = fmap.size(1), w = fmap.size(2), DIM = imap.size(0);
  TORCH_CHECK(imap.size(1) == h && imap.size(2) == w, "fmap and imap differ in size");
  TORCH_CHECK(coords.dim() == 2 && coords.size(1) == 2 && coords.size(0) > 0, "coords: [M, 2]");
  const int64_t M = coords.size(0);
  TORCH_CHECK(gmap_ring.dim() >= 3 && gmap_ring.size(-1) == gmap_ring.size(-2),
              "gmap ring: [.., C, P, P]");
  const int64_t P = gmap_ring.size(-1);
  TORCH_CHECK(gmap_ring.numel() % (M * C * P * P) == 0 && gmap_ring.numel() > 0,
              "gmap ring: [pmem, M, C, P, P]");
  const int64_t pmem = gmap_ring.numel() / (M * C * P * P);
  TORCH_CHECK(imap_ring.numel() == pmem * M * DIM, "imap ring: [pmem, M, DIM]");
  TORCH_CHECK(patches_out.numel() == M * 3 * P * P, "patches_out: float32 [M, 3, P, P]");
  TORCH_CHECK(colors.numel() % (3 * M) == 0 && colors.numel() > 0, "colors: uint8 [N, M, 3]");
  const int64_t N = colors.numel() / (3 * M);
  TORCH_CHECK(N < (1LL << 31) && M < (1LL << 31) && pmem < (1LL << 31), "too large");
  TORCH_CHECK(res > 0 && image.size(1) >= res * h && image.size(2) >= res * w,
              "image must cover res x the feature map");
  const Count nc = a.count(n, n_dev, "n", 0, N - 1);
  const DeviceGuard guard(fmap.device());
  check_status(dpvo_frame_sample(fp, ip, gp, cp, gr, ir, gd, po, co, (int)h, (int)w,
                                 (int)image.size(1), (int)image.size(2), (int)C, (int)DIM, (int)M,
                                 (int)P, (int)res, (int)pmem, (int)N, nc.host, nc.dev,
                                 current_stream()),
               a.fn());
}

// torch.quantile(delta.norm(dim=-1).float(), 0.5) -> fp32 device scalar
torch::Tensor probe_median(torch::Tensor delta) {
  const Entry a("cuda_ba.probe_median");
  int dt;
  const void* dp = a.in(delta, "delta", kF32 | kF16, &dt);
  TORCH_CHECK(delta.numel() > 0 && delta.size(-1) == 2, "delta: [M, 2]");
  const DeviceGuard guard(delta.device());
  const int64_t M = delta.numel() / 2;
  TORCH_CHECK(M < (1LL << 31), "too large");
  auto out = torch::empty({}, delta.options().dtype(torch::kFloat32));
  check_status(dpvo_probe_median(dp, dt, (int)M, out.data_ptr<float>(), current_stream()), a.fn());
  return out;
}

// dpvo.py:805-810 into the patch graph's target / weight rows [0, E)
void update_targets(torch::Tensor coords, torch::Tensor delta, torch::Tensor w,
                    torch::Tensor target, torch::Tensor weight, int64_t E,
                    c10::optional<torch::Tensor> E_dev) {
  const Entry a("cuda_ba.update_targets");
  const float* cp = a.in<float>(coords, "coords");
  int dt;
  const void* dp = a.in(delta, "delta", kF32 | kF16, &dt);
  const void* wp = a.in(w, "w (of delta's dtype)", dt == DPVO_F32 ? kF32 : kF16);
  float* tp = a.buf<float>(target, "target");
  float* gp = a.buf<float>(weight, "weight");
  TORCH_CHECK(coords.dim() >= 3 && coords.size(-1) == coords.size(-2), "coords: [.., E, 2, P, P]");
  const int64_t P = coords.size(-1);
  const int64_t cap = std::min({coords.numel() / (2 * P * P), delta.numel() / 2, w.numel() / 2,
                                target.numel() / 2, weight.numel() / 2});
  TORCH_CHECK(cap < (1LL << 30), "too large");
  const Count ec = a.count(E, E_dev, "E", 0, cap);
  const DeviceGuard guard(coords.device());
  check_status(dpvo_update_targets(cp, dp, wp, dt, tp, gp, (int)P, ec.host, ec.dev, (int)cap,
                                   current_stream()),
               a.fn());
}

// dpvo.py:834-836, the centre pixel only, into points rows [0, m)
void map_points(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                torch::Tensor ix, torch::Tensor points, int64_t m,
                c10::optional<torch::Tensor> m_dev) {
  const Entry a("cuda_ba.map_points");
  const float* pp = a.in<float>(poses, "poses");
  const float* tp = a.in<float>(patches, "patches");
  const float* ip = a.in<float>(intrinsics, "intrinsics");
  const int64_t* xp = a.in<int64_t>(ix, "ix");
  float* op = a.buf<float>(points, "points");
  TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "points: float32 [*, 3]");
  TORCH_CHECK(poses.dim() == 2 && poses.size(1) == 7 && poses.size(0) > 0, "poses: [N, 7]");
  const int64_t N = poses.size(0);
  TORCH_CHECK(intrinsics.numel() == 4 * N, "intrinsics: [N, 4]");
  TORCH_CHECK(patches.dim() == 4 && patches.size(1) == 3 && patches.size(2) == patches.size(3),
              "patches: [*, 3, P, P]");
  const int64_t cap = std::min({patches.size(0), points.size(0), ix.numel()});
  TORCH_CHECK(cap < (1LL << 31) && N < (1LL << 31), "too large");
  const Count mc = a.count(m, m_dev, "m", 0, cap);
  const DeviceGuard guard(poses.device());
  check_status(dpvo_map_points(pp, tp, ip, xp, op, (int)N, (int)patches.size(-1), mc.host, mc.dev,
                               (int)cap, current_stream()),
               a.fn());
}

// ---- match.hip / triangulate.hip: the front half of the long-term loop closure ---
// -> [partner0 [N0], partner1 [N1], matches [min(N0, N1), 2] (int64), dist2, count (int32 [1])]
std::vector<torch::Tensor> match_descriptors(torch::Tensor desc0, torch::Tensor desc1,
                                             double ratio, double max_dist, int64_t n0,
                                             c10::optional<torch::Tensor> n0_dev, int64_t n1,
                                             c10::optional<torch::Tensor> n1_dev) {
  const Entry a("cuda_ba.match_descriptors");
  int dt;
  const void* p0 = a.in(desc0, "desc0", kF32 | kF16, &dt);
  const void* p1 = a.in(desc1, "desc1 (of desc0's dtype)", dt == DPVO_F32 ? kF32 : kF16);
  TORCH_CHECK(desc0.dim() == 2 && desc1.dim() == 2 && desc0.size(1) == desc1.size(1),
              "match_descriptors: desc0 [N0, D], desc1 [N1, D]");
  a.same_device({desc0, desc1});
  const int64_t N0 = desc0.size(0), N1 = desc1.size(0), D = desc0.size(1);
  TORCH_CHECK(N0 >= 1 && N1 >= 1 && N0 <= 4096 && N1 <= 4096,
              "match_descriptors: 1 <= N0, N1 <= 4096, got ", N0, " and ", N1);
  TORCH_CHECK(D >= 4 && D <= 256 && D % 4 == 0,
              "match_descriptors: D must be a multiple of 4 in [4, 256], got ", D);
  TORCH_CHECK(ratio >= 0.0 && max_dist >= 0.0, "match_descriptors: ratio and max_dist must be >= 0");
  const int32_t* d0 = a.opt_buf<int32_t>(n0_dev, "n0");
  const int32_t* d1 = a.opt_buf<int32_t>(n1_dev, "n1");
  // rows are read four elements at a time: a view at an odd offset is copied
  const uintptr_t al = dt == DPVO_F16 ? 7 : 15;
  if ((uintptr_t)p0 & al) p0 = a.in(desc0 = desc0.clone(), "desc0", kF32 | kF16);
  if ((uintptr_t)p1 & al) p1 = a.in(desc1 = desc1.clone(), "desc1", kF32 | kF16);
  const DeviceGuard guard(desc0.device());
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
  check_status(dpvo_match_descriptors(p0, p1, dt, (int)N0, (int)N1, (int)D, d0 ? 0 : (int)n0, d0,
                                      d1 ? 0 : (int)n1, d1, r2, md2, partner0.data_ptr<int64_t>(),
                                      partner1.data_ptr<int64_t>(), matches.data_ptr<int64_t>(),
                                      dist2.data_ptr<float>(), count.data_ptr<int32_t>(),
                                      ws.data_ptr(), wsb, current_stream()),
               a.fn());
  return {partner0, partner1, matches, dist2, count};
}

// -> [points [N1, 3], disp [N1], keep [N1] (bool), sel [N1] (int64), count (int32 [1])]
std::vector<torch::Tensor> triangulate_tracks(torch::Tensor poses, torch::Tensor intrinsics,
                                              torch::Tensor disps, torch::Tensor kps0,
                                              torch::Tensor kps1, torch::Tensor kps2,
                                              torch::Tensor m10, torch::Tensor m12,
                                              double max_depth, double max_residual,
                                              int64_t iterations, double lmbda) {
  const Entry a("cuda_ba.triangulate_tracks");
  const float* pp = a.in<float>(poses, "poses");
  const float* ip = a.in<float>(intrinsics, "intrinsics");
  const float* k0 = a.in<float>(kps0, "kps0");
  const float* k1 = a.in<float>(kps1, "kps1");
  const float* k2 = a.in<float>(kps2, "kps2");
  const int64_t* m0 = a.in<int64_t>(m10, "m10");
  const int64_t* m2 = a.in<int64_t>(m12, "m12");
  // a strided column of the patch depths is read where it is
  const float* dp = a.view<float>(disps, "disps");
  TORCH_CHECK(disps.dim() == 1 && disps.numel() >= 1,
              "triangulate_tracks: disps must be float32 [M]");
  if (disps.stride(0) < 1) dp = a.in<float>(disps, "disps");
  const int64_t stride = disps.stride(0);
  TORCH_CHECK(poses.numel() == 21 && intrinsics.numel() == 12,
              "triangulate_tracks: poses [3, 7] and intrinsics [3, 4] of frames i-1, i, i+1");
  for (const auto* k : {&kps0, &kps1, &kps2})
    TORCH_CHECK(k->dim() == 2 && k->size(1) == 2 && k->size(0) >= 1,
                "triangulate_tracks: keypoints must be [N, 2] with N >= 1");
  const int64_t M = disps.numel(), N0 = kps0.size(0), N1 = kps1.size(0), N2 = kps2.size(0);
  TORCH_CHECK(m10.numel() == N1 && m12.numel() == N1, "triangulate_tracks: m10 / m12 must be [N1]");
  TORCH_CHECK(M <= 1024, "triangulate_tracks: M <= 1024, got ", M);
  TORCH_CHECK(N1 <= 4096 && N0 < (1LL << 31) && N2 < (1LL << 31) && stride < (1LL << 31),
              "triangulate_tracks: N1 <= 4096, got ", N1);
  TORCH_CHECK(iterations >= 0 && lmbda >= 0.0, "triangulate_tracks: iterations, lmbda >= 0");
  const DeviceGuard guard(poses.device());
  auto points = torch::empty({N1, 3}, poses.options());
  auto disp = torch::empty({N1}, poses.options());
  auto keep = torch::empty({N1}, poses.options().dtype(torch::kBool));
  auto sel = torch::empty({N1}, poses.options().dtype(torch::kInt64));
  auto count = torch::empty({1}, poses.options().dtype(torch::kInt32));
  check_status(dpvo_triangulate_tracks(pp, ip, dp, (int)stride, (int)M, k0, (int)N0, k1, (int)N1,
                                       k2, (int)N2, m0, m2, (float)max_depth, (float)max_residual,
                                       (int)iterations, (float)lmbda, points.data_ptr<float>(),
                                       disp.data_ptr<float>(),
                                       reinterpret_cast<uint8_t*>(keep.data_ptr<bool>()),
                                       sel.data_ptr<int64_t>(), count.data_ptr<int32_t>(),
                                       current_stream()),
               a.fn());
  return {points, disp, keep, sel, count};
}

}  // namespace

void bind_tracker(py::module_& m) {
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
}
