// ext_ba_graph.cpp -- cuda_ba, part 2: PatchGraph bookkeeping and the keyframe
// decision on the device (dpvo.py:480-673, patchgraph.py:65-91), bound to
// pg.hip / keyframe.hip.  No call synchronises with the host.
#include "ext_common.hpp"

using namespace dpvo_ext;

namespace {

// append_factors: n (device scalar) or kk_new.numel() new edges
void append(const char* fn, torch::Tensor ix, torch::Tensor kk_new, torch::Tensor jj_new,
            const torch::Tensor* n_dev, const std::vector<torch::Tensor>& live,
            const torch::Tensor& counts) {
  const Entry a(fn);
  const int64_t* ixp = a.in<int64_t>(ix, "ix");
  const int64_t* kn = a.in<int64_t>(kk_new, "kk");
  const int64_t* jn = a.in<int64_t>(jj_new, "jj");
  TORCH_CHECK(kk_new.numel() == jj_new.numel(), fn, ": kk / jj sizes differ");
  const EdgeStore l = a.edge_store(live, "ii / jj / kk / net", 4);
  int32_t* cp = a.buf<int32_t>(counts, "counts (edges, inactive edges, errors)", 3);
  const int32_t* nd = n_dev ? a.buf<int32_t>(*n_dev, "n_dev", 1) : nullptr;
  const DeviceGuard guard(counts.device());
  if (nd)
    check_status(dpvo_pg_append_dev(ixp, kn, jn, nd, (int)kk_new.numel(), l.ii, l.jj, l.kk, l.net,
                                    l.DIM, cp, l.max_edges, current_stream()),
                 fn);
  else
    check_status(dpvo_pg_append(ixp, kn, jn, kk_new.numel(), l.ii, l.jj, l.kk, l.net, l.DIM, cp,
                                l.max_edges, current_stream()),
                 fn);
}

void pg_append(torch::Tensor ix, torch::Tensor kk_new, torch::Tensor jj_new, torch::Tensor ii,
               torch::Tensor jj, torch::Tensor kk, torch::Tensor net, torch::Tensor counts) {
  append("cuda_ba.pg_append", ix, kk_new, jj_new, nullptr, {ii, jj, kk, net}, counts);
}

void pg_append_dev(torch::Tensor ix, torch::Tensor kk_new, torch::Tensor jj_new,
                   torch::Tensor n_dev, torch::Tensor ii, torch::Tensor jj, torch::Tensor kk,
                   torch::Tensor net, torch::Tensor counts) {
  append("cuda_ba.pg_append_dev", ix, kk_new, jj_new, &n_dev, {ii, jj, kk, net}, counts);
}

// what the three removals share: the active and back stores, the inactive one
// (absent for the frame drop), counts and the pos scratch [max_edges]
struct Removal {
  EdgeStore A, B, I;
  int32_t *counts, *pos;
};

Removal removal(const Entry& a, const std::vector<torch::Tensor>& act,
                const std::vector<torch::Tensor>& back, const std::vector<torch::Tensor>* inac,
                const torch::Tensor& counts, const torch::Tensor& pos) {
  Removal r;
  r.A = a.edge_store(act, "act", 6);
  r.B = a.edge_store(back, "back", 6);
  r.I = inac ? a.edge_store(*inac, "inac", 5) : EdgeStore{};
  r.counts = a.buf<int32_t>(counts, "counts");
  r.pos = a.buf<int32_t>(pos, "pos");
  return r;
}

// the sizes, after every tensor of the entry has passed its own checks: the
// kernels index all stores and pos by the active store's max_edges, and keep
// the new edge counts in counts[3..4] between their two launches
void removal_sizes(const Entry& a, const Removal& r, bool inac, const torch::Tensor& counts,
                   const torch::Tensor& pos) {
  TORCH_CHECK(r.B.max_edges >= r.A.max_edges && r.B.DIM == r.A.DIM &&
                  (!inac || r.I.max_edges >= r.A.max_edges) && pos.numel() >= r.A.max_edges,
              a.fn(), ": back, inac and pos must be as large as act (", r.A.max_edges,
              " edges, DIM ", r.A.DIM, ")");
  TORCH_CHECK(counts.numel() >= 5, a.fn(), ": counts needs 5 int32 words (edges, inactive edges, "
              "errors, 2 scratch), has ", counts.numel());
}

void pg_remove(c10::optional<torch::Tensor> mask, c10::optional<torch::Tensor> ix, int64_t thresh,
               int64_t lc_min, bool store, std::vector<torch::Tensor> act,
               std::vector<torch::Tensor> back, std::vector<torch::Tensor> inac,
               torch::Tensor counts, torch::Tensor pos) {
  const Entry a("cuda_ba.pg_remove");
  const Removal r = removal(a, act, back, &inac, counts, pos);
  const bool masked = mask && mask->defined();
  if (masked) a.on_gpu(*mask, "mask");
  const int64_t* ixp = a.opt_in<int64_t>(ix, "ix");
  removal_sizes(a, r, true, counts, pos);
  const DeviceGuard guard(counts.device());
  torch::Tensor m8;
  if (masked) m8 = mask->to(torch::kUInt8);
  const uint8_t* mp = masked ? a.in<uint8_t>(m8, "mask") : nullptr;
  check_status(dpvo_pg_remove(mp, ixp, thresh, lc_min, store ? 1 : 0, r.A.ii, r.A.jj, r.A.kk,
                              r.A.net, r.A.weight, r.A.target, r.B.ii, r.B.jj, r.B.kk, r.B.net,
                              r.B.weight, r.B.target, r.I.ii, r.I.jj, r.I.kk, r.I.weight, r.I.target,
                              r.A.DIM, r.counts, r.pos, r.A.max_edges, current_stream()),
               a.fn());
}

void pg_remove_window_dev(torch::Tensor ix, torch::Tensor n_dev, int64_t thresh_off,
                          int64_t lc_off, bool lc_on, bool store, std::vector<torch::Tensor> act,
                          std::vector<torch::Tensor> back, std::vector<torch::Tensor> inac,
                          torch::Tensor counts, torch::Tensor pos) {
  const Entry a("cuda_ba.pg_remove_window_dev");
  const Removal r = removal(a, act, back, &inac, counts, pos);
  const int64_t* ixp = a.in<int64_t>(ix, "ix");
  const int32_t* nd = a.buf<int32_t>(n_dev, "n_dev", 1);
  removal_sizes(a, r, true, counts, pos);
  const DeviceGuard guard(counts.device());
  check_status(dpvo_pg_remove_window_dev(ixp, nd, thresh_off, lc_off, lc_on ? 1 : 0, store ? 1 : 0,
                                         r.A.ii, r.A.jj, r.A.kk, r.A.net, r.A.weight, r.A.target,
                                         r.B.ii, r.B.jj, r.B.kk, r.B.net, r.B.weight, r.B.target,
                                         r.I.ii, r.I.jj, r.I.kk, r.I.weight, r.I.target, r.A.DIM,
                                         r.counts, r.pos, r.A.max_edges, current_stream()),
               a.fn());
}

void pg_remove_frame_dev(torch::Tensor kf, std::vector<torch::Tensor> act,
                         std::vector<torch::Tensor> back, torch::Tensor counts, torch::Tensor pos) {
  const Entry a("cuda_ba.pg_remove_frame_dev");
  const Removal r = removal(a, act, back, nullptr, counts, pos);
  const int32_t* kp = a.buf<int32_t>(kf, "kf", 2);
  removal_sizes(a, r, false, counts, pos);
  const DeviceGuard guard(counts.device());
  check_status(dpvo_pg_remove_frame_dev(kp, r.A.ii, r.A.jj, r.A.kk, r.A.net, r.A.weight, r.A.target,
                                        r.B.ii, r.B.jj, r.B.kk, r.B.net, r.B.weight, r.B.target,
                                        r.A.DIM, r.counts, r.pos, r.A.max_edges, current_stream()),
               a.fn());
}

// DPVO.keyframe decision (dpvo.py:586-624): kf = {drop, k}, mag = both motionmags
void kf_motion(torch::Tensor ii, torch::Tensor jj, torch::Tensor kk, torch::Tensor counts,
               torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
               torch::Tensor st, int64_t keyframe_index, double keyframe_thresh, torch::Tensor kf,
               torch::Tensor mag) {
  const Entry a("cuda_ba.kf_motion");
  const float* pp = a.buf<float>(poses, "poses");
  const float* tp = a.buf<float>(patches, "patches");
  const float* ip = a.buf<float>(intrinsics, "intrinsics");
  int32_t* kp = a.buf<int32_t>(kf, "kf", 2);
  float* mp = a.buf<float>(mag, "mag", 2);
  const int64_t* iip = a.in<int64_t>(ii, "ii");
  const int64_t* jjp = a.in<int64_t>(jj, "jj");
  const int64_t* kkp = a.in<int64_t>(kk, "kk");
  const int32_t* cp = a.buf<int32_t>(counts, "counts", 1);
  const int32_t* sp = a.buf<int32_t>(st, "st", 1);
  const DeviceGuard guard(poses.device());
  check_status(dpvo_kf_motion(iip, jjp, kkp, cp, pp, tp, ip, (int)patches.size(-1), sp,
                              (int)keyframe_index, keyframe_thresh, kp, mp, current_stream()),
               a.fn());
}

// the rest of the frame drop (dpvo.py:626-673); frames: per-frame arrays whose
// leading dim is the frame (ring 0) or a ring slot (ring > 0)
void kf_shift(torch::Tensor kf, int64_t M, torch::Tensor st, torch::Tensor ii, torch::Tensor jj,
              torch::Tensor kk, torch::Tensor counts, std::vector<torch::Tensor> frames,
              std::vector<int64_t> rings, c10::optional<torch::Tensor> poses,
              c10::optional<torch::Tensor> tstamps, c10::optional<torch::Tensor> delta_log,
              c10::optional<torch::Tensor> delta_tstamps, c10::optional<torch::Tensor> delta_count) {
  const Entry a("cuda_ba.kf_shift");
  TORCH_CHECK(frames.size() == rings.size(), a.fn(), ": one ring size per frame array");
  std::vector<void*> ptrs;
  std::vector<int64_t> bytes;
  std::vector<int32_t> ring;
  for (size_t f = 0; f < frames.size(); f++) {
    ptrs.push_back(a.buf_bytes(frames[f], "frame array"));
    TORCH_CHECK(frames[f].dim() >= 1, a.fn(), ": frame arrays need a leading frame dimension");
    bytes.push_back(frames[f].numel() / frames[f].size(0) * frames[f].element_size());
    ring.push_back((int32_t)rings[f]);
  }
  const bool log = delta_log && delta_log->defined();
  float* dl = nullptr;
  int64_t* dt = nullptr;
  int32_t* dc = nullptr;
  const float* pp = nullptr;
  const int64_t* ts = nullptr;
  int cap = 0;
  if (log) {
    TORCH_CHECK(poses && tstamps && delta_tstamps && delta_count, a.fn(),
                ": delta log needs all buffers");
    dl = a.buf<float>(*delta_log, "delta_log");
    dt = a.buf<int64_t>(*delta_tstamps, "delta_tstamps");
    dc = a.buf<int32_t>(*delta_count, "delta_count", 1);
    pp = a.buf<float>(*poses, "poses");
    ts = a.buf<int64_t>(*tstamps, "tstamps");
    cap = (int)(delta_log->numel() / 7);
  }
  // with a delta log the kernel ORs its overflow bit into counts[2]
  // (keyframe.hip kf_delta_kernel): counts must hold the error word too
  int32_t* cp = a.buf<int32_t>(counts, "counts (n, m, errors)", log ? 3 : 1);
  const int32_t* kp = a.buf<int32_t>(kf, "kf", 2);
  int32_t* sp = a.buf<int32_t>(st, "st (n, m)", 2);
  int64_t* iip = a.buf<int64_t>(ii, "ii");
  int64_t* jjp = a.buf<int64_t>(jj, "jj", ii.numel());
  int64_t* kkp = a.buf<int64_t>(kk, "kk", ii.numel());
  const DeviceGuard guard(counts.device());
  check_status(dpvo_kf_shift(kp, (int)M, sp, iip, jjp, kkp, cp, (int)ii.numel(), ptrs.data(),
                             bytes.data(), ring.data(), (int)ptrs.size(), pp, ts, dl, dt, dc, cap,
                             current_stream()),
               a.fn());
}

// PatchGraph.edges_loop (patchgraph.py:65-91) gated as dpvo.py:984-988
void edges_loop(torch::Tensor poses, torch::Tensor patches, torch::Tensor intrinsics,
                torch::Tensor ix, int64_t M, torch::Tensor st, int64_t n_cap,
                c10::optional<torch::Tensor> last_global_ba, int64_t removal_window,
                int64_t max_edge_age, int64_t global_opt_freq, int64_t keyframe_index,
                double backend_thresh, int64_t max_num_edges, int64_t nms, torch::Tensor work,
                torch::Tensor out_kk, torch::Tensor out_jj, torch::Tensor out_n,
                c10::optional<torch::Tensor> errors) {
  const Entry a("cuda_ba.edges_loop");
  const float* pp = a.buf<float>(poses, "poses");
  const float* tp = a.buf<float>(patches, "patches");
  const float* ip = a.buf<float>(intrinsics, "intrinsics");
  const int64_t* ixp = a.in<int64_t>(ix, "ix");
  const int32_t* sp = a.buf<int32_t>(st, "st", 1);
  int32_t* lb = a.opt_buf<int32_t>(last_global_ba, "last_global_ba");
  int32_t* err = a.opt_buf<int32_t>(errors, "errors");
  float* wp = a.buf<float>(work, "work", (int64_t)dpvo_edges_loop_work_floats());
  TORCH_CHECK(M > 0 && patches.dim() >= 1 &&
                  patches.numel() % (M * 3 * patches.size(-1) * patches.size(-1)) == 0,
              a.fn(), ": patches must be [N * M, 3, P, P]");
  TORCH_CHECK(max_num_edges >= 0, a.fn(), ": max_num_edges < 0");
  int64_t* ok = a.buf<int64_t>(out_kk, "out_kk (max_num_edges x M)", max_num_edges * M);
  int64_t* oj = a.buf<int64_t>(out_jj, "out_jj (max_num_edges x M)", max_num_edges * M);
  int32_t* on = a.buf<int32_t>(out_n, "out_n", 1);
  const DeviceGuard guard(poses.device());
  check_status(dpvo_edges_loop(pp, tp, ip, ixp, (int)patches.size(-1), (int)M, sp, (int)n_cap, lb,
                               (int)removal_window, (int)max_edge_age, (int)global_opt_freq,
                               (int)keyframe_index, (float)backend_thresh, (int)max_num_edges,
                               (int)nms, wp, ok, oj, on, err, current_stream()),
               a.fn());
}

}  // namespace

void bind_graph(py::module_& m) {
  m.def("pg_append", &pg_append, "PatchGraph.append_factors on the device (dpvo.py:480-521)");
  m.def("pg_remove", &pg_remove, "PatchGraph.remove_factors on the device (dpvo.py:523-568)");
  m.def("pg_remove_window_dev", &pg_remove_window_dev,
        "DPVO.keyframe window removal with thresholds relative to a device frame count");
  m.def("pg_append_dev", &pg_append_dev, "append_factors with a device edge count");
  m.def("pg_remove_frame_dev", &pg_remove_frame_dev,
        "DPVO.keyframe frame-drop removal predicated on the device decision kf");
  m.def("kf_motion", &kf_motion, "DPVO.keyframe motion magnitude + decision (dpvo.py:586-624)");
  m.def("kf_shift", &kf_shift, "DPVO.keyframe frame drop: delta log, edge / frame shift, counters",
        py::arg("kf"), py::arg("M"), py::arg("st"), py::arg("ii"), py::arg("jj"), py::arg("kk"),
        py::arg("counts"), py::arg("frames"), py::arg("rings"), py::arg("poses") = py::none(),
        py::arg("tstamps") = py::none(), py::arg("delta_log") = py::none(),
        py::arg("delta_tstamps") = py::none(), py::arg("delta_count") = py::none());
  m.def("edges_loop", &edges_loop, "PatchGraph.edges_loop (patchgraph.py:65-91), device count");
  m.def("edges_loop_work_floats", []() { return (int64_t)dpvo_edges_loop_work_floats(); });
}
