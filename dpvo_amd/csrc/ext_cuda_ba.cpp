// ext_cuda_ba.cpp -- the `cuda_ba` extension module (drop-in for
// dpvo/fastba/ba.cpp:183-189), bound to the C ABI in dpvo_hot.h.  One module,
// four sources, one per subsystem:
//   ext_ba_solve.cpp    BA, reprojection, BA status, split / large-graph BA,
//                       SPD solves, pose-graph solve / residual, RANSAC-Umeyama
//   ext_ba_graph.cpp    patch graph and keyframe (pg_*, kf_*, edges_loop)
//   ext_ba_train.cpp    differentiable BA layer, transforms, losses, dataset
//   ext_ba_tracker.cpp  tracker, front end, stream, evaluate, match, triangulate
#include "ext_common.hpp"

void bind_solve(py::module_& m);
void bind_graph(py::module_& m);
void bind_train(py::module_& m);
void bind_tracker(py::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  bind_solve(m);
  bind_graph(m);
  bind_train(m);
  bind_tracker(m);
  m.attr("native_library") = dpvo_version();
}
