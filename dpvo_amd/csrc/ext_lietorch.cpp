// ext_lietorch.cpp -- the `lietorch_backends` extension module (drop-in for
// dpvo/lietorch/src/lietorch.cpp:286-316), bound to the C ABI in dpvo_hot.h.
// Group ids follow dispatch.h:24-45; this build implements SO3 (1), SE3 (3),
// the groups on DPVO's hot path, and Sim3 (4), the group of the loop-closure
// pose graph.  RxSO3 (2) is not built: nothing in DPVO uses it on its own.
#include <climits>

#include "ext_common.hpp"

using namespace dpvo_ext;

enum { OP_EXP = 0, OP_LOG, OP_INV, OP_MUL, OP_ADJ, OP_ADJT, OP_ACT, OP_ACT4, OP_MATRIX, OP_PROJ,
       OP_JINV };

static void check_group(int g) {
  TORCH_CHECK(g == 1 || g == 3 || g == 4, "lietorch_backends: group ", g,
              " not supported by the MI355X build (SO3=1, SE3=3, Sim3=4 implemented)");
}
static int K_of(int g) { return g == 1 ? 3 : g == 3 ? 6 : 7; }
static int N_of(int g) { return K_of(g) + 1; }

// per-op row widths: what the kernels of lie.hip read from X, Y and grad
static int x_dim(int g, int op) { return op == OP_EXP ? K_of(g) : N_of(g); }
static int y_dim(int g, int op) {
  switch (op) {
    case OP_MUL: return N_of(g);
    case OP_ADJ: case OP_ADJT: case OP_JINV: return K_of(g);
    case OP_ACT: return 3;
    case OP_ACT4: return 4;
    default: return 0;  // unary
  }
}
static int grad_dim(int g, int op) {
  switch (op) {
    case OP_EXP: case OP_INV: case OP_MUL: return N_of(g);
    case OP_ACT: return 3;
    case OP_ACT4: return 4;
    default: return K_of(g);  // LOG, ADJ, ADJT
  }
}

// every operand is [n, width] contiguous rows of X's dtype (float32 / float64,
// dispatch.h:41-42) on X's device: the kernels index n * width elements of
// each, so anything else is refused here
static void check_rows(const torch::Tensor& t, const char* name, const torch::Tensor& X, int64_t n,
                       int width) {
  TORCH_CHECK(t.dim() == 2, "lietorch_backends: ", name, " must be 2-D [n, ", width, "], got ",
              t.dim(), "-D");
  TORCH_CHECK(t.size(1) == width, "lietorch_backends: ", name, " must have ", width,
              " columns, got ", t.size(1));
  TORCH_CHECK(t.size(0) == n, "lietorch_backends: ", name, " has ", t.size(0), " rows, X has ", n);
  TORCH_CHECK(t.scalar_type() == X.scalar_type(), "lietorch_backends: ", name,
              " dtype mismatch with X");
}

struct Operands {
  int n, dtype;
  const void *X, *Y, *grad;  // Y / grad null where the op has none
};

// shapes and dtypes of all operands first, then where they live; `grad` is
// null for a forward op
static Operands check_operands(int g, int op, const torch::Tensor& X, const torch::Tensor& Y,
                               const torch::Tensor* grad) {
  const Entry a("lietorch_backends");
  check_group(g);
  TORCH_CHECK(X.defined(), "lietorch_backends: X is undefined");
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 || X.scalar_type() == torch::kFloat64,
              "lietorch_backends: float32 / float64 only (dispatch.h:41-42)");
  TORCH_CHECK(X.dim() == 2, "lietorch_backends: X must be 2-D [n, ", x_dim(g, op), "], got ",
              X.dim(), "-D");
  const int64_t n = X.size(0);
  TORCH_CHECK(n <= INT_MAX, "lietorch_backends: too many rows");
  check_rows(X, "X", X, n, x_dim(g, op));
  const int yd = y_dim(g, op);
  TORCH_CHECK(Y.defined() == (yd > 0), "lietorch_backends: op ", op,
              yd > 0 ? " needs a second operand" : " takes one operand");
  if (yd > 0) check_rows(Y, "Y", X, n, yd);
  if (grad) {
    TORCH_CHECK(grad->defined(), "lietorch_backends: grad is undefined");
    check_rows(*grad, "grad", X, n, grad_dim(g, op));
  }
  Operands o = {(int)n, 0, nullptr, nullptr, nullptr};
  o.X = a.buf(X, "X", kF32 | kF64, &o.dtype);
  if (yd > 0) o.Y = a.buf(Y, "Y", kF32 | kF64);
  if (grad) o.grad = a.buf(*grad, "grad", kF32 | kF64);
  if (yd > 0) a.same_device({X, Y});
  if (grad) a.same_device({X, *grad});
  return o;
}

static torch::Tensor fwd(int g, int op, torch::Tensor X, torch::Tensor Y, int out_dim) {
  const Operands o = check_operands(g, op, X, Y, nullptr);
  const DeviceGuard guard(X.device());
  auto out = torch::empty({o.n, out_dim}, X.options());
  check_status(dpvo_lie_forward(g, op, o.dtype, o.n, o.X, o.Y, out.data_ptr(), current_stream()),
               "lietorch_backends forward");
  return out;
}

static std::vector<torch::Tensor> bwd(int g, int op, torch::Tensor grad, torch::Tensor X,
                                      torch::Tensor Y, int d0, int d1) {
  const Operands o = check_operands(g, op, X, Y, &grad);
  const DeviceGuard guard(X.device());
  auto o0 = torch::empty({o.n, d0}, X.options());
  auto o1 = d1 > 0 ? torch::empty({o.n, d1}, X.options()) : torch::Tensor();
  check_status(dpvo_lie_backward(g, op, o.dtype, o.n, o.grad, o.X, o.Y, o0.data_ptr(),
                                 d1 > 0 ? o1.data_ptr() : nullptr, current_stream()),
               "lietorch_backends backward");
  if (d1 > 0) return {o0, o1};
  return {o0};
}

// ---- lietorch.cpp:18-283 ----
torch::Tensor expm(int g, torch::Tensor a) { return fwd(g, OP_EXP, a, {}, N_of(g)); }
std::vector<torch::Tensor> expm_backward(int g, torch::Tensor grad, torch::Tensor a) {
  return bwd(g, OP_EXP, grad, a, {}, K_of(g), 0);
}
torch::Tensor logm(int g, torch::Tensor X) { return fwd(g, OP_LOG, X, {}, K_of(g)); }
std::vector<torch::Tensor> logm_backward(int g, torch::Tensor grad, torch::Tensor X) {
  return bwd(g, OP_LOG, grad, X, {}, N_of(g), 0);
}
torch::Tensor inv(int g, torch::Tensor X) { return fwd(g, OP_INV, X, {}, N_of(g)); }
std::vector<torch::Tensor> inv_backward(int g, torch::Tensor grad, torch::Tensor X) {
  return bwd(g, OP_INV, grad, X, {}, N_of(g), 0);
}
torch::Tensor mul(int g, torch::Tensor X, torch::Tensor Y) { return fwd(g, OP_MUL, X, Y, N_of(g)); }
std::vector<torch::Tensor> mul_backward(int g, torch::Tensor grad, torch::Tensor X,
                                        torch::Tensor Y) {
  return bwd(g, OP_MUL, grad, X, Y, N_of(g), N_of(g));
}
torch::Tensor adj(int g, torch::Tensor X, torch::Tensor a) { return fwd(g, OP_ADJ, X, a, K_of(g)); }
std::vector<torch::Tensor> adj_backward(int g, torch::Tensor grad, torch::Tensor X,
                                        torch::Tensor a) {
  return bwd(g, OP_ADJ, grad, X, a, N_of(g), K_of(g));
}
torch::Tensor adjT(int g, torch::Tensor X, torch::Tensor a) {
  return fwd(g, OP_ADJT, X, a, K_of(g));
}
std::vector<torch::Tensor> adjT_backward(int g, torch::Tensor grad, torch::Tensor X,
                                         torch::Tensor a) {
  return bwd(g, OP_ADJT, grad, X, a, N_of(g), K_of(g));
}
torch::Tensor act(int g, torch::Tensor X, torch::Tensor p) { return fwd(g, OP_ACT, X, p, 3); }
std::vector<torch::Tensor> act_backward(int g, torch::Tensor grad, torch::Tensor X,
                                        torch::Tensor p) {
  return bwd(g, OP_ACT, grad, X, p, N_of(g), 3);
}
torch::Tensor act4(int g, torch::Tensor X, torch::Tensor p) { return fwd(g, OP_ACT4, X, p, 4); }
std::vector<torch::Tensor> act4_backward(int g, torch::Tensor grad, torch::Tensor X,
                                         torch::Tensor p) {
  return bwd(g, OP_ACT4, grad, X, p, N_of(g), 4);
}
torch::Tensor projector(int g, torch::Tensor X) {
  return fwd(g, OP_PROJ, X, {}, N_of(g) * N_of(g)).view({X.size(0), N_of(g), N_of(g)});
}
torch::Tensor as_matrix(int g, torch::Tensor X) {
  return fwd(g, OP_MATRIX, X, {}, 16).view({X.size(0), 4, 4});
}
torch::Tensor Jinv(int g, torch::Tensor X, torch::Tensor a) {
  return fwd(g, OP_JINV, X, a, K_of(g));
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("expm", &expm, "exp map forward");
  m.def("expm_backward", &expm_backward, "exp map backward");
  m.def("logm", &logm, "log map forward");
  m.def("logm_backward", &logm_backward, "log map backward");
  m.def("inv", &inv, "inverse operator");
  m.def("inv_backward", &inv_backward, "inverse operator backward");
  m.def("mul", &mul, "group operator");
  m.def("mul_backward", &mul_backward, "group operator backward");
  m.def("adj", &adj, "adjoint operator");
  m.def("adj_backward", &adj_backward, "adjoint operator backward");
  m.def("adjT", &adjT, "transposed adjoint operator");
  m.def("adjT_backward", &adjT_backward, "transposed adjoint operator backward");
  m.def("act", &act, "action on point");
  m.def("act_backward", &act_backward, "action on point backward");
  m.def("act4", &act4, "action on homogeneous point");
  m.def("act4_backward", &act4_backward, "action on homogeneous point backward");
  m.def("as_matrix", &as_matrix, "convert to matrix");
  m.def("projector", &projector, "orthogonal projection matrix");
  m.def("Jinv", &Jinv, "left inverse jacobian operator");
  m.attr("native_library") = dpvo_version();
}
