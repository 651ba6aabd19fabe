// ext_common.hpp -- shared glue of the five extension modules (cuda_corr,
// cuda_ba, lietorch_backends, dpvo_update, dpvo_encoder): current HIP stream,
// status -> RuntimeError, and the one vocabulary of argument checks.  A binding
// reaches a caller's tensor only through an Entry method, which checks device,
// dtype and layout before it hands out a pointer; every entry runs its checks
// first and constructs its device guard afterwards, from a checked tensor.
#pragma once

#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <functional>
#include <initializer_list>
#include <vector>

#include "dpvo_hot.h"

namespace dpvo_ext {

using DeviceGuard = c10::hip::OptionalHIPGuardMasqueradingAsCUDA;

inline void* current_stream() {
  return reinterpret_cast<void*>(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream());
}

// true while the current stream is being captured into a hipGraph
inline bool is_capturing() {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream(), &cs);
  return cs != hipStreamCaptureStatusNone;
}

inline void check_status(int st, const char* what) {
  TORCH_CHECK(st == DPVO_OK, what, " failed: ", dpvo_status_string(st), " (status ", st, ")");
}

// floating dtypes an argument may have, as a mask
enum : unsigned { kF32 = 1, kF16 = 2, kF64 = 4 };

inline int dtype_code(const torch::Tensor& t) {
  switch (t.scalar_type()) {
    case torch::kFloat32: return DPVO_F32;
    case torch::kFloat16: return DPVO_F16;
    case torch::kFloat64: return DPVO_F64;
    default: TORCH_CHECK(false, "unsupported dtype ", t.scalar_type());
  }
  return -1;
}

inline const char* dtype_name(c10::ScalarType s) {
  switch (s) {
    case torch::kFloat32: return "float32";
    case torch::kFloat16: return "float16";
    case torch::kFloat64: return "float64";
    case torch::kInt64: return "int64 (long)";
    case torch::kInt32: return "int32";
    case torch::kUInt8: return "uint8";
    default: return c10::toString(s);
  }
}

// host value, or the int32 device scalar read by the kernel when one is given
struct Count {
  int host;
  const int32_t* dev;
};

// the edge sextuple (poses, patches, intrinsics, ii, jj, kk) of the BA,
// reprojection, BA-layer and transform entries; T = float, or void where the
// entry accepts more than one dtype (`dtype` is its DPVO_F* code)
template <class T>
struct Edges {
  T* poses;
  T* patches;
  const T* intrinsics;
  const int64_t *ii, *jj, *kk;
  int E, P, num_poses, num_patches, dtype;
};

// one edge store of the patch graph (Entry::edge_store); absent members are null
struct EdgeStore {
  int64_t *ii, *jj, *kk;
  float *net, *weight, *target;
  int max_edges, DIM;
};

// the new frame and the pyramid slots it is inserted into
struct Pyramid {
  const void* src;
  std::vector<void*> dst;
  std::vector<int> scales;
  int C, H, W, dtype;
};

// The argument checks of one binding function; `fn` names it in every message.
class Entry {
 public:
  explicit Entry(const char* fn) : fn_(fn) {}

  void on_gpu(const torch::Tensor& t, const char* name) const {
    TORCH_CHECK(t.is_cuda(), fn_, ": ", name,
                " must be a GPU (HIP) tensor; the MI355X build has no CPU path");
  }

  // read-only input of dtype T: on the GPU, of that dtype; `t` is made
  // contiguous where it stands (which keeps a copy alive for the call), and a
  // tensor that is contiguous already is kept: no copy, no allocation, no
  // device query
  template <class T>
  const T* in(torch::Tensor& t, const char* name) const {
    typed(t, name, c10::CppTypeToScalarType<T>::value);
    t = t.contiguous();
    return t.data_ptr<T>();
  }
  // ... of one of the floating dtypes of `accept`; *code: its DPVO_F* code
  const void* in(torch::Tensor& t, const char* name, unsigned accept, int* code = nullptr) const {
    floating(t, name, accept, code);
    t = t.contiguous();
    return t.data_ptr();
  }

  // in-place buffer of dtype T: on the GPU, of that dtype, contiguous as it is
  // (a copy would take the kernel's writes with it), at least min_numel long
  template <class T>
  T* buf(const torch::Tensor& t, const char* name, int64_t min_numel = 0) const {
    typed(t, name, c10::CppTypeToScalarType<T>::value);
    dense(t, name, min_numel);
    return t.data_ptr<T>();
  }
  void* buf(const torch::Tensor& t, const char* name, unsigned accept, int* code = nullptr) const {
    floating(t, name, accept, code);
    dense(t, name, 0);
    return t.data_ptr();
  }
  // input of dtype T read where it stands: the entry hands its strides on
  template <class T>
  const T* view(const torch::Tensor& t, const char* name) const {
    typed(t, name, c10::CppTypeToScalarType<T>::value);
    return t.data_ptr<T>();
  }
  const void* view(const torch::Tensor& t, const char* name, unsigned accept,
                   int* code = nullptr) const {
    floating(t, name, accept, code);
    return t.data_ptr();
  }
  // ... of any dtype (frame arrays that are moved as bytes)
  void* buf_bytes(const torch::Tensor& t, const char* name) const {
    on_gpu(t, name);
    dense(t, name, 0);
    return t.data_ptr();
  }
  // a uint8 blob / workspace on `dev`: at least `need` bytes, or exactly
  void* bytes(const torch::Tensor& t, const char* name, const torch::Device& dev, size_t need = 0,
              bool exact = false) const {
    void* p = buf<uint8_t>(t, name);
    TORCH_CHECK(t.device() == dev, fn_, ": ", name, " is on another device than the inputs");
    TORCH_CHECK(exact ? (size_t)t.numel() == need : (size_t)t.numel() >= need, fn_, ": ", name,
                " has ", t.numel(), " bytes, expected ", exact ? "" : "at least ", need);
    return p;
  }

  // optional forms: an undefined, absent or empty tensor gives nullptr
  template <class T>
  T* opt_buf(const torch::Tensor& t, const char* name, int64_t min_numel = 0) const {
    return t.defined() && t.numel() ? buf<T>(t, name, min_numel) : nullptr;
  }
  template <class T>
  T* opt_buf(const c10::optional<torch::Tensor>& t, const char* name, int64_t min_numel = 0) const {
    return t ? opt_buf<T>(*t, name, min_numel) : nullptr;
  }
  template <class T>
  const T* opt_in(c10::optional<torch::Tensor>& t, const char* name) const {
    return t && t->defined() && t->numel() ? in<T>(*t, name) : nullptr;
  }

  // host value v in [lo, hi], or the int32 device scalar `dev` when given
  Count count(int64_t v, const c10::optional<torch::Tensor>& dev, const char* name, int64_t lo,
              int64_t hi) const {
    const int32_t* d = opt_buf<int32_t>(dev, name);
    TORCH_CHECK(d || (v >= lo && v <= hi), fn_, ": ", name, " = ", v, " outside [", lo, ", ", hi,
                "]");
    return {d ? 0 : (int)v, d};
  }

  void same_device(std::initializer_list<std::reference_wrapper<const torch::Tensor>> ts) const {
    for (const torch::Tensor& t : ts)
      TORCH_CHECK(t.device() == ts.begin()->get().device(), fn_, ": tensors on different devices");
  }

  // the kernels read jj[e] and kk[e] for every e < ii.numel()
  void one_length(const torch::Tensor& ii, const torch::Tensor& jj, const torch::Tensor& kk) const {
    TORCH_CHECK(jj.numel() == ii.numel() && kk.numel() == ii.numel(), fn_,
                ": ii, jj, kk must have equal length");
  }

  // The edge inputs: GPU tensors of one floating dtype of `accept` / int64,
  // made contiguous, ii / jj / kk of one length.  Non-contiguous poses /
  // patches are copied, which suits every reader; the in-place BA entries
  // check them with buf() first.  shapes: poses [.., N, 7], patches
  // [.., M, 3, P, P], intrinsics [.., N, 4] are required too.
  Edges<void> edges(torch::Tensor& poses, torch::Tensor& patches, torch::Tensor& intrinsics,
                    torch::Tensor& ii, torch::Tensor& jj, torch::Tensor& kk, unsigned accept,
                    bool shapes) const {
    Edges<void> e;
    e.poses = const_cast<void*>(in(poses, "poses", accept, &e.dtype));
    const unsigned same = e.dtype == DPVO_F32 ? kF32 : e.dtype == DPVO_F64 ? kF64 : kF16;
    e.patches = const_cast<void*>(in(patches, "patches", same));
    e.intrinsics = in(intrinsics, "intrinsics", same);
    e.ii = in<int64_t>(ii, "ii");
    e.jj = in<int64_t>(jj, "jj");
    e.kk = in<int64_t>(kk, "kk");
    one_length(ii, jj, kk);
    if (shapes) {
      TORCH_CHECK(poses.dim() >= 2 && poses.size(-1) == 7, fn_, ": poses must be [.., N, 7]");
      TORCH_CHECK(patches.dim() >= 4 && patches.size(-3) == 3 &&
                      patches.size(-1) == patches.size(-2),
                  fn_, ": patches must be [.., M, 3, P, P]");
    }
    e.E = ii.numel();
    e.P = patches.size(-1);
    e.num_poses = poses.numel() / 7;
    e.num_patches = patches.numel() / (3 * (int64_t)e.P * e.P);
    TORCH_CHECK(!shapes || intrinsics.numel() == 4 * (int64_t)e.num_poses, fn_,
                ": intrinsics must be [.., N, 4]");
    return e;
  }
  // float32 only, with typed pointers
  Edges<float> edges(torch::Tensor& poses, torch::Tensor& patches, torch::Tensor& intrinsics,
                     torch::Tensor& ii, torch::Tensor& jj, torch::Tensor& kk,
                     bool shapes = false) const {
    const Edges<void> v = edges(poses, patches, intrinsics, ii, jj, kk, kF32, shapes);
    return {static_cast<float*>(v.poses), static_cast<float*>(v.patches),
            static_cast<const float*>(v.intrinsics), v.ii, v.jj, v.kk, v.E, v.P, v.num_poses,
            v.num_patches, v.dtype};
  }

  // one edge store of the patch graph from its list of n tensors, every one an
  // in-place buffer: [ii, jj, kk, net, weight, target] (6), the same without
  // net (5), or the live arrays [ii, jj, kk, net] alone (4).  ii fixes
  // max_edges, the others are at least as long; net may be empty
  EdgeStore edge_store(const std::vector<torch::Tensor>& s, const char* name, size_t n) const {
    TORCH_CHECK(s.size() == n, fn_, ": ", name, " must hold ", n, " tensors of [ii, jj, kk, net, "
                "weight, target]");
    EdgeStore e = {};
    e.ii = buf<int64_t>(s[0], name);
    e.max_edges = s[0].numel();
    e.jj = buf<int64_t>(s[1], name, e.max_edges);
    e.kk = buf<int64_t>(s[2], name, e.max_edges);
    if (n != 5) e.net = opt_buf<float>(s[3], name);
    e.DIM = e.net && e.max_edges ? (int)(s[3].numel() / e.max_edges) : 0;
    if (n > 4) e.weight = buf<float>(s[n - 2], name, 2 * (int64_t)e.max_edges);
    if (n > 4) e.target = buf<float>(s[n - 1], name, 2 * (int64_t)e.max_edges);
    return e;
  }

  // The frame insertion of a channels-last pyramid: src [C, H, W] (the level-1
  // NCHW frame, float32 / float16, made contiguous), dst[l] [C, H/s, W/s] views
  // of src's dtype in channels-last memory (one ring slot); `name` names dst
  Pyramid pyramid(torch::Tensor& src, const std::vector<torch::Tensor>& dst,
                  const std::vector<int64_t>& scales, const char* name) const {
    Pyramid p;
    on_gpu(src, "src");
    TORCH_CHECK(src.dim() == 3, fn_, ": src must be [C, H, W]");
    TORCH_CHECK(dst.size() == scales.size() && !dst.empty(), fn_, ": one scale per ", name,
                " level");
    p.src = in(src, "src", kF32 | kF16, &p.dtype);
    p.C = src.size(0), p.H = src.size(1), p.W = src.size(2);
    for (size_t l = 0; l < dst.size(); l++) {
      const torch::Tensor& d = dst[l];
      on_gpu(d, name);
      const int s = (int)scales[l];
      TORCH_CHECK(d.scalar_type() == src.scalar_type() && d.dim() == 3 && d.size(0) == p.C &&
                      s > 0 && d.size(1) == p.H / s && d.size(2) == p.W / s,
                  fn_, ": ", name, " level ", l, " must be [C, H/s, W/s] of src's dtype");
      TORCH_CHECK(d.stride(0) == 1 && d.stride(2) == p.C &&
                      d.stride(1) == (int64_t)p.C * d.size(2),
                  fn_, ": ", name, " level ", l, " must be channels-last");
      p.dst.push_back(d.data_ptr());
      p.scales.push_back(s);
    }
    return p;
  }

  // ---- the weight-packing glue of dpvo_update / dpvo_encoder ----
  int wdtype_code(int64_t code) const {
    TORCH_CHECK(code == DPVO_F32 || code == DPVO_F16, fn_, ": weights are float32 or float16");
    return (int)code;
  }
  // n CPU float32 tensors in state_dict order, numel(i) elements each (made contiguous)
  std::vector<const float*> host_params(std::vector<torch::Tensor>& ts, size_t n,
                                        const std::function<int64_t(size_t)>& numel) const {
    TORCH_CHECK(ts.size() == n, fn_, ": expected the ", n, " parameter tensors, got ", ts.size());
    std::vector<const float*> ptrs;
    for (size_t i = 0; i < n; i++) {
      torch::Tensor& t = ts[i];
      TORCH_CHECK(!t.is_cuda() && t.scalar_type() == torch::kFloat32, fn_, ": tensor ", i,
                  " must be a CPU float32 tensor");
      TORCH_CHECK(t.numel() == numel(i), fn_, ": tensor ", i, " has ", t.numel(),
                  " elements, expected ", numel(i));
      t = t.contiguous();
      ptrs.push_back(t.data_ptr<float>());
    }
    return ptrs;
  }
  // n contiguous float32 tensors on `dev`, numel(i) elements each
  std::vector<float*> device_params(const std::vector<torch::Tensor>& ts, size_t n,
                                    const std::function<int64_t(size_t)>& numel,
                                    const torch::Device& dev, const char* what) const {
    TORCH_CHECK(ts.size() == n, fn_, ": expected ", n, " ", what, " tensors, got ", ts.size());
    std::vector<float*> ptrs;
    for (size_t i = 0; i < n; i++) {
      ptrs.push_back(buf<float>(ts[i], what));
      TORCH_CHECK(ts[i].device() == dev && ts[i].numel() == numel(i), fn_, ": ", what, " tensor ",
                  i, " must have ", numel(i), " elements on the inputs' device");
    }
    return ptrs;
  }

  const char* fn() const { return fn_; }

 private:
  void typed(const torch::Tensor& t, const char* name, c10::ScalarType want) const {
    on_gpu(t, name);
    TORCH_CHECK(t.scalar_type() == want, fn_, ": ", name, " must be ", dtype_name(want), ", got ",
                t.scalar_type());
  }
  void floating(const torch::Tensor& t, const char* name, unsigned accept, int* code) const {
    on_gpu(t, name);
    const auto s = t.scalar_type();
    const unsigned bit = s == torch::kFloat32 ? kF32 : s == torch::kFloat16 ? kF16
                         : s == torch::kFloat64 ? kF64 : 0u;
    TORCH_CHECK(bit & accept, fn_, ": ", name, " must be ",
                accept == kF32 ? "float32" : accept == kF64 ? "float64" : accept == kF16 ? "float16"
                : accept == (kF32 | kF16) ? "float32 or float16" : accept == (kF32 | kF64)
                ? "float32 or float64" : "float32, float16 or float64", ", got ", s);
    if (code) *code = dtype_code(t);
  }
  void dense(const torch::Tensor& t, const char* name, int64_t min_numel) const {
    TORCH_CHECK(t.is_contiguous(), fn_, ": ", name, " must be contiguous (updated in place)");
    TORCH_CHECK(t.numel() >= min_numel, fn_, ": ", name, " needs at least ", min_numel,
                " elements, has ", t.numel());
  }

  const char* fn_;
};

}  // namespace dpvo_ext
