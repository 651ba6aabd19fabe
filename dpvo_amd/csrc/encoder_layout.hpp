// encoder_layout.hpp -- what encoder.hip (forward) and encoder_bwd.hip
// (backward) share: the eleven convolutions' shapes, the size rules and the
// layout of the `saved` buffer that dpvo_encoder_forward_train fills and
// dpvo_encoder_backward reads.
#pragma once

#include "common.hpp"

namespace dpvo {
namespace enc {

constexpr int kConvs = 11;
constexpr float kInEps = 1e-5f;
constexpr int kK0 = 147, kK0Pad = 160;

struct ConvShape { int cin, cout, kh, stride; };
inline ConvShape conv_shape(int ci, int out_dim) {
  switch (ci) {
    case 0: return {3, 32, 7, 2};
    case 1: case 2: case 3: case 4: return {32, 32, 3, 1};
    case 5: return {32, 64, 3, 2};
    case 7: return {32, 64, 1, 2};
    case 10: return {64, out_dim, 1, 1};
    default: return {64, 64, 3, 1};
  }
}
inline bool out_dim_ok(int d) { return d >= 64 && d <= 1024 && d % 64 == 0; }
inline bool norm_ok(int norm) {
  return norm == DPVO_ENCODER_NORM_NONE || norm == DPVO_ENCODER_NORM_INSTANCE;
}
inline int down(int n) { return (n - 1) / 2 + 1; }
inline size_t r256(size_t n) { return (n + 255) & ~(size_t)255; }
inline size_t max_parts(int H1, int W1) { return (size_t)((H1 + 3) / 4) * ((W1 + 15) / 16); }
inline bool dims_ok(int n, int H, int W) {
  // grid limits and 32-bit pixel counts
  return n <= 65535 && H <= 65536 && W <= 65536 &&
         (size_t)n * down(H) * down(W) <= (size_t)0x7fffffff / 64;
}

struct Dims { int n, H, W, H1, W1, H2, W2; };
inline Dims make_dims(int n, int H, int W) {
  return Dims{n, H, W, down(H), down(W), down(down(H)), down(down(W))};
}

// --- the saved buffer (channels-last fp32 planes, each rounded up to 256 B) ----
//   'instance': h[0..4] raw y0..y4, h[5], h[6] the outputs of layer1.0, layer1.1
//               q[0..4] raw y5..y9, q[5], q[6] the outputs of layer2.0, layer2.1
//               part    the forward's statistic partials (scratch)
//               stat    ten (mean, rstd) sets [n, 64, 2], conv i at set i
//   'none':     h[0..4], q[0..4] the post-epilogue outputs of convs 0..4, 5..9
// h planes are [n, H1, W1, 32], q planes [n, H2, W2, 64].
struct Saved {
  float* h[7];
  float* q[7];
  double* part;
  float* stat;
};
inline size_t half_plane_bytes(const Dims& d) { return r256((size_t)d.n * d.H1 * d.W1 * 32 * 4); }
inline size_t quarter_plane_bytes(const Dims& d) { return r256((size_t)d.n * d.H2 * d.W2 * 64 * 4); }
inline size_t stat_part_bytes(const Dims& d) {
  return r256((size_t)d.n * max_parts(d.H1, d.W1) * 64 * 3 * 8);
}
inline size_t stat_bytes(const Dims& d) { return r256((size_t)10 * d.n * 64 * 2 * 4); }
inline size_t saved_bytes(const Dims& d, bool instance) {
  const int planes = instance ? 7 : 5;
  return planes * (half_plane_bytes(d) + quarter_plane_bytes(d)) +
         (instance ? stat_part_bytes(d) + stat_bytes(d) : 0);
}
inline Saved saved_carve(void* base, const Dims& d, bool instance) {
  const int planes = instance ? 7 : 5;
  char* p = (char*)base;
  Saved s{};
  for (int i = 0; i < planes; i++) { s.h[i] = (float*)p; p += half_plane_bytes(d); }
  for (int i = 0; i < planes; i++) { s.q[i] = (float*)p; p += quarter_plane_bytes(d); }
  if (instance) {
    s.part = (double*)p;
    p += stat_part_bytes(d);
    s.stat = (float*)p;
  }
  return s;
}
inline float* saved_stat(const Saved& s, const Dims& d, int i) {
  return s.stat + (size_t)i * d.n * 64 * 2;
}

}  // namespace enc
}  // namespace dpvo
