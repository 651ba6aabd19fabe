// sim3_host_main.cpp -- dpvo_amd/csrc/sim3.hpp on the host, for
// tests/test_sim3_host.py.  Compiled as HIP (the header's functions are
// __host__ __device__), it makes no HIP call and needs no device:
//
//   sim3_host fwd|bwd OP N IN OUT
//
// IN and OUT are files of raw doubles, row-major blocks of N rows each:
//   fwd: IN = X [N, xin], Y [N, yin]            OUT = out [N, out]
//   bwd: IN = grad [N, gin], X [N, xin], Y      OUT = o0 [N, d0], o1 [N, d1]
// with the widths of lietorch group 4 (K = 7, N = 8), the ones lie.hip uses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sim3.hpp"

namespace {

constexpr int K = 7, N = 8;
struct Dims { int xin, yin, out, gin, o0, o1; };

Dims fwd_dims(int op) {
  using namespace dpvo::sim3;
  switch (op) {
    case EXP: return {K, 0, N, 0, 0, 0};
    case LOG: return {N, 0, K, 0, 0, 0};
    case INV: return {N, 0, N, 0, 0, 0};
    case MUL: return {N, N, N, 0, 0, 0};
    case ACT: return {N, 3, 3, 0, 0, 0};
    case ACT4: return {N, 4, 4, 0, 0, 0};
    case MATRIX: return {N, 0, 16, 0, 0, 0};
    case PROJ: return {N, 0, N * N, 0, 0, 0};
    default: return {N, K, K, 0, 0, 0};  // ADJ, ADJT, JINV
  }
}
Dims bwd_dims(int op) {
  using namespace dpvo::sim3;
  switch (op) {
    case EXP: return {K, 0, 0, N, K, 0};
    case LOG: return {N, 0, 0, K, N, 0};
    case INV: return {N, 0, 0, N, N, 0};
    case MUL: return {N, N, 0, N, N, N};
    case ACT: return {N, 3, 0, 3, N, 3};
    case ACT4: return {N, 4, 0, 4, N, 4};
    default: return {N, K, 0, K, N, K};  // ADJ, ADJT
  }
}

bool read_all(const char* path, std::vector<double>& v) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  const size_t got = std::fread(v.data(), sizeof(double), v.size(), f);
  const bool end = std::fgetc(f) == EOF;
  std::fclose(f);
  return got == v.size() && end;
}
bool write_all(const char* path, const std::vector<double>& v) {
  FILE* f = std::fopen(path, "wb");
  if (!f) return false;
  const size_t put = std::fwrite(v.data(), sizeof(double), v.size(), f);
  return std::fclose(f) == 0 && put == v.size();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s fwd|bwd OP N IN OUT\n", argv[0]);
    return 2;
  }
  const bool back = std::strcmp(argv[1], "bwd") == 0;
  if (!back && std::strcmp(argv[1], "fwd") != 0) return 2;
  const int op = std::atoi(argv[2]);
  const long n = std::atol(argv[3]);
  if (op < 0 || op > (back ? dpvo::sim3::ACT4 : dpvo::sim3::JINV) || n < 0 || n > (1 << 20)) return 2;
  const Dims d = back ? bwd_dims(op) : fwd_dims(op);
  std::vector<double> in((size_t)n * (d.gin + d.xin + d.yin));
  std::vector<double> out((size_t)n * (d.out + d.o0 + d.o1));
  if (!read_all(argv[4], in)) {
    std::fprintf(stderr, "%s: expected %zu doubles\n", argv[4], in.size());
    return 3;
  }
  const double* G = in.data();
  const double* X = G + (size_t)n * d.gin;
  const double* Y = X + (size_t)n * d.xin;
  double* O0 = out.data();
  double* O1 = O0 + (size_t)n * d.o0;
  for (long i = 0; i < n; i++) {
    // the registers of lie_fwd_kernel / lie_bwd_kernel
    double x[8] = {0}, y[8] = {0}, g[8] = {0}, a[8] = {0}, b[8] = {0}, o[64];
    for (int k = 0; k < d.xin; k++) x[k] = X[i * d.xin + k];
    for (int k = 0; k < d.yin; k++) y[k] = Y[i * d.yin + k];
    if (!back) {
      dpvo::sim3::fwd(op, x, y, o);
      for (int k = 0; k < d.out; k++) out[i * d.out + k] = o[k];
    } else {
      for (int k = 0; k < d.gin; k++) g[k] = G[i * d.gin + k];
      dpvo::sim3::bwd(op, g, x, y, a, b);
      for (int k = 0; k < d.o0; k++) O0[i * d.o0 + k] = a[k];
      for (int k = 0; k < d.o1; k++) O1[i * d.o1 + k] = b[k];
    }
  }
  return write_all(argv[5], out) ? 0 : 4;
}
