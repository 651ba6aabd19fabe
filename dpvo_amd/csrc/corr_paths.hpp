// corr_paths.hpp -- what the A-CORR translation units share on the host:
// corr.hip (C ABI, dispatch, VALU kernels), corr_nchw.hip, corr_nhwc.hip
// (matrix-core kernels, frame insertion) and the insertion's users in ba.hip /
// ba_window.hip.  One call descriptor, one validation and one selection for
// every forward entry, their limits, and the only declaration of every function
// that crosses between the files.  No device code.  A new path or limit is added
// here; tests/corr_cases.py restates it (pinned through dpvo_corr_query_path).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "dpvo_hot.h"

namespace dpvo {

constexpr int kCorrNpMax = 16;    // p * p, every kernel (one MFMA row tile, NPT <= 16)
constexpr int kCorrValuMaxL = 8;  // levels of the VALU launch (CorrLevels)
constexpr int kNhwcC = 128;       // channels (DPVO gmap / fmap width)
constexpr int kMaxL = 4;          // levels per channels-last launch
constexpr int kNhwcMaxOut = 512;  // (2R+1)^2 * p*p outputs per level (8 per lane)
constexpr int kLvlMaxTiles = 10;  // box up to 160 pixels on the matrix path
constexpr int kLvlBoxStride = 16 * kLvlMaxTiles + 4;
constexpr int kNcC = 128, kNcMaxL = 4;             // the NCHW matrix-core kernel
constexpr int kOrdMaxE = 16384, kOrdMaxN2 = 2048;  // its ordered launch (nc_order's LDS)

// One forward call as the C ABI receives it.  entry: DPVO_CORR_FORWARD (one
// level, scale == nullptr = coordinates as given, out in the fmap dtype) or
// DPVO_CORR_LEVELS / _LEVELS_NHWC (out [.., L] float32).  The level table is
// the caller's four host arrays.
struct CorrCall {
  int entry;
  const void* fmap1;
  const void* const* fmap2;
  const int *H2, *W2;
  const float* scale;
  int L;
  const float* coords;
  const int64_t *ii, *jj;
  const int* order;  // channels-last only: edge order (B == 1) or null
  int B, M, C, H, W, N1, N2, radius, dtype;
  void* out;
  int np() const { return H * W; }
};

struct CorrChoice {
  int status, path;  // DPVO_CORR_PATH_*; NONE: nothing to launch
  int pb[kNcMaxL];   // NCHW_MMA*: widest aligned piece of a level's rows in bytes (16 or 8)
};

// What every forward entry answers before it launches, in one order:
//   1. argument errors -> INVALID   2. envelope -> UNSUPPORTED
//   3. B * M == 0 -> OK, *work = false
//   4. what the entries have always looked at only with work to do: the
//      single-level entry's pointers, the level values, the raw path's G size
inline int corr_validate(const CorrCall& c, bool* work) {
  *work = false;
  const bool single = c.entry == DPVO_CORR_FORWARD, nhwc = c.entry == DPVO_CORR_LEVELS_NHWC;
  if ((!single && !nhwc && c.entry != DPVO_CORR_LEVELS) || c.B < 0 || c.M < 0 || c.C <= 0 ||
      c.H <= 0 || c.W <= 0 || c.radius < 0 || c.radius > 7 || c.L <= 0 ||
      (!nhwc && c.L > kCorrValuMaxL) || !c.fmap2 || !c.H2 || !c.W2 ||
      (single ? (c.H2[0] <= 0 || c.W2[0] <= 0)
              : (!c.fmap1 || !c.coords || !c.ii || !c.jj || !c.out || !c.scale)))
    return DPVO_ERR_INVALID;
  const int np = c.np(), Dp = 2 * c.radius + 1, D = Dp + 1;
  if (np > kCorrNpMax) return DPVO_ERR_UNSUPPORTED;
  if (nhwc && ((c.dtype != DPVO_F32 && c.dtype != DPVO_F16) || c.C != kNhwcC || c.L > kMaxL ||
               Dp * Dp * np > kNhwcMaxOut))
    return DPVO_ERR_UNSUPPORTED;
  if (c.B * c.M == 0) return DPVO_OK;
  if (single && (!c.fmap1 || !c.fmap2[0] || !c.coords || !c.ii || !c.jj || !c.out))
    return DPVO_ERR_INVALID;
  for (int l = 0; l < c.L && !single; l++)
    if (!c.fmap2[l] || c.H2[l] <= 0 || c.W2[l] <= 0 || !(c.scale[l] > 0.f))
      return DPVO_ERR_INVALID;
  // G is np x kLvlBoxStride per wave; the raw path keeps np x D x D dot products there
  if (nhwc && D * D > kLvlBoxStride) return DPVO_ERR_UNSUPPORTED;
  *work = true;
  return DPVO_OK;
}

// The kernel of a call; pure (device pointers are looked at for their
// alignment only).  NCHW levels take the matrix cores when fp16 / fp32,
// C == 128, L <= 4, fmap1 16-B aligned and every level's rows split into
// aligned 8-B pieces at least, else the VALU kernels (fp64: single entry only).
inline CorrChoice corr_select(const CorrCall& c) {
  CorrChoice ch = {DPVO_OK, DPVO_CORR_PATH_NONE, {}};
  bool work;
  ch.status = corr_validate(c, &work);
  if (!work) return ch;
  const bool nhwc = c.entry == DPVO_CORR_LEVELS_NHWC;
  const int es = c.dtype == DPVO_F16 ? 2 : 4;
  bool mma = !nhwc && (c.dtype == DPVO_F16 || c.dtype == DPVO_F32) && c.C == kNcC &&
             c.L <= kNcMaxL && reinterpret_cast<uintptr_t>(c.fmap1) % 16 == 0;
  size_t ring = 0;  // largest level of the ring in bytes
  for (int l = 0; l < c.L && mma; l++) {
    const uintptr_t p = reinterpret_cast<uintptr_t>(c.fmap2[l]);
    // widest piece whose alignment every row start keeps
    if ((c.W2[l] * es) % 16 == 0 && p % 16 == 0) ch.pb[l] = 16;
    else if ((c.W2[l] * es) % 8 == 0 && p % 8 == 0) ch.pb[l] = 8;
    else mma = false;
    const size_t r = (size_t)c.N2 * kNcC * c.H2[l] * c.W2[l] * es;
    ring = r > ring ? r : ring;
  }
  // XCD-aware order (corr_nchw.hip: nc_order) for one batch when some level's
  // ring is larger than the L2s together (8 x 4 MB): its prologue costs ~6 us
  // per workgroup and pays only where lines are re-fetched (cfg2 fp16 level 1,
  // 177 MB: 51 -> 31 us; level 4, 11 MB: 21 -> 23 us)
  if (nhwc)
    ch.path = DPVO_CORR_PATH_NHWC;
  else if (mma)
    ch.path = c.B == 1 && c.M <= kOrdMaxE && c.N2 >= 1 && c.N2 <= kOrdMaxN2 &&
                      ring > ((size_t)32 << 20)
                  ? DPVO_CORR_PATH_NCHW_MMA_ORDERED
                  : DPVO_CORR_PATH_NCHW_MMA;
  else if (c.dtype == DPVO_F32 || c.dtype == DPVO_F16 ||
           (c.dtype == DPVO_F64 && c.entry == DPVO_CORR_FORWARD))
    ch.path = DPVO_CORR_PATH_VALU;
  else
    ch.status = c.entry == DPVO_CORR_FORWARD ? DPVO_ERR_INVALID : DPVO_ERR_UNSUPPORTED;
  return ch;
}

// The launches of a chosen path: they decide nothing about support (only that
// corr_nchw_mma is UNSUPPORTED where its LDS attribute cannot be set: then VALU)
int corr_nchw_mma(const CorrCall& c, const CorrChoice& ch, void* stream);  // corr_nchw.hip
int corr_nhwc_launch(const CorrCall& c, void* stream);                     // corr_nhwc.hip

// ---- frame insertion of a channels-last pyramid (pyr_insert.hpp: ins_tile)
constexpr int kInsMaxL = 4;  // levels per insertion

struct InsLevels {
  void* dst[kInsMaxL];  // float or __half (the source's dtype)
  int s[kInsMaxL];
  // ring variant (graph-replayed frames): dst[l] is slot 0 of level l, the
  // slot is *slot_dev % mem, slots slot_bytes[l] apart; null = dst as given
  const int* slot_dev;
  int mem;
  long long slot_bytes[kInsMaxL];
};

// The insertion's levels, checked and filled (dst[l] the channels-last slot of
// level l, scale[l] in {1, 2, 4, 8}; slot_dev == nullptr: no ring)
inline int ins_levels(InsLevels* lv, void* const* dst, const int* scale, int L, int dtype,
                      const int32_t* slot_dev, int mem, const int64_t* slot_bytes) {
  if (!dst || !scale || L <= 0) return DPVO_ERR_INVALID;
  if ((dtype != DPVO_F32 && dtype != DPVO_F16) || L > kInsMaxL) return DPVO_ERR_UNSUPPORTED;
  if (slot_dev && (mem <= 0 || !slot_bytes)) return DPVO_ERR_INVALID;
  *lv = {};
  lv->slot_dev = (const int*)slot_dev;
  lv->mem = mem > 0 ? mem : 1;
  for (int l = 0; l < L; l++) {
    if (!dst[l]) return DPVO_ERR_INVALID;
    if (scale[l] != 1 && scale[l] != 2 && scale[l] != 4 && scale[l] != 8)
      return DPVO_ERR_UNSUPPORTED;
    lv->dst[l] = dst[l], lv->s[l] = scale[l];
    if (slot_dev) lv->slot_bytes[l] = slot_bytes[l];
  }
  return DPVO_OK;
}

}  // namespace dpvo
