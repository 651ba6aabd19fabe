"""Shared inputs, references and case tables of the A-CORR tests
(test_corr_gpu.py, test_corr_dispatch_gpu.py) and the Python restatement of
the forward dispatch that test_oracle_corr_cases.py pins on the CPU.

The forward has three implementations (corr_nhwc.hip: channels-last levels on
the matrix cores; corr_nchw.hip: NCHW levels on the matrix cores; corr.hip:
VALU) and host predicates that choose between them silently.  A test that
means to run one branch therefore has to prove that its inputs reach it:
`nhwc_supported`, `nchw_mma_supported`, `nchw_ordered`, `unit_classes`,
`valu_fast` and `nchw_modes` restate the predicates and the kernels' box
arithmetic, the tables below say which branch every case is for, and the CPU
test checks the two against each other and the predicates against the native
selection (dpvo_corr_query_path).  No GPU, no test functions."""
import numpy as np
import torch

import oracle


def _t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.to(dtype) if dtype is not None else t


def _close(out, ref, tol=1e-5):
    ref = np.asarray(ref, np.float64)
    out = np.asarray(out, np.float64)
    assert out.shape == ref.shape
    err = np.abs(out - ref).max() if ref.size else 0.0
    assert err <= tol * max(1.0, np.abs(ref).max() if ref.size else 1.0), err


# fp16 output: one fp16 rounding of each value (2^-11 relative, 2^-10 allowed)
# plus fp32 summation noise (2e-5 of max|ref|)
def _close_f16(out, ref):
    out = np.asarray(out, np.float64)
    ref = np.asarray(ref, np.float64)
    assert out.shape == ref.shape
    tol = 2.0 ** -10 * np.abs(ref) + 2e-5 * max(1.0, np.abs(ref).max() if ref.size else 1.0)
    bad = np.abs(out - ref) > tol
    assert not bad.any(), (np.abs(out - ref).max(), int(bad.sum()))


def _case(seed, B=1, M=37, C=128, N1=9, N2=4, H2=24, W2=32, p=3, R=3, spread=0.3, far=0.1,
          Hp=None, Wp=None):
    r = np.random.default_rng(seed)
    Hp = Hp or p
    Wp = Wp or p
    f1 = (0.25 * r.standard_normal((B, N1, C, Hp, Wp))).astype(np.float32)
    f2 = (0.25 * r.standard_normal((B, N2, C, H2, W2))).astype(np.float32)
    cx = r.uniform(-4, W2 + 4, (B, M, 1, 1))
    cy = r.uniform(-4, H2 + 4, (B, M, 1, 1))
    gx = np.arange(Wp)[None, None, None, :] - Wp // 2 + spread * r.standard_normal((B, M, Hp, Wp))
    gy = np.arange(Hp)[None, None, :, None] - Hp // 2 + spread * r.standard_normal((B, M, Hp, Wp))
    co = np.stack([cx + gx, cy + gy], 2).astype(np.float32)
    co[:, : int(far * M), 0] += 5 * W2  # windows completely outside the map
    ii = r.integers(0, N1, M)
    jj = r.integers(0, N2, M)
    return f1, f2, co, ii, jj, R


# ---- fp32 features over a wide dynamic range (test_channels_last_fp32_wide_range)
def _wide(seed, kind):
    f1, f2, co, ii, jj, R = _case(seed, M=96, C=128, H2=40, W2=48)
    r = np.random.default_rng(seed + 7)
    if kind == "channel_scales":  # per-channel scales 1e-4 .. 1e3 on both sides
        f1 = f1 * 10.0 ** r.uniform(-4, 3, (1, 1, 128, 1, 1))
        f2 = f2 * 10.0 ** r.uniform(-4, 3, (1, 1, 128, 1, 1))
    elif kind == "tiny":  # every feature ~1e-4 (f16-subnormal territory)
        f1, f2 = f1 * 1e-4, f2 * 1e-4
    elif kind == "large_a_tiny_b":
        f1, f2 = f1 * 1e3, f2 * 1e-4
    elif kind == "f16_edges":  # magnitudes at 2^-24, 2^-14, 2^-3, 1, 16
        e = r.choice([-24, -14, -3, 0, 4], size=f2.shape)
        f2 = np.sign(f2) * 2.0 ** e * (1 + 0.01 * r.standard_normal(f2.shape))
        e1 = r.choice([-14, -3, 0], size=f1.shape)
        f1 = np.sign(f1) * 2.0 ** e1 * (1 + 0.01 * r.standard_normal(f1.shape))
    elif kind == "beyond_f16":  # |b| >= 65520 in some pixels of the fine level
        m = r.random(f2.shape) < 0.02
        f2 = np.where(m, np.sign(f2) * r.uniform(65520, 3e5, f2.shape), f2)
    return f1.astype(np.float32), f2.astype(np.float32), co, ii, jj, R


# ---------------------------------------------------------------- references
def rounded(a, dtype):
    """`a` as float32 after one rounding to `dtype` (the values a kernel of
    that feature dtype is given)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).float().numpy()


def pyramid(f2, levels, dtype):
    """CPU pyramid of level-1 features f2 [B, N2, C, H2, W2]: level s =
    avg_pool2d(level 1, s, s) summed in fp32 and rounded once to `dtype`
    (level 1 = f2 rounded to dtype).  float32 numpy arrays of the rounded
    values: both what the test uploads and what the oracle is run on."""
    lv1 = torch.from_numpy(rounded(f2, dtype))
    out = []
    for s in levels:
        if s == 1:
            out.append(lv1.numpy())
            continue
        B, N = lv1.shape[:2]
        lv = torch.nn.functional.avg_pool2d(lv1.flatten(0, 1), s, s).unflatten(0, (B, N))
        out.append(lv.to(dtype).float().numpy())
    return out


def levels_ref(f1, pyr, co, ii, jj, R, scales):
    """The oracle per level (coords / scale, dpvo.py:462-463) stacked on the
    last axis: [B, M, Dp, Dp, Hp, Wp, L]."""
    return np.stack([oracle.corr_fwd(f1, np.asarray(p), co / np.float32(s), ii, jj, R)
                     for p, s in zip(pyr, scales)], -1)


def poison(shape, device):
    """Allocate a float32 tensor of the output's shape, fill it with NaN and
    drop it: the block the extension's torch::empty reuses next then does not
    already hold a right answer from an earlier call, and an edge or level
    that no wave wrote shows up as NaN."""
    t = torch.full(tuple(int(s) for s in shape), float("nan"), dtype=torch.float32, device=device)
    torch.cuda.synchronize(device)
    del t


# ------------------------------------------------- the dispatch, restated
kNhwcC, kMaxL, kOutPerLane, kNpMax, kWave = 128, 4, 8, 16, 64  # corr_nhwc.hip
kLvlMaxTiles = 10
kLvlBoxStride = 16 * kLvlMaxTiles + 4
kBoxPx = 2 * kWave                                             # corr.hip
kNcMaxTiles, kNcMaxL = 17, 4                                   # corr_nchw.hip
kOrdMaxE, kOrdMaxN2 = 16384, 2048


def nhwc_refusals(p_h, p_w, R, C, L, dtype):
    """Why dpvo_corr_forward_levels_nhwc_ordered returns DPVO_ERR_UNSUPPORTED
    (empty: it runs the matrix-core kernel)."""
    np_, Dp, D = p_h * p_w, 2 * R + 1, 2 * R + 2
    why = set()
    if dtype not in (torch.float32, torch.float16):
        why.add("dtype")
    if C != kNhwcC:
        why.add("C")
    if L > kMaxL:
        why.add("L")
    if np_ > kNpMax:
        why.add("np")
    if Dp * Dp * np_ > kOutPerLane * kWave:
        why.add("nout")
    if D * D > kLvlBoxStride:
        why.add("D2")
    return why


def nhwc_supported(p_h, p_w, R, C, L, dtype):
    return not nhwc_refusals(p_h, p_w, R, C, L, dtype)


def nchw_mma_supported(p_h, p_w, R, C, L, level_shapes, dtype):
    """corr_select's predicate (corr_paths.hpp) for the NCHW matrix-core kernel,
    for 16-B aligned level bases: else the VALU kernels of corr.hip run."""
    if dtype not in (torch.float32, torch.float16) or C != 128:
        return False
    if not (1 <= p_h * p_w <= 16 and 1 <= L <= kNcMaxL and 0 <= R <= 7):
        return False
    es = 2 if dtype == torch.float16 else 4
    return all((W2 * es) % 8 == 0 for _, W2 in level_shapes)


def nchw_ordered(B, M, N2, level_shapes, dtype):
    """Whether corr_select picks the ordered launch (nc_order's prologue)."""
    es = 2 if dtype == torch.float16 else 4
    ring = max(N2 * 128 * H2 * W2 * es for H2, W2 in level_shapes)
    return B == 1 and M <= kOrdMaxE and 1 <= N2 <= kOrdMaxN2 and ring > (32 << 20)


def _ifloor_safe(v):
    f = np.floor(np.asarray(v, np.float32))
    return np.fmin(np.fmax(f, np.float32(-1.0e8)), np.float32(1.0e8)).astype(np.int64)


def boxes(co, scale, H2, W2, R, valid=None):
    """The kernels' union box of one level for every edge: coords [B, M, 2,
    Hp, Wp] / scale, floor, min / max over the patch, +-R (+1), clamp to the
    map.  `valid` [M]: edges whose ii / jj are in range (others: empty box)."""
    B, M = co.shape[:2]
    x = (co[:, :, 0] / np.float32(scale)).reshape(B, M, -1)
    y = (co[:, :, 1] / np.float32(scale)).reshape(B, M, -1)
    xf, yf = _ifloor_safe(x), _ifloor_safe(y)
    lo_x, hi_x, lo_y, hi_y = xf.min(-1), xf.max(-1), yf.min(-1), yf.max(-1)
    xlo, ylo = np.maximum(lo_x - R, 0), np.maximum(lo_y - R, 0)
    xhi, yhi = np.minimum(hi_x + R + 1, W2 - 1), np.minimum(hi_y + R + 1, H2 - 1)
    bw, bh = xhi - xlo + 1, yhi - ylo + 1
    empty = (bw <= 0) | (bh <= 0)
    if valid is not None:
        empty = empty | ~np.asarray(valid, bool)[None, :]
    inner = ~empty & (lo_x - R >= 0) & (lo_y - R >= 0) & (hi_x + R + 1 <= W2 - 1) & \
        (hi_y + R + 1 <= H2 - 1)
    return dict(xlo=xlo, xhi=xhi, ylo=ylo, yhi=yhi, bw=np.where(empty, 0, bw),
                bh=np.where(empty, 0, bh), npx=np.where(empty, 0, bw * bh), empty=empty,
                inner=inner)


def unit_classes(co, scales, level_shapes, R, p, valid=None):
    """corr_nhwc_lvl_kernel's class of every (edge, level) unit, [B, M, L] of
    'empty' (box outside the map), 'inner' (box not clamped), 'clipped'
    (clamped, ntile <= 10: matrix path with clamped taps) and 'raw'
    (ntile > 10: per-tap dot products)."""
    p_h, p_w = (p, p) if np.isscalar(p) else p
    assert co.shape[3:] == (p_h, p_w)
    out = []
    for s, (H2, W2) in zip(scales, level_shapes):
        b = boxes(co, s, H2, W2, R, valid)
        ntile = (b["npx"] + 15) // 16
        cls = np.where(b["empty"], "empty",
                       np.where(ntile > kLvlMaxTiles, "raw",
                                np.where(b["inner"], "inner", "clipped")))
        out.append(cls)
    return np.stack(out, -1)


def valu_fast(co, scales, level_shapes, R, p, valid=None):
    """corr.hip's corr_edge: `npx <= kBoxPx && np == NPT` ([B, M, L] bool; the
    box GEMM, else per-tap dot products)."""
    p_h, p_w = (p, p) if np.isscalar(p) else p
    exact = p_h * p_w in (1, 4, 9, 16)
    return np.stack([(boxes(co, s, H2, W2, R, valid)["npx"] <= kBoxPx) & exact
                     for s, (H2, W2) in zip(scales, level_shapes)], -1)


def nchw_modes(co, scales, level_shapes, R, p, dtype, valid=None):
    """nc_edge's load shape of every unit, [B, M, L] ints: -1 empty box, 1 =
    16-B pieces x 2 channels, 2 = 16-B pieces x 1 channel (fp32 only), 3 = 8-B
    pieces, 0 = raw path."""
    es = 2 if dtype == torch.float16 else 4
    out = []
    for s, (H2, W2) in zip(scales, level_shapes):
        b = boxes(co, s, H2, W2, R, valid)
        pb = 16 if (W2 * es) % 16 == 0 else 8

        def fits(pbytes, lanes):
            G = pbytes // es
            xs = b["xlo"] & ~(G - 1)
            npr = (b["xhi"] - xs) // G + 1
            nt = ((b["bh"] * npr * G + 15) >> 4) | 1
            return (nt <= kNcMaxTiles) & (b["bh"] * npr <= lanes)

        m1 = fits(16, kWave // 2) if pb == 16 else np.zeros_like(b["empty"])
        m2 = fits(16, kWave) if (pb == 16 and es == 4) else np.zeros_like(b["empty"])
        mode = np.where(m1, 1, np.where(m2, 2, np.where(fits(8, kWave), 3, 0)))
        out.append(np.where(b["npx"] > 0, mode, -1))
    return np.stack(out, -1)


def level_shapes(H2, W2, levels):
    return [(H2 // s, W2 // s) for s in levels]


# --------------------------------------------------------------- case tables
DTYPES = (torch.float32, torch.float16)
SCALES = (1, 2, 4, 8)

# A. channels-last, run-time shape (RAW9 = false): (Hp, Wp, R)
A_SHAPES = [(1, 1, 0), (1, 1, 5), (2, 2, 3), (2, 2, 5), (2, 3, 4), (3, 3, 0), (3, 3, 1),
            (3, 3, 2), (4, 4, 2), (4, 4, 1)]
A_LEVELS = [(1,), (1, 4), (1, 2, 4), (1, 2, 4, 8)]
A_SEED = 51


def a_cases():
    """(id, _case kwargs, levels, mark); mark: 'rt' = matrix path, run-time
    shape; 'rt-mixed' = the same with raw and matrix units mixed."""
    out = []
    for hp, wp, R in A_SHAPES:
        for lv in A_LEVELS:
            out.append((f"{hp}x{wp}-R{R}-L{len(lv)}", dict(Hp=hp, Wp=wp, R=R), lv, "rt"))
    for hp, wp, R in [(2, 2, 3), (4, 4, 2)]:
        out.append((f"{hp}x{wp}-R{R}-spread", dict(Hp=hp, Wp=wp, R=R, spread=4.0, H2=40, W2=48),
                    (1, 2, 4, 8), "rt-mixed"))  # 40 x 48: level-1 boxes past 10 tiles
        out.append((f"{hp}x{wp}-R{R}-far", dict(Hp=hp, Wp=wp, R=R, far=0.5), (1, 2, 4, 8), "rt"))
    # tiny map: every window clipped (level 4 is a single pixel)
    out.append(("2x2-R3-tiny-L1", dict(Hp=2, Wp=2, R=3, H2=5, W2=6), (1,), "rt"))
    out.append(("2x2-R3-tiny-L3", dict(Hp=2, Wp=2, R=3, H2=5, W2=6), (1, 2, 4), "rt"))
    return out


# B. level counts and tails: (Hp = Wp, R, dtype) x L x edge counts
B_SHAPES = [(3, 3, torch.float32), (3, 3, torch.float16), (2, 3, torch.float32)]
B_UNORDERED = [(1, 1), (1, 2), (1, 3), (1, 5), (1, 67), (2, 3), (2, 5)]  # (B, M)
B_ORDERED_M = [1, 7, 8, 9, 15, 17, 130]
B_SEED = 61


def orders(M, seed):
    """identity, reversed and a seeded random permutation (int32)."""
    ident = np.arange(M, dtype=np.int32)
    return {"identity": ident, "reversed": ident[::-1].copy(),
            "random": np.random.default_rng(seed).permutation(M).astype(np.int32)}


# C. host fall-backs of a channels-last pyramid: (id, kwargs, levels, reasons)
C_CASES = [
    ("p3-R4", dict(p=3, R=4), (1, 4), {"nout"}),
    ("p4-R3", dict(p=4, R=3), (1, 4), {"nout"}),
    ("p1-R6", dict(p=1, R=6), (1, 4), {"D2"}),
    ("p3-R7", dict(p=3, R=7), (1, 4), {"nout", "D2"}),
    ("C64", dict(C=64), (1, 4), {"C"}),
    ("L5", dict(H2=48, W2=64), (1, 2, 4, 8, 16), {"L"}),
    ("mixed-layout", dict(), (1, 4), set()),  # level 0 channels-last, level 1 NCHW
]
C_SEED = 71

# D. NCHW pyramids corr_nchw_mma refuses -> corr_fwd_levels_kernel (VALU):
# (id, kwargs, levels, dtype)
D_CASES = [
    ("f32-W30", dict(W2=30), (1, 2), torch.float32),        # level 2: 15 x 4 B rows
    ("f16-W36", dict(W2=36), (1, 2), torch.float16),        # level 2: 18 x 2 B rows
    ("C37-f32", dict(C=37), (1, 4), torch.float32),
    ("C37-f16", dict(C=37), (1, 4), torch.float16),
    ("L5-f32", dict(H2=48, W2=64), (1, 2, 4, 8, 16), torch.float32),
    ("L5-f16", dict(H2=48, W2=64), (1, 2, 4, 8, 16), torch.float16),
    ("L8-f32", dict(H2=48, W2=64), (1, 1, 2, 2, 4, 4, 8, 8), torch.float32),
    ("L8-f16", dict(H2=48, W2=64), (1, 1, 2, 2, 4, 4, 8, 8), torch.float16),
    ("p1-W30", dict(p=1, W2=30), (1, 4), torch.float32),
    ("p2-W30", dict(p=2, W2=30), (1, 4), torch.float32),
    ("p4-W30", dict(p=4, W2=30), (1, 4), torch.float32),
    ("2x3-W30", dict(Hp=2, Wp=3, W2=30), (1, 4), torch.float32),
    ("2x3-W30-f16", dict(Hp=2, Wp=3, W2=30), (1, 4), torch.float16),
]
D_SEED = 81

# E. NCHW ordered prologue (nc_order) at small sizes: a ring just over 32 MiB
E_RINGS = {torch.float32: dict(N2=1100, H2=8, W2=8), torch.float16: dict(N2=2048, H2=8, W2=12)}
E_M = [1, 3, 4, 5, 257, 1030]
E_N1 = 9
E_SEED = 91


def e_edges(seed, M, N2, H2, W2, kind="spread", N1=E_N1):
    """gmap patches, coords and indices of M edges over an N2-frame ring of
    H2 x W2 maps.  kind: 'spread' (jj over the whole ring), 'one_frame'
    (every jj equal), 'oob' (20 % of jj out of range: -1 and N2 + 3)."""
    r = np.random.default_rng(seed)
    f1 = (0.25 * r.standard_normal((1, N1, 128, 3, 3))).astype(np.float32)
    cx = r.uniform(-4, W2 + 4, (1, M, 1, 1))
    cy = r.uniform(-4, H2 + 4, (1, M, 1, 1))
    gx = np.arange(3)[None, None, None, :] - 1 + 0.3 * r.standard_normal((1, M, 3, 3))
    gy = np.arange(3)[None, None, :, None] - 1 + 0.3 * r.standard_normal((1, M, 3, 3))
    co = np.stack([cx + gx, cy + gy], 2).astype(np.float32)
    ii = r.integers(0, N1, M)
    jj = r.integers(0, N2, M)
    if kind == "one_frame":
        jj[:] = N2 // 3
    elif kind == "oob":
        bad = r.permutation(M)[: max(1, M // 5)]
        jj[bad] = np.where(np.arange(len(bad)) % 2 == 0, -1, N2 + 3)
    return f1, co, ii, jj


def ring_subset_ref(f1, ring, co, ii, jj, R, scales=None):
    """The oracle on the frames the edges use (the ring itself is tens of MiB):
    `ring` a float32 numpy [1, N2, C, H2, W2]; every jj in range."""
    used, inv = np.unique(jj, return_inverse=True)
    sub = np.ascontiguousarray(ring[:, used])
    if scales is None:
        return oracle.corr_fwd(f1, sub, co, ii, inv, R)
    return levels_ref(f1, [sub] * len(scales), co, ii, inv, R, scales)


# F. out-of-range indices and coordinates: the three kernels
F_KERNELS = {"nhwc": dict(C=128, layout="cl"), "nchw_mma": dict(C=128, layout="nchw"),
             "valu": dict(C=64, layout="nchw")}
F_LEVELS = [(1,), (1, 2, 4, 8)]
F_SEED = 101


def f_bad_indices(seed, ii, jj, N1, N2):
    """ii / jj with a seeded quarter of the edges out of range (-1, N1, N1 + 5,
    -7 for ii; -1, N2, 2 N2, -7 for jj; some edges both) and the mask of the
    edges left valid."""
    r = np.random.default_rng(seed)
    M = len(ii)
    ii, jj = ii.copy(), jj.copy()
    bad = r.permutation(M)[: max(8, M // 4)]
    vi = [-1, N1, N1 + 5, -7]
    vj = [-1, N2, 2 * N2, -7]
    for n, e in enumerate(bad):
        if n % 3 != 1:
            ii[e] = vi[n % 4]
        if n % 3 != 0:
            jj[e] = vj[(n // 2) % 4]
    valid = (ii >= 0) & (ii < N1) & (jj >= 0) & (jj < N2)
    return ii, jj, valid


def f_bad_coords(seed, co, values, whole_patch):
    """co with one patch pixel (or all of them) of a seeded tenth of the edges
    set to `values` (cycled; x, y or both), the mask [B, M, Hp, Wp] of those
    pixels, and a copy with benign coordinates there for the oracle."""
    r = np.random.default_rng(seed)
    B, M, _, Hp, Wp = co.shape
    bad, ok = co.copy(), co.copy()
    mask = np.zeros((B, M, Hp, Wp), bool)
    edges = r.permutation(M)[: max(4, M // 10)]
    for n, e in enumerate(edges):
        v = np.float32(values[n % len(values)])
        sel = np.ones((Hp, Wp), bool) if whole_patch else np.zeros((Hp, Wp), bool)
        if not whole_patch:
            sel[r.integers(0, Hp), r.integers(0, Wp)] = True
        for b in range(B):
            for axis in ((0,), (1,), (0, 1))[n % 3]:
                bad[b, e, axis][sel] = v
            mask[b, e] |= sel
            ok[b, e][:, sel] = 0.5  # any finite in-map coordinate: outputs ignored
    return bad, mask, ok
