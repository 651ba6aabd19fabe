"""GPU: every forward dispatch branch of A-CORR at small and odd sizes against
the oracle (tests/corr_cases.py holds the inputs, the case tables and the
restated predicates; test_oracle_corr_cases.py proves on the CPU that each
case reaches the branch it is named for).

Tolerances are the project's (test_corr_gpu.py): fp32 1e-5 of max(1, max|ref|)
per level, fp16 features with float32 output 2e-5, fp16 output _close_f16; the
fp16 reference is the oracle on the fp16-rounded inputs.  Every output block is
poisoned with NaN before the call (corr_cases.poison), so an edge or level that
no wave wrote fails the no-NaN assertion."""
import numpy as np
import pytest
import torch

import corr_cases as C
import oracle
from corr_cases import _case, _close, _close_f16, _t, _wide

pytestmark = pytest.mark.gpu

_DT = pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f16"])


def _id(case):
    return case[0]


@pytest.fixture(scope="module")
def cc(gpu):
    import dpvo_amd

    return dpvo_amd.load_extension("cuda_corr")


def _upload(gpu, pyr, dtype, layout):
    from dpvo_amd import synthetic

    lv = [_t(p, gpu, dtype) for p in pyr]
    if layout == "cl":
        lv = [synthetic.channels_last(x) for x in lv]
    elif layout == "mixed":  # level 0 channels-last, the others NCHW
        lv = [synthetic.channels_last(lv[0])] + lv[1:]
    return lv


def _levels(gpu, f1, pyr, co, ii, jj, R, scales, dtype, layout, order=None):
    """altcorr.corr_levels on the uploaded case -> float32 tensor
    [B, M, Dp, Dp, Hp, Wp, L] (output block poisoned before the call)."""
    from dpvo_amd import altcorr

    args = (_t(f1, gpu, dtype), _upload(gpu, pyr, dtype, layout), _t(co, gpu), _t(ii, gpu),
            _t(jj, gpu))
    order = None if order is None else _t(order, gpu)
    Dp = 2 * R + 1
    shape = co.shape[:2] + (Dp, Dp) + co.shape[3:] + (len(scales),)
    C.poison(shape, gpu)
    out = altcorr.corr_levels(*args, R, scales=scales, order=order)
    assert out.dtype == torch.float32
    return out.view(shape)


def _check_levels(out, ref, dtype):
    out = out.cpu().numpy() if torch.is_tensor(out) else out
    assert out.shape == ref.shape
    assert not np.isnan(out).any()
    for l in range(ref.shape[-1]):
        _close(out[..., l], ref[..., l], 1e-5 if dtype == torch.float32 else 2e-5)


def _inputs(seed, kw, levels, dtype):
    f1, f2, co, ii, jj, R = _case(seed, **kw)
    return C.rounded(f1, dtype), C.pyramid(f2, levels, dtype), co, ii, jj, R


# ---- A. channels-last, run-time shape: corr_nhwc_lvl_kernel<T, 2, false, PAIRED>
@_DT
@pytest.mark.parametrize("case", C.a_cases(), ids=_id)
def test_channels_last_runtime_shape(gpu, case, dtype):
    _, kw, levels, _ = case
    f1, pyr, co, ii, jj, R = _inputs(C.A_SEED, kw, levels, dtype)
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, "cl")
    _check_levels(out, C.levels_ref(f1, pyr, co, ii, jj, R, levels), dtype)


@_DT
def test_forward_channels_last_level_runtime_shape(cc, gpu, dtype):
    """cuda_corr.forward on one channels-last level at p = 2: the run-time
    shape kernel, output [B, M, 7, 7, 2, 2] in the fmap dtype."""
    f1, pyr, co, ii, jj, R = _inputs(C.A_SEED + 1, dict(p=2, R=3), (1,), dtype)
    lv, = _upload(gpu, pyr, dtype, "cl")
    assert not lv.is_contiguous()
    args = (_t(f1, gpu, dtype), lv, _t(co, gpu), _t(ii, gpu), _t(jj, gpu))
    C.poison((1, len(ii), 7, 7, 2, 2, 1), gpu)
    out, = cc.forward(*args, R)
    assert out.dtype == dtype and out.shape == (1, len(ii), 2 * R + 1, 2 * R + 1, 2, 2)
    ref = oracle.corr_fwd(f1, pyr[0], co, ii, jj, R)
    o = out.float().cpu().numpy()
    assert not np.isnan(o).any()
    if dtype == torch.float32:
        _close(o, ref, 1e-5)
    else:
        _close_f16(o, ref)


# ---- B. level counts and tails (pair_ok, half = (per + 1) / 2, npos = 4 / L,
# the ordered per = (M + 7) / 8 split, b = edge / M), DPVO and run-time shape
def _b_inputs(shape, L, B, M):
    p, R, dtype = shape
    levels = C.SCALES[:L]
    return _inputs(C.B_SEED + M, dict(B=B, M=M, p=p, R=R), levels, dtype) + (levels, dtype)


_B_SHAPE = pytest.mark.parametrize("shape", C.B_SHAPES, ids=["3x3-f32", "3x3-f16", "2x2-f32"])
_B_L = pytest.mark.parametrize("L", [1, 2, 3, 4])


@_B_L
@_B_SHAPE
@pytest.mark.parametrize("BM", C.B_UNORDERED, ids=lambda bm: f"B{bm[0]}-M{bm[1]}")
def test_channels_last_level_counts_and_tails(gpu, shape, L, BM):
    f1, pyr, co, ii, jj, R, levels, dtype = _b_inputs(shape, L, *BM)
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, "cl")
    _check_levels(out, C.levels_ref(f1, pyr, co, ii, jj, R, levels), dtype)


@_B_L
@_B_SHAPE
@pytest.mark.parametrize("M", C.B_ORDERED_M)
def test_channels_last_ordered_tails(gpu, shape, L, M):
    """order = identity, reversed, random permutation: the oracle's values,
    and bit-identical to the unordered launch ("same results")."""
    f1, pyr, co, ii, jj, R, levels, dtype = _b_inputs(shape, L, 1, M)
    ref = C.levels_ref(f1, pyr, co, ii, jj, R, levels)
    a = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, "cl")
    _check_levels(a, ref, dtype)
    for name, order in C.orders(M, C.B_SEED).items():
        b = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, "cl", order=order)
        _check_levels(b, ref, dtype)
        assert torch.equal(a, b), name


def test_order_with_batch_raises(gpu):
    f1, pyr, co, ii, jj, R = _inputs(C.B_SEED, dict(B=2, M=8), (1, 4), torch.float32)
    with pytest.raises(RuntimeError):
        _levels(gpu, f1, pyr, co, ii, jj, R, (1, 4), torch.float32, "cl",
                order=np.arange(8, dtype=np.int32))


@pytest.mark.parametrize("levels", [(1, 2, 4), (1, 2, 4, 8)])
def test_channels_last_fp32_wide_range_paired(gpu, levels):
    """test_channels_last_fp32_wide_range's two bars (relative error <= 1e-4
    wherever |ref| >= 1e-3 max|ref|; everywhere |err| <= 1e-4 |ref| + 2^-20 S)
    on the paired kernels, L = 3 and L = 4."""
    f1, f2, co, ii, jj, R = _wide(41, "channel_scales")
    pyr = C.pyramid(f2, levels, torch.float32)
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, torch.float32, "cl").double().cpu().numpy()
    assert not np.isnan(out).any()
    for l, s in enumerate(levels):
        ref = oracle.corr_fwd(f1, pyr[l], co / s, ii, jj, R).astype(np.float64)
        mag = oracle.corr_fwd(np.abs(f1), np.abs(pyr[l]), co / s, ii, jj, R).astype(np.float64)
        err = np.abs(out[..., l] - ref)
        big = np.abs(ref) >= 1e-3 * np.abs(ref).max()
        rel = (err[big] / np.abs(ref[big])).max()
        assert rel <= 1e-4, (s, rel)
        assert (err <= 1e-4 * np.abs(ref) + 2.0 ** -20 * mag).all(), s


# ---- C. host fall-backs of a channels-last pyramid (.contiguous() ->
# dpvo_corr_forward_levels): still the oracle's values
@_DT
@pytest.mark.parametrize("case", C.C_CASES, ids=_id)
def test_channels_last_fallbacks(gpu, case, dtype):
    name, kw, levels, _ = case
    f1, pyr, co, ii, jj, R = _inputs(C.C_SEED, kw, levels, dtype)
    layout = "mixed" if name == "mixed-layout" else "cl"
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, layout)
    _check_levels(out, C.levels_ref(f1, pyr, co, ii, jj, R, levels), dtype)


# ---- D. corr_fwd_levels_kernel (VALU): NCHW pyramids corr_nchw_mma refuses
@pytest.mark.parametrize("case", C.D_CASES, ids=_id)
def test_valu_levels_kernel(cc, gpu, case):
    """Against the oracle, and (fp32) against per-level cuda_corr.forward
    calls stacked to 1e-6 of max(1, max|ref|): the same per-level arithmetic.
    fp16 is left out of the second check: the per-level entry rounds its
    output to fp16, the fused one returns float32."""
    _, kw, levels, dtype = case
    f1, pyr, co, ii, jj, R = _inputs(C.D_SEED, kw, levels, dtype)
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, "nchw")
    _check_levels(out, C.levels_ref(f1, pyr, co, ii, jj, R, levels), dtype)
    if dtype == torch.float32:
        f1d, cod, iid, jjd = _t(f1, gpu), _t(co, gpu), _t(ii, gpu), _t(jj, gpu)
        per = [cc.forward(f1d, _t(p, gpu), cod / s, iid, jjd, R)[0] for p, s in zip(pyr, levels)]
        ref = torch.stack(per, -1)
        err = (out - ref).abs().max().item()
        assert err <= 1e-6 * max(1.0, ref.abs().max().item()), err


@_DT
def test_nchw_mma_three_levels(gpu, dtype):
    """corr_nchw.hip with levels (1, 2, 4) on a 48 x 64 map (W2 = 64, 32, 16)."""
    levels = (1, 2, 4)
    f1, pyr, co, ii, jj, R = _inputs(C.D_SEED + 1, dict(M=150, H2=48, W2=64), levels, dtype)
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, "nchw")
    _check_levels(out, C.levels_ref(f1, pyr, co, ii, jj, R, levels), dtype)


# ---- E. the NCHW ordered prologue (nc_order) at small sizes: a ring just
# over 32 MiB of small maps
@pytest.fixture(scope="module")
def rings(gpu):
    """dtype -> (host float32 numpy, device tensor) of a 0.25 randn ring, one
    frame longer than corr_cases.E_RINGS says (the N2 threshold test)."""
    cache = {}

    def get(dtype):
        if dtype not in cache:
            s = C.E_RINGS[dtype]
            g = torch.Generator().manual_seed(C.E_SEED)
            host = (0.25 * torch.randn(1, s["N2"] + 1, 128, s["H2"], s["W2"], generator=g)).to(dtype)
            cache[dtype] = (host.float().numpy(), host.to(gpu))
        return cache[dtype]

    return get


def _cmp_out(o, ref, dtype):
    (_close if dtype == torch.float32 else _close_f16)(o, ref)


def _fwd(cc, gpu, f1, ring, co, ii, jj, dtype, R=3):
    args = (_t(f1, gpu, dtype), ring, _t(co, gpu), _t(ii, gpu), _t(jj, gpu))
    C.poison((1, co.shape[1], 2 * R + 1, 2 * R + 1, 3, 3), gpu)
    out, = cc.forward(*args, R)
    assert out.dtype == dtype
    return out


@_DT
@pytest.mark.parametrize("kind,M", [("spread", m) for m in C.E_M] +
                         [("one_frame", 5), ("one_frame", 257), ("oob", 257)])
def test_nchw_ordered_small(cc, gpu, rings, dtype, kind, M):
    """cuda_corr.forward (L = 1) and corr_levels (L = 2: the ring once more at
    scale 2) on the ordered path; out-of-range jj rows are exactly 0."""
    from dpvo_amd import altcorr

    s = C.E_RINGS[dtype]
    host, dev = rings(dtype)
    N2 = s["N2"]
    host, dev = host[:, :N2], dev[:, :N2]
    f1, co, ii, jj = C.e_edges(C.E_SEED + M, M, N2, s["H2"], s["W2"], kind)
    f1 = C.rounded(f1, dtype)
    ok = (jj >= 0) & (jj < N2)
    out = _fwd(cc, gpu, f1, dev, co, ii, jj, dtype).float().cpu().numpy()
    assert not np.isnan(out).any()
    _cmp_out(out[:, ok], C.ring_subset_ref(f1, host, co[:, ok], ii[ok], jj[ok], 3), dtype)
    assert (out[:, ~ok] == 0).all()
    args = (_t(f1, gpu, dtype), [dev, dev], _t(co, gpu), _t(ii, gpu), _t(jj, gpu))
    C.poison((1, M, 7, 7, 3, 3, 2), gpu)
    out2 = altcorr.corr_levels(*args, 3, scales=(1, 2)).view(1, M, 7, 7, 3, 3, 2).cpu().numpy()
    _check_levels(out2[:, ok], C.ring_subset_ref(f1, host, co[:, ok], ii[ok], jj[ok], 3, (1, 2)),
                  dtype)
    assert (out2[:, ~ok] == 0).all()


def test_nchw_ordered_edge_count_threshold(cc, gpu, rings):
    """M = 16384 (ordered) and 16385 (not) on the same first 16384 edges:
    bit-identical rows; the oracle on every 97th edge."""
    dtype = torch.float32
    s = C.E_RINGS[dtype]
    host, dev = rings(dtype)
    N2, M = s["N2"], C.kOrdMaxE
    host, dev = host[:, :N2], dev[:, :N2]
    f1, co, ii, jj = C.e_edges(C.E_SEED + 7, M + 1, N2, s["H2"], s["W2"])
    a = _fwd(cc, gpu, f1, dev, co[:, :M], ii[:M], jj[:M], dtype)
    b = _fwd(cc, gpu, f1, dev, co, ii, jj, dtype)
    assert torch.equal(a, b[:, :M])
    sel = np.arange(0, M, 97)
    _cmp_out(a.cpu().numpy()[:, sel],
             C.ring_subset_ref(f1, host, co[:, sel], ii[sel], jj[sel], 3), dtype)


def test_nchw_ordered_frame_count_threshold(cc, gpu, rings):
    """N2 = 2048 (ordered) and 2049 (not) on the same first 2048 frames."""
    dtype = torch.float16
    s = C.E_RINGS[dtype]
    host, dev = rings(dtype)
    N2, M = C.kOrdMaxN2, 1030
    assert s["N2"] == N2 and dev.shape[1] == N2 + 1
    f1, co, ii, jj = C.e_edges(C.E_SEED + 8, M, N2, s["H2"], s["W2"])
    f1 = C.rounded(f1, dtype)
    a = _fwd(cc, gpu, f1, dev[:, :N2], co, ii, jj, dtype)
    b = _fwd(cc, gpu, f1, dev, co, ii, jj, dtype)
    assert torch.equal(a, b)
    sel = np.arange(0, M, 97)
    _cmp_out(a.float().cpu().numpy()[:, sel],
             C.ring_subset_ref(f1, host, co[:, sel], ii[sel], jj[sel], 3), dtype)


# ---- F. out-of-range indices and coordinates: idx_ok and ifloor_safe of the
# three kernels.  The reference is undefined there; the contract under test is
# this project's: an edge with an index out of range gives zeros, a coordinate
# beyond every map gives zeros (frac = 0, every tap outside), the other edges
# are untouched.
_F_K = pytest.mark.parametrize("kernel", list(C.F_KERNELS))
_F_L = pytest.mark.parametrize("levels", C.F_LEVELS, ids=["L1", "L4"])


def _f_inputs(kernel, levels, dtype):
    f1, pyr, co, ii, jj, R = _inputs(C.F_SEED, dict(M=67, C=C.F_KERNELS[kernel]["C"]), levels,
                                     dtype)
    return f1, pyr, co, ii, jj, R, C.F_KERNELS[kernel]["layout"]


@_F_L
@_DT
@_F_K
def test_out_of_range_indices(gpu, kernel, dtype, levels):
    f1, pyr, co, ii, jj, R, layout = _f_inputs(kernel, levels, dtype)
    ii, jj, ok = C.f_bad_indices(C.F_SEED, ii, jj, f1.shape[1], pyr[0].shape[1])
    out = _levels(gpu, f1, pyr, co, ii, jj, R, levels, dtype, layout).cpu().numpy()
    assert not np.isnan(out).any()
    assert (out[:, ~ok] == 0).all()
    _check_levels(out[:, ok], C.levels_ref(f1, pyr, co[:, ok], ii[ok], jj[ok], R, levels), dtype)


@pytest.mark.parametrize("whole", [False, True], ids=["pixel", "patch"])
@_F_L
@_DT
@_F_K
def test_out_of_range_coordinates(gpu, kernel, dtype, levels, whole):
    """+-1e9 and +-3e38 on one patch pixel, or all, of a tenth of the edges:
    those pixels' outputs are exactly 0, every other value (the other pixels
    of the same edges included: a pixel's output depends on its own
    coordinate only) is the oracle's."""
    f1, pyr, co, ii, jj, R, layout = _f_inputs(kernel, levels, dtype)
    bad, mask, benign = C.f_bad_coords(C.F_SEED + 1, co, (1e9, -1e9, 3e38, -3e38), whole)
    out = _levels(gpu, f1, pyr, bad, ii, jj, R, levels, dtype, layout).cpu().numpy()
    assert not np.isnan(out).any()
    ref = C.levels_ref(f1, pyr, benign, ii, jj, R, levels)
    by_px = np.moveaxis(ref, (4, 5), (2, 3))  # a view: [B, M, Hp, Wp, Dp, Dp, L]
    by_px[mask] = 0
    assert (np.moveaxis(out, (4, 5), (2, 3))[mask] == 0).all()
    _check_levels(out, ref, dtype)


@_F_L
@_DT
@_F_K
def test_non_finite_coordinates_leave_other_edges(gpu, kernel, dtype, levels):
    """NaN and +-inf coordinates: only that every OTHER edge still matches the
    oracle (the affected rows are undefined in the reference)."""
    f1, pyr, co, ii, jj, R, layout = _f_inputs(kernel, levels, dtype)
    bad, mask, _ = C.f_bad_coords(C.F_SEED + 2, co, (np.nan, np.inf, -np.inf), False)
    keep = ~mask.any((0, 2, 3))
    out = _levels(gpu, f1, pyr, bad, ii, jj, R, levels, dtype, layout).cpu().numpy()
    _check_levels(out[:, keep],
                  C.levels_ref(f1, pyr, co[:, keep], ii[keep], jj[keep], R, levels), dtype)
