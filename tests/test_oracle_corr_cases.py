"""CPU: tests/corr_cases.py pinned.  The helper restates the host predicates
and the box arithmetic of the three A-CORR forward kernels; here hand-made
inputs pin that restatement, and every case of the tables that
test_corr_dispatch_gpu.py runs is shown to reach the branch it is named for
(the conditions are on the chosen seeds, so they are checked, not assumed)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import corr_cases as C
import oracle
from corr_cases import _case

F32, F16 = torch.float32, torch.float16


# ---------------------------------------------------------------- the helper
def _co(points):
    """coords [1, M, 2, 1, 1] of single-pixel patches at (x, y)."""
    return np.asarray(points, np.float32).reshape(1, -1, 2, 1, 1)


def test_boxes_and_classes_by_hand():
    # 24 x 32 map, R = 3, one-pixel patches: window = floor - 3 .. floor + 4
    co = _co([(10.5, 10.5), (0.5, 0.5), (200.0, 5.0), (-9.0, 5.0), (31.9, 23.9), (3.0, 3.0)])
    b = C.boxes(co, 1, 24, 32, 3)
    assert b["npx"][0].tolist() == [64, 25, 0, 0, 16, 64]
    assert b["inner"][0].tolist() == [True, False, False, False, False, True]
    cls = C.unit_classes(co, (1,), [(24, 32)], 3, 1)[0, :, 0].tolist()
    assert cls == ["inner", "clipped", "empty", "empty", "clipped", "inner"]
    # scale 2 halves the coordinates before the floor
    assert C.boxes(co, 2, 12, 16, 3)["xlo"][0, 0] == 2
    # an index out of range empties the box
    v = np.array([True, False, True, True, True, True])
    assert C.unit_classes(co, (1,), [(24, 32)], 3, 1, v)[0, :, 0].tolist()[:2] == ["inner", "empty"]


def test_raw_threshold_by_hand():
    # 3 x 3 patch spread over 6 x 6 floors, R = 3: box 13 x 13 = 169 px = 11 tiles
    xs = np.array([10.0, 12.5, 15.0])
    co = np.zeros((1, 1, 2, 3, 3), np.float32)
    co[0, 0, 0], co[0, 0, 1] = xs[None, :] + 5, xs[:, None] + 5
    assert C.boxes(co, 1, 40, 48, 3)["npx"][0, 0] == 13 * 13
    assert C.unit_classes(co, (1,), [(40, 48)], 3, 3)[0, 0, 0] == "raw"
    assert not C.valu_fast(co, (1,), [(40, 48)], 3, 3)[0, 0, 0]          # 169 > kBoxPx
    co[0, 0] = (co[0, 0] - 15) * 0.5 + 15                                  # 3 x 3 floors: 10 x 10
    assert C.unit_classes(co, (1,), [(40, 48)], 3, 3)[0, 0, 0] == "inner"
    assert C.valu_fast(co, (1,), [(40, 48)], 3, 3)[0, 0, 0]
    # np != NPT (2 x 3 patch in the 9-pixel instantiation): never the box GEMM
    assert not C.valu_fast(np.full((1, 1, 2, 2, 3), 9.5, np.float32), (1,), [(40, 48)], 3,
                           (2, 3))[0, 0, 0]


def test_ifloor_safe_restated():
    v = np.array([1.5, -1.5, 1e9, -1e9, 3e38, -3e38, np.nan, np.inf, -np.inf], np.float32)
    assert C._ifloor_safe(v).tolist() == [1, -2, 10 ** 8, -10 ** 8, 10 ** 8, -10 ** 8, -10 ** 8,
                                          10 ** 8, -10 ** 8]


def test_nchw_modes_by_hand():
    co = _co([(16.5, 10.5), (200.0, 5.0)])
    # fp16, W2 = 32: box x 13 .. 21 -> 16-B pieces (8 halves) from 8: 2 pieces x 9 rows
    assert C.nchw_modes(co, (1,), [(24, 32)], 3, 1, F16)[0, :, 0].tolist() == [1, -1]
    # W2 = 36 (72-B rows): 8-B pieces only
    assert C.nchw_modes(co, (1,), [(24, 36)], 3, 1, F16)[0, 0, 0] == 3
    # a 30 x 30 box is past the 17-tile image: raw path
    big = np.zeros((1, 1, 2, 2, 2), np.float32)
    big[0, 0, 0], big[0, 0, 1] = [[4, 26], [4, 26]], [[4, 4], [26, 26]]
    assert C.nchw_modes(big, (1,), [(40, 48)], 3, 2, F32)[0, 0, 0] == 0


def test_predicates_by_hand():
    assert C.nhwc_supported(3, 3, 3, 128, 4, F32) and C.nhwc_supported(4, 4, 2, 128, 1, F16)
    assert C.nhwc_refusals(3, 3, 3, 128, 2, torch.float64) == {"dtype"}
    assert C.nhwc_refusals(2, 2, 5, 128, 4, F32) == set()          # nout = 484
    assert C.nhwc_refusals(2, 3, 4, 128, 4, F32) == set()          # nout = 486
    assert C.nhwc_refusals(5, 4, 0, 128, 4, F32) == {"np"}
    assert C.nchw_mma_supported(3, 3, 3, 128, 4, [(24, 32), (3, 4)], F16)
    assert not C.nchw_mma_supported(3, 3, 3, 128, 2, [(24, 30), (12, 15)], F32)
    assert C.nchw_mma_supported(3, 3, 3, 128, 1, [(24, 30)], F32)  # 120-B rows: 8-B pieces
    assert not C.nchw_mma_supported(3, 3, 3, 128, 5, [(8, 8)] * 5, F32)
    assert C.nchw_ordered(1, 2048, 36, [(120, 160)], F16)          # cfg2
    assert not C.nchw_ordered(2, 2048, 36, [(120, 160)], F16)
    assert not C.nchw_ordered(1, 2048, 36, [(30, 40)], F16)        # 11 MB ring


def test_levels_ref_and_pyramid():
    f1, f2, co, ii, jj, R = _case(3, M=5, C=8, H2=8, W2=12)
    for dtype in C.DTYPES:
        pyr = C.pyramid(f2, (1, 2, 4), dtype)
        assert [p.shape[3:] for p in pyr] == [(8, 12), (4, 6), (2, 3)]
        assert np.array_equal(pyr[0], C.rounded(f2, dtype))
        assert np.array_equal(pyr[1], C.rounded(pyr[1], dtype))
        ref = C.levels_ref(f1, pyr, co, ii, jj, R, (1, 2, 4))
        assert ref.shape == (1, 5, 7, 7, 3, 3, 3)
        assert np.array_equal(ref[..., 2], oracle.corr_fwd(f1, pyr[2], co / np.float32(4), ii,
                                                            jj, R))
    mean = f2.reshape(1, 4, 8, 4, 2, 6, 2).mean((4, 6))
    assert np.abs(C.pyramid(f2, (2,), F32)[0] - mean).max() < 1e-6


# ------------------------------------------------ the tables reach their branches
def _classes(kw, levels, seed, valid=None):
    f1, f2, co, ii, jj, R = _case(seed, **kw)
    shapes = C.level_shapes(f2.shape[3], f2.shape[4], levels)
    return C.unit_classes(co, levels, shapes, R, f1.shape[3:], valid)


def _patch(kw):
    p = kw.get("p", 3)
    return kw.get("Hp", p), kw.get("Wp", p), kw.get("R", 3)


@pytest.mark.parametrize("case", C.a_cases(), ids=lambda c: c[0])
def test_a_cases_take_the_runtime_shape_kernel(case):
    _, kw, levels, mark = case
    hp, wp, R = _patch(kw)
    assert (hp, wp, R) != (3, 3, 3)
    for dtype in C.DTYPES:
        assert C.nhwc_supported(hp, wp, R, kw.get("C", 128), len(levels), dtype)
    cls = _classes(kw, levels, C.A_SEED)
    assert min(C.level_shapes(kw.get("H2", 24), kw.get("W2", 32), levels)[-1]) >= 1
    if mark == "rt-mixed":
        assert (cls == "raw").mean() >= 0.1
        assert ((cls == "inner") | (cls == "clipped")).mean() >= 0.1


def test_a_table_is_the_issue_list():
    ids = [c[0] for c in C.a_cases()]
    assert len(ids) == len(set(ids)) == 10 * 4 + 4 + 2
    assert {len(lv) for lv in C.A_LEVELS} == {1, 2, 3, 4}   # unpaired (L <= 2) and paired
    assert {c[3] for c in C.a_cases()} == {"rt", "rt-mixed"}


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f16"])
def test_every_unit_class_is_reached(dtype):
    """empty, inner, clipped and raw over the run-time shape table, and over
    the DPVO-shape table of section B, for each feature dtype."""
    seen = set()
    for _, kw, levels, _ in C.a_cases():
        assert C.nhwc_supported(*_patch(kw), 128, len(levels), dtype)
        seen |= set(np.unique(_classes(kw, levels, C.A_SEED)))
    assert seen == {"empty", "inner", "clipped", "raw"}
    seen = set()
    for p, R, dt in C.B_SHAPES:
        if dt != dtype or (p, R) != (3, 3):
            continue
        for B, M in C.B_UNORDERED:
            seen |= set(np.unique(_classes(dict(B=B, M=M, p=p, R=R), C.SCALES, C.B_SEED + M)))
    assert {"empty", "inner", "clipped"} <= seen


def test_b_table_is_the_issue_list():
    assert [m for b, m in C.B_UNORDERED if b == 1] == [1, 2, 3, 5, 67]
    assert [m for b, m in C.B_UNORDERED if b == 2] == [3, 5]
    assert C.B_ORDERED_M == [1, 7, 8, 9, 15, 17, 130]
    assert {(p, R, dt) for p, R, dt in C.B_SHAPES} == {(3, 3, F32), (3, 3, F16), (2, 3, F32)}
    for p, R, dt in C.B_SHAPES:
        for L in (1, 2, 3, 4):
            assert C.nhwc_supported(p, p, R, 128, L, dt)
    for M in C.B_ORDERED_M:
        o = C.orders(M, C.B_SEED)
        assert set(o) == {"identity", "reversed", "random"}
        for v in o.values():
            assert v.dtype == np.int32 and sorted(v.tolist()) == list(range(M))
    # odd edge counts leave a half-filled pair (half = (per + 1) / 2); counts
    # below 8 leave whole XCD shares of the ordered split (per = (M + 7) / 8) empty
    assert any(m % 2 for _, m in C.B_UNORDERED) and any(m < 8 for m in C.B_ORDERED_M)
    assert any(m % 8 == 1 for m in C.B_ORDERED_M) and any(m % 8 == 7 for m in C.B_ORDERED_M)


@pytest.mark.parametrize("case", C.C_CASES, ids=lambda c: c[0])
def test_c_cases_fall_back_for_the_stated_reason(case):
    name, kw, levels, why = case
    hp, wp, R = _patch(kw)
    for dtype in C.DTYPES:
        assert C.nhwc_refusals(hp, wp, R, kw.get("C", 128), len(levels), dtype) == why
        assert C.nhwc_supported(hp, wp, R, kw.get("C", 128), len(levels), dtype) == (not why)
    assert bool(why) != (name == "mixed-layout")  # there the layout alone sends it back
    assert min(C.level_shapes(kw.get("H2", 24), kw.get("W2", 32), levels)[-1]) >= 1


@pytest.mark.parametrize("case", C.D_CASES, ids=lambda c: c[0])
def test_d_cases_take_the_valu_levels_kernel(case):
    _, kw, levels, dtype = case
    hp, wp, R = _patch(kw)
    shapes = C.level_shapes(kw.get("H2", 24), kw.get("W2", 32), levels)
    assert not C.nchw_mma_supported(hp, wp, R, kw.get("C", 128), len(levels), shapes, dtype)
    assert 1 <= len(levels) <= 8 and hp * wp <= 16


def test_d_table_reaches_both_valu_paths_on_a_late_level():
    """The box GEMM and the per-tap path, on levels past the first (where a
    kernel that read level 0's parameters would go wrong)."""
    fast = []
    for _, kw, levels, _ in C.D_CASES:
        f1, f2, co, ii, jj, R = _case(C.D_SEED, **kw)
        shapes = C.level_shapes(f2.shape[3], f2.shape[4], levels)
        fast.append(C.valu_fast(co, levels, shapes, R, f1.shape[3:])[..., 1:].ravel())
    fast = np.concatenate(fast)
    assert fast.any() and not fast.all()
    assert {len(lv) for _, _, lv, _ in C.D_CASES} >= {2, 5, 8}


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f16"])
def test_e_cases_run_the_ordered_prologue(dtype):
    s = C.E_RINGS[dtype]
    shape = [(s["H2"], s["W2"])]
    assert C.nchw_mma_supported(3, 3, 3, 128, 2, shape * 2, dtype)
    for M in C.E_M + [C.kOrdMaxE]:
        assert C.nchw_ordered(1, M, s["N2"], shape, dtype)
    assert not C.nchw_ordered(1, C.kOrdMaxE + 1, s["N2"], shape, dtype)
    assert not C.nchw_ordered(1, 1030, s["N2"] // 2, shape, dtype)  # a ring under 32 MiB
    assert not C.nchw_ordered(1, 1030, C.kOrdMaxN2 + 1, shape, dtype)
    # M % 4 != 0 (the last chunk wants positions >= M), M < 4, M > 256 (K > 1)
    assert any(m % 4 for m in C.E_M) and any(m < 4 for m in C.E_M) and any(m > 256 for m in C.E_M)
    for M in C.E_M:
        _, _, ii, jj = C.e_edges(C.E_SEED + M, M, s["N2"], s["H2"], s["W2"])
        assert jj.min() >= 0 and jj.max() < s["N2"]
        assert s["N2"] - len(np.unique(jj)) >= 64 * 4  # hundreds of empty bins
    _, _, _, jj = C.e_edges(C.E_SEED + 257, 257, s["N2"], s["H2"], s["W2"], "one_frame")
    assert len(np.unique(jj)) == 1
    _, _, _, jj = C.e_edges(C.E_SEED + 257, 257, s["N2"], s["H2"], s["W2"], "oob")
    assert (jj == -1).sum() >= 20 and (jj == s["N2"] + 3).sum() >= 20
    assert 0.19 <= ((jj < 0) | (jj >= s["N2"])).mean() <= 0.21


def test_e_threshold_ring_is_the_fp16_one():
    assert C.E_RINGS[F16]["N2"] == C.kOrdMaxN2
    s = C.E_RINGS[F16]
    assert not C.nchw_ordered(1, 1030, s["N2"] + 1, [(s["H2"], s["W2"])], F16)


# ------------------------------------- the restatement pinned to the native code
FORWARD, LEVELS, LEVELS_NHWC = 0, 1, 2                  # dpvo_hot.h: DPVO_CORR_*
NONE, NHWC, NCHW_MMA, NCHW_MMA_ORDERED, VALU = range(5)  # DPVO_CORR_PATH_*
_CASE_DEFAULTS = {k: v.default for k, v in inspect.signature(_case).parameters.items()
                  if v.default is not inspect.Parameter.empty}


@pytest.fixture(scope="module")
def lib():
    import dpvo_amd

    return dpvo_amd.c_abi()


def _query(lib, entry, hp, wp, R, Cc, shapes, dtype, B, M, N2, align=16, f1=16):
    """dpvo_corr_query_path on a call of these sizes; fmap1 is the address
    `f1`, every level `align` (the tables' tensors are torch allocations: 16-B
    aligned)."""
    L = len(shapes)
    p = ctypes.c_void_p(f1)
    f2 = (ctypes.c_void_p * L)(*[align] * L)
    H2 = (ctypes.c_int * L)(*[h for h, _ in shapes])
    W2 = (ctypes.c_int * L)(*[w for _, w in shapes])
    sc = (ctypes.c_float * L)(*[1.0] * L)
    path = ctypes.c_int(-1)
    st = lib.dpvo_corr_query_path(entry, p, f2, H2, W2, sc, L, p, p, p, None, B, M, Cc, hp, wp, 9,
                                  N2, R, {F32: 0, F16: 1}[dtype], p, ctypes.byref(path))
    return st, path.value


def _pin(lib, hp, wp, R, Cc, shapes, dtype, B, M, N2, single=False):
    """The native selection of one call against nhwc_refusals / nhwc_supported,
    nchw_mma_supported and nchw_ordered; returns the path of the call sequence
    of the extension for a channels-last and for an NCHW pyramid."""
    L = len(shapes)
    why = C.nhwc_refusals(hp, wp, R, Cc, L, dtype)
    assert C.nhwc_supported(hp, wp, R, Cc, L, dtype) == (not why)
    assert _query(lib, LEVELS_NHWC, hp, wp, R, Cc, shapes, dtype, B, M, N2) == \
        ((3, NONE) if why else (0, NHWC)), why
    want = VALU
    if C.nchw_mma_supported(hp, wp, R, Cc, L, shapes, dtype):
        want = NCHW_MMA_ORDERED if C.nchw_ordered(B, M, N2, shapes, dtype) else NCHW_MMA
    assert _query(lib, LEVELS, hp, wp, R, Cc, shapes, dtype, B, M, N2) == (0, want)
    if single:
        assert L == 1
        assert _query(lib, FORWARD, hp, wp, R, Cc, shapes, dtype, B, M, N2) == (0, want)
    return (want if why else NHWC), want


def _pin_case(lib, kw, levels, dtype, **over):
    d = dict(_CASE_DEFAULTS, **kw)
    d.update(over)
    hp, wp = d["Hp"] or d["p"], d["Wp"] or d["p"]
    return _pin(lib, hp, wp, d["R"], d["C"], C.level_shapes(d["H2"], d["W2"], levels), dtype,
                d["B"], d["M"], d["N2"])


@pytest.mark.parametrize("dtype", C.DTYPES, ids=["f32", "f16"])
def test_tables_select_what_the_restatement_predicts(lib, dtype):
    """Every case of the A .. F tables, and the two threshold cases of
    test_corr_dispatch_gpu.py, through dpvo_corr_query_path."""
    for _, kw, levels, _ in C.a_cases():
        assert _pin_case(lib, kw, levels, dtype)[0] == NHWC
    for p, R, _ in C.B_SHAPES:
        for L in (1, 2, 3, 4):
            for B, M in C.B_UNORDERED + [(1, m) for m in C.B_ORDERED_M]:
                assert _pin_case(lib, dict(B=B, M=M, p=p, R=R), C.SCALES[:L], dtype)[0] == NHWC
    for name, kw, levels, why in C.C_CASES:
        cl, nchw = _pin_case(lib, kw, levels, dtype)
        assert (cl == NHWC) == (not why)
        # what the NCHW entry then runs: C = 64 and five levels are past the matrix cores too
        assert nchw == (VALU if why & {"C", "L"} else NCHW_MMA), name
    for name, kw, levels, dt in C.D_CASES:  # pinned for both dtypes, VALU for the case's own
        assert _pin_case(lib, kw, levels, dtype)[1] == VALU or dt != dtype, name
    s = C.E_RINGS[dtype]
    shape = [(s["H2"], s["W2"])]
    for M in C.E_M + [5, 257]:
        assert _pin(lib, 3, 3, 3, 128, shape, dtype, 1, M, s["N2"], single=True)[1] == \
            NCHW_MMA_ORDERED
        assert _pin(lib, 3, 3, 3, 128, shape * 2, dtype, 1, M, s["N2"])[1] == NCHW_MMA_ORDERED
    for kernel, spec in C.F_KERNELS.items():
        for levels in C.F_LEVELS:
            cl, nchw = _pin_case(lib, dict(M=67, C=spec["C"]), levels, dtype)
            got = cl if spec["layout"] == "cl" else nchw
            assert got == {"nhwc": NHWC, "nchw_mma": NCHW_MMA, "valu": VALU}[kernel]
    # test_nchw_ordered_edge_count_threshold (fp32 ring) / _frame_count_threshold (fp16 ring)
    s = C.E_RINGS[F32]
    for M, want in ((C.kOrdMaxE, NCHW_MMA_ORDERED), (C.kOrdMaxE + 1, NCHW_MMA)):
        assert _pin(lib, 3, 3, 3, 128, [(s["H2"], s["W2"])], F32, 1, M, s["N2"], True)[1] == want
    s = C.E_RINGS[F16]
    for N2, want in ((C.kOrdMaxN2, NCHW_MMA_ORDERED), (C.kOrdMaxN2 + 1, NCHW_MMA)):
        assert _pin(lib, 3, 3, 3, 128, [(s["H2"], s["W2"])], F16, 1, 1030, N2, True)[1] == want


def test_alignment_the_restatement_assumes(lib):
    """nchw_mma_supported is stated for 16-B aligned bases: an 8-B aligned level
    still takes the matrix cores (8-B pieces), a 4-B aligned one or an fmap1
    off 16 B the VALU kernel."""
    args = (3, 3, 3, 128, [(24, 32)], F32, 1, 37, 4)
    assert _query(lib, LEVELS, *args, align=16) == (0, NCHW_MMA)
    assert _query(lib, LEVELS, *args, align=8) == (0, NCHW_MMA)
    assert _query(lib, LEVELS, *args, align=4) == (0, VALU)
    assert _query(lib, LEVELS, *args, f1=8) == (0, VALU)


@pytest.mark.parametrize("levels", C.F_LEVELS, ids=["L1", "L4"])
@pytest.mark.parametrize("kernel", list(C.F_KERNELS))
def test_f_cases(kernel, levels):
    spec = C.F_KERNELS[kernel]
    f1, f2, co, ii, jj, R = _case(C.F_SEED, M=67, C=spec["C"])
    N1, N2 = f1.shape[1], f2.shape[1]
    shapes = C.level_shapes(24, 32, levels)
    for dtype in C.DTYPES:
        nhwc = C.nhwc_supported(3, 3, R, spec["C"], len(levels), dtype)
        mma = C.nchw_mma_supported(3, 3, R, spec["C"], len(levels), shapes, dtype)
        assert (kernel == "nhwc") == (spec["layout"] == "cl")
        assert nhwc == (spec["C"] == 128) and mma == (spec["C"] == 128)
        assert not C.nchw_ordered(1, 67, N2, shapes, dtype)
    i2, j2, ok = C.f_bad_indices(C.F_SEED, ii, jj, N1, N2)
    assert (i2 < 0).any() and (i2 >= N1).any() and (j2 < 0).any() and (j2 >= N2).any()
    assert ok.mean() >= 0.5 and (~ok).sum() >= 8
    assert np.array_equal(i2[ok], ii[ok]) and np.array_equal(j2[ok], jj[ok])
    for whole in (False, True):
        bad, mask, benign = C.f_bad_coords(C.F_SEED + 1, co, (1e9, -1e9, 3e38, -3e38), whole)
        touched = mask.any((0, 2, 3))
        assert 4 <= touched.sum() <= 67 // 10 + 1
        assert (mask.sum((2, 3))[0][touched] == (9 if whole else 1)).all()
        assert np.isfinite(bad).all() and (np.abs(bad[:, touched]) >= 1e9).any()
        assert np.array_equal(bad[:, ~touched], co[:, ~touched])
        assert np.abs(benign).max() < 1e3
        # every affected pixel has |x| or |y| >= 1e9: outside every map at every scale
        far = (np.abs(bad[:, :, 0]) >= 1e9) | (np.abs(bad[:, :, 1]) >= 1e9)
        assert np.array_equal(far, mask)
    bad, mask, _ = C.f_bad_coords(C.F_SEED + 2, co, (np.nan, np.inf, -np.inf), False)
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    assert np.array_equal(~np.isfinite(bad).all(2), mask)
