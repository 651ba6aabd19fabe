"""GPU: how corr_nhwc_lvl_kernel stores the edges' [nout][L] output blocks.

The blocks leave the workgroup's LDS as 16-B write-through stores (four levels)
or as scalar stores (fewer levels), by the whole workgroup after its barrier;
which edges a workgroup holds depends on the edge count, the level count and
the XCD order.  Cases (tests/corr_store_cases.py): E in {1, 2, 3, 9, 17} with
and without the order of fastba.reproject(..., mem=) -- workgroups with a first
unit and no second, and with neither; 17 puts a pair across a half boundary --
levels [1,2,4,8], [1,2,4], [1,4], [1]; fp32 and fp16 features; p = 3, R = 3 and
the run-time shape p = 2, R = 2; an edge whose boxes are empty on every level
and an edge whose ii is out of range (their blocks: stored, all zero).

Every case: the output block holds NaN before the call and is finite after it;
it equals, bit for bit, what the commit before the store change returned on the
same inputs (tests/golden/corr_store_parent.npz, recorded by
scripts/make_corr_store_golden.py); it matches the oracle at this path's
tolerance (test_corr_dispatch_gpu.py: 1e-5 of max(1, max|ref|) per level for
fp32 features, 2e-5 for fp16 features); and the same call repeated into the
NaN-refilled block returns the same bits."""
import os

import numpy as np
import pytest

import corr_cases as C
import corr_store_cases as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corr_store_parent.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", S.cases(), ids=S.case_id)
def test_store_paths(gpu, golden, case):
    out, again, (f1, pyr, co, ii, jj, R) = S.run(gpu, case)
    assert np.isfinite(out).all()
    assert np.array_equal(out, again)
    want = golden[S.key(case["shape"], case["dname"], case["levels"], case["bad"])][:, :case["E"]]
    assert out.shape == want.shape
    assert np.array_equal(out, want)
    # the oracle on the edges whose indices are in range; the others are zero blocks
    ok = (ii >= 0) & (ii < f1.shape[1])
    assert not out[:, ~ok].any()
    ref = C.levels_ref(f1, pyr, co[:, ok], ii[ok], jj[ok], R, case["levels"])
    tol = 1e-5 if case["dname"] == "f32" else 2e-5
    for l in range(len(case["levels"])):
        C._close(out[:, ok][..., l], ref[..., l], tol)
    if case["bad"]:  # edge 0: windows outside every map
        assert not out[:, 0].any()
