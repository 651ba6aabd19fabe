"""GPU: projective_ops.transform_fused (train.hip) against the fp64
restatement of train_ref, forward and backward.

Bar, per output tensor: max-abs error against the restatement no more than
twice the max-abs error of the parent's fp32 composition (pops.transform
through the lietorch ops, forward and autograd.grad, same inputs) against the
same restatement, with the floor 2^-22 max|ref| (the rounding of an fp32
output).  Both are fp32 evaluations of one formula that differ only in where
they round; the factor 2 covers the different rounding points.
"""
import functools

import pytest
import torch

import train_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 0.02  # every Z of the restatement stays this far from 0.1 and 0.2


@functools.lru_cache(maxsize=None)
def case(P, N, E):
    """fp32 inputs on the CPU.  Frame f sits at about (0.05, -0.03, -0.25) f
    with a small rotation, so Z = 1 - 0.25 (j - i) d (roughly) crosses both
    thresholds for depths around 3-4; intrinsics differ per frame; kk is
    unsorted; patch M - 1 is never used, nor (N = 5) pose 4."""
    g = torch.Generator().manual_seed(1000 * P + 100 * N + E)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    M, used = 7, (4 if N == 5 else N)
    f = torch.arange(N, dtype=torch.float64)[:, None]
    t = f * torch.tensor([0.05, -0.03, -0.25], dtype=torch.float64) + 0.02 * (rnd(N, 3) - 0.5)
    q = torch.cat([0.08 * (rnd(N, 3) - 0.5), torch.ones(N, 1, dtype=torch.float64)], 1)
    q = q * (0.7 + 0.6 * rnd(N, 1))  # not normalised: the ops normalise on load
    poses = torch.cat([t, q], 1)
    intr = torch.cat([80 + 5 * f, 85 + 3 * f, 48 + f, 32 - f], 1)
    c = torch.stack([5 + 85 * rnd(M), 5 + 55 * rnd(M)], 1)  # centres
    off = torch.arange(P, dtype=torch.float64) - P // 2
    x = c[:, 0, None, None] + off[None, None, :].expand(M, P, P)
    y = c[:, 1, None, None] + off[None, :, None].expand(M, P, P)
    d = (0.3 + 4.2 * rnd(M))[:, None, None] * (1 + 0.02 * (rnd(M, P, P) - 0.5))
    patches = torch.stack([x, y, d], 1)
    ii = torch.randint(0, used, (E,), generator=g)
    jj = torch.randint(0, used, (E,), generator=g)
    kk = torch.randint(0, M - 3, (E,), generator=g)
    if E >= 3:
        jj[1] = ii[1]                      # an ii == jj edge
        ii[2], kk[2] = ii[0], kk[0]        # edges sharing a pose and a patch
    poses, patches, intr = poses.float(), patches.float(), intr.float()
    if E >= 63:  # one edge each with Z = 0.05 and Z = 0.15, on patches of their own
        for e, k, target in ((5, M - 3, 0.05), (6, M - 2, 0.15)):
            ii[e], jj[e], kk[e] = 0, 1, k
            z = []
            for scale in (1.0, 2.0):  # Z is affine in the depth
                q = patches.clone()
                q[k, 2] *= scale
                z.append(R.transform(poses, q, intr, ii[e:e + 1], jj[e:e + 1], kk[e:e + 1])["Z"]
                         [0, P // 2, P // 2])
            patches[k, 2] *= float(1.0 + (target - z[0]) / (z[1] - z[0]))
    for _ in range(50):  # move depths until no Z is near a threshold
        Z = R.transform(poses, patches, intr, ii, jj, kk)["Z"]
        near = ((Z - 0.1).abs() < 1.5 * MARGIN) | ((Z - 0.2).abs() < 1.5 * MARGIN)
        if not near.any():
            break
        bad = kk[near.flatten(1).any(1)].unique()
        patches[bad, 2] *= 1.06
    cot = torch.randn(E, P, P, 2, generator=g)
    return {"poses": poses, "patches": patches, "intr": intr, "ii": ii, "jj": jj, "kk": kk,
            "cot": cot, "N": N, "M": M, "P": P, "E": E}


@functools.lru_cache(maxsize=None)
def reference(P, N, E):
    c = case(P, N, E)
    return R.transform(c["poses"], c["patches"], c["intr"], c["ii"], c["jj"], c["kk"], c["cot"])


def on_device(c, dev, noncontig=False, grad=(True, True)):
    """The case's tensors on the device: poses [1, N, 7], patches
    [1, M, 3, P, P], intrinsics [1, N, 4]; with noncontig as strided views."""
    def put(t):
        t = t.to(dev)
        if noncontig:
            big = torch.zeros(t.shape + (2,), device=dev, dtype=t.dtype)
            big[..., 1] = t
            t = big[..., 1]
            assert not t.is_contiguous() or t.numel() <= 1
        return t[None]

    Pd, Kd = put(c["poses"]), put(c["patches"])
    Pd.requires_grad_(grad[0])
    Kd.requires_grad_(grad[1])
    idx = [put(c[k])[0] for k in ("ii", "jj", "kk")]
    return Pd, Kd, put(c["intr"]), idx


def run(fn, c, dev, **kw):
    """fn = 'fused' or 'parent' -> coords, valid, g_poses [N, 6], g_patches, pad."""
    from dpvo_amd import projective_ops as pops
    from dpvo_amd.lietorch import SE3

    Pd, Kd, intr, (ii, jj, kk) = on_device(c, dev, **kw)
    f = pops.transform_fused if fn == "fused" else pops.transform
    coords, valid = f(SE3(Pd), Kd, intr, ii, jj, kk, valid=True)
    need = [t for t in (Pd, Kd) if t.requires_grad]
    grads = list(torch.autograd.grad((coords * c["cot"].to(dev)[None]).sum(), need))
    gP = grads.pop(0) if Pd.requires_grad else None
    gK = grads.pop(0) if Kd.requires_grad else None
    out = {"coords": coords[0], "valid": valid[0],
           "g_poses": None if gP is None else gP[0, :, :6],
           "g_pad": None if gP is None else gP[0, :, 6],
           "g_patches": None if gK is None else gK[0]}
    return {k: None if v is None else v.detach().double().cpu() for k, v in out.items()}


def check(got, par, ref, tag):
    bad = {}
    for t in ("coords", "g_poses", "g_patches"):
        scale = float(ref[t].abs().max())
        e_new = float((got[t] - ref[t]).abs().max()) if ref[t].numel() else 0.0
        e_par = float((par[t] - ref[t]).abs().max()) if ref[t].numel() else 0.0
        bound = max(2 * e_par, 2.0 ** -22 * scale)
        print(f"PARITY transform {tag} {t}: fused {e_new:.3e} parent {e_par:.3e} "
              f"bound {bound:.3e} max|ref| {scale:.3e}")
        if not e_new <= bound:
            bad[t] = (e_new, bound)
    assert not bad, bad


SHAPES = [(P, N, E) for P in (1, 3) for N in (2, 5) for E in (1, 63, 65, 257)]


@pytest.mark.parametrize("P,N,E", SHAPES)
def test_case_keeps_its_margins(P, N, E):
    """The property the comparison rests on, asserted on the restatement."""
    Z = reference(P, N, E)["Z"]
    assert ((Z - 0.1).abs() >= MARGIN).all() and ((Z - 0.2).abs() >= MARGIN).all()
    if E >= 63:
        assert (Z < 0.1).any() and ((Z > 0.1) & (Z < 0.2)).any() and (Z > 0.2).any()
        c = case(P, N, E)
        assert (c["ii"] == c["jj"]).any() and not (c["kk"] == c["M"] - 1).any()
        assert c["kk"].tolist() != sorted(c["kk"].tolist())


@pytest.mark.parametrize("noncontig", [False, True])
@pytest.mark.parametrize("P,N,E", SHAPES)
def test_matches_restatement(gpu, P, N, E, noncontig):
    c, ref = case(P, N, E), reference(P, N, E)
    got = run("fused", c, gpu, noncontig=noncontig)
    par = run("parent", c, gpu, noncontig=noncontig)
    assert torch.equal(got["valid"], ref["valid"])
    assert got["coords"].shape == (E, P, P, 2) and got["g_patches"].shape == (c["M"], 3, P, P)
    check(got, par, ref, f"P{P} N{N} E{E}{' strided' if noncontig else ''}")
    assert (got["g_pad"] == 0).all()
    # what no edge uses gets exactly zero
    assert (got["g_patches"][c["M"] - 1] == 0).all()
    if N == 5:
        assert (got["g_poses"][4] == 0).all()


def test_repeats_are_bit_identical(gpu):
    c = case(3, 5, 257)
    a, b = run("fused", c, gpu), run("fused", c, gpu)
    for t in ("coords", "valid", "g_poses", "g_patches"):
        assert torch.equal(a[t], b[t]), t


def test_needs_input_grad_is_honoured(gpu):
    c = case(3, 5, 65)
    both = run("fused", c, gpu)
    only_p = run("fused", c, gpu, grad=(True, False))
    only_k = run("fused", c, gpu, grad=(False, True))
    assert only_p["g_patches"] is None and only_k["g_poses"] is None
    assert torch.equal(only_p["g_poses"], both["g_poses"])
    assert torch.equal(only_k["g_patches"], both["g_patches"])
    # no input needs a gradient: the outputs carry none
    from dpvo_amd import projective_ops as pops

    Pd, Kd, intr, (ii, jj, kk) = on_device(c, gpu, grad=(False, False))
    assert not pops.transform_fused(Pd, Kd, intr, ii, jj, kk).requires_grad


def test_corr_layout_is_the_same_launch_output(gpu):
    from dpvo_amd import projective_ops as pops

    c = case(3, 5, 65)
    Pd, Kd, intr, (ii, jj, kk) = on_device(c, gpu, grad=(False, False))
    coords, corr = pops.transform_fused(Pd, Kd, intr, ii, jj, kk, corr_layout=True)
    assert corr.shape == (1, 65, 2, 3, 3) and corr.is_contiguous()
    assert torch.equal(corr, coords.permute(0, 1, 4, 2, 3))


def test_no_edges(gpu):
    from dpvo_amd import projective_ops as pops

    c = case(3, 5, 65)
    Pd, Kd, intr, (ii, jj, kk) = on_device(c, gpu)
    coords, valid = pops.transform_fused(Pd, Kd, intr, ii[:0], jj[:0], kk[:0], valid=True)
    assert coords.shape == (1, 0, 3, 3, 2) and valid.shape == (1, 0, 3, 3)
    gP, gK = torch.autograd.grad(coords.sum(), (Pd, Kd))
    assert gP.shape == Pd.shape and gK.shape == Kd.shape
    assert (gP == 0).all() and (gK == 0).all()


def test_out_of_range_edges_are_closed(gpu):
    """An index outside [0, N) / [0, M): NaN coords, valid 0, no gradient, no
    read; the other edges are what they are without those edges."""
    P, N, E = 3, 5, 65
    c = dict(case(P, N, E))
    ii, jj, kk = c["ii"].clone(), c["jj"].clone(), c["kk"].clone()
    ii[3], jj[10], kk[20], kk[21], jj[40] = -1, N, c["M"], -1, 1 << 40
    closed = [3, 10, 20, 21, 40]
    keep = torch.tensor([e for e in range(E) if e not in closed])
    c.update(ii=ii, jj=jj, kk=kk)
    got = run("fused", c, gpu)
    assert got["coords"][closed].isnan().all() and (got["valid"][closed] == 0).all()
    sub = dict(c, ii=ii[keep], jj=jj[keep], kk=kk[keep], cot=c["cot"][keep], E=len(keep))
    ref = R.transform(sub["poses"], sub["patches"], sub["intr"], sub["ii"], sub["jj"], sub["kk"],
                      sub["cot"])
    par = run("parent", sub, gpu)
    kept = dict(got, coords=got["coords"][keep])
    assert torch.equal(got["valid"][keep], ref["valid"])
    check(kept, par, ref, "out-of-range")
    assert got["g_poses"].isfinite().all() and got["g_patches"].isfinite().all()


def test_no_host_synchronisation(gpu):
    c = case(3, 5, 257)
    run("fused", c, gpu)  # warm-up: module load, allocator
    Pd, Kd, intr, (ii, jj, kk) = on_device(c, gpu)
    cot = c["cot"].to(gpu)[None]
    from dpvo_amd import projective_ops as pops

    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        coords, valid = pops.transform_fused(Pd, Kd, intr, ii, jj, kk, valid=True)
        gP, gK = torch.autograd.grad((coords * cot).sum(), (Pd, Kd))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert gP.isfinite().all() and gK.isfinite().all()


def test_unsupported_patch_size_raises(gpu):
    from dpvo_amd import projective_ops as pops

    Pd = torch.zeros(1, 2, 7, device=gpu)
    Pd[..., 6] = 1
    Kd = torch.ones(1, 3, 3, 2, 2, device=gpu)
    intr = torch.ones(1, 2, 4, device=gpu)
    z = torch.zeros(1, dtype=torch.long, device=gpu)
    with pytest.raises(RuntimeError):
        pops.transform_fused(Pd, Kd, intr, z, z, z)


def test_c_abi_accepts_the_advertised_workspace(gpu):
    """dpvo_transform_backward with real buffers: exactly
    dpvo_transform_workspace_bytes(E, P) bytes are accepted and give the
    gradients of the Python surface; one byte less is DPVO_ERR_WORKSPACE."""
    import ctypes

    import dpvo_amd

    lib = dpvo_amd.c_abi()
    lib.dpvo_transform_workspace_bytes.restype = ctypes.c_size_t
    c = case(3, 5, 65)
    want = run("fused", c, gpu)
    Pd, Kd, intr, (ii, jj, kk) = on_device(c, gpu, grad=(False, False))
    cot = c["cot"].to(gpu).contiguous()
    need = lib.dpvo_transform_workspace_bytes(65, 3)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    gP = torch.full((5, 6), float("nan"), device=gpu)
    gK = torch.full((c["M"], 3, 3, 3), float("nan"), device=gpu)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nbytes):
        return lib.dpvo_transform_backward(ptr(Pd), ptr(Kd), ptr(intr), ptr(ii), ptr(jj), ptr(kk), 65,
                                           3, 5, c["M"], ptr(cot), ptr(gP), ptr(gK), ptr(ws),
                                           ctypes.c_size_t(nbytes), stream)

    assert call(need - 1) == 4
    torch.cuda.synchronize()
    assert gP.isnan().all() and gK.isnan().all()  # rejected on the host: nothing written
    assert call(need) == 0
    torch.cuda.synchronize()
    assert torch.equal(gP.double().cpu(), want["g_poses"])
    assert torch.equal(gK.double().cpu(), want["g_patches"])
