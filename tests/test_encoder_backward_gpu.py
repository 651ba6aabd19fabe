"""GPU: the encoders' training forward and HIP backward (csrc/encoder.hip,
csrc/encoder_bwd.hip, dpvo_amd.extractor with differentiable=True) against
torch.autograd through the fp64 restatement (tests/encoder_ref.py) on the same
device.

Bar, per gradient tensor: max|got - ref| <= 1e-5 max|ref| (the forward's fp32
bar; the float32 autograd of the same restatement lands within 2.2e-6).  With
instance norm the bias gradients of convs 0..9 are compared with exact zero,
not with the reference's rounding noise.  Every gradient buffer is pre-filled
with NaN through the extension's `backward` and must be finite afterwards.
"""
import numpy as np
import pytest
import torch

import encoder_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9, 11), (1, 16, 16), (2, 30, 46), (3, 9, 11), (1, 38, 54), (1, 6, 150), (1, 150, 6),
          (1, 96, 128)]
KINDS = [("instance", 128), ("none", 384)]
NAMES = [n for n, _ in encoder_ref.param_shapes(128)]


def make(norm, out_dim, dev, differentiable=True):
    from dpvo_amd.extractor import BasicEncoder4

    enc = BasicEncoder4(out_dim, norm, torch.float32, differentiable=differentiable)
    P = encoder_ref.formula_params(out_dim, norm)
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in P.items()})
    return enc.to(dev)


def images(shape, dev):
    """Seeded U(-1, 1) images [1, n, 3, H, W], as test_encoder_gpu.case."""
    n, H, W = shape
    rng = np.random.RandomState(1000 + H * 7 + W)
    return torch.as_tensor(rng.uniform(-1, 1, (1, n, 3, H, W)).astype(np.float32), device=dev)


def cotangent(shape4, dev):
    n = int(np.prod(shape4))
    c = encoder_ref._hash01(np.arange(n, dtype=np.float64), 7.0).reshape(shape4)
    return torch.as_tensor(c, dtype=torch.float64, device=dev)


def ref_grads(P, img4, norm, cot):
    """fp64 autograd through the restatement: out and the 22 gradients in state_dict order."""
    P = {k: v.clone().requires_grad_() for k, v in P.items()}
    out = encoder_ref.encoder_ref(P, img4.double(), norm)
    g = torch.autograd.grad((out * cot).sum(), [P[k] for k in NAMES])
    return out.detach(), list(g)


_cache = {}


def case(gpu, shape, norm, out_dim):
    """(images, cotangent, reference output, reference gradients): once per (shape, norm)."""
    key = (shape, norm)
    if key not in _cache:
        img = images(shape, gpu)
        P = encoder_ref.to_torch(encoder_ref.formula_params(out_dim, norm), gpu)
        h, w = encoder_ref.out_size(encoder_ref.out_size(shape[1])), \
            encoder_ref.out_size(encoder_ref.out_size(shape[2]))
        cot = cotangent((shape[0], out_dim, h, w), gpu)
        out, g = ref_grads(P, img[0], norm, cot)
        _cache[key] = (img, cot, out, g)
    return _cache[key]


def run_ext(enc, img4, cot=None, channels_last=False, state=None):
    """pack_weights_device + forward_train (+ backward with NaN-filled gradient
    buffers) through the extension.  Returns (out, grads, state)."""
    from dpvo_amd import extractor

    e = extractor.ext()
    dev = img4.device
    N, _, H, W = img4.shape
    od, nc = enc.output_dim, enc._ncode()
    params = [p.detach().contiguous() for p in enc.parameters()]
    if state is None:
        blob = torch.empty(e.packed_bytes(od, e.F32), dtype=torch.uint8, device=dev)
        e.pack_weights_device(params, od, nc, e.F32, blob)
        saved = torch.empty(e.saved_bytes(N, H, W, od, nc), dtype=torch.uint8, device=dev)
        h, w = extractor.out_size(extractor.out_size(H)), extractor.out_size(extractor.out_size(W))
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        out = torch.full((N, od, h, w), float("nan"), dtype=torch.float32,
                         device=dev).contiguous(memory_format=fmt)
        e.forward_train(blob, e.F32, nc, img4.contiguous(), out, saved)
        assert torch.isfinite(out).all()
        state = (out, saved)
    out, saved = state
    if cot is None:
        return out, None, state
    grads = [torch.full_like(p, float("nan")) for p in params]
    ws = torch.empty(e.backward_workspace_bytes(N, H, W, od), dtype=torch.uint8, device=dev)
    e.backward(nc, params, img4.contiguous(), saved, cot, grads, ws)
    for name, g in zip(NAMES, grads):
        assert torch.isfinite(g).all(), name + ": not fully written"
    return out, grads, state


def check_grads(got, ref, norm, label):
    """The bar on each of the 22 tensors; returns the worst ratio err / max|ref|."""
    worst, worst_name, bad = 0.0, "", []
    for i, (name, g, r) in enumerate(zip(NAMES, got, ref)):
        assert g.shape == r.shape, name
        if norm == "instance" and name.endswith("bias") and i < 20:
            # the bias cancels in the mean subtraction: exact zero (the reference: ~1e-15 noise)
            assert not g.any(), name + ": must be exact zero"
            continue
        err, scale = float((g.double() - r).abs().max()), float(r.abs().max())
        ratio = err / scale
        if ratio > worst:
            worst, worst_name = ratio, name
        if not err <= 1e-5 * scale:
            bad.append((name, ratio))
    print(f"PARITY grad {norm} {label} worst err/max|ref| = {worst:.3e} ({worst_name}) (bar 1e-5)")
    assert not bad, bad
    return worst


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradients_match_autograd_of_the_restatement(gpu, shape, norm, out_dim):
    img, cot, ref_out, ref = case(gpu, shape, norm, out_dim)
    enc = make(norm, out_dim, gpu)
    out, got, _ = run_ext(enc, img[0], cot.float())
    assert float((out.double() - ref_out).abs().max()) <= 1e-5 * float(ref_out.abs().max())
    check_grads(got, ref, norm, shape)


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_training_forward_equals_inference_forward(gpu, norm, out_dim):
    from dpvo_amd import extractor

    img = images((2, 30, 46), gpu)
    enc = make(norm, out_dim, gpu)
    e = extractor.ext()
    for cl in (False, True):
        fmt = torch.channels_last if cl else torch.contiguous_format
        inf = torch.full((2, out_dim, 8, 12), float("nan"), device=gpu).contiguous(memory_format=fmt)
        e.forward(enc.packed(gpu), e.F32, enc._ncode(), img[0].contiguous(), inf,
                  enc.workspace(2, 30, 46, gpu))
        out, _, _ = run_ext(enc, img[0], channels_last=cl)
        assert out.is_contiguous(memory_format=fmt)
        assert torch.equal(out, inf)
        # the module: grad mode against no_grad
        a = enc(img, channels_last=cl)
        with torch.no_grad():
            b = enc(img, channels_last=cl)
        assert a.grad_fn is not None and a.requires_grad and b.grad_fn is None
        assert a.shape == b.shape == (1, 2, out_dim, 8, 12) and a.stride() == b.stride()
        assert torch.equal(a.detach(), b) and torch.equal(b[0], inf)


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_cotangent_layouts_and_repeats_are_bit_identical(gpu, norm, out_dim):
    img, cot, _, _ = case(gpu, (2, 30, 46), norm, out_dim)
    enc = make(norm, out_dim, gpu)
    c = cot.float().contiguous()
    _, a, st = run_ext(enc, img[0], c)
    _, b, _ = run_ext(enc, img[0], c, state=st)  # the same saved state again
    ccl = c.contiguous(memory_format=torch.channels_last)
    assert not ccl.is_contiguous()
    _, d, _ = run_ext(enc, img[0], ccl, state=st)
    for name, x, y, z in zip(NAMES, a, b, d):
        assert torch.equal(x, y), name + ": two calls differ"
        assert torch.equal(x, z), name + ": channels-last cotangent differs"
    # through autograd: contiguous, channels-last strides and a non-contiguous slice
    wide = torch.zeros(1, 2, out_dim, 8, 13, device=gpu)
    wide[..., :12] = c
    sliced = wide[..., :12]
    assert not sliced.is_contiguous()
    for cv in (c.view(1, 2, out_dim, 8, 12), ccl.view(1, 2, out_dim, 8, 12), sliced):
        enc.zero_grad(set_to_none=True)
        enc(img).backward(cv)
        for name, p, x in zip(NAMES, enc.parameters(), a):
            assert torch.equal(p.grad, x), name


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_autograd_plumbing(gpu, norm, out_dim):
    from dpvo_amd.extractor import BasicEncoder4

    img, cot, _, _ = case(gpu, (1, 16, 16), norm, out_dim)
    c = cot.float().view(1, 1, out_dim, 4, 4)
    enc = make(norm, out_dim, gpu)
    (enc(img) * c).sum().backward()
    first = [p.grad.clone() for p in enc.parameters()]
    (enc(img) * c).sum().backward()
    for name, p, g in zip(NAMES, enc.parameters(), first):
        assert torch.equal(p.grad, 2 * g), name + ": .grad must accumulate"
    # one optimiser step writes every parameter in place; the next forward sees it
    before = [p.detach().clone() for p in enc.parameters()]
    torch.optim.SGD(enc.parameters(), lr=1e-3).step()
    assert any(not torch.equal(p.detach(), q) for p, q in zip(enc.parameters(), before))
    out = enc(img)
    P = {k: p.detach().double() for k, p in zip(NAMES, enc.parameters())}
    ref = encoder_ref.encoder_ref(P, img[0].double(), norm)
    assert float((out[0].detach().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    old = encoder_ref.encoder_ref({k: q.double() for k, q in zip(NAMES, before)}, img[0].double(), norm)
    assert float((ref - old).abs().max()) > 1e-4 * float(ref.abs().max())  # the step moved the output
    # refusals
    with pytest.raises(ValueError):
        enc(img.clone().requires_grad_())
    with pytest.raises(ValueError):
        BasicEncoder4(out_dim, norm, torch.float16, differentiable=True)
    with torch.no_grad():
        o = enc(img)
    assert o.grad_fn is None and not o.requires_grad
    plain = make(norm, out_dim, gpu, differentiable=False)
    assert plain(img).grad_fn is None  # the default stays inference only


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_no_host_synchronisation(gpu, norm, out_dim):
    img, cot, _, _ = case(gpu, (1, 16, 16), norm, out_dim)
    c = cot.float().view(1, 1, out_dim, 4, 4)
    enc = make(norm, out_dim, gpu)
    enc(img).backward(c)  # warm-up: library load
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        enc(img).backward(c)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.isfinite(p.grad).all() for p in enc.parameters())


@pytest.mark.parametrize("wname", ["F32", "F16"])
@pytest.mark.parametrize("norm,out_dim", [("instance", 64), ("none", 64), ("instance", 384),
                                          ("none", 384)])
def test_device_pack_equals_host_pack(gpu, norm, out_dim, wname):
    from dpvo_amd import extractor

    e = extractor.ext()
    wd = getattr(e, wname)
    nc = e.NORM_INSTANCE if norm == "instance" else e.NORM_NONE
    P = encoder_ref.formula_params(out_dim, norm)
    host = [torch.as_tensor(P[n]) for n, _ in encoder_ref.param_shapes(out_dim)]
    host[2].view(-1)[:5] = torch.tensor([0.0, 1e-9, -3e-6, 65519.9, -1e6])  # zero, subnormal halves, overflow
    want = e.pack_weights(host, out_dim, nc, wd).to(gpu)
    blob = torch.full((e.packed_bytes(out_dim, wd),), 0xAB, dtype=torch.uint8, device=gpu)
    e.pack_weights_device([t.to(gpu) for t in host], out_dim, nc, wd, blob)
    assert torch.equal(blob, want)


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_constant_image_gives_finite_gradients(gpu, norm, out_dim):
    enc = make(norm, out_dim, gpu)
    img = torch.full((1, 3, 30, 46), 0.25, device=gpu)
    cot = cotangent((1, out_dim, 8, 12), gpu).float()
    run_ext(enc, img, cot)  # asserts finiteness (ill-conditioned by construction)


def test_patchifier_gradients(gpu):
    from dpvo_amd.net import Patchifier

    n, H, W, M = 1, 38, 54, 7
    h, w = 10, 14
    pf = Patchifier(dtype=torch.float32, differentiable=True)
    Pf, Pi = encoder_ref.formula_params(128, "instance"), encoder_ref.formula_params(384, "none")
    pf.fnet.load_state_dict({k: torch.as_tensor(v) for k, v in Pf.items()})
    pf.inet.load_state_dict({k: torch.as_tensor(v) for k, v in Pi.items()})
    pf = pf.to(gpu)
    img = images((n, H, W), gpu)
    coords = torch.tensor([[[1, 1], [w - 2, h - 2], [1, h - 2], [w - 2, 1], [5, 4], [6, 4], [9, 7]]],
                          dtype=torch.float32, device=gpu)
    hashw = lambda shape, salt: torch.as_tensor(
        encoder_ref._hash01(np.arange(int(np.prod(shape)), dtype=np.float64), salt).reshape(shape),
        device=gpu)
    wf, wg, wi = hashw((1, n, 128, h, w), 11.0), hashw((1, n * M, 128, 3, 3), 12.0), \
        hashw((1, n * M, 384, 1, 1), 13.0)
    fmap, gmap, imap, patches, index = pf(img, coords=coords)
    assert fmap.requires_grad and gmap.requires_grad and imap.requires_grad
    assert not patches.requires_grad
    ((fmap * wf.float()).sum() + (gmap * wg.float()).sum() + (imap * wi.float()).sum()).backward()
    # the same loss through the restatement
    Rf = {k: v.requires_grad_() for k, v in encoder_ref.to_torch(Pf, gpu).items()}
    Ri = {k: v.requires_grad_() for k, v in encoder_ref.to_torch(Pi, gpu).items()}
    fref = encoder_ref.encoder_ref(Rf, img[0].double(), "instance")
    iref = encoder_ref.encoder_ref(Ri, img[0].double(), "none")
    gref = encoder_ref.gather_ref(fref, coords.double(), 1).reshape(1, n * M, 128, 3, 3)
    imref = encoder_ref.gather_ref(iref, coords.double(), 0).reshape(1, n * M, 384, 1, 1)
    loss = (fref[None] * wf).sum() + (gref * wg).sum() + (imref * wi).sum()
    ref = torch.autograd.grad(loss, [Rf[k] for k in NAMES] + [Ri[k] for k in NAMES])
    check_grads([p.grad for p in pf.fnet.parameters()], ref[:22], "instance", "patchifier fnet")
    check_grads([p.grad for p in pf.inet.parameters()], ref[22:], "none", "patchifier inet")
    # without the flag nothing changes: no graph
    plain = Patchifier(dtype=torch.float32).to(gpu)
    assert all(not t.requires_grad for t in plain(img, coords=coords)[:3])
