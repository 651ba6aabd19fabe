"""GPU: the HIP feature encoders (csrc/encoder.hip, dpvo_amd.extractor) and
dpvo_amd.net.Patchifier against the fp64 restatement (tests/encoder_ref.py)
run on the same device.

Bars: fp32 weights max|got - ref| <= 1e-5 max|ref|; fp16 weights at most 4 x
the error of the restatement's f16_operand mode on the same inputs.  Every
output is pre-filled with NaN by the test (through the extension's `out`
argument) and must be finite afterwards.
"""
import numpy as np
import pytest
import torch

from conftest import golden
import encoder_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9, 11), (1, 16, 16), (2, 30, 46), (1, 38, 54), (1, 96, 128)]
KINDS = [("instance", 128), ("none", 384)]


def make(norm, out_dim, dtype, dev):
    from dpvo_amd.extractor import BasicEncoder4

    enc = BasicEncoder4(out_dim, norm, dtype)
    P = encoder_ref.formula_params(out_dim, norm)
    enc.load_state_dict({k: torch.as_tensor(v) for k, v in P.items()})
    return enc.to(dev)


def run_nan_filled(enc, images, channels_last=False):
    """enc.forward with the output tensor pre-filled with NaN."""
    from dpvo_amd import extractor

    b, n, _, H, W = images.shape
    dev = images.device
    h, w = extractor.out_size(extractor.out_size(H)), extractor.out_size(extractor.out_size(W))
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    out = torch.full((b * n, enc.output_dim, h, w), float("nan"), dtype=torch.float32,
                     device=dev).contiguous(memory_format=fmt)
    extractor.ext().forward(enc.packed(dev), enc._wcode(), enc._ncode(),
                            images.reshape(b * n, 3, H, W).contiguous(), out,
                            enc.workspace(b * n, H, W, dev))
    assert torch.isfinite(out).all()
    return out


_cache = {}


def case(gpu, shape, norm, out_dim):
    """Seeded U(-1, 1) images, the fp64 reference and the error of the
    f16_operand restatement: computed once per (shape, norm), never modified."""
    key = (shape, norm)
    if key not in _cache:
        n, H, W = shape
        rng = np.random.RandomState(1000 + H * 7 + W)
        img = torch.as_tensor(rng.uniform(-1, 1, (1, n, 3, H, W)).astype(np.float32), device=gpu)
        P = encoder_ref.to_torch(encoder_ref.formula_params(out_dim, norm), gpu)
        ref = encoder_ref.encoder_ref(P, img[0].double(), norm)
        emu = encoder_ref.encoder_ref(P, img[0].double(), norm, f16_operand=True)
        _cache[key] = (img, ref, float((emu - ref).abs().max()))
    return _cache[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["w32", "w16"])
@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_encoder_matches_restatement(gpu, shape, norm, out_dim, dtype):
    img, ref, emu_err = case(gpu, shape, norm, out_dim)
    enc = make(norm, out_dim, dtype, gpu)
    got = run_nan_filled(enc, img)
    assert got.shape == ref.shape
    err = float((got.double() - ref).abs().max())
    scale = float(ref.abs().max())
    if dtype == torch.float32:
        print(f"PARITY {norm} {shape} w32 err/max|ref| = {err / scale:.3e} (bar 1e-5)")
        assert err <= 1e-5 * scale
    else:
        print(f"PARITY {norm} {shape} w16 err/max|ref| = {err / scale:.3e} "
              f"emu = {emu_err / scale:.3e} ratio = {err / emu_err:.3f} (bar 4)")
        assert err <= 4.0 * emu_err


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["w32", "w16"])
@pytest.mark.parametrize("which,norm,out_dim", [("fnet", "instance", 128), ("inet", "none", 384)])
def test_fixture_from_the_reference(gpu, which, norm, out_dim, dtype):
    g = golden("encoder_a")
    img = torch.as_tensor(g[which + "_images"], device=gpu)
    ref = torch.as_tensor(g[which + "_out"][0] / 4.0, device=gpu)
    enc = make(norm, out_dim, dtype, gpu)
    got = run_nan_filled(enc, img).double()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"PARITY fixture {which} {dtype} err/max|ref| = {err / scale:.3e}")
    if dtype == torch.float32:
        assert err <= 1e-5 * scale
    else:
        P = encoder_ref.to_torch(encoder_ref.formula_params(out_dim, norm), gpu)
        emu = encoder_ref.encoder_ref(P, img[0].double(), norm, f16_operand=True)
        assert err <= 4.0 * float((emu - ref).abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["w32", "w16"])
@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_layouts_and_repeats_are_bit_identical(gpu, norm, out_dim, dtype):
    img, _, _ = case(gpu, (2, 30, 46), norm, out_dim)
    enc = make(norm, out_dim, dtype, gpu)
    a = run_nan_filled(enc, img)
    b = run_nan_filled(enc, img)
    c = run_nan_filled(enc, img, channels_last=True)
    assert c.is_contiguous(memory_format=torch.channels_last) and not c.is_contiguous()
    assert torch.equal(a, b)
    assert torch.equal(a, c)
    # the module's own forward: same values, [b, n, C, h, w], channels-last strides on request
    d = enc(img)
    e = enc(img, channels_last=True)
    assert d.shape == (1, 2, out_dim, 8, 12) and d.is_contiguous()
    assert e.shape == d.shape and e.stride()[2] == 1
    assert torch.equal(d[0], a) and torch.equal(e, d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["w32", "w16"])
@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_constant_image_is_finite(gpu, norm, out_dim, dtype):
    enc = make(norm, out_dim, dtype, gpu)
    img = torch.full((1, 1, 3, 30, 46), 0.25, device=gpu)
    run_nan_filled(enc, img)  # asserts finiteness (ill-conditioned by construction)


def test_patchifier_with_given_centres(gpu):
    from dpvo_amd.net import Patchifier

    n, H, W, M = 1, 38, 54, 7
    h, w = 10, 14
    pf = Patchifier(dtype=torch.float32)
    Pf, Pi = encoder_ref.formula_params(128, "instance"), encoder_ref.formula_params(384, "none")
    pf.fnet.load_state_dict({k: torch.as_tensor(v) for k, v in Pf.items()})
    pf.inet.load_state_dict({k: torch.as_tensor(v) for k, v in Pi.items()})
    pf = pf.to(gpu)
    img, fref, _ = case(gpu, (n, H, W), "instance", 128)
    _, iref, _ = case(gpu, (n, H, W), "none", 384)
    coords = torch.tensor([[[1, 1], [w - 2, h - 2], [1, h - 2], [w - 2, 1], [5, 4], [6, 4], [9, 7]]],
                          dtype=torch.float32, device=gpu)
    assert coords.shape == (n, M, 2)
    disps = torch.as_tensor(np.random.RandomState(3).uniform(0.1, 2.0, (1, n, h, w)).astype(np.float32),
                            device=gpu)
    for dsp in (None, disps):
        fmap, gmap, imap, patches, index, clr = pf(img, disps=dsp, return_color=True, coords=coords)
        want = encoder_ref.patchifier_ref(fref, iref, img[0].double(), coords.double(),
                                          None if dsp is None else dsp[0].double())
        gref, imref, pref, xref, cref = want
        assert fmap.shape == (1, n, 128, h, w) and gmap.shape == (1, n * M, 128, 3, 3)
        assert imap.shape == (1, n * M, 384, 1, 1) and patches.shape == (1, n * M, 3, 3, 3)
        assert clr.shape == (1, n * M, 3) and index.shape == (n * M,)
        assert float((fmap[0].double() - fref).abs().max()) <= 1e-5 * float(fref.abs().max())
        assert float((gmap.double() - gref).abs().max()) <= 1e-5 * float(fref.abs().max())
        assert float((imap.double() - imref).abs().max()) <= 1e-5 * float(iref.abs().max())
        assert torch.equal(patches.double(), pref)  # coordinates and fp32 disparities: exact
        assert torch.equal(index, xref) and index.dtype == torch.int64
        assert torch.equal(clr.double(), cref)


@pytest.mark.parametrize("strat", ["RANDOM", "GRADIENT_BIAS"])
def test_patchifier_draws_centres_inside_the_map(gpu, strat):
    from dpvo_amd.net import Patchifier

    torch.manual_seed(5)
    n, H, W, M = 2, 30, 46, 9
    h, w = 8, 12
    pf = Patchifier().to(gpu)
    img, _, _ = case(gpu, (n, H, W), "instance", 128)
    fmap, gmap, imap, patches, index = pf(img, patches_per_image=M, centroid_sel_strat=strat)
    assert fmap.shape == (1, n, 128, h, w) and gmap.shape == (1, n * M, 128, 3, 3)
    assert imap.shape == (1, n * M, 384, 1, 1) and patches.shape == (1, n * M, 3, 3, 3)
    assert torch.equal(index.cpu(), torch.arange(n).repeat_interleave(M))
    x, y = patches[0, :, 0, 1, 1], patches[0, :, 1, 1, 1]
    assert torch.equal(x, x.round()) and torch.equal(y, y.round())
    assert x.min() >= 1 and x.max() <= w - 2 and y.min() >= 1 and y.max() <= h - 2
    assert torch.equal(patches[0, :, 2], torch.ones(n * M, 3, 3, device=gpu))
    coords = torch.stack([x, y], dim=-1).view(n, M, 2)
    want = encoder_ref.gather_ref(fmap[0], coords, 1).view(1, n * M, 128, 3, 3)
    assert torch.isfinite(gmap).all() and torch.equal(gmap, want)
    with pytest.raises(NotImplementedError):
        pf(img, centroid_sel_strat="GRID")


def test_load_state_dict_and_repack_after_a_parameter_write(gpu):
    from dpvo_amd.extractor import BasicEncoder4
    from dpvo_amd.net import Patchifier

    img, ref, _ = case(gpu, (1, 16, 16), "instance", 128)
    # a checkpoint-shaped dict with the reference's names
    P = encoder_ref.formula_params(128, "instance")
    ckpt = {"fnet." + k: torch.as_tensor(v) for k, v in P.items()}
    ckpt.update({"inet." + k: torch.as_tensor(v)
                 for k, v in encoder_ref.formula_params(384, "none").items()})
    pf = Patchifier(dtype=torch.float32)
    res = pf.load_state_dict(ckpt)
    assert not res.missing_keys and not res.unexpected_keys
    enc = pf.fnet.to(gpu)
    a = enc(img)
    assert float((a[0].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    blob = enc.packed(gpu)
    assert enc.packed(gpu) is blob  # cached
    with torch.no_grad():
        enc.conv2.bias.add_(1.0)
    b = enc(img)
    assert enc.packed(gpu) is not blob
    # out = conv2(x) / 4: the bias moves every output by 0.25
    assert float((b - a - 0.25).abs().max()) <= 1e-5
    clone = BasicEncoder4.from_reference(enc, dtype=torch.float32).to(gpu)
    assert clone.norm_fn == "instance" and clone.output_dim == 128
    assert torch.equal(clone(img), b)


@pytest.mark.parametrize("norm,out_dim", KINDS, ids=["fnet", "inet"])
def test_graph_capture_replays_bit_identically(gpu, norm, out_dim):
    img, _, _ = case(gpu, (2, 30, 46), norm, out_dim)
    enc = make(norm, out_dim, torch.float16, gpu)
    eager = enc(img).clone()
    static_in = img.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(static_in)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = enc(static_in)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    # a second image through the same graph
    img2 = (-img).contiguous()
    static_in.copy_(img2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, enc(img2))
