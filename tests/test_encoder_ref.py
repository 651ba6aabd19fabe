"""CPU: the fp64 restatement of the feature encoder (tests/encoder_ref.py)
reproduces the fixture that scripts/make_encoder_golden.py recorded from the
reference's own BasicEncoder4 (fnet: 128, 'instance'; inet: 384, 'none'), and
the project's module has the reference's parameter names."""
import numpy as np
import pytest
import torch

from conftest import golden
import encoder_ref


@pytest.fixture(scope="module")
def g():
    return golden("encoder_a")


@pytest.mark.parametrize("which,out_dim,norm,n", [("fnet", 128, "instance", 2),
                                                   ("inet", 384, "none", 1)])
def test_restatement_reproduces_reference(g, which, out_dim, norm, n):
    img, want = g[which + "_images"], g[which + "_out"]
    assert img.dtype == np.float32 and img.shape == (1, n, 3, 30, 46)
    assert want.dtype == np.float64 and want.shape == (1, n, out_dim, 8, 12)
    P = encoder_ref.to_torch(encoder_ref.formula_params(out_dim, norm))
    got = encoder_ref.encoder_ref(P, torch.as_tensor(img[0], dtype=torch.float64), norm)
    ref = want[0] / 4.0  # the restatement includes Patchifier's / 4
    err = np.abs(got.numpy() - ref).max()
    print(which, "max|ref|", np.abs(ref).max(), "err", err)
    assert err <= 1e-12 * np.abs(ref).max()


def test_module_has_the_reference_parameter_names(g):
    from dpvo_amd.extractor import BasicEncoder4

    keys = [str(k) for k in g["keys"]]
    assert len(keys) == 22
    assert list(BasicEncoder4().state_dict().keys()) == keys
    assert list(BasicEncoder4(384, "none", torch.float32).state_dict().keys()) == keys
    assert keys == [n for n, _ in encoder_ref.param_shapes(128)]
    enc = BasicEncoder4(384, "none")
    for (name, shape), (k, v) in zip(encoder_ref.param_shapes(384), enc.state_dict().items()):
        assert name == k and tuple(v.shape) == shape and v.dtype == torch.float32


def test_module_rejects_other_norms_and_dtypes():
    from dpvo_amd.extractor import BasicEncoder4

    for bad in ("batch", "group", None):
        with pytest.raises(ValueError):
            BasicEncoder4(128, bad)
    with pytest.raises(ValueError):
        BasicEncoder4(128, "instance", torch.bfloat16)
    with pytest.raises(ValueError):
        BasicEncoder4(100, "instance")


def test_package_exports_the_classes():
    import dpvo_amd
    from dpvo_amd.extractor import BasicEncoder4
    from dpvo_amd.net import Patchifier

    assert dpvo_amd.BasicEncoder4 is BasicEncoder4 and dpvo_amd.Patchifier is Patchifier
    p = Patchifier()
    assert p.fnet.norm_fn == "instance" and p.fnet.output_dim == 128
    assert p.inet.norm_fn == "none" and p.inet.output_dim == 384
    ref = {"fnet." + k for k, _ in encoder_ref.param_shapes(128)}
    ref |= {"inet." + k for k, _ in encoder_ref.param_shapes(384)}
    assert set(p.state_dict().keys()) == ref


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (9, 11), (30, 46), (38, 54), (37, 53), (480, 752)])
def test_output_size_rule_at_odd_sizes(H, W):
    from dpvo_amd.extractor import out_size

    P = encoder_ref.to_torch(encoder_ref.formula_params(64, "none"))
    if H * W <= 64 * 64:
        out = encoder_ref.encoder_ref(P, torch.zeros(1, 3, H, W, dtype=torch.float64), "none")
        assert out.shape == (1, 64, out_size(out_size(H)), out_size(out_size(W)))
    assert encoder_ref.out_size(H) == out_size(H) == -(-H // 2)
    assert out_size(out_size(H)) == -(-H // 4) and out_size(out_size(W)) == -(-W // 4)


def test_formula_params_are_deterministic_and_scaled():
    a, b = encoder_ref.formula_params(128, "instance"), encoder_ref.formula_params(128, "instance")
    assert list(a) == [n for n, _ in encoder_ref.param_shapes(128)] and len(a) == 22
    for k in a:
        assert np.array_equal(a[k], b[k])
        if k.endswith("bias"):
            assert np.abs(a[k]).min() > 0 and 0.05 < a[k].astype(np.float64).std() < 0.15
    W = a["layer2.1.conv1.weight"].astype(np.float64)
    assert abs(W.std() / np.sqrt(2.0 / 576) - 1.0) < 0.05 and abs(W.mean()) < 0.01
    c = encoder_ref.formula_params(128, "none")
    assert not np.array_equal(a["conv1.weight"], c["conv1.weight"])


@pytest.mark.parametrize("norm", ["instance", "none"])
def test_f16_operand_mode_only_rounds_conv_operands(norm):
    P = encoder_ref.to_torch(encoder_ref.formula_params(128, norm))
    img = torch.as_tensor(np.random.RandomState(0).uniform(-1, 1, (1, 3, 30, 46)))
    ref = encoder_ref.encoder_ref(P, img, norm)
    emu = encoder_ref.encoder_ref(P, img, norm, f16_operand=True)
    rel = float((emu - ref).abs().max() / ref.abs().max())
    assert 1e-5 < rel < 5e-3, rel  # fp16 operand rounding, not fp64 noise


def test_gathers_restated():
    n, h, w = 2, 5, 7
    fmap = torch.arange(n * 4 * h * w, dtype=torch.float64).view(n, 4, h, w)
    coords = torch.tensor([[[1, 1], [5, 3]], [[2, 2], [3, 1]]], dtype=torch.float64)
    out = encoder_ref.gather_ref(fmap, coords, 1)
    assert out.shape == (n, 2, 4, 3, 3)
    assert out[0, 1, 2, 0, 0] == fmap[0, 2, 2, 4] and out[1, 1, 3, 2, 2] == fmap[1, 3, 2, 4]
    assert torch.equal(encoder_ref.gather_ref(fmap, coords, 0)[1, 0, :, 0, 0], fmap[1, :, 2, 2])
