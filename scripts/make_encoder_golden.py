#!/usr/bin/env python3
"""Regenerate tests/golden/encoder_a.npz from the reference's own BasicEncoder4.

    python scripts/make_encoder_golden.py --reference /path/to/DPVO

CPU only.  Loads the reference's ``dpvo/extractor.py`` by file path (it
imports only torch), loads tests/encoder_ref.formula_params into
``BasicEncoder4(...).double()`` and runs fnet (128, 'instance') on a
[1, 2, 3, 30, 46] image pair and inet (384, 'none') on a [1, 1, 3, 30, 46]
image.  Stored: the state-dict key names, the fp32-representable images and
the fp64 outputs of the reference modules (before Patchifier's / 4).
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import encoder_ref  # noqa: E402

H, W = 30, 46


def load_extractor(path):
    spec = importlib.util.spec_from_file_location("reference_extractor",
                                                  os.path.join(path, "dpvo", "extractor.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(mod, out_dim, norm, images):
    torch.manual_seed(0)
    enc = mod.BasicEncoder4(output_dim=out_dim, norm_fn=norm).double().eval()
    P = encoder_ref.formula_params(out_dim, norm)
    res = enc.load_state_dict({k: torch.as_tensor(v, dtype=torch.float64) for k, v in P.items()})
    assert not res.missing_keys and not res.unexpected_keys, res
    with torch.no_grad():
        out = enc(torch.as_tensor(images, dtype=torch.float64))
    return list(enc.state_dict().keys()), out.numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference DPVO")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "encoder_a.npz"))
    a = ap.parse_args()
    mod = load_extractor(a.reference)
    rng = np.random.RandomState(7)
    img_f = rng.uniform(-1, 1, (1, 2, 3, H, W)).astype(np.float32)
    img_i = rng.uniform(-1, 1, (1, 1, 3, H, W)).astype(np.float32)
    keys_f, out_f = run(mod, 128, "instance", img_f)
    keys_i, out_i = run(mod, 384, "none", img_i)
    assert keys_f == keys_i
    np.savez_compressed(a.out, keys=np.array(keys_f), fnet_images=img_f, fnet_out=out_f,
                        inet_images=img_i, inet_out=out_i)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
