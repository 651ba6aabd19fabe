#!/usr/bin/env python3
"""Regenerate tests/golden/update_fork_a.npz from the reference's own Update.

    python scripts/make_update_golden.py --reference /path/to/DPVO

CPU only (never on the GPU box).  Imports the reference's ``dpvo.net`` with
empty stand-ins for its native / optional modules (torch_scatter, cuda_ba,
cuda_corr, lietorch_backends: none of them is touched by Update.forward),
loads tests/update_ref.formula_params into ``Update(3).double()`` and runs it
at E = 48 on a DPVO-shaped graph.  Every softmax logit is asserted to have
|g| < 50, so the fork's clamp (net.py:692) is inert and the fixture equals the
max-subtracted softmax.  Stored: ii, jj, kk, neighbors_tensor's ix / jx,
fp32-representable net / inp / corr, fp64 net_out / d / w.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import update_ref  # noqa: E402

E, K0 = 48, 882


class _Stub(types.ModuleType):
    """Any attribute exists and is None: enough for `from m import f` and
    `g = m.f` at import time; calling one would fail loudly."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def import_reference_net(path):
    for name in ("torch_scatter", "cuda_ba", "cuda_corr", "lietorch_backends"):
        if name not in sys.modules:
            sys.modules[name] = _Stub(name)
    sys.path.insert(0, path)
    import dpvo.net as net

    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference DPVO")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "update_fork_a.npz"))
    a = ap.parse_args()
    net_mod = import_reference_net(a.reference)
    torch.manual_seed(0)
    upd = net_mod.Update(3).double().eval()
    P = update_ref.formula_params(K0)
    missing = upd.load_state_dict({k: torch.as_tensor(v, dtype=torch.float64) for k, v in P.items()})
    assert not missing.missing_keys and not missing.unexpected_keys, missing

    logits = []
    for agg in (upd.agg_kk, upd.agg_ij):
        agg.g.register_forward_hook(lambda m, i, o: logits.append(float(o.abs().max())))

    ii, jj, kk = update_ref.dpvo_graph(E, M=4, seed=3)
    net, inp, corr = update_ref.inputs(E, K0, seed=3)
    ix, jx = net_mod.neighbors_tensor(torch.as_tensor(kk), torch.as_tensor(jj))
    t = lambda x: torch.as_tensor(x, dtype=torch.float64)[None]
    with torch.no_grad():
        net_out, (d, w, _) = upd(t(net), t(inp), t(corr), None, torch.as_tensor(ii),
                                 torch.as_tensor(jj), torch.as_tensor(kk))
    assert len(logits) == 2 and max(logits) < 50.0, logits
    print("max |g| logits:", logits)
    np.savez_compressed(a.out, ii=ii, jj=jj, kk=kk, ix=ix.numpy().astype(np.int64),
                        jx=jx.numpy().astype(np.int64), net=net, inp=inp, corr=corr,
                        net_out=net_out[0].numpy(), d=d[0].numpy(), w=w[0].numpy())
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
