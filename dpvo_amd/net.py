"""DPVO's update operator (dpvo/net.py:175-339), patchifier (net.py:344-407),
CorrBlock (410-423) and VONet with its training unroll (426-522) on the MI355X.

``Update`` has the reference module's parameter names, so a DPVO checkpoint's
``update.*`` keys load unchanged, and the reference's call signature; the
forward pass is the fused HIP operator of csrc/update_op.hip, and with
``differentiable=True`` its backward is csrc/update_bwd.hip.
The parameters stay fp32 tensors; ``dtype`` chooses how they are packed for
the matrix cores: ``torch.float16`` (fp16 operands, fp32 accumulation) or
``torch.float32`` (exact fp32 products).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ._native import load_extension, require_gpu

DIM = 384

_ext = None


def ext():
    global _ext
    if _ext is None:
        _ext = load_extension("dpvo_update")
    return _ext


class _GatedResidual(nn.Module):  # blocks.py:15-29 (parameters only)
    def __init__(self, dim):
        super().__init__()
        self.gate = nn.Sequential(nn.Linear(dim, dim), nn.Sigmoid())
        self.res = nn.Sequential(nn.Linear(dim, dim), nn.ReLU(inplace=True), nn.Linear(dim, dim))


class _SoftAgg(nn.Module):  # blocks.py:31-38 / net.py:671-676 (parameters only)
    def __init__(self, dim):
        super().__init__()
        self.f = nn.Linear(dim, dim)
        self.g = nn.Linear(dim, dim)
        self.h = nn.Linear(dim, dim)


def _mlp(i, o):
    return nn.Sequential(nn.Linear(i, o), nn.ReLU(inplace=True), nn.Linear(o, o))


class _UpdateFunction(torch.autograd.Function):
    """forward_train + backward of the update operator.  Inputs: the module, the
    index tensors (ix, jx, gk, gij: int64 [E], no gradient), net, inp [E, 384],
    corr [E, K0] (contiguous fp32) and the 50 parameters.  The blob is packed
    on the device from the parameters' current values and ``saved`` is
    allocated per call, so neither an optimiser step nor further forward calls
    before the backward disturb it.  Once-differentiable; no host
    synchronisation in either direction."""

    @staticmethod
    def forward(ctx, mod, ix, jx, gk, gij, net, inp, corr, *params):
        x = ext()
        dev = net.device
        E, K0 = net.shape[0], mod.corr_dim
        ps = [p.detach().contiguous() for p in params]
        blob = torch.empty(x.packed_bytes(K0, x.F32), dtype=torch.uint8, device=dev)
        x.pack_weights_device(ps, K0, x.F32, blob)
        saved = torch.empty(x.saved_bytes(E, K0), dtype=torch.uint8, device=dev)
        net_out = torch.empty(E, DIM, dtype=torch.float32, device=dev)
        d = torch.empty(E, 2, dtype=torch.float32, device=dev)
        w = torch.empty(E, 2, dtype=torch.float32, device=dev)
        ws = mod.workspace(E, dev)
        x.plan(gk, gij, ws)
        x.forward_train(blob, net, inp, corr, ix, jx, ws, saved, net_out, d, w)
        ctx.K0 = K0
        ctx.saved = saved
        ctx.set_materialize_grads(False)  # an unused output's cotangent stays None: no zeros
        ctx.save_for_backward(ix, jx, *params)
        return net_out, d, w

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_net_out, g_d, g_w):
        x = ext()
        ix, jx, *params = ctx.saved_tensors
        E, K0, dev = ix.numel(), ctx.K0, ix.device
        need = ctx.needs_input_grad  # mod, ix, jx, gk, gij, net, inp, corr, params...
        cot = [None if g is None else g.to(torch.float32).contiguous()
               for g in (g_net_out, g_d, g_w)]
        out = [torch.empty(E, c, dtype=torch.float32, device=dev) if need[5 + i] else None
               for i, c in enumerate((DIM, DIM, K0))]
        ps = [p.detach().contiguous() for p in params]
        want = any(need[8:])
        grads = [torch.empty_like(p) for p in ps] if want else []
        ws = torch.empty(x.backward_workspace_bytes(E, K0), dtype=torch.uint8, device=dev)
        x.backward(ps, ctx.saved, ix, jx, K0, cot[0], cot[1], cot[2], out[0], out[1], out[2], grads,
                   ws)
        pg = tuple(g if n else None for g, n in zip(grads, need[8:])) if want \
            else (None,) * len(params)
        return (None,) * 5 + tuple(out) + pg


class Update(nn.Module):
    """Drop-in for ``dpvo.net.Update``.

    forward(net, inp, corr, flow, ii, jj, kk, ix=None, jx=None, gk=None, gij=None)
    -> (net, (d, w, None)), shapes [1, E, .] as in the reference.  ix / jx
    default to ``fastba.neighbors(kk, jj)`` (-1 = missing, masked), gk to kk and
    gij to ``ii * 12345 + jj``: the original DPVO.  For the fork's live Update
    pass ``ix, jx = neighbors_tensor(kk, jj)`` and ``gij=ii``.

    ``differentiable=False`` (default): inference, under ``no_grad``.
    ``differentiable=True`` (``dtype`` must be ``torch.float32``): when grad
    mode is on, net / inp / corr are fp32 and any of them or a parameter
    requires grad, the outputs (the same bits as the inference path) carry
    gradients to net, inp, corr and the 50 parameters, formed by the HIP
    backward for exactly the inputs that need them.  The gradient of
    ``agg_*.g.bias`` is analytically zero; what arrives is rounding noise.
    """

    def __init__(self, p=3, dtype=torch.float16, corr_dim=None, differentiable=False):
        super().__init__()
        if dtype not in (torch.float16, torch.float32):
            raise ValueError("Update: dtype (the packed weight type) is float16 or float32")
        if differentiable and dtype != torch.float32:
            raise ValueError("Update: differentiable=True needs dtype=torch.float32")
        self.differentiable = bool(differentiable)
        self.wdtype = dtype
        self.corr_dim = int(corr_dim) if corr_dim is not None else 2 * 49 * p * p
        self.c1 = _mlp(DIM, DIM)
        self.c2 = _mlp(DIM, DIM)
        self.norm = nn.LayerNorm(DIM, eps=1e-3)
        self.agg_kk = _SoftAgg(DIM)
        self.agg_ij = _SoftAgg(DIM)
        self.gru = nn.Sequential(nn.LayerNorm(DIM, eps=1e-3), _GatedResidual(DIM),
                                 nn.LayerNorm(DIM, eps=1e-3), _GatedResidual(DIM))
        self.corr = nn.Sequential(nn.Linear(self.corr_dim, DIM), nn.ReLU(inplace=True),
                                  nn.Linear(DIM, DIM), nn.LayerNorm(DIM, eps=1e-3),
                                  nn.ReLU(inplace=True), nn.Linear(DIM, DIM))
        self.d = nn.Sequential(nn.ReLU(inplace=False), nn.Linear(DIM, 2), nn.Identity())
        self.w = nn.Sequential(nn.ReLU(inplace=False), nn.Linear(DIM, 2), nn.Identity(),
                               nn.Sigmoid())
        self._blob = None
        self._blob_key = None
        self._ws = None

    @classmethod
    def from_reference(cls, module, dtype=torch.float16):
        """Copy an existing reference ``Update`` (any device / dtype)."""
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in module.state_dict().items()}
        new = cls(dtype=dtype, corr_dim=sd["corr.0.weight"].shape[1])
        new.load_state_dict(sd)
        return new

    # -- packed weights ------------------------------------------------------
    def _wcode(self):
        return ext().F16 if self.wdtype == torch.float16 else ext().F32

    def _key(self, device):
        return (str(device), self.wdtype) + tuple((p.data_ptr(), p._version)
                                                  for p in self.parameters())

    def packed(self, device):
        """The device blob of the packed weights; packed on first use and again
        whenever a parameter was written or replaced."""
        key = self._key(device)
        if self._blob is None or key != self._blob_key:
            tensors = [p.detach().to("cpu", torch.float32).contiguous() for p in self.parameters()]
            if len(tensors) != 50:
                raise RuntimeError("Update: expected 50 parameter tensors")
            host = ext().pack_weights(tensors, self.corr_dim, self._wcode())
            self._blob = host.to(device)
            self._blob_key = key
        return self._blob

    def workspace(self, E, device):
        need = ext().workspace_bytes(E, self.corr_dim)
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def forward(self, net, inp, corr, flow, ii, jj, kk, ix=None, jx=None, gk=None, gij=None):
        train = (self.differentiable and torch.is_grad_enabled()
                 and all(t.dtype == torch.float32 for t in (net, inp, corr))
                 and (any(t.requires_grad for t in (net, inp, corr))
                      or any(p.requires_grad for p in self.parameters())))
        if train:
            return self._forward_train(net, inp, corr, ii, jj, kk, ix, jx, gk, gij)
        with torch.no_grad():
            return self._forward(net, inp, corr, ii, jj, kk, ix, jx, gk, gij)

    def _indices(self, ii, jj, kk, ix, jx, gk, gij):
        ii, jj, kk = (t.reshape(-1).long() for t in (ii, jj, kk))
        if ix is None or jx is None:
            from . import fastba

            ix, jx = fastba.neighbors(kk, jj)
        gk = kk if gk is None else gk
        gij = ii * 12345 + jj if gij is None else gij
        return tuple(t.reshape(-1).long().contiguous() for t in (ix, jx, gk, gij))

    def _forward_train(self, net, inp, corr, ii, jj, kk, ix, jx, gk, gij):
        require_gpu(net)
        if net.dim() != 3 or net.shape[0] != 1 or net.shape[2] != DIM:
            raise ValueError("Update: net must be [1, E, 384]")
        E = net.shape[1]
        if corr.shape[-1] != self.corr_dim:
            raise ValueError(f"Update: corr has {corr.shape[-1]} features, the module "
                             f"{self.corr_dim}")
        if E == 0:
            with torch.no_grad():
                return self._forward(net, inp, corr, ii, jj, kk, ix, jx, gk, gij)
        with torch.no_grad():
            ix, jx, gk, gij = self._indices(ii, jj, kk, ix, jx, gk, gij)
        params = list(self.parameters())
        if len(params) != 50:
            raise RuntimeError("Update: expected 50 parameter tensors")
        net_out, d, w = _UpdateFunction.apply(
            self, ix, jx, gk, gij, net.reshape(E, DIM).contiguous(),
            inp.reshape(E, DIM).contiguous(), corr.reshape(E, self.corr_dim).contiguous(), *params)
        return net_out.view(1, E, DIM), (d.view(1, E, 2), w.view(1, E, 2), None)

    def _forward(self, net, inp, corr, ii, jj, kk, ix=None, jx=None, gk=None, gij=None):
        require_gpu(net)
        if net.dim() != 3 or net.shape[0] != 1 or net.shape[2] != DIM:
            raise ValueError("Update: net must be [1, E, 384]")
        E, dev = net.shape[1], net.device
        if corr.shape[-1] != self.corr_dim:
            raise ValueError(f"Update: corr has {corr.shape[-1]} features, the module "
                             f"{self.corr_dim}")
        ii, jj, kk = (t.reshape(-1).long() for t in (ii, jj, kk))
        if ix is None or jx is None:
            from . import fastba

            ix, jx = fastba.neighbors(kk, jj)
        gk = kk if gk is None else gk
        gij = ii * 12345 + jj if gij is None else gij
        io = net.dtype
        net_out = torch.empty_like(net, memory_format=torch.contiguous_format)
        d = torch.empty(1, E, 2, dtype=torch.float32, device=dev)
        w = torch.empty(1, E, 2, dtype=torch.float32, device=dev)
        if E == 0:
            return net_out, (d, w, None)
        blob, ws = self.packed(dev), self.workspace(E, dev)
        x = ext()
        x.plan(gk.reshape(-1).long(), gij.reshape(-1).long(), ws)
        x.forward(blob, self._wcode(), net.reshape(E, DIM).contiguous(),
                  inp.reshape(E, DIM).to(io).contiguous(),
                  corr.reshape(E, self.corr_dim).to(io).contiguous(), ix.reshape(-1).long(),
                  jx.reshape(-1).long(), ws, net_out.view(E, DIM), d.view(E, 2), w.view(E, 2))
        return net_out, (d, w, None)


class Patchifier(nn.Module):
    """Drop-in for ``dpvo.net.Patchifier`` (net.py:344-407, inference): the two
    HIP encoders and the patch gathers.

    forward(images [b, n, 3, H, W], ...) -> (fmap, gmap, imap, patches, index
    [, clr]) as in the reference.  ``coords`` ([n, M, 2] float, integer-valued
    (x, y) centres at quarter resolution, 1 <= x <= w - 2, 1 <= y <= h - 2)
    replaces the random draw when given.
    """

    def __init__(self, patch_size=3, dtype=torch.float16, differentiable=False):
        super().__init__()
        from .extractor import BasicEncoder4

        self.patch_size = patch_size
        self.differentiable = bool(differentiable)
        self.fnet = BasicEncoder4(output_dim=128, norm_fn="instance", dtype=dtype,
                                  differentiable=differentiable)
        self.inet = BasicEncoder4(output_dim=DIM, norm_fn="none", dtype=dtype,
                                  differentiable=differentiable)

    @staticmethod
    def _image_gradient(images):  # net.py:351-357
        gray = ((images + 0.5) * (255.0 / 2)).sum(dim=2)
        dx = gray[..., :-1, 1:] - gray[..., :-1, :-1]
        dy = gray[..., 1:, :-1] - gray[..., :-1, :-1]
        g = torch.sqrt(dx ** 2 + dy ** 2)
        return torch.nn.functional.avg_pool2d(g, 4, 4)

    def forward(self, images, patches_per_image=80, disps=None, centroid_sel_strat="RANDOM",
                return_color=False, coords=None):
        """With ``differentiable=True`` (and grad mode on) fmap, gmap and imap
        carry gradients to the encoders' parameters; otherwise the whole call
        runs under ``no_grad``."""
        with torch.set_grad_enabled(self.differentiable and torch.is_grad_enabled()):
            return self._forward(images, patches_per_image, disps, centroid_sel_strat,
                                 return_color, coords)

    def _forward(self, images, patches_per_image, disps, centroid_sel_strat, return_color, coords):
        from . import altcorr

        require_gpu(images)
        fmap = self.fnet(images)  # the / 4 of net.py:361-362 is inside the encoders
        imap = self.inet(images)
        b, n, c, h, w = fmap.shape
        dev = images.device
        P = self.patch_size
        if coords is not None:
            coords = coords.to(dev, torch.float32)
            if coords.dim() != 3 or coords.shape[0] != n or coords.shape[2] != 2:
                raise ValueError("Patchifier: coords must be [n, M, 2]")
            patches_per_image = coords.shape[1]
        elif centroid_sel_strat == "GRADIENT_BIAS":  # net.py:369-379
            g = self._image_gradient(images)
            x = torch.randint(1, w - 1, size=[n, 3 * patches_per_image], device=dev)
            y = torch.randint(1, h - 1, size=[n, 3 * patches_per_image], device=dev)
            cand = torch.stack([x, y], dim=-1).float()
            g = altcorr.patchify(g[0, :, None].contiguous(), cand, 0).view(n, 3 * patches_per_image)
            ix = torch.argsort(g, dim=1)
            x = torch.gather(x, 1, ix[:, -patches_per_image:])
            y = torch.gather(y, 1, ix[:, -patches_per_image:])
            coords = torch.stack([x, y], dim=-1).float()
        elif centroid_sel_strat == "RANDOM":
            x = torch.randint(1, w - 1, size=[n, patches_per_image], device=dev)
            y = torch.randint(1, h - 1, size=[n, patches_per_image], device=dev)
            coords = torch.stack([x, y], dim=-1).float()
        else:
            raise NotImplementedError(
                f"Patch centroid selection not implemented: {centroid_sel_strat}")

        imap = altcorr.patchify(imap[0], coords, 0).view(b, -1, DIM, 1, 1)
        gmap = altcorr.patchify(fmap[0], coords, P // 2).view(b, -1, 128, P, P)
        if return_color:
            clr = altcorr.patchify(images[0].float().contiguous(), 4 * (coords + 0.5), 0).view(b, -1, 3)
        if disps is None:
            disps = torch.ones(b, n, h, w, device=dev)
        # (x, y, disps) per pixel: utils.py:39-54
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev),
                                torch.arange(w, dtype=torch.float32, device=dev), indexing="ij")
        grid = torch.stack([xs.expand(b, n, h, w), ys.expand(b, n, h, w),
                            disps.to(dev, torch.float32)], dim=2)
        patches = altcorr.patchify(grid[0].contiguous(), coords, P // 2).view(b, -1, 3, P, P)
        index = torch.arange(n, device=dev).view(n, 1).repeat(1, patches_per_image).reshape(-1)
        if return_color:
            return fmap, gmap, imap, patches, index, clr
        return fmap, gmap, imap, patches, index


class CorrBlock:
    """``dpvo.net.CorrBlock`` (net.py:410-423): the correlation of every edge's
    gmap patch against an ``avg_pool2d`` pyramid of fmap, through
    ``altcorr.corr`` (A-CORR and A-CORR-BWD).  ``dropout`` is the fraction of
    edges whose gradient the backward keeps (correlation.py:31-36; 1 keeps all,
    no random draw)."""

    def __init__(self, fmap, gmap, radius=3, dropout=0.2, levels=(1, 4)):
        self.dropout = dropout
        self.radius = radius
        self.levels = tuple(levels)
        self.gmap = gmap
        b, n, c, h, w = fmap.shape
        self.pyramid = [torch.nn.functional.avg_pool2d(fmap.view(b * n, c, h, w), l, stride=l)
                        .view(b, n, c, h // l, w // l) for l in self.levels]

    def __call__(self, ii, jj, coords):
        from . import altcorr

        corrs = [altcorr.corr(self.gmap, self.pyramid[i], coords / self.levels[i], ii, jj,
                              self.radius, self.dropout) for i in range(len(self.levels))]
        return torch.stack(corrs, -1).view(1, len(ii), -1)


def _schedule(n_frames, patches_per_image, steps, init_frames=8, drop=None):
    """The steps of net.py:458-497 on the host, as dicts of numpy int64 arrays:
    ii / jj / kk / n, ``new`` (edges prepended at this step), ``keep`` (indices
    kept by the 10 % removal, or None) and ``loss`` (indices of the edges with
    0 < |ii - jj| <= 2)."""
    import numpy as np

    if n_frames < init_frames or init_frames < 2 or patches_per_image < 1:
        # a new frame's depth is the median of the two frames before it
        raise ValueError("training_schedule: need 2 <= init_frames <= n_frames, "
                         "patches_per_image >= 1")
    if drop is None:
        def drop(step):
            return np.random.rand() < 0.1
    ix = np.arange(n_frames * patches_per_image, dtype=np.int64) // patches_per_image

    def mesh(a, b):  # flatmeshgrid(a, b, indexing='ij')
        return np.repeat(a, len(b)), np.tile(b, len(a))

    kk, jj = mesh(np.nonzero(ix < init_frames)[0], np.arange(0, init_frames, dtype=np.int64))
    ii = ix[kk]
    out = []
    while len(out) < steps:
        n = int(ii.max()) + 1
        new, keep = 0, None
        if len(out) >= init_frames and n < n_frames:
            kk1, jj1 = mesh(np.nonzero(ix < n)[0], np.arange(n, n + 1, dtype=np.int64))
            kk2, jj2 = mesh(np.nonzero(ix == n)[0], np.arange(0, n + 1, dtype=np.int64))
            ii = np.concatenate([ix[kk1], ix[kk2], ii])
            jj = np.concatenate([jj1, jj2, jj])
            kk = np.concatenate([kk1, kk2, kk])
            new = len(kk1) + len(kk2)
            if drop(len(out)):
                keep = np.nonzero((ii != n - 4) & (jj != n - 4))[0]
                ii, jj, kk = ii[keep], jj[keep], kk[keep]
            n = int(ii.max()) + 1
        dij = np.abs(ii - jj)
        out.append({"ii": ii, "jj": jj, "kk": kk, "n": n, "new": new, "keep": keep,
                    "loss": np.nonzero((dij > 0) & (dij <= 2))[0]})
    return out


def training_schedule(n_frames, patches_per_image, steps, init_frames=8, drop=None):
    """The edge lists ``(ii, jj, kk, n)`` of every unrolled step of
    ``VONet.forward`` (net.py:458-497), built on the host: patch k lies in frame
    ``k // patches_per_image``, so nothing is read from the device.  The graph
    starts on ``init_frames`` (at least 2) frames; from step ``init_frames`` on, each step
    adds one frame until ``n_frames`` are in, its edges prepended in the
    reference's order of ``cat``s.  ``drop`` (``step -> bool``; default: a host
    RNG draw < 0.1 per growth step) decides the removal of every edge that
    touches frame ``n - 4``.  ii / jj / kk are int64 CPU tensors, n an int."""
    return [(torch.from_numpy(s["ii"]), torch.from_numpy(s["jj"]), torch.from_numpy(s["kk"]), s["n"])
            for s in _schedule(n_frames, patches_per_image, steps, init_frames, drop)]


class VONet(nn.Module):
    """``dpvo.net.VONet`` (net.py:426-522) with the reference's attribute
    names, so a DPVO checkpoint's ``patchify.*`` / ``update.*`` keys load
    unchanged.  ``dtype`` is the packed weight type of both modules;
    ``differentiable`` goes to the patchifier's encoders and to the update
    operator (fp32 only) and decides whether ``forward`` builds a graph."""

    def __init__(self, dtype=torch.float16, differentiable=False):
        super().__init__()
        self.P = 3
        self.patchify = Patchifier(self.P, dtype=dtype, differentiable=differentiable)
        self.update = Update(p=self.P, dtype=dtype, differentiable=differentiable)
        self.DIM = DIM
        self.RES = 4
        self.differentiable = bool(differentiable)
        self.wdtype = dtype

    def forward(self, images, poses, disps, intrinsics, M=1024, STEPS=12, P=1,
                structure_only=False, rescale=False, *, patches_per_image=80, init_frames=8,
                coords=None, init_disps=None, edge_drop=0.1, corr_dropout=0.2):
        """The training unroll of net.py:438-522, line for line: images
        [1, N, 3, H, W] in 0..255, poses the ground-truth SE3 [1, N, 7], disps
        [1, N, H, W], intrinsics [1, N, 4] at full resolution -> the list of
        STEPS tuples ``(valid, coords, coords_gt, Gs[:, :n], Ps[:, :n], kl)``.
        M, P and rescale are accepted and unused, as in the reference.

        With ``differentiable=True, dtype=torch.float32`` (and grad mode on)
        the trajectory carries gradients to every parameter tensor (22 per
        encoder, 50 of the update operator): Gs and
        patches are detached at the head of every step, the hidden state
        ``net`` is not.  Otherwise the same values come out under ``no_grad``.
        Batch size 1.  Autocast is off.  All three reprojections per step are
        ``projective_ops.transform_fused``; the edge lists come from
        ``training_schedule`` in one host-to-device copy; ``kl`` is a 0-d
        device zero.

        This build's additions (keyword-only): ``patches_per_image`` (the
        reference's default 80) and ``init_frames`` (the reference's 8);
        ``coords`` [N, patches_per_image, 2], the patch centres instead of the
        random draw; ``init_disps`` [1, N * patches_per_image], the initial
        patch depths instead of ``rand``; ``edge_drop``, the probability of
        the removal of frame n - 4's edges at a growth step (0 never, 1
        always); ``corr_dropout``, ``CorrBlock``'s."""
        grad = (self.differentiable and self.wdtype == torch.float32 and torch.is_grad_enabled())
        with torch.autocast("cuda", enabled=False), torch.set_grad_enabled(grad):
            return self._unroll(images, poses, disps, intrinsics, STEPS, structure_only,
                                patches_per_image, init_frames, coords, init_disps, edge_drop,
                                corr_dropout)

    def _unroll(self, images, poses, disps, intrinsics, STEPS, structure_only, ppi, init_frames,
                centres, init_disps, edge_drop, corr_dropout):
        import numpy as np

        from . import projective_ops as pops
        from .ba import BA
        from .lietorch import SE3

        require_gpu(images)
        if images.dim() != 5 or images.shape[0] != 1:
            raise ValueError("VONet.forward: batch size 1 (images [1, N, 3, H, W])")
        dev = images.device
        images = 2 * (images / 255.0) - 0.5
        intrinsics = intrinsics / 4.0
        disps = disps[:, :, 1::4, 1::4].float()
        if centres is not None:
            ppi = centres.shape[1]

        fmap, gmap, imap, patches, ix = self.patchify(images, patches_per_image=ppi, disps=disps,
                                                      coords=centres)
        corr_fn = CorrBlock(fmap, gmap, dropout=corr_dropout)
        b, N, c, h, w = fmap.shape
        p = self.P

        patches_gt = patches.clone()
        Ps = poses if isinstance(poses, SE3) else SE3(poses)
        d = patches[..., 2, p // 2, p // 2]
        depth = torch.rand_like(d) if init_disps is None else init_disps.to(dev, d.dtype).view(d.shape)
        patches = patches.clone()
        patches[..., 2, :, :] = depth[..., None, None]

        # every step's edge lists, the loss edges and the kept edges of a
        # removal: one pinned buffer, one asynchronous copy
        sched = _schedule(N, ppi, STEPS, init_frames,
                          lambda step: np.random.rand() < edge_drop)
        parts, spans = [], []
        for s in sched:
            arrs = [s["ii"], s["jj"], s["kk"], s["loss"]] + ([] if s["keep"] is None else [s["keep"]])
            spans.append([a.size for a in arrs])
            parts += arrs
        host = torch.from_numpy(np.concatenate(parts) if parts else np.zeros(0, np.int64))
        flat = host.pin_memory().to(dev, non_blocking=True)

        imap = imap.view(b, -1, DIM)
        net = torch.zeros(b, sched[0]["ii"].size if sched else 0, DIM, device=dev,
                          dtype=torch.float32)
        gdata = torch.zeros(1, N, 7, device=dev, dtype=torch.float32)  # SE3.IdentityLike(poses)
        gdata[..., 6] = 1.0
        Gs = SE3(Ps.data.detach().to(torch.float32).clone()) if structure_only else SE3(gdata)
        kl = torch.zeros((), device=dev)

        traj = []
        bounds = [-64, -64, w + 64, h + 64]
        at = 0
        for s, span in zip(sched, spans):
            idx = []
            for m in span:
                idx.append(flat[at:at + m])
                at += m
            ii, jj, kk, lk = idx[:4]
            n = s["n"]
            Gs = Gs.detach()
            patches = patches.detach()
            if s["new"]:
                f = n - 1  # the frame that joins the graph at this step
                if not structure_only:
                    Gs = SE3(Gs.data.clone())
                    Gs.data[:, f] = Gs.data[:, f - 1]
                net = torch.cat([torch.zeros(b, s["new"], DIM, device=dev), net], dim=1)
                if s["keep"] is not None:
                    net = net[:, idx[4]]
                patches = patches.clone()  # the median of the two frames before: a contiguous slice
                patches[:, f * ppi:(f + 1) * ppi, 2] = torch.median(
                    patches[:, (f - 2) * ppi:f * ppi, 2])

            coords, coords1 = pops.transform_fused(Gs, patches, intrinsics, ii, jj, kk,
                                                   corr_layout=True)
            corr = corr_fn(kk, jj, coords1)
            net, (delta, weight, _) = self.update(net, imap[:, kk], corr, None, ii, jj, kk)

            lmbda = 1e-4
            target = coords[..., p // 2, p // 2, :] + delta
            ep = 10
            for itr in range(2):
                Gs, patches = BA(Gs, patches, intrinsics, target, weight, lmbda, ii, jj, kk, bounds,
                                 ep=ep, fixedp=1, structure_only=structure_only, num_poses=n)

            il, jl, kl_ = ii[lk], jj[lk], kk[lk]  # 0 < |ii - jj| <= 2
            coords = pops.transform_fused(Gs, patches, intrinsics, il, jl, kl_)
            coords_gt, valid = pops.transform_fused(Ps, patches_gt, intrinsics, il, jl, kl_,
                                                    valid=True)
            traj.append((valid[..., p // 2, p // 2], coords, coords_gt, Gs[:, :n], Ps[:, :n], kl))
        return traj

    def load_checkpoint(self, path_or_state_dict):
        """Load a DPVO checkpoint (a path for ``torch.load`` or a state dict):
        a leading ``module.`` is stripped and keys containing ``update.lmbda``
        are dropped, as DPVO.load_weights does; strict otherwise."""
        sd = path_or_state_dict
        if not isinstance(sd, dict):
            sd = torch.load(sd, map_location="cpu")
        new = {}
        for k, v in sd.items():
            if "update.lmbda" in k:
                continue
            new[k[len("module."):] if k.startswith("module.") else k] = v
        self.load_state_dict(new, strict=True)
        return self
