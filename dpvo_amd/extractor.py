"""DPVO's feature encoders (dpvo/extractor.py:200-264) on the MI355X.

``BasicEncoder4`` has the reference module's parameter names, so a DPVO
checkpoint's ``patchify.fnet.*`` / ``patchify.inet.*`` keys load unchanged; the
forward pass is the implicit-GEMM HIP encoder of csrc/encoder.hip and already
includes Patchifier's ``/ 4``.  The parameters stay fp32 tensors; ``dtype``
chooses how they are packed for the matrix cores: ``torch.float16`` (fp16
operands, fp32 accumulation) or ``torch.float32`` (exact fp32 products).
With ``differentiable=True`` (fp32 only) the forward keeps its planes and the
HIP backward of csrc/encoder_bwd.hip gives the gradients of the 22 parameters.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ._native import load_extension, require_gpu

DIM = 32

_ext = None


def ext():
    global _ext
    if _ext is None:
        _ext = load_extension("dpvo_encoder")
    return _ext


def out_size(n):
    """Rows (or columns) after one stride-2 stage: (n - 1) // 2 + 1."""
    return (n - 1) // 2 + 1


class _ResidualBlock(nn.Module):  # extractor.py:6-55 (parameters only)
    def __init__(self, in_planes, planes, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        if stride != 1:
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1,
                                                      stride=stride))


class _EncoderFunction(torch.autograd.Function):
    """forward_train + backward of one encoder.  Inputs: the module, the images
    [N, 3, H, W] (contiguous fp32, no gradient), the output memory format and
    the 22 parameters.  The blob is packed on the device from the parameters'
    current values and ``saved`` is allocated per call, so neither an
    optimiser step nor a second forward before the backward disturbs it.  No
    host synchronisation in either direction."""

    @staticmethod
    def forward(ctx, enc, x, fmt, *params):
        e = ext()
        dev = x.device
        N, _, H, W = x.shape
        ps = [p.detach().contiguous() for p in params]
        blob = torch.empty(e.packed_bytes(enc.output_dim, e.F32), dtype=torch.uint8, device=dev)
        e.pack_weights_device(ps, enc.output_dim, enc._ncode(), e.F32, blob)
        need = e.saved_bytes(N, H, W, enc.output_dim, enc._ncode())
        if need <= 0:
            raise ValueError(f"BasicEncoder4: unsupported size {N} x {H} x {W}")
        saved = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(N, enc.output_dim, out_size(out_size(H)), out_size(out_size(W)),
                          dtype=torch.float32, device=dev, memory_format=fmt)
        e.forward_train(blob, e.F32, enc._ncode(), x, out, saved)
        ctx.enc = enc
        ctx.saved = saved
        ctx.save_for_backward(x, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        e = ext()
        enc = ctx.enc
        x, *params = ctx.saved_tensors
        N, _, H, W = x.shape
        if not (grad_out.is_contiguous()
                or grad_out.is_contiguous(memory_format=torch.channels_last)):
            grad_out = grad_out.contiguous()
        ps = [p.detach().contiguous() for p in params]
        grads = [torch.empty_like(p) for p in ps]
        ws = torch.empty(e.backward_workspace_bytes(N, H, W, enc.output_dim), dtype=torch.uint8,
                         device=x.device)
        e.backward(enc._ncode(), ps, x, ctx.saved, grad_out.to(torch.float32), grads, ws)
        return (None, None, None) + tuple(grads)


class BasicEncoder4(nn.Module):
    """Drop-in for ``dpvo.extractor.BasicEncoder4`` with ``norm_fn``
    'instance' or 'none'.

    forward(images [b, n, 3, H, W], channels_last=False) -> [b, n, output_dim,
    h, w] float32, **already divided by 4** (net.py:361-362); with
    ``channels_last`` the same values in channels-last memory.

    ``differentiable=False`` (default): inference, under ``no_grad``.
    ``differentiable=True`` (``dtype`` must be ``torch.float32``): when grad
    mode is on and a parameter requires grad, the output carries gradients to
    the 22 parameters (same values, bit for bit, as the inference path).  The
    images get no gradient (``images.requires_grad`` raises ``ValueError``).
    With ``norm_fn='instance'`` the bias of every conv but ``conv2`` cancels
    in the mean subtraction: its gradient is exact zero here, where torch's
    autograd returns rounding noise.  The fp16 pack has no gradient because
    it has no yardstick: the autograd of a restatement that rounds the
    operands to fp16 differs from the exact gradient by up to 0.36 max|g| at
    test sizes, so it cannot serve as a reference.
    """

    def __init__(self, output_dim=128, norm_fn="instance", dtype=torch.float16,
                 differentiable=False):
        super().__init__()
        if norm_fn not in ("instance", "none"):
            raise ValueError("BasicEncoder4: norm_fn is 'instance' or 'none'")
        if dtype not in (torch.float16, torch.float32):
            raise ValueError("BasicEncoder4: dtype (the packed weight type) is float16 or float32")
        if output_dim % 64 or not 64 <= output_dim <= 1024:
            raise ValueError("BasicEncoder4: output_dim is a multiple of 64 in [64, 1024]")
        if differentiable and dtype != torch.float32:
            raise ValueError("BasicEncoder4: differentiable=True needs dtype=torch.float32 "
                             "(the fp16 pack has no gradient)")
        self.differentiable = bool(differentiable)
        self.norm_fn = norm_fn
        self.output_dim = int(output_dim)
        self.wdtype = dtype
        self.conv1 = nn.Conv2d(3, DIM, kernel_size=7, stride=2, padding=3)
        self.layer1 = nn.Sequential(_ResidualBlock(DIM, DIM, 1), _ResidualBlock(DIM, DIM, 1))
        self.layer2 = nn.Sequential(_ResidualBlock(DIM, 2 * DIM, 2),
                                    _ResidualBlock(2 * DIM, 2 * DIM, 1))
        self.conv2 = nn.Conv2d(2 * DIM, output_dim, kernel_size=1)
        for m in self.modules():  # extractor.py:233-235
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        self._blob = None
        self._blob_key = None
        self._ws = None

    @classmethod
    def from_reference(cls, module, dtype=torch.float16):
        """Copy an existing reference ``BasicEncoder4`` (any device / dtype)."""
        sd = {k: v.detach().to("cpu", torch.float32) for k, v in module.state_dict().items()}
        new = cls(output_dim=sd["conv2.weight"].shape[0], norm_fn=module.norm_fn, dtype=dtype)
        new.load_state_dict(sd)
        return new

    # -- packed weights ------------------------------------------------------
    def _wcode(self):
        return ext().F16 if self.wdtype == torch.float16 else ext().F32

    def _ncode(self):
        return ext().NORM_INSTANCE if self.norm_fn == "instance" else ext().NORM_NONE

    def _key(self, device):
        return (str(device), self.wdtype) + tuple((p.data_ptr(), p._version)
                                                  for p in self.parameters())

    def packed(self, device):
        """The device blob of the packed weights; packed on first use and again
        whenever a parameter was written or replaced."""
        key = self._key(device)
        if self._blob is None or key != self._blob_key:
            tensors = [p.detach().to("cpu", torch.float32).contiguous() for p in self.parameters()]
            if len(tensors) != 22:
                raise RuntimeError("BasicEncoder4: expected 22 parameter tensors")
            host = ext().pack_weights(tensors, self.output_dim, self._ncode(), self._wcode())
            self._blob = host.to(device)
            self._blob_key = key
        return self._blob

    def workspace(self, n, H, W, device):
        need = ext().workspace_bytes(n, H, W, self.output_dim)
        if need <= 0:
            raise ValueError(f"BasicEncoder4: unsupported size {n} x {H} x {W}")
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self._ws

    def forward(self, images, channels_last=False):
        train = (self.differentiable and torch.is_grad_enabled()
                 and any(p.requires_grad for p in self.parameters()))
        with torch.set_grad_enabled(train):
            return self._forward(images, channels_last, train)

    def _forward(self, images, channels_last, train):
        require_gpu(images)
        if train and images.requires_grad:
            raise ValueError("BasicEncoder4: the image gradient is not provided "
                             "(images.requires_grad must be False)")
        if images.dim() != 5 or images.shape[2] != 3:
            raise ValueError("BasicEncoder4: images must be [b, n, 3, H, W]")
        b, n, _, H, W = images.shape
        if b * n < 1 or H < 1 or W < 1:
            raise ValueError("BasicEncoder4: empty images")
        dev = images.device
        x = images.reshape(b * n, 3, H, W).to(torch.float32).contiguous()
        h, w = out_size(out_size(H)), out_size(out_size(W))
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        if train:
            params = list(self.parameters())
            if len(params) != 22:
                raise RuntimeError("BasicEncoder4: expected 22 parameter tensors")
            out = _EncoderFunction.apply(self, x, fmt, *params)
        else:
            out = torch.empty(b * n, self.output_dim, h, w, dtype=torch.float32, device=dev,
                              memory_format=fmt)
            ext().forward(self.packed(dev), self._wcode(), self._ncode(), x, out,
                          self.workspace(b * n, H, W, dev))
        if channels_last:  # [b, n, C, h, w] with the channels-last strides kept
            return out.permute(0, 2, 3, 1).reshape(b, n, h, w, self.output_dim).permute(0, 1, 4, 2, 3)
        return out.view(b, n, self.output_dim, h, w)
