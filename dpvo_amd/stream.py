"""Image stream on the device (csrc/stream.hip): frame in, tracker input out.

read_calib     the np.loadtxt of dpvo/stream.py:11: 4, 8 or 9 numbers
               fx fy cx cy [k1 k2 p1 p2 [k3]].
prepare_frame  undistort (when the calibration has more than four numbers,
               stream.py:26-27), halve (video_stream's INTER_AREA, :78) and crop
               to a multiple of 16 (:36-37) in one launch -> the [3, H, W] uint8
               image and the float32 intrinsics that DPVO.__call__ takes.
ImageStream    the reference's image_stream over a directory, without cv2 and
               without a reader process: PIL decodes into a reused pinned
               buffer, the copy and the kernel are asynchronous.

The undistortion is OpenCV's camera model with its 1/32-pixel map quantisation
and an exact integer bilinear blend (include/dpvo_hot.h states it operation
for operation); it is not claimed bit-equal to cv2.undistort.
"""
from __future__ import annotations

from itertools import chain
from pathlib import Path

import numpy as np
import torch

from ._native import load_extension, require_gpu

IMG_EXTS = ("*.png", "*.jpeg", "*.jpg")


def read_calib(path):
    """The calibration line of calib/*.txt as float64 [4 | 8 | 9]."""
    calib = np.atleast_1d(np.loadtxt(path, delimiter=" ")).astype(np.float64).reshape(-1)
    if calib.size not in (4, 8, 9):
        raise ValueError(f"{path}: expected 4, 8 or 9 numbers fx fy cx cy [k1 k2 p1 p2 [k3]], "
                         f"got {calib.size}")
    return calib


def prepare_frame(raw, calib, scale=1.0, swap_rb=False, out=None):
    """raw uint8 [H0, W0, 3] (interleaved) or [H0, W0] (grey, replicated) on the
    device -> (image uint8 [3, H, W], intrinsics float32 [4]).

    calib: 4, 8 or 9 numbers; with 4 there is no remap.  scale: 1 or 0.5 (0.5
    needs even H0 and W0).  swap_rb: plane p takes channel 2 - p.  out: a
    contiguous uint8 [3, H, W] device tensor to write into (a reused buffer).
    H, W = the scaled size cropped top-left to multiples of 16; intrinsics =
    (fx, fy, cx, cy) * scale.  One launch, no host synchronisation."""
    ext = load_extension("cuda_ba")
    require_gpu(raw)
    calib = [float(v) for v in np.asarray(calib, dtype=np.float64).reshape(-1)]
    image, intrinsics = ext.frame_prepare(raw, calib, float(scale), bool(swap_rb), out)
    return image, intrinsics


def list_images(imagedir, stride=1, skip=0):
    """stream.py:20-21: the sorted *.png / *.jpeg / *.jpg of imagedir, [skip::stride]."""
    if not Path(imagedir).is_dir():
        raise FileNotFoundError(imagedir)
    return sorted(chain.from_iterable(Path(imagedir).glob(e) for e in IMG_EXTS))[skip::stride]


class ImageStream:
    """for t, image, intrinsics in ImageStream(imagedir, calib): slam(t, image, intrinsics)

    calib: a path (read_calib) or the numbers.  Frames are decoded with PIL:
    a grey file stays one channel (the kernel replicates it), anything else is
    converted to RGB -- cv2.imread delivers BGR, so pass swap_rb=True for the
    reference's channel order.  Every frame must have the size of the first."""

    def __init__(self, imagedir, calib, stride=1, skip=0, scale=1.0, swap_rb=False, device="cuda"):
        self.files = list_images(imagedir, stride, skip)
        self.calib = read_calib(calib) if isinstance(calib, (str, Path)) else np.asarray(
            calib, dtype=np.float64).reshape(-1)
        self.scale, self.swap_rb = float(scale), bool(swap_rb)
        self.device = torch.device(device)
        self._pinned = None
        self._copied = None

    def __len__(self):
        return len(self.files)

    @staticmethod
    def decode(path):
        """uint8 [H0, W0] (grey files) or [H0, W0, 3] (RGB) as PIL decodes it."""
        from PIL import Image

        with Image.open(path) as im:
            if im.mode not in ("L", "RGB"):
                im = im.convert("L" if im.mode in ("1", "I;16", "I", "F", "LA") else "RGB")
            return np.asarray(im, dtype=np.uint8)

    def __iter__(self):
        for t, path in enumerate(self.files):
            frame = self.decode(path)
            if self._pinned is None:
                self._pinned = torch.empty(frame.shape, dtype=torch.uint8).pin_memory()
            if tuple(self._pinned.shape) != frame.shape:
                raise ValueError(f"{path}: frame {frame.shape} differs from the first "
                                 f"{tuple(self._pinned.shape)}")
            # the previous copy out of the pinned buffer has to be over before it is
            # rewritten; the host waits for that copy alone, not for the tracker
            if self._copied is not None:
                self._copied.synchronize()
            self._pinned.numpy()[...] = frame
            raw = self._pinned.to(self.device, non_blocking=True)
            with torch.cuda.device(self.device):
                self._copied = torch.cuda.Event()
                self._copied.record()
            image, intrinsics = prepare_frame(raw, self.calib, self.scale, self.swap_rb)
            yield t, image, intrinsics
