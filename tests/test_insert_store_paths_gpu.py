"""GPU: the store paths of the frame insertion (pyr_insert.hpp), through the
stand-alone kernel (altcorr.insert_frame / insert_frame_ring) and the fused
start-of-update launch (fastba.reproject(..., insert=), C = 128 only).

Level 1 leaves the LDS tile as 16 B of 4 channels per lane (fp32: non-temporal
stores; fp16: 8 B), pooled levels one channel per lane, channel tails
(C % 4 != 0) as scalars.  Sizes: one tile (8 x 16), W % 4 == 0 with half a tile
in x (24 x 40), W % 4 != 0 (16 x 18: the scalar load path) and the 120 x 160
frame once; C = 32, 128 and 30 (channel tail); levels [1,2,4,8] and [1,4]; fp32
and fp16.  Expected, exactly: level 1 = the input in channels-last memory,
level s = avg_pool2d(x, s, s) (fp16: summed in fp32, rounded once).  Ring of 3
slots, slot from a device scalar 0, 2, 5 and -1 (both wrap); the other slots
keep their sentinel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MEM, SENTINEL = 3, 7.0
SIZES = [(8, 16), (24, 40), (16, 18)]
DTYPES = [torch.float32, torch.float16]
_DT = pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16"])
_LV = pytest.mark.parametrize("scales", [(1, 2, 4, 8), (1, 4)], ids=["L4", "L2"])


def _frame(C, H, W, dtype, dev):
    g = torch.Generator(device="cpu").manual_seed(1000 * C + 10 * H + W)
    return torch.randn(C, H, W, generator=g).to(dev).to(dtype)


def _refs(fmap, scales):
    return [fmap if s == 1 else
            torch.nn.functional.avg_pool2d(fmap[None].float(), s, s)[0].to(fmap.dtype)
            for s in scales]


def _ring(C, H, W, scales, dtype, dev):
    from dpvo_amd import synthetic

    return [synthetic.channels_last(torch.full((1, MEM, C, H // s, W // s), SENTINEL, device=dev,
                                               dtype=dtype)) for s in scales]


def _check(pyr, refs, scales, slot):
    others = [k for k in range(MEM) if k != slot]
    for p, s, ref in zip(pyr, scales, refs):
        assert p[0, slot].permute(1, 2, 0).is_contiguous()  # channels-last memory
        assert torch.equal(p[0, slot], ref), (s, slot)
        assert bool((p[0, others] == SENTINEL).all()), (s, slot)


def _standalone(gpu, C, H, W, scales, dtype):
    from dpvo_amd import altcorr

    fmap = _frame(C, H, W, dtype, gpu)
    refs = _refs(fmap, scales)
    for sd in (0, 2, 5, -1):
        pyr = _ring(C, H, W, scales, dtype, gpu)
        altcorr.insert_frame_ring(fmap, pyr, torch.tensor([sd], dtype=torch.int32, device=gpu),
                                  scales)
        _check(pyr, refs, scales, sd % MEM)
    pyr = _ring(C, H, W, scales, dtype, gpu)
    altcorr.insert_frame(fmap, pyr, 1, scales)
    _check(pyr, refs, scales, 1)


@_DT
@_LV
@pytest.mark.parametrize("C", [32, 128, 30])
@pytest.mark.parametrize("HW", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_standalone_insert(gpu, HW, C, scales, dtype):
    _standalone(gpu, C, *HW, scales, dtype)


@_DT
def test_standalone_insert_full_frame(gpu, dtype):
    _standalone(gpu, 128, 120, 160, (1, 2, 4, 8), dtype)


def _fused(gpu, H, W, scales, dtype):
    """reproject(mem=, plan_window=, insert=) writes slot views: every slot of the ring in turn."""
    from dpvo_amd import fastba, synthetic

    G = synthetic.make_config("cfg1", seed=3)
    D = G.to(gpu)
    fmap = _frame(128, H, W, dtype, gpu)
    refs = _refs(fmap, scales)
    for slot in range(MEM):
        pyr = _ring(128, H, W, scales, dtype, gpu)
        fastba.reproject(D.poses, D.patches, D.intrinsics, D.ii, D.jj, D.kk, mem=G.F + 2,
                         plan_window=(1, G.F), insert=(fmap, [p[0, slot] for p in pyr], scales))
        torch.cuda.synchronize()
        _check(pyr, refs, scales, slot)


@_DT
@_LV
@pytest.mark.parametrize("HW", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_fused_insert(gpu, HW, scales, dtype):
    _fused(gpu, *HW, scales, dtype)


@_DT
def test_fused_insert_full_frame(gpu, dtype):
    _fused(gpu, 120, 160, (1, 2, 4, 8), dtype)
