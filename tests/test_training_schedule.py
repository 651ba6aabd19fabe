"""CPU: dpvo_amd.net.training_schedule against this file's restatement of
net.py:458-497 written with meshgrid as the reference does; exact over ii, jj,
kk and n at every step."""
import pytest
import torch

from dpvo_amd.net import training_schedule


def flatmeshgrid(a, b):
    x, y = torch.meshgrid(a, b, indexing="ij")
    return x.reshape(-1), y.reshape(-1)


def restated(n_frames, ppi, steps, init_frames=8, drop=lambda step: False):
    ix = torch.arange(n_frames).view(n_frames, 1).repeat(1, ppi).reshape(-1)
    kk, jj = flatmeshgrid(torch.where(ix < init_frames)[0], torch.arange(0, init_frames))
    ii = ix[kk]
    out = []
    while len(out) < steps:
        n = ii.max() + 1
        if len(out) >= init_frames and n < n_frames:
            kk1, jj1 = flatmeshgrid(torch.where(ix < n)[0], torch.arange(n, n + 1))
            kk2, jj2 = flatmeshgrid(torch.where(ix == n)[0], torch.arange(0, n + 1))
            ii = torch.cat([ix[kk1], ix[kk2], ii])
            jj = torch.cat([jj1, jj2, jj])
            kk = torch.cat([kk1, kk2, kk])
            if drop(len(out)):
                k = (ii != (n - 4)) & (jj != (n - 4))
                ii, jj, kk = ii[k], jj[k], kk[k]
            n = ii.max() + 1
        out.append((ii, jj, kk, int(n)))
    return out


def loss_edges(ii, jj):
    d = (ii - jj).abs()
    return int(((d > 0) & (d <= 2)).sum())


def same(a, b):
    assert len(a) == len(b)
    for s, ((i0, j0, k0, n0), (i1, j1, k1, n1)) in enumerate(zip(a, b)):
        assert n0 == n1, s
        for x, y in ((i0, i1), (j0, j1), (k0, k1)):
            assert x.dtype == torch.int64 and x.device.type == "cpu"
            assert torch.equal(x, y), s


never, always = (lambda step: False), (lambda step: True)


@pytest.mark.parametrize("shape", [(10, 4, 11, 8), (15, 80, 18, 8), (6, 4, 6, 4), (9, 3, 5, 8),
                                   (8, 2, 12, 8), (12, 1, 14, 3)])
@pytest.mark.parametrize("drop", [never, always, lambda step: step % 2 == 0])
def test_matches_restatement(shape, drop):
    n_frames, ppi, steps, init = shape
    same(training_schedule(n_frames, ppi, steps, init_frames=init, drop=drop),
         restated(n_frames, ppi, steps, init, drop))


def test_anchor_counts():
    s = training_schedule(10, 4, 11, drop=never)
    assert [len(x[0]) for x in s] == [256] * 8 + [324, 400, 400]
    assert [loss_edges(x[0], x[1]) for x in s] == [104] * 8 + [120, 136, 136]
    assert [x[3] for x in s] == [8] * 8 + [9, 10, 10]
    s = training_schedule(10, 4, 11, drop=always)
    assert [len(x[0]) for x in s] == [256] * 8 + [256, 264, 264]
    assert [loss_edges(x[0], x[1]) for x in s][8:] == [88, 80, 80]


def test_training_shape():
    s = training_schedule(15, 80, 18, drop=never)
    assert len(s) == 18 and s[-1][3] == 15
    assert len(s[-1][0]) == 18000 and loss_edges(s[-1][0], s[-1][1]) == 4320


def test_small_init_and_short_runs():
    s = training_schedule(6, 4, 6, init_frames=4, drop=never)
    assert [x[3] for x in s] == [4, 4, 4, 4, 5, 6]
    assert [len(x[0]) for x in s] == [64, 64, 64, 64, 100, 144]
    s = training_schedule(10, 4, 3, drop=never)  # steps < init_frames: the graph never grows
    assert len(s) == 3 and all(x[3] == 8 and len(x[0]) == 256 for x in s)
    assert training_schedule(10, 4, 0) == []


def test_drop_is_asked_once_per_growth_step():
    asked = []
    training_schedule(10, 4, 12, drop=lambda step: asked.append(step) or False)
    assert asked == [8, 9]


def test_default_drop_draws_from_the_host_rng():
    import numpy as np

    np.random.seed(3)
    draws = np.random.rand(2) < 0.1
    np.random.seed(3)
    got = training_schedule(10, 4, 11)
    same(got, restated(10, 4, 11, 8, lambda step: bool(draws[step - 8])))


def test_rejects_too_few_frames():
    with pytest.raises(ValueError):
        training_schedule(5, 4, 3)


def test_rejects_a_single_initial_frame():
    """A new frame's depth is the median of the two frames before it."""
    with pytest.raises(ValueError):
        training_schedule(5, 2, 3, init_frames=1)
    assert len(training_schedule(5, 2, 4, init_frames=2, drop=never)) == 4


def test_sequence_loss_rejects_an_empty_trajectory():
    from dpvo_amd.training import sequence_loss

    with pytest.raises(ValueError):
        sequence_loss([])
