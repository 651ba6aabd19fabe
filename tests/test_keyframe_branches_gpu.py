"""GPU: every case of tests/keyframe_cases.py (the branches of
dpvo_amd/csrc/keyframe.hip: DPVO.keyframe's frame drop and
PatchGraph.edges_loop, away from the defaults) against the oracle, exactly.

test_oracle_keyframe_cases.py shows without a device that each case reaches
the branch it is named for.  Here every output is compared bit for bit: kf,
mag, the edge lists, net / weight / target, every shifted array, st, the delta
log and the error word; for edges_loop kk, jj, the count, last_global_ba, the
per-group values in the work buffer and ii = ix[kk] after the append.  Output
buffers are pre-filled with a sentinel: nothing beyond count (or ng) may be
written.  The refusals (KEYFRAME_INDEX > 17, a ring no larger than the moved
frames, more than 12 arrays) launch nothing."""
import numpy as np
import pytest
import torch

from keyframe_cases import DROP_CASES, GRAPH_FRAMES, LOOP_CASES, build_drop, build_loop

pytestmark = pytest.mark.gpu

SENT = -7
WORK_SENT = 0x7FC0DEAD  # a NaN pattern no kernel writes
EDGE_ARRAYS = ("net", "weight", "target")


def _T(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _drop_setup(gpu, b):
    from dpvo_amd.patchgraph import DevicePatchGraph

    c, st = b["case"], b["state"]
    N, M, E = c["N"], c["M"], st["num_edges"]
    pg = DevicePatchGraph(max_edges=c["ME"], DIM=16, device=gpu)
    ix = torch.arange(N * M, device=gpu) // M
    pg.append_factors(ix, _T(st["kk"][:E], gpu), _T(st["jj"][:E], gpu))
    for name in EDGE_ARRAYS:
        getattr(pg, name)[0, :E] = _T(st[name][:E], gpu)
    dev = {k: _T(st[k], gpu) for k in ("poses", "patches", "intrinsics", "tstamps")}
    dev.update({k: _T(st[k], gpu) for k in b["rings"]})
    dst = torch.tensor([st["n"], st["m"]], dtype=torch.int32, device=gpu)
    cap = 2 * GRAPH_FRAMES + 1
    log = (torch.full((cap, 7), float(SENT), device=gpu),
           torch.full((cap, 2), SENT, dtype=torch.long, device=gpu),
           torch.zeros(1, dtype=torch.int32, device=gpu))
    kf = torch.full((2,), SENT, dtype=torch.int32, device=gpu)
    mag = torch.full((2,), float(SENT), device=gpu)

    def call():
        pg.keyframe(dst, dev["poses"], dev["patches"], dev["intrinsics"], M,
                    frames=[dev[k] for k in b["rings"]], rings=list(b["rings"].values()),
                    tstamps=dev["tstamps"], keyframe_index=c["KI"], keyframe_thresh=b["thresh"],
                    kf=kf, mag=mag, delta=log)

    return pg, dev, dst, log, kf, mag, call


def _drop_check(b, pg, dev, dst, log, kf, mag):
    steps = b["steps"]
    rs, info = steps[-1]
    m = mag.cpu().numpy()
    ref = np.array(info["mag"], np.float32)
    print(b["case"]["name"], "mag", m, "oracle", ref, "drops", [s[1]["drop"] for s in steps])
    np.testing.assert_array_equal(m.view(np.uint32), ref.view(np.uint32))
    assert kf.cpu().tolist() == [int(info["drop"]), info["k"]]
    ne = rs["num_edges"]
    assert pg.num_edges == ne and pg.errors == 0
    for name in ("ii", "jj", "kk"):
        np.testing.assert_array_equal(getattr(pg, name)[:ne].cpu().numpy(), rs[name][:ne], name)
    for name in EDGE_ARRAYS:
        np.testing.assert_array_equal(getattr(pg, name)[0, :ne].cpu().numpy(), rs[name][:ne],
                                      name)
    assert dst.cpu().tolist() == [rs["n"], rs["m"]]
    for name, t in dev.items():
        np.testing.assert_array_equal(t.cpu().numpy(), rs[name], name)
    recs = [s[1]["delta"] for s in steps if s[1]["drop"]]
    assert int(log[2].item()) == len(recs)
    dl, dt = log[0].cpu().numpy(), log[1].cpu().numpy()
    for r, (t1, t0, dp) in enumerate(recs):
        assert dt[r].tolist() == [t1, t0]
        np.testing.assert_array_equal(dl[r].view(np.uint32), dp.view(np.uint32))
    assert (dl[len(recs):] == SENT).all() and (dt[len(recs):] == SENT).all()


@pytest.mark.parametrize("name", [c["name"] for c in DROP_CASES if not c["graph"]])
def test_frame_drop_case(gpu, name):
    b = build_drop(name)
    pg, dev, dst, log, kf, mag, call = _drop_setup(gpu, b)
    for _ in range(b["case"]["drops"]):
        call()
    torch.cuda.synchronize()
    _drop_check(b, pg, dev, dst, log, kf, mag)


@pytest.mark.parametrize("name", [c["name"] for c in DROP_CASES if c["graph"]])
def test_frame_drop_sequence_replays_from_a_graph(gpu, name):
    """Two keyframe calls and the arrival of a frame, captured once and
    replayed: the decisions, the two buffer swaps per replay and the delta log
    follow st, which moves underneath the graph."""
    b = build_drop(name)
    pg, dev, dst, log, kf, mag, call = _drop_setup(gpu, b)
    inc = torch.tensor([1, b["case"]["M"]], dtype=torch.int32, device=gpu)

    def frame():
        for _ in range(b["case"]["drops"]):
            call()
        dst.add_(inc)

    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        frame()  # warm on the side stream: the first frame of the sequence
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(g):
        frame()
    for _ in range(GRAPH_FRAMES - 1):
        g.replay()
    torch.cuda.synchronize()
    _drop_check(b, pg, dev, dst, log, kf, mag)


@pytest.mark.parametrize("name", [c["name"] for c in LOOP_CASES])
def test_edges_loop_case(gpu, name):
    from dpvo_amd.patchgraph import DevicePatchGraph

    b = build_loop(name)
    c, par = b["case"], b["par"]
    n, M, N = c["n"], c["M"], b["N"]
    rk, rj = b["kk"], b["jj"]
    pg = DevicePatchGraph(max_edges=len(rk) + 64, DIM=16, device=gpu, net=False)
    st = torch.tensor([n, n * M], dtype=torch.int32, device=gpu)
    last = None if c["last"] is None else torch.tensor([c["last"]], dtype=torch.int32, device=gpu)
    cap = (par["max_num_edges"] + 2) * M
    W = pg._ext.edges_loop_work_floats()
    work = torch.full((W,), WORK_SENT, dtype=torch.int32, device=gpu)
    out = (torch.full((cap,), SENT, dtype=torch.long, device=gpu),
           torch.full((cap,), SENT, dtype=torch.long, device=gpu),
           torch.full((1,), SENT, dtype=torch.int32, device=gpu), work.view(torch.float32))
    dix = _T(b["ix"], gpu)
    kk, jj, cnt = pg.edges_loop(_T(b["poses"], gpu), _T(b["patches"], gpu),
                                _T(b["intrinsics"], gpu), dix, st, N, M, last_global_ba=last,
                                out=out, **par)
    torch.cuda.synchronize()
    cn = int(cnt.item())
    print(name, "count", cn, "oracle", len(rk))
    # the per-group values and source frames, and nothing behind them
    w = work.cpu().numpy()
    g = b["groups_written"]
    ng = 0 if g is None else g["ng"]
    half = W // 2
    if ng:
        np.testing.assert_array_equal(w[:ng].view(np.uint32), g["fm"].view(np.uint32))
        np.testing.assert_array_equal(w[half:half + ng], g["gi"].astype(np.int32))
    assert (w[ng:half] == WORK_SENT).all() and (w[half + ng:] == WORK_SENT).all()
    # the selection
    assert cn == len(rk)
    hk, hj = kk.cpu().numpy(), jj.cpu().numpy()
    np.testing.assert_array_equal(hk[:cn], rk)
    np.testing.assert_array_equal(hj[:cn], rj)
    assert (hk[cn:] == SENT).all() and (hj[cn:] == SENT).all()
    if last is not None:
        assert int(last.item()) == b["last_after"]
    assert pg.errors == 0
    assert st.cpu().tolist() == [n, n * M]
    # the append of the device count gives ii = ix[kk]
    pg.append_factors_dev(dix, kk, jj, cnt)
    assert pg.num_edges == cn and pg.errors == 0
    np.testing.assert_array_equal(pg.ii[:cn].cpu().numpy(), b["ix"][rk])
    np.testing.assert_array_equal(pg.kk[:cn].cpu().numpy(), rk)
    np.testing.assert_array_equal(pg.jj[:cn].cpu().numpy(), rj)


# --------------------------------------------------------------------------- the refusals
def _snapshot(pg, dev, dst, log, kf, mag):
    ts = [pg.ii, pg.jj, pg.kk, pg.net, pg.weight, pg.target, pg.counts, dst, kf, mag, *log,
          *dev.values()]
    return [t.clone() for t in ts], ts


def _unchanged(snap):
    torch.cuda.synchronize()
    return all(torch.equal(a, b) for a, b in zip(*snap))


def test_keyframe_index_above_17_is_refused_before_any_launch(gpu):
    """A drop would move KEYFRAME_INDEX - 1 > 16 frames, more than the shift
    kernel holds: an exception from DevicePatchGraph.keyframe and from the
    entry that knows the index, the graph and st unchanged."""
    b = build_drop("ki17_moves_16_frames")
    pg, dev, dst, log, kf, mag, _ = _drop_setup(gpu, b)
    snap = _snapshot(pg, dev, dst, log, kf, mag)
    a_before = pg._a
    with pytest.raises(ValueError, match="16"):
        pg.keyframe(dst, dev["poses"], dev["patches"], dev["intrinsics"], 4, tstamps=dev["tstamps"],
                    keyframe_index=18, kf=kf, mag=mag, delta=log)
    with pytest.raises(RuntimeError):
        pg._ext.kf_motion(pg.ii, pg.jj, pg.kk, pg.counts, dev["poses"], dev["patches"],
                          dev["intrinsics"], dst, 18, 12.5, kf, mag)
    assert pg._a is a_before and _unchanged(snap)


def test_ring_no_larger_than_the_moved_frames_is_refused(gpu):
    """0 < ring <= KEYFRAME_INDEX - 1: the reference's frame-by-frame copy
    re-reads rows it has overwritten, the device reads all rows first; the
    case is refused, ring = KEYFRAME_INDEX is the smallest accepted (the
    ring_min_rows_wrap case)."""
    b = build_drop("ki4_moves_3_frames")
    pg, dev, dst, log, kf, mag, _ = _drop_setup(gpu, b)
    snap = _snapshot(pg, dev, dst, log, kf, mag)
    a_before = pg._a
    for ring in (1, 2, 3):
        with pytest.raises(ValueError, match="ring"):
            pg.keyframe(dst, dev["poses"], dev["patches"], dev["intrinsics"], 4,
                        frames=[dev["gmap"]], rings=[ring], tstamps=dev["tstamps"],
                        keyframe_index=4, kf=kf, mag=mag, delta=log)
    with pytest.raises(ValueError, match="12"):
        pg.keyframe(dst, dev["poses"], dev["patches"], dev["intrinsics"], 4,
                    frames=[dev["colors"]] * 9, rings=[0] * 9, tstamps=dev["tstamps"],
                    kf=kf, mag=mag, delta=log)
    assert pg._a is a_before and _unchanged(snap)


def test_edges_loop_bad_window_is_refused(gpu):
    """keyframe_index < 0 (target frames past n) and global_opt_freq >
    removal_window + 1 (target frames before 0) raise and write nothing."""
    from dpvo_amd.patchgraph import DevicePatchGraph

    b = build_loop("nms_1")
    c = b["case"]
    pg = DevicePatchGraph(max_edges=64, DIM=16, device=gpu, net=False)
    st = torch.tensor([c["n"], c["n"] * c["M"]], dtype=torch.int32, device=gpu)
    W = pg._ext.edges_loop_work_floats()
    out = (torch.full((64,), SENT, dtype=torch.long, device=gpu),
           torch.full((64,), SENT, dtype=torch.long, device=gpu),
           torch.full((1,), SENT, dtype=torch.int32, device=gpu),
           torch.full((W,), float(SENT), device=gpu))
    args = (_T(b["poses"], gpu), _T(b["patches"], gpu), _T(b["intrinsics"], gpu),
            _T(b["ix"], gpu), st, b["N"], c["M"])
    for bad in (dict(keyframe_index=-1), dict(removal_window=20, global_opt_freq=22)):
        with pytest.raises(RuntimeError):
            pg.edges_loop(*args, out=out, max_num_edges=8, **bad)
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in out) and pg.errors == 0
