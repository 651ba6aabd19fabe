"""Scene builders and the case tables of the keyframe tests
(dpvo_amd/csrc/keyframe.hip: DPVO.keyframe's frame drop and
PatchGraph.edges_loop).

* test_keyframe_gpu.py imports the builders;
* test_oracle_keyframe_cases.py shows on the oracle alone (no device) that
  every case of DROP_CASES / LOOP_CASES reaches the branch its name says;
* test_keyframe_branches_gpu.py runs every case on the device and compares
  every output with the oracle exactly.

A built case is cached, so the oracle's results are computed once and shared
(they are not to be modified by a test)."""
import functools

import numpy as np

import oracle


def _quat(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([np.sin(ang / 2) * axis, [np.cos(ang / 2)]])


def _scene(rng, N, M, P, motion, n):
    """poses (world->camera, lietorch [t, q]) along x with step `motion`,
    small rotations; patches inside a 160 x 120 image with inverse depth in
    [0.2, 1]."""
    poses = np.zeros((N, 7), np.float32)
    for f in range(N):
        q = _quat(rng.normal(size=3), 0.01 * rng.normal())
        poses[f, :3] = [-motion[f] if f < n else 0.0, 0.01 * rng.normal(), 0.01 * rng.normal()]
        poses[f, 3:] = q
    pts = np.zeros((N * M, 3, P, P), np.float32)
    cx = rng.uniform(10, 150, N * M)
    cy = rng.uniform(10, 110, N * M)
    off = np.arange(P) - P // 2
    pts[:, 0] = cx[:, None, None] + off[None, None, :]
    pts[:, 1] = cy[:, None, None] + off[None, :, None]
    pts[:, 2] = rng.uniform(0.2, 1.0, N * M)[:, None, None]
    intr = np.tile(np.array([100.0, 100.0, 80.0, 60.0], np.float32), (N, 1))
    return poses, pts, intr


def _edges(n, M, r=3):
    ii, jj, kk = [], [], []
    for a in range(n):
        for b in range(max(0, a - r), min(n, a + r + 1)):
            for m in range(M):
                ii.append(a)
                jj.append(b)
                kk.append(a * M + m)
    return np.array(ii, np.int64), np.array(jj, np.int64), np.array(kk, np.int64)


def _loop_scene(rng, N, M, P, n, period=40):
    """a camera circling with `period` frames per lap: frame pairs one lap
    apart see the same view (small flow), others do not."""
    poses = np.zeros((N, 7), np.float32)
    for f in range(N):
        th = 2 * np.pi * f / period
        R = _quat([0, 1, 0], -th)
        c = np.array([0.6 * np.sin(th), 0.0, 0.6 * (1 - np.cos(th))])
        # world->camera: t = -R c (rotation about y applied to the centre)
        ca, sa = np.cos(-th), np.sin(-th)
        Rm = np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
        poses[f, :3] = -Rm @ c + 0.002 * rng.normal(size=3)
        poses[f, 3:] = R
    _, pts, intr = _scene(rng, N, M, P, np.zeros(N), 0)
    pts[:, 2] = rng.uniform(0.5, 1.5, N * M)[:, None, None]
    return poses, pts, intr


def _rot(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def depth_after_transform(poses, pts, intr, ii, jj, kk):
    """Z of every patch pixel of the edges (ii -> jj, patch kk) in frame jj, in
    fp64 straight from the definition (poses[jj] * poses[ii]^-1 applied to the
    back-projected pixel): an independent look at which pixels take the
    fmaxf(Z, 0.1) clamp and which fail Z > 0.2.  [E, P, P]."""
    out = []
    for a, b, k in zip(ii, jj, kk):
        Ri, Rj = _rot(poses[a, 3:]), _rot(poses[b, 3:])
        R = Rj @ Ri.T
        t = poses[b, :3].astype(np.float64) - R @ poses[a, :3].astype(np.float64)
        fx, fy, cx, cy = intr[a].astype(np.float64)
        X = (pts[k, 0].astype(np.float64) - cx) / fx
        Y = (pts[k, 1].astype(np.float64) - cy) / fy
        out.append(R[2, 0] * X + R[2, 1] * Y + R[2, 2] + t[2] * pts[k, 2].astype(np.float64))
    return np.array(out)


# --------------------------------------------------------------------------- frame drop
# frame arrays: (name, dtype, shape of one frame, ring).  ring 0: row = frame.
# "ki" / "ki+?" ring sizes are relative to KEYFRAME_INDEX (ring = nm + 1 = KI is
# the smallest the device supports).
_BASIC = (("gmap", np.float32, (2, 4, 3, 3), "ki+2"), ("colors", np.uint8, (10, 3), 0))
_DROP_DEFAULT = dict(N=32, M=4, P=3, n=20, KI=4, seed=7, still=True, edges="band", E=None,
                     thresh=12.5, clamp=False, frames=_BASIC, drops=1, graph=False, ME=2048,
                     expect_drop=True)


def _d(name, **kw):
    unknown = set(kw) - set(_DROP_DEFAULT)
    assert not unknown, unknown
    return dict(_DROP_DEFAULT, name=name, **kw)


DROP_CASES = [
    # frames moved: KEYFRAME_INDEX - 1 = 0, 1, 3, 16 (the most the kernel holds)
    _d("ki1_moves_0_frames", KI=1),
    _d("ki2_moves_1_frame", KI=2),
    _d("ki4_moves_3_frames", KI=4),
    _d("ki17_moves_16_frames", KI=17, n=26, frames=(("gmap", np.float32, (5,), "ki"),
                                                      ("colors", np.uint8, (10, 3), 0))),
    _d("ki4_large_motion_is_kept", still=False, expect_drop=False),
    _d("n_eq_ki_has_no_candidate", n=4, expect_drop=False),
    # which of the i <-> j edges exist
    _d("edges_i_to_j_only", edges="fwd"),
    _d("edges_j_to_i_only", edges="rev"),
    _d("edges_neither_is_a_drop", edges="none", still=False),
    # active edge count at the strides of the one-workgroup kernels
    _d("edge_count_0", edges="count", E=0, still=False),
    _d("edge_count_1", edges="count", E=1),
    _d("edge_count_255", edges="count", E=255),
    _d("edge_count_256", edges="count", E=256),
    _d("edge_count_257", edges="count", E=257),
    _d("edge_count_1025", edges="count", E=1025),
    # the strict comparison against KEYFRAME_THRESH
    _d("thresh_equal_is_kept", thresh="mid", expect_drop=False),
    _d("thresh_next_up_is_a_drop", thresh="mid_up"),
    # Z < 0.1 (clamp) and 0.1 < Z < 0.2, quaternions of norm 1.001
    _d("clamped_projection", clamp=True, thresh=1e6),
    _d("patch_1x1", P=1),
    _d("patch_2x2", P=2),
    _d("patch_4x4", P=4),
    # rings
    _d("ring_min_rows_wrap", n=22, frames=(("r4", np.float32, (5,), "ki"),
                                           ("r4b", np.uint8, (3,), "ki"))),
    _d("ring_much_larger_than_n", frames=(("big", np.float32, (3,), 1000),)),
    # bytes per frame: byte path (1, 7, 30), word path (4), > 256 words (4100)
    _d("frame_bytes_1", frames=(("a", np.uint8, (), 0),)),
    _d("frame_bytes_7", frames=(("a", np.uint8, (7,), 0), ("r", np.uint8, (7,), "ki+1"))),
    _d("frame_bytes_30", frames=(("a", np.uint8, (10, 3), 0),)),
    _d("frame_bytes_4_fp16", frames=(("a", np.float16, (2,), 0), ("r", np.float16, (2,), "ki"))),
    _d("frame_bytes_4100_fp16", frames=(("a", np.float16, (2050,), 0),
                                        ("r", np.float16, (2050,), "ki+3"))),
    _d("frame_int64", frames=(("a", np.int64, (3,), 0),)),
    # kMaxShift: poses, patches, intrinsics, tstamps + 8
    _d("twelve_arrays", frames=tuple((f"x{a}", (np.float32, np.uint8, np.int64, np.float16)[a % 4],
                                      (a + 1,), (0, "ki", 0, "ki+5")[a % 4]) for a in range(8))),
    # ping-pong buffers swap twice, two delta records
    _d("two_drops_in_a_row", drops=2),
    _d("two_drops_graph_replay", drops=2, graph=True, N=40, seed=21),
]
GRAPH_FRAMES = 4  # frames of the replayed sequence (1 warm-up + 3 replays), each two keyframe calls


def _ring(r, KI):
    if isinstance(r, str):
        return KI + int(r[2:] or 0)
    return r


def _drop_edges(c, rng, i, j, k):
    n, M = c["n"], c["M"]
    if c["edges"] == "count":
        E = c["E"]
        a, b = rng.integers(0, n, E), rng.integers(0, n, E)
        u = rng.uniform(size=E)
        a[u < 0.15], b[u < 0.15] = i, j
        s = (u >= 0.15) & (u < 0.3)
        a[s], b[s] = j, i
        a[(u >= 0.3) & (u < 0.4)] = k
        b[(u >= 0.4) & (u < 0.5)] = k
        if E >= 1:  # one in the middle, and the very last edge: the tail of a strided loop
            a[E // 2], b[E // 2] = i, j
        if E >= 2:
            a[E - 1], b[E - 1] = j, i
        return a.astype(np.int64), b.astype(np.int64), (a * M + rng.integers(0, M, E)).astype(np.int64)
    ne = c["N"] if c["graph"] else n  # the replayed sequence grows into frames that have edges
    ii, jj, kk = _edges(ne, M)
    fwd, rev = (ii == i) & (jj == j), (ii == j) & (jj == i)
    keep = {"band": ii >= 0, "fwd": ~rev, "rev": ~fwd, "none": ~(fwd | rev)}[c["edges"]]
    return ii[keep], jj[keep], kk[keep]


@functools.lru_cache(maxsize=None)
def build_drop(name):
    """The numpy state of a frame-drop case (the dict oracle.keyframe takes, plus
    the case's parameters under "case", the ring sizes under "rings" and the
    resolved threshold under "thresh") and the oracle's results: "steps" is a
    list of (state after, info) per keyframe call."""
    c = next(c for c in DROP_CASES if c["name"] == name)
    rng = np.random.default_rng(c["seed"])
    N, M, P, n, KI = c["N"], c["M"], c["P"], c["n"], c["KI"]
    i, j, k = n - KI - 1, n - KI + 1, n - KI
    f = np.arange(N)
    if c["graph"]:  # still and moving stretches: some calls drop, some keep
        step = np.where((f // 3) % 2 == 0, 0.002, 0.5)
    else:
        step = np.where((f >= i - 3) & (f <= j + 1), 0.002 if c["still"] else 0.5, 0.05)
    poses, pts, intr = _scene(rng, N, M, P, np.cumsum(step), N if c["graph"] else n)
    if c["clamp"]:
        # frame j one unit behind frame i along the optical axis: Z ~ 1 - d
        poses[j, 2] = poses[i, 2] - 1.0
        pts[i * M:(i + 1) * M, 2] = np.array([0.95, 0.85, 0.5, 0.3], np.float32)[:, None, None]
        poses[:, 3:] *= np.float32(1.001)
    ii, jj, kk = _drop_edges(c, rng, i, j, k)
    E, ME = len(ii), c["ME"]
    st = {"n": n, "m": n * M, "num_edges": E, "poses": poses, "patches": pts, "intrinsics": intr,
          "tstamps": (np.arange(N) * 3 + 1).astype(np.int64)}
    for nm_, a in (("ii", ii), ("jj", jj), ("kk", kk),
                   ("net", rng.normal(size=(E, 16)).astype(np.float32)),
                   ("weight", rng.uniform(size=(E, 2)).astype(np.float32)),
                   ("target", rng.normal(size=(E, 2)).astype(np.float32))):
        full = np.zeros((ME,) + a.shape[1:], a.dtype)
        full[:E] = a
        st[nm_] = full
    rings = {}
    for fname, dt, shape, r in c["frames"]:
        r = _ring(r, KI)
        # a ring array is allocated with at least N rows: the rows past the ring
        # must come back untouched
        rows = max(r, N)
        if np.issubdtype(dt, np.integer):
            a = rng.integers(0, 255, size=(rows,) + shape).astype(dt)
        else:
            a = rng.normal(size=(rows,) + shape).astype(dt)
        st[fname] = a
        rings[fname] = r
    thresh = c["thresh"]
    if isinstance(thresh, str):
        m0, m1 = oracle.motionmag(st, i, j), oracle.motionmag(st, j, i)
        thresh = (float(m0) + float(m1)) / 2
        if c["thresh"] == "mid_up":
            thresh = float(np.nextafter(thresh, np.inf))
    steps, cur = [], st
    calls = c["drops"] * (GRAPH_FRAMES if c["graph"] else 1)
    for s in range(calls):
        cur, info = oracle.keyframe(cur, M, keyframe_index=KI, keyframe_thresh=thresh, rings=rings)
        if c["graph"] and s % 2 == 1:  # a new frame arrives after every second call
            cur = dict(cur, n=cur["n"] + 1, m=cur["m"] + M)
        steps.append((cur, info))
    return {"case": c, "state": st, "rings": rings, "thresh": thresh, "steps": steps}


# --------------------------------------------------------------------------- edges_loop
_LOOP_DEFAULT = dict(M=4, P=3, n=50, period=40, rw=20, age=1000, gof=15, ki=4, thresh=64.0,
                     max_edges=1000, nms=1, seed=5, last=None, gate=None, tie=None,
                     expect="edges")


def _l(name, **kw):
    unknown = set(kw) - set(_LOOP_DEFAULT)
    assert not unknown, unknown
    return dict(_LOOP_DEFAULT, name=name, **kw)


# expect: "edges" (count > 0), "none" (count 0, window open), "closed" (nothing
# runs: count 0, last_global_ba untouched, no group value written)
LOOP_CASES = [
    # the window
    _l("n_eq_removal_window", n=20, last=0, expect="closed"),
    _l("n_eq_removal_window_plus_1", n=41, rw=40, period=33),
    _l("max_edge_age_1", n=60, rw=40, age=1, period=33),
    _l("max_edge_age_4", n=60, rw=40, age=4, period=33),
    _l("gof_eq_keyframe_index_no_targets", gof=4, last=0, expect="closed"),
    _l("non_default_window", n=45, rw=9, gof=8, ki=2, age=40, period=33),
    _l("candidates_all_closer_than_30", n=34, period=10, last=0, expect="none"),
    # BACKEND_THRESH (strict)
    _l("thresh_eq_smallest_group_no_key", thresh="min", last=0, expect="none"),
    _l("thresh_next_above_smallest_one_key", thresh="min_up"),
    # the lane-strided patch loop
    _l("patches_1", M=1),
    _l("patches_3", M=3),
    _l("patches_63", M=63),
    _l("patches_64", M=64),
    _l("patches_65", M=65),
    _l("patches_130", M=130),
    # count > 0.75 M: gate = (source frame, target frame, valid patches)
    _l("gate_M8_6_valid_is_inf", M=8, nms=0, gate=(5, 40, 6)),
    _l("gate_M8_7_valid_is_finite", M=8, nms=0, gate=(5, 40, 7)),
    _l("gate_M4_3_valid_is_inf", M=4, nms=0, gate=(5, 40, 3)),
    _l("gate_M4_4_valid_is_finite", M=4, nms=0, gate=(5, 40, 4)),
    # max_num_edges
    _l("max_num_edges_0", max_edges=0, last=0, expect="none"),
    _l("max_num_edges_1", max_edges=1),
    _l("max_num_edges_2", max_edges=2),
    _l("max_num_edges_one_less_than_found", max_edges="found-1"),
    # suppression radius
    _l("nms_0", nms=0),
    _l("nms_1", nms=1),
    _l("nms_5", nms=5),
    _l("nms_larger_than_frame_count", nms=1000),
    # bit-equal group values: the order of the tied pair decides
    _l("exact_tie_order", tie=3, nms=1),
    # sort sizes ng = nj x nf
    _l("sort_ng_1", n=60, rw=40, age=1, gof=5, ki=4, period=36),
    _l("sort_ng_2", n=60, rw=40, age=2, gof=5, ki=4, period=36),
    _l("sort_ng_3", n=60, rw=40, age=1, gof=7, ki=4, period=36),
    _l("sort_ng_1023", n=67, rw=36, gof=37, ki=4, age=31),
    _l("sort_ng_1024", n=67, rw=35, gof=36, ki=4, age=32),
    _l("sort_ng_1025", n=71, rw=30, gof=29, ki=4, age=41),
    _l("sort_ng_4400_several_pairs_per_thread", n=420, M=2, seed=3),
    _l("sort_ng_16384_capacity", n=1044, M=2, rw=20, gof=20, ki=4, age=1024),
    # dpvo.py:984
    _l("gate_closed_one_frame_early", last=50 - 14, expect="closed"),
    _l("gate_open_at_global_opt_freq", last=50 - 15),
]


def loop_window(c):
    """(j0, nj, lo, nf) of a case, or None when PatchGraph.edges_loop has
    nothing to look at (l <= 0, no target frame, or its caller's gate)."""
    n = c["n"]
    if c["last"] is not None and n - c["last"] < c["gof"]:
        return None
    l = n - c["rw"]
    nj = max(c["gof"] - c["ki"], 0)
    if l <= 0 or nj == 0:
        return None
    lo = max(l - c["age"], 0)
    return n - c["gof"], nj, lo, l - lo


def _loop_groups(c, poses, pts, intr, ix):
    """the per-group values exactly as oracle.edges_loop forms them, with the
    source / target frame and the valid count of every group"""
    w = loop_window(dict(c, last=None))
    if w is None:
        return None
    j0, nj, lo, nf = w
    M = c["M"]
    J, K = np.meshgrid(np.arange(j0, j0 + nj), np.arange(lo * M, (lo + nf) * M), indexing="ij")
    J, K = J.reshape(-1), K.reshape(-1)
    fl, val = oracle.flow_mag(poses, pts, intr, ix[K], J, K, 0.5, pixel=(1, 1))
    G = len(K) // M
    fl, val = fl.reshape(G, M), val.reshape(G, M)
    s = np.array([oracle._sum_f32(np.where(val[g], fl[g], 0.0)) for g in range(G)], np.float32)
    cnt = val.sum(1)
    cf = cnt.astype(np.float32)
    fm = np.where(cf > M * 0.75, s / np.maximum(cf, np.float32(1)), np.float32(np.inf))
    return {"fm": fm.astype(np.float32), "cnt": cnt, "gi": ix[K[::M]], "gj": J[::M], "ng": G,
            "nj": nj, "nf": nf}


@functools.lru_cache(maxsize=None)
def build_loop(name):
    """Inputs of an edges_loop case, its resolved parameters ("par": the keyword
    arguments both oracle.edges_loop and DevicePatchGraph.edges_loop take), the
    oracle's group values ("groups", None without a window) and its result
    ("kk", "jj", "last_after")."""
    c = next(c for c in LOOP_CASES if c["name"] == name)
    rng = np.random.default_rng(c["seed"])
    M, P, n = c["M"], c["P"], c["n"]
    N = n + 8
    poses, pts, intr = _loop_scene(rng, N, M, P, n, period=c["period"])
    ix = np.repeat(np.arange(N), M).astype(np.int64)
    if c["gate"] is not None:
        # the target frame half a unit behind the source frame along the optical
        # axis, same rotation: Z1 = 1 - d / 2.  d = 0.5: valid; d = 2: Z1 = 0.
        f, j, valid = c["gate"]
        poses[j] = poses[f]
        poses[j, 2] -= np.float32(0.5)
        d = np.where(np.arange(M) < valid, 0.5, 2.0).astype(np.float32)
        pts[f * M:(f + 1) * M, 2] = d[:, None, None]
    if c["tie"] is not None:
        f = c["tie"]
        poses[f + 1] = poses[f]
        pts[(f + 1) * M:(f + 2) * M] = pts[f * M:(f + 1) * M]
    groups = _loop_groups(c, poses, pts, intr, ix)
    par = dict(removal_window=c["rw"], max_edge_age=c["age"], global_opt_freq=c["gof"],
               keyframe_index=c["ki"], backend_thresh=c["thresh"], max_num_edges=c["max_edges"],
               nms=c["nms"])
    if isinstance(c["thresh"], str):
        lo = groups["fm"].min()
        par["backend_thresh"] = float(lo if c["thresh"] == "min" else
                                      np.nextafter(lo, np.float32(np.inf)))
    if c["max_edges"] == "found-1":
        par["max_num_edges"] = 1000
        rk, _ = oracle.edges_loop(poses, pts, intr, ix, n, M, **par)
        par["max_num_edges"] = len(rk) // M - 1
    if loop_window(c) is None:
        rk = rj = np.zeros(0, np.int64)
        groups_written = None
    else:
        rk, rj = oracle.edges_loop(poses, pts, intr, ix, n, M, **par)
        groups_written = groups
    last_after = c["last"]
    if c["last"] is not None and len(rk):
        last_after = n
    return {"case": c, "poses": poses, "patches": pts, "intrinsics": intr, "ix": ix, "N": N,
            "par": par, "groups": groups, "groups_written": groups_written, "kk": rk, "jj": rj,
            "last_after": last_after}
