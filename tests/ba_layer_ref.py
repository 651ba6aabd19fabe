"""Shared by the BA-layer tests: a differentiable torch restatement of the
layer (dpvo_amd.ba.BA, one Gauss-Newton step of dpvo/ba.py BA, B = 1), written
from the formulas and out of place throughout, the Euclidean -> left-tangent
conversion of its pose gradient, and the test cases with their margins.

    G_ij = T_j T_i^-1,  X1 = G_ij ((x-cx)/fx, (y-cy)/fy, 1, d),  proj = K_j X1
    r = target - proj;  open <=> |r| < 250, Z > 0.2, proj strictly inside bounds
    a = [Ji at i-fixedp | Jj at j-fixedp],  z = Jz,  w = open * weight
    B = sum w a a^T, E[:, k] = sum w a z, C_k = sum w z^2, v = sum w a r, u_k = sum w z r
    Q = 1 / (C + lmbda), S = B - E Q E^T, y = v - E Q u, A = S + ep I + 1e-4 diag S
    dX = A^-1 y (0 when the factorisation fails), dZ = Q (u - E^T dX)
    poses[fixedp:n] <- Exp(dX) poses[fixedp:n];  d <- clamp(d + dZ, 1e-3, 10)
"""
import functools

import numpy as np
import torch

INTR = (80.0, 80.0, 80.0, 60.0)
BOUNDS = (0.0, 0.0, 159.0, 119.0)


# ------------------------------------------------------------------ SE3 pieces
def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot(q, p):
    v, w = q[..., :3], q[..., 3:]
    uv = 2 * torch.linalg.cross(v, p)
    return p + w * uv + torch.linalg.cross(v, uv)


def se3_exp(xi):
    """Exp of (tau, phi) -> (t, q); Taylor branch near phi = 0 (no NaN gradient)."""
    tau, phi = xi[..., :3], xi[..., 3:]
    th2 = (phi * phi).sum(-1, keepdim=True)
    small = th2 < 1e-16
    t2 = torch.where(small, torch.ones_like(th2), th2)
    th = t2.sqrt()
    a = torch.where(small, 0.5 - th2 / 24, (1 - th.cos()) / t2)
    b = torch.where(small, 1.0 / 6 - th2 / 120, (th - th.sin()) / (t2 * th))
    im = torch.where(small, 0.5 - th2 / 48, (0.5 * th).sin() / th)
    re = torch.where(small, 1 - th2 / 8, (0.5 * th).cos())
    pt = torch.linalg.cross(phi, tau)
    t = tau + a * pt + b * torch.linalg.cross(phi, pt)
    return torch.cat([t, im * phi, re], -1)


def se3_mul(A, B):
    return torch.cat([A[..., :3] + qrot(A[..., 3:], B[..., :3]), qmul(A[..., 3:], B[..., 3:])], -1)


def act(poses, pts):
    """R p + t of every pose on its own points [N, k, 3]."""
    return qrot(poses[:, None, 3:], pts) + poses[:, None, :3]


def to_tangent(poses, g):
    """Euclidean gradient g [N, 7] of a function of the pose data -> gradient
    in the left tangent (tau, phi) of T' = Exp(xi) T, with the first-order
    perturbation (t + tau + phi x t, q + 1/2 (phi, 0) q)."""
    t, q = poses[:, :3], poses[:, 3:]
    out = [g[:, :3]]
    for a in range(3):
        e = torch.zeros_like(t)
        e[:, a] = 1.0
        dt = torch.linalg.cross(e, t)
        dq = 0.5 * qmul(torch.cat([e, torch.zeros_like(e[:, :1])], -1), q)
        out.append(((g[:, :3] * dt).sum(-1) + (g[:, 3:] * dq).sum(-1))[:, None])
    return torch.cat(out, -1)


# ------------------------------------------------------------------ the layer
def linearise(poses, patches, intr, ii, jj, kk):
    """proj [E, 2], Z [E], Ji / Jj [E, 2, 6], Jz [E, 2] at the patch centre.
    Where Z <= 0.2 (closed whatever else holds) Z is replaced by 1 in the
    divisions, so that the masked values and their gradients stay finite."""
    c = patches.shape[-1] // 2
    x, y, d = patches[kk, 0, c, c], patches[kk, 1, c, c], patches[kk, 2, c, c]
    Ki, Kj = intr[ii], intr[jj]
    X0 = torch.stack([(x - Ki[:, 2]) / Ki[:, 0], (y - Ki[:, 3]) / Ki[:, 1], torch.ones_like(x)], -1)
    Ti, Tj = poses[ii], poses[jj]
    qic = torch.cat([-Ti[:, 3:6], Ti[:, 6:]], -1)
    q = qmul(Tj[:, 3:], qic)
    # T_j * (T_i^-1) as lietorch composes it: two rotations of t_i, which differs from
    # one rotation by q_ij when the stored quaternions are not exactly unit
    t = Tj[:, :3] - qrot(Tj[:, 3:], qrot(qic, Ti[:, :3]))
    X1 = qrot(q, X0) + t * d[:, None]
    X, Y, Z = X1.unbind(-1)
    di = 1.0 / torch.where(Z > 0.2, Z, torch.ones_like(Z))
    fx, fy, cx, cy = Kj.unbind(-1)
    proj = torch.stack([fx * X * di + cx, fy * Y * di + cy], -1)
    o = torch.zeros_like(X)
    a0, c0, b1, c1 = fx * di, -fx * X * di * di, fy * di, -fy * Y * di * di
    Jj = torch.stack([torch.stack([a0 * d, o, c0 * d, c0 * Y, a0 * Z - c0 * X, -a0 * Y], -1),
                      torch.stack([o, b1 * d, c1 * d, c1 * Y - b1 * Z, -c1 * X, b1 * X], -1)], 1)
    qinv = torch.cat([-q[:, :3], q[:, 3:]], -1)[:, None]
    tt = t[:, None].expand(-1, 2, -1)
    Ji = -torch.cat([qrot(qinv, Jj[..., :3]),
                     qrot(qinv, torch.linalg.cross(Jj[..., :3], tt) + Jj[..., 3:])], -1)
    Jz = torch.stack([a0 * t[:, 0] + c0 * t[:, 2], b1 * t[:, 1] + c1 * t[:, 2]], -1)
    return proj, Z, Ji, Jj, Jz


def gates(proj, Z, targets, bounds):
    """The four gate groups as booleans [E] each: residual, depth, x / y bounds."""
    r = targets - proj
    return {"r": r.norm(dim=-1) < 250, "z": Z > 0.2, "x0": proj[:, 0] > bounds[0],
            "y0": proj[:, 1] > bounds[1], "x1": proj[:, 0] < bounds[2], "y1": proj[:, 1] < bounds[3]}


def ba_layer(poses, patches, intr, targets, weights, lmbda, ii, jj, kk, bounds=BOUNDS, ep=100.0,
             fixedp=1, structure_only=False, n=None, constant_jacobians=False):
    """-> (poses', patches', aux) with aux = dict(dX, dZ, failed, open).
    poses [N, 7], patches [M, 3, p, p], intr [N, 4], targets / weights [E, 2].
    constant_jacobians: the (wrong) gradient that treats Ji / Jj / Jz as
    constants, to show that a test can tell the difference."""
    N, M, E = poses.shape[0], patches.shape[0], ii.numel()
    n = int(max(ii.max(), jj.max())) + 1 if n is None else n
    nf = 0 if structure_only else max(n - fixedp, 0)
    proj, Z, Ji, Jj, Jz = linearise(poses, patches, intr, ii, jj, kk)
    if constant_jacobians:
        Ji, Jj, Jz = Ji.detach(), Jj.detach(), Jz.detach()
    with torch.no_grad():
        g = gates(proj, Z, targets, bounds)
        op = functools.reduce(torch.logical_and, g.values()).to(poses.dtype)
    r = op[:, None] * (targets - proj)
    w = op[:, None] * weights
    Pk = torch.nn.functional.one_hot(kk, M).to(poses.dtype)
    C = torch.einsum("ec,ec,ec,em->m", w, Jz, Jz, Pk)
    u = torch.einsum("ec,ec,ec,em->m", w, Jz, r, Pk)
    Q = 1.0 / (C + lmbda)
    failed = False
    if nf > 0:
        def hot(idx):
            f = idx - fixedp
            return (torch.nn.functional.one_hot(f.clamp(min=0), nf) * (f >= 0)[:, None]).to(poses.dtype)

        a = (torch.einsum("en,ecd->ecnd", hot(ii), Ji) + torch.einsum("en,ecd->ecnd", hot(jj), Jj))
        a = a.reshape(E, 2, 6 * nf)
        B = torch.einsum("ec,eca,ecb->ab", w, a, a)
        Em = torch.einsum("ec,eca,ec,em->am", w, a, Jz, Pk)
        v = torch.einsum("ec,eca,ec->a", w, a, r)
        S = B - (Em * Q) @ Em.T
        y = v - Em @ (Q * u)
        A = S + torch.diag_embed(ep + 1e-4 * torch.diagonal(S))
        L, info = torch.linalg.cholesky_ex(A)
        failed = bool(info.item())
        if failed:
            dX = torch.zeros(6 * nf, dtype=poses.dtype)
        else:
            dX = torch.cholesky_solve(y[:, None], L)[:, 0]
        dZ = Q * (u - Em.T @ dX)
    else:
        dX = torch.zeros(0, dtype=poses.dtype)
        dZ = Q * u
    disp = (patches[:, 2] + dZ[:, None, None])
    new_patches = torch.stack([patches[:, 0], patches[:, 1], disp.clamp(1e-3, 10.0)], 1)
    new_poses = poses
    if nf > 0 and not failed:
        new_poses = torch.cat([poses[:fixedp], se3_mul(se3_exp(dX.view(nf, 6)), poses[fixedp:n]),
                               poses[n:]], 0)
    aux = {"dX": dX.view(-1, 6), "dZ": dZ, "failed": failed, "open": op.bool(), "gates": g,
           "pre_clamp": disp.detach(), "proj": proj.detach(), "Z": Z.detach(),
           "rnorm": (targets - proj).norm(dim=-1).detach()}
    return new_poses, new_patches, aux


# ------------------------------------------------------------------ cases
class Case:
    def __init__(self, name, poses, patches, intr, targets, weights, ii, jj, kk, fixedp=1,
                 structure_only=False, ep=10.0, lmbda=1e-4, bounds=BOUNDS):
        self.name = name
        self.poses, self.patches, self.intr = poses, patches, intr
        self.targets, self.weights = targets, weights
        self.ii, self.jj, self.kk = ii, jj, kk
        self.fixedp, self.structure_only, self.ep, self.lmbda = fixedp, structure_only, ep, lmbda
        self.bounds = bounds
        self.n = int(max(ii.max(), jj.max())) + 1

    def replace(self, name, **kw):
        d = dict(poses=self.poses, patches=self.patches, intr=self.intr, targets=self.targets,
                 weights=self.weights, ii=self.ii, jj=self.jj, kk=self.kk, fixedp=self.fixedp,
                 structure_only=self.structure_only, ep=self.ep, lmbda=self.lmbda,
                 bounds=self.bounds)
        d.update(kw)
        return Case(name, **d)

    def run(self, dtype=torch.float64, **over):
        t = lambda x: x.to(dtype)  # noqa: E731
        return ba_layer(t(self.poses), t(self.patches), t(self.intr), t(self.targets),
                        t(self.weights), self.lmbda, self.ii, self.jj, self.kk, self.bounds,
                        self.ep, self.fixedp, self.structure_only, over.get("n", self.n))


def margins(case):
    """Distance of every edge from every gate and of every depth from the
    clamp limits, in fp64: (gate margin ok, clamp margin ok)."""
    _, _, aux = case.run()
    rn, Z, pr = aux["rnorm"], aux["Z"], aux["proj"]
    b = case.bounds
    ok = ((rn - 250).abs() > 250e-3) & ((Z - 0.2).abs() > 0.2e-3)
    for col, lim in ((0, b[0]), (1, b[1]), (0, b[2]), (1, b[3])):
        ok &= (pr[:, col] - lim).abs() > 1e-3
    pc = aux["pre_clamp"]
    clamp_ok = ((pc - 1e-3).abs() > 1e-6) & ((pc - 10.0).abs() > 1e-6)
    # an edge closed by Z <= 0.2 has no meaningful projection: only its Z margin counts
    zclosed = Z <= 0.2
    ok = torch.where(zclosed, (Z - 0.2).abs() > 0.2e-3, ok)
    return bool(ok.all()), bool(clamp_ok.all())


def _trajectory(N, g):
    xi = torch.zeros(N, 6, dtype=torch.float64)
    xi[:, 2] = 0.05 * torch.arange(N, dtype=torch.float64)
    xi += 0.02 * torch.randn(N, 6, generator=g, dtype=torch.float64)
    return se3_exp(xi)


def _random(name, N, M, E, p, seed, ii=None, jj=None, kk=None, noise=0.3, **kw):
    """Poses on a forward trajectory, patch centres inside the image, every
    patch anchored in a frame of its own, targets = projection + noise.  The
    seed is advanced until the margins hold (deterministic)."""
    for s in range(seed, seed + 50):
        g = torch.Generator().manual_seed(s)
        poses = _trajectory(N, g)
        src = torch.randint(0, N, (M,), generator=g)
        c = p // 2
        off = torch.arange(p, dtype=torch.float64) - c
        patches = torch.zeros(M, 3, p, p, dtype=torch.float64)
        patches[:, 0] = (torch.rand(M, generator=g, dtype=torch.float64) * 120 + 20).view(-1, 1, 1) + off.view(1, 1, p)
        patches[:, 1] = (torch.rand(M, generator=g, dtype=torch.float64) * 80 + 20).view(-1, 1, 1) + off.view(1, p, 1)
        patches[:, 2] = (torch.rand(M, generator=g, dtype=torch.float64) * 0.8 + 0.4).view(-1, 1, 1)
        k = torch.randint(0, M, (E,), generator=g) if kk is None else kk
        i = src[k] if ii is None else ii
        j = torch.randint(0, N, (E,), generator=g) if jj is None else jj
        if jj is None:
            j[0], j[-1] = N - 1, 0  # n = N whatever the draw
        intr = torch.tensor(INTR, dtype=torch.float64).repeat(N, 1)
        proj = linearise(poses, patches, intr, i, j, k)[0]
        targets = proj + noise * torch.randn(E, 2, generator=g, dtype=torch.float64)
        weights = 0.1 + 0.9 * torch.rand(E, 2, generator=g, dtype=torch.float64)
        case = Case(name, poses, patches, intr, targets, weights, i.long(), j.long(), k.long(), **kw)
        if all(margins(case)):
            return case
    raise AssertionError(f"no seed gives case {name} its margins")


@functools.lru_cache(maxsize=None)
def case(name):
    L = torch.tensor
    if name in ("a_p1", "a_p3"):
        return _random(name, 2, 1, 1, int(name[-1]), 1, ii=L([0]), jj=L([1]), kk=L([0]))
    if name == "b":
        # duplicated (kk, jj) = (1, 2); ii == jj on edge 2; edge 3 between the fixed poses 0, 1;
        # patch 4 has no edge; kk unsorted
        return _random(name, 3, 5, 7, 3, 2, ii=L([0, 0, 2, 0, 1, 2, 1]), jj=L([2, 2, 2, 1, 2, 0, 0]),
                       kk=L([3, 1, 1, 0, 2, 3, 1]), fixedp=2)
    if name.startswith("c_"):
        return _random(name, 5, 13, int(name[2:]), 3, 3)
    if name.startswith("d_"):
        return fixture_case(name[2:])
    if name == "e":
        return gate_case()
    if name.startswith("f_"):
        tag = name[2:]
        base = _random(name, 5, 11, 40, 3, 4)
        if tag == "so":
            return base.replace(name, structure_only=True)
        return base.replace(name, fixedp=int(tag))
    if name == "g":
        return _random(name, 24, 50, 600, 3, 5)  # 6 * 23 = 138 <= 142: the largest in-LDS fp64 solve
    if name == "h":
        return _random(name, 5, 13, 65, 3, 3).replace(name, ep=-1e6)
    if name.startswith("w_"):
        return window_case(name, int(name[2:]))
    raise KeyError(name)


def unit(poses):
    """Quaternions renormalised in fp64.  The fixtures and synthetic graphs
    store fp32 poses, unit to 6e-8 only; lietorch normalises a quaternion when
    it loads one (so the layer's retraction does), the restatement and
    cpu_baseline.ba_step do not.  On unit input the two agree to rounding."""
    return torch.cat([poses[:, :3], poses[:, 3:] / poses[:, 3:].norm(dim=-1, keepdim=True)], -1)


def fixture_case(fx):
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fx + ".npz"))
    t = lambda k: torch.from_numpy(np.asarray(z[k])).double()  # noqa: E731
    cx, cy = float(z["intrinsics"][0, 2]), float(z["intrinsics"][0, 3])
    N = t("poses").shape[0]
    return Case("d_" + fx, unit(t("poses")), t("patches"), t("intrinsics")[:1].repeat(N, 1), t("target"),
                t("weight"), torch.from_numpy(z["ii"]).long(), torch.from_numpy(z["jj"]).long(),
                torch.from_numpy(z["kk"]).long(), fixedp=int(z["t0"]), ep=1.0,
                bounds=(-64.0, -64.0, 2 * cx + 64.0, 2 * cy + 64.0))


def window_case(name, n_free, fixedp=4):
    """synthetic.make_dpvo_window (DPVO's own edge pattern, M = 6 patches a
    frame, lifetime 8: a few thousand edges) with n_free free poses behind
    `fixedp` fixed ones.  6 n_free = 96: the pose system factors in LDS above
    64 KB; 144: in the workspace in HBM, where the backward's solve reads the
    factor.  The seed is advanced until the margins hold (deterministic)."""
    from dpvo_amd.synthetic import make_dpvo_window

    for seed in range(50):
        G = make_dpvo_window(n=n_free + fixedp, M=6, lifetime=8, seed=seed)
        c = Case(name, unit(G.poses.double()), G.patches.double(), G.intrinsics.double(),
                 G.target.double(), G.weight.double(), G.ii, G.jj, G.kk, fixedp=fixedp, ep=100.0)
        assert c.n == n_free + fixedp
        if all(margins(c)):
            return c
    raise AssertionError(f"no seed gives case {name} its margins")


WINDOW_CASES = ["w_16", "w_24"]  # 6 n_free = 96 (LDS above 64 KB), 144 (HBM)


def permuted(c, seed=11):
    """The case with its edges under one fixed permutation -> (case, perm):
    the same sums in another order."""
    perm = torch.randperm(c.ii.numel(), generator=torch.Generator().manual_seed(seed))
    cp = c.replace(c.name + "_perm", ii=c.ii[perm], jj=c.jj[perm], kk=c.kk[perm],
                   targets=c.targets[perm], weights=c.weights[perm])
    cp.n = c.n
    return cp, perm


GATE_BOUNDS = (25.0, 20.0, 135.0, 100.0)


def gate_case():
    """synthetic.make_graph with every gate exercised: a residual outlier, a
    patch so near that Z <= 0.2 on some edges, bounds inside the image, a patch
    whose edges are all closed, and depths that end on both clamp limits."""
    from dpvo_amd.synthetic import make_graph

    for seed in range(50):
        G = make_graph(5, 8, 100, seed=seed)
        tg, pt = G.target.double().clone(), G.patches.double().clone()
        tg[0] += 400.0                      # |r| >= 250
        dead = int(G.kk[50])
        tg[G.kk == dead] += 400.0           # every edge of this patch closed: dZ = 0
        pt[dead, 2] = 1e-4                  # ... and its depth ends on the lower limit
        cand = G.kk[(G.ii == 4) & (G.jj < 3)]
        if not len(cand):
            continue
        near = int(cand[0])
        if near == dead or int(G.kk[0]) in (dead, near):
            continue
        pt[near, 2] = 12.0                  # Z = 1 + t_z d <= 0.2 towards earlier frames; ends on 10
        c = Case("e", unit(G.poses.double()), pt, G.intrinsics.double(), tg, G.weight.double(), G.ii, G.jj,
                 G.kk, fixedp=1, bounds=GATE_BOUNDS)
        if all(margins(c)) and gate_content(c)["ok"]:
            return c
    raise AssertionError("no seed gives the gate case its content")


def gate_content(c):
    _, newp, aux = c.run()
    g = aux["gates"]
    only = {k: int((~v).sum()) for k, v in g.items()}
    dead = [k for k in c.kk.unique().tolist() if not aux["open"][c.kk == k].any()]
    d = newp[:, 2, 1, 1]
    res = {"closed_by": only, "all_closed_patches": len(dead), "at_lo": int((d == 1e-3).sum()),
           "at_hi": int((d == 10.0).sum()), "open": int(aux["open"].sum())}
    res["ok"] = (all(v >= 1 for v in only.values()) and len(dead) >= 1 and res["at_lo"] >= 1
                 and res["at_hi"] >= 1 and res["open"] >= 20)
    return res


GPU_CASES = ["a_p1", "a_p3", "b", "c_63", "c_64", "c_65", "c_257", "d_ba_py_a", "d_ba_py_b", "e",
             "f_0", "f_1", "f_2", "f_5", "f_so", "g", "h"]


# ------------------------------------------------------------------ a loss both sides can take
def cotangents(c, seed=7):
    g = torch.Generator().manual_seed(seed)
    N, M, p = c.poses.shape[0], c.patches.shape[0], c.patches.shape[-1]
    return {"pts": torch.randn(N, 3, 3, generator=g, dtype=torch.float64),
            "cP": torch.randn(N, 3, 3, generator=g, dtype=torch.float64),
            "cK": torch.randn(M, 3, p, p, generator=g, dtype=torch.float64)}


def ref_grads(c, cot, dtype=torch.float64, chain=1, constant_jacobians=False):
    """Outputs and the four gradients of L = <cP, T' pts> + <cK, patches'> of
    the restatement (chain = 2: two calls sharing targets / weights).  The pose
    gradient is returned in the left tangent."""
    P, K, T, W = (x.to(dtype).clone().requires_grad_() for x in
                  (c.poses, c.patches, c.targets, c.weights))
    intr = c.intr.to(dtype)
    p, k = P, K
    for _ in range(chain):
        p, k, aux = ba_layer(p, k, intr, T, W, c.lmbda, c.ii, c.jj, c.kk, c.bounds, c.ep, c.fixedp,
                             c.structure_only, c.n, constant_jacobians)
    loss =(cot["cP"].to(dtype) * act(p, cot["pts"].to(dtype))).sum() + (cot["cK"].to(dtype) * k).sum()
    gP, gK, gT, gW = torch.autograd.grad(loss, (P, K, T, W), allow_unused=True)
    z = lambda g, x: torch.zeros_like(x) if g is None else g  # noqa: E731
    return {"poses": p.detach(), "patches": k.detach(), "g_poses": to_tangent(P.detach(), z(gP, P)),
            "g_patches": z(gK, K), "g_targets": z(gT, T), "g_weights": z(gW, W), "aux": aux}
