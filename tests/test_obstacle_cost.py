"""Per-instance obstacle-avoidance costs (DDP_HIP_FLAG_OBSTACLE_COST, include/ddp_hip/ddp_hip.h): collision spheres on the robot
(point k: off_k fixed in joint_k, radius r_k, world position p_k(q)) against per-instance obstacle slots,

    sphere      geom = (c, rho):  d_ko = |p_k - c| - (r_k + rho),   u_ko = (p_k - c) / |p_k - c|
    half-space  geom = (n, h):    d_ko = n . p_k - h - r_k,         u_ko = n
    l(t, x, u) += 1/2 sum_k sum_o w[b][t][o] e_ko^2,   lf alike at T,   e_ko = d_ko < 0 ? d_ko : 0

The oracle has no such cost, so the yardstick is the numpy restatement below, built on Oracle.frame_position and
Oracle.frame_jacobian(world_aligned=True): z_ko = P_k^T u_ko, lx += w e z, lxx += w z z^T over the pairs with w != 0 and e != 0.
The helpers of test_tracking_cost.py, test_frame_cost.py, test_state_limits.py, test_com_cost.py and test_frame_vel_cost.py are
reused by import; tolerances are theirs.

The task generator places every slot relative to a chosen point on the trajectory, which then penetrates by 0.01 .. 0.1 or stays
clear by as much; check_task asserts on the yardstick alone that no live pair sits within 1e-6 of the surface (or, for a sphere,
within 1e-3 of the centre), so that device and numpy cannot disagree about which pairs are active."""
import os
import re

import numpy as np
import pytest

import test_com_cost as cm
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_frame_vel_cost as fv
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = fc.DERIVS
NAMES = fc.NAMES
SPHERE, HALFSPACE = 0, 1
make_any = cm.make_any
_trajs, _setup = tc._trajs, tc._setup
RADII = (0.05, 0.0, 0.08, 0.03, 0.06)
KINDS = (SPHERE, HALFSPACE, SPHERE)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def pick_points(model, n=5):
    """the four frames of fc.pick_frames (a root-side joint, a mid-tree joint, two leaves) and a second point on the mid-tree
    joint, each (joint, off, radius); one radius is 0"""
    fr = fc.pick_frames(model, 4)
    pts = [(j, off) for j, off in fr] + [(fr[1][0], (0.06, 0.02, -0.11))]
    return [(j, off, RADII[k]) for k, (j, off) in enumerate(pts)][:n]


def pair(kind, g, p, r):
    """(d_ko, u_ko) of one pair; u is None at a sphere's centre"""
    if kind == HALFSPACE:
        return float(g[:3] @ p - g[3] - r), np.asarray(g[:3], dtype=float)
    diff = p - g[:3]
    dist = float(np.sqrt(diff @ diff))
    return dist - (r + g[3]), (diff / dist if dist != 0.0 else None)


def positions(o, pts, q):
    return [o.frame_position(j, off, q) for j, off, _ in pts]


def ob_term(o, pts, kinds, q, geom_t, w_t):
    """1/2 sum_k sum_o w e^2 at one configuration, the points then the slots in ascending order; and whether a pair is active"""
    total, active = 0.0, False
    for k, p in enumerate(positions(o, pts, q)):
        s, act = 0.0, False
        for s_, kind in enumerate(kinds):
            if w_t[s_] == 0.0:
                continue
            d, _ = pair(kind, geom_t[s_], p, pts[k][2])
            if d < 0:
                s += w_t[s_] * d * d
                act = True
        if act:
            total += 0.5 * s
            active = True
    return total, active


def ob_terms(o, pts, kinds, xs, geom, w):
    """the obstacle terms of one instance per t (T+1 values; the last belongs to lf); geom (T+1, n_obs, 4), w (T+1, n_obs)"""
    X = xs.reshape(o.T + 1, o.nx)
    return np.array([ob_term(o, pts, kinds, X[t][:o.nq], geom[t], w[t])[0] for t in range(o.T + 1)])


def ob_clearance(o, pts, kinds, xs, geom, w):
    """min over points and live slots of d_ko per t; +inf where no slot is live"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.full(o.T + 1, np.inf)
    for t in range(o.T + 1):
        for k, p in enumerate(positions(o, pts, X[t][:o.nq])):
            for s_, kind in enumerate(kinds):
                if w[t][s_] != 0.0:
                    out[t] = min(out[t], pair(kind, geom[t][s_], p, pts[k][2])[0])
    return out


def ob_grad_hess(o, model, pts, kinds, x, geom_t, w_t):
    """(lx, lxx) contributions at one state, n and n x n, and the tangent rows of the active points' paths (a mask over n):
    sum w e z and the Gauss-Newton sum w z z^T on the q rows, over the pairs with w != 0 and e != 0"""
    nv, n = o.nv, o.n
    g, Hm, rows = np.zeros(n), np.zeros((n, n)), np.zeros(n, dtype=bool)
    q = x[:o.nq]
    for k, (j, off, r) in enumerate(pts):
        p = o.frame_position(j, off, q)
        P = None
        for s_, kind in enumerate(kinds):
            if w_t[s_] == 0.0:
                continue
            d, u = pair(kind, geom_t[s_], p, r)
            if not d < 0 or u is None:
                continue
            if P is None:
                P = o.frame_jacobian(j, off, q, world_aligned=True)
                for i in fv.path_of(model, j):
                    rows[fv.cols_of(model, i)] = True
            z = P.T @ u
            g[:nv] += w_t[s_] * d * z
            Hm[:nv, :nv] += w_t[s_] * np.outer(z, z)      # entry (i, j) and (j, i) alike: symmetric bit for bit
    return g, Hm, rows


def ob_derivs(o, model, pts, kinds, xs, geom, w):
    """what the obstacle terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout, and the
    active rows per t"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": [], "rows": []}
    for t in range(o.T + 1):
        g, Hm, rows = ob_grad_hess(o, model, pts, kinds, X[t], geom[t], w[t])
        out["rows"].append(rows)
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def random_task(o, pts, kinds, xs, B, seed, wscale=1.0, p_clear=0.5):
    """geom (B, T+1, n_obs, 4) and weights (B, T+1, n_obs).  Per (instance, t): with probability p_clear a block that nothing
    touches (every slot clear of its chosen point by 0.01 .. 0.1 and of every other point by more), else a block in which each
    slot's chosen point penetrates by 0.01 .. 0.1 (at least one slot) or stays clear by as much, the other points falling where
    they fall"""
    rng = np.random.default_rng(seed)
    T, no = o.T, len(kinds)
    geom, w = np.zeros((B, T + 1, no, 4)), wscale * rng.uniform(0.5, 5.0, size=(B, T + 1, no))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            P = positions(o, pts, X[t][:o.nq])
            clear_block = rng.uniform() < p_clear
            forced = int(rng.integers(no))
            for s_, kind in enumerate(kinds):
                k = int(rng.integers(len(pts)))
                depth = rng.uniform(0.01, 0.1)
                inside = (not clear_block) and (s_ == forced or rng.uniform() < 0.6)
                sd = -depth if inside else depth                                # the chosen point's signed distance
                for _ in range(200):
                    if kind == HALFSPACE:
                        n = _unit(rng)
                        if clear_block:                                          # the chosen point: the one nearest the plane
                            k = int(np.argmin([n @ P[i] - pts[i][2] for i in range(len(pts))]))
                        g = np.concatenate([n, [n @ P[k] - pts[k][2] - sd]])
                    else:
                        rho = rng.uniform(0.15, 0.3)
                        g = np.concatenate([P[k] - _unit(rng) * (sd + pts[k][2] + rho), [rho]])
                    ds = [pair(kind, g, P[i], pts[i][2])[0] for i in range(len(pts))]
                    if not clear_block or min(ds) >= min(depth, 0.01) - 1e-12:
                        break
                else:
                    raise AssertionError("no clear placement found")
                geom[b, t, s_] = g
    return geom, w


def check_task(o, pts, kinds, xs, geom, w, fractions=True):
    """the conditions on the inputs, on the yardstick alone: every live pair is at least 1e-6 off the surface and, for a sphere,
    1e-3 off the centre; at least a quarter of the (instance, t) blocks have an active pair and at least a quarter have none.
    Returns the blocks' activity (B, T+1)"""
    B, T = xs.shape[0], o.T
    active = np.zeros((B, T + 1), dtype=bool)
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for k, p in enumerate(positions(o, pts, X[t][:o.nq])):
                for s_, kind in enumerate(kinds):
                    if w[b, t, s_] == 0.0:
                        continue
                    d, _ = pair(kind, geom[b, t, s_], p, pts[k][2])
                    assert abs(d) >= 1e-6, (b, t, k, s_, d)
                    if kind == SPHERE:
                        assert np.linalg.norm(p - geom[b, t, s_, :3]) >= 1e-3, (b, t, k, s_)
                    active[b, t] |= d < 0
    if fractions:
        assert 4 * active.sum() >= active.size and 4 * (~active).sum() >= active.size, (active.sum(), active.size)
    return active


def set_task(ctx, pts, kinds, geom=None, weight=None):
    ctx.set_obstacle_points(points=pts, kinds=kinds)
    if geom is not None or weight is not None:
        ctx.set_obstacle_cost(geom=geom, weight=weight)


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
W5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))


@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff", "table7"])
def test_yardstick_gradient(name):
    """z_ko = P_k^T u_ko against the 5-point central difference of d_ko along x (+) (+-h e_j), for both kinds and every point;
    lx against the central difference of the term at states with active pairs; lxx symmetric bit for bit with zero velocity
    rows and columns"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    pts = pick_points(model)
    xs, us = _trajs(o, model, 1, 3)
    geom, w = random_task(o, pts, KINDS, xs, 1, 4, p_clear=0.0)
    check_task(o, pts, KINDS, xs, geom, w, fractions=False)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    for t in (1, T):
        q = X[t][:o.nq]
        for k, (j, off, r) in enumerate(pts):
            P = o.frame_jacobian(j, off, q, world_aligned=True)
            for s_, kind in enumerate(KINDS):
                d0, u = pair(kind, geom[0, t, s_], o.frame_position(j, off, q), r)
                z = P.T @ u
                fd = np.zeros(nv)
                for c in range(nv):
                    e = np.zeros(nv); e[c] = H
                    fd[c] = sum(cw * pair(kind, geom[0, t, s_], o.frame_position(j, off, o.integrate(q, s * e)), r)[0] for s, cw in W5) / H
                assert np.max(np.abs(fd - z)) <= 1e-8 * max(1.0, np.max(np.abs(z))), (k, s_, np.max(np.abs(fd - z)))
        g, Hm, rows = ob_grad_hess(o, model, pts, KINDS, X[t], geom[0, t], w[0, t])
        assert np.max(np.abs(g[:nv])) > 0 and rows.any()

        def cost_at(dx):
            return ob_term(o, pts, KINDS, tc._integrate_x(o, X[t], dx)[:o.nq], geom[0, t], w[0, t])[0]
        fd = np.zeros(n)
        for c in range(n):
            e = np.zeros(n); e[c] = H
            fd[c] = sum(cw * cost_at(s * e) for s, cw in W5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        assert np.array_equal(Hm, Hm.T)
        assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(g[nv:] == 0.0)
        assert np.all(g[~rows] == 0.0) and np.all(Hm[~rows, :] == 0.0)
        assert np.min(np.linalg.eigvalsh(Hm)) >= -1e-12 * np.max(np.abs(Hm))


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_OBSTACLE_COST == 512 and re.search(r"#define\s+DDP_HIP_FLAG_OBSTACLE_COST\s+512u", header)
    assert capi.MAX_COLLISION_POINTS == 16 and re.search(r"#define\s+DDP_HIP_MAX_COLLISION_POINTS\s+16\b", header)
    assert capi.MAX_OBSTACLES == 8 and re.search(r"#define\s+DDP_HIP_MAX_OBSTACLES\s+8\b", header)
    assert capi.OBSTACLE_SPHERE == 0 and re.search(r"#define\s+DDP_HIP_OBSTACLE_SPHERE\s+0\b", header)
    assert capi.OBSTACLE_HALFSPACE == 1 and re.search(r"#define\s+DDP_HIP_OBSTACLE_HALFSPACE\s+1\b", header)
    L = capi.lib()
    for name in ("ddp_hip_obstacle_set_points", "ddp_hip_obstacle_upload", "ddp_hip_obstacle_download", "ddp_hip_obstacle_clearance"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    for name in ("set_obstacle_points", "set_obstacle_cost", "obstacle_cost", "obstacle_clearance"):
        assert hasattr(capi.Context, name), name
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B, no = 5, 2, 3
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h, ctx.n_obstacles = spec, B, None, no
    ctx.n_obstacles = 0
    with pytest.raises(ValueError, match="set_obstacle_points"):
        ctx.set_obstacle_cost(weight=np.zeros(no))
    ctx.n_obstacles = no
    for kw in (dict(geom=np.zeros((no, 3))), dict(geom=np.zeros(4)), dict(geom=0.0), dict(geom=np.zeros((T, no, 4))),
               dict(geom=np.zeros((B + 1, T + 1, no, 4))), dict(geom=np.zeros((T + 1, no + 1, 4))),
               dict(weight=np.zeros(no + 1)), dict(weight=0.0), dict(weight=np.zeros((T, no))),
               dict(weight=np.zeros((B, T + 1, no)), count=1), dict(weight=np.zeros((T + 1, no, 4))),
               dict(geom=np.zeros((no, 4)), weight=np.zeros((T + 1, no + 1)))):
        with pytest.raises(ValueError):
            ctx.set_obstacle_cost(**kw)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("table7", 2, None, ""), ("tree38", 2, None, "all")]


def _lin_task(o, model, xs, B, T):
    pts = pick_points(model)
    geom, w = random_task(o, pts, KINDS, xs, B, 43)
    w[1, 2, 1] = 0.0; w[0, T, 2] = 0.0; w[2, 3, 0] = 0.0   # one slot's weight off at single (instance, t) entries
    return pts, geom, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different obstacles per instance,
    5 points (one of radius 0) and 3 slots of mixed kinds, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST);
    LXX / LFXX symmetric bit for bit; LU, LUU, LUX, every velocity row and column and the q rows off the active points' paths
    bit for bit the flag-off values; blocks without an active pair bit for bit flag-off, blocks with one differ.  "all":
    tracking, frame positions, orientations and velocities, state limits and the CoM cost live beside it"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    pts, geom, w = _lin_task(o, model, xs, B, T)
    active = check_task(o, pts, KINDS, xs, geom, w)
    frames = fc.pick_frames(model, 3)
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "all":
        base |= (capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_FRAME_VEL_COST
                 | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST)
        ref = tc.random_ref(o, model, xs, us, B, 44)
        ftask = fc.random_task(o, xs, frames, B, 45)
        otask = fo.random_orient(o, xs, frames, B, 47)
        vtask = fv.random_task(o, xs, frames, B, 49)
        lim = sl.random_limits(o, xs, B, 46)
        ctask = cm.random_task(o, model, xs, B, 48)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_OBSTACLE_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "all":
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(frames=frames, target=ftask[0], weight=ftask[1])
                ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
                ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
            if on:
                set_task(ctx, pts, KINDS, geom, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = ob_derivs(o, model, pts, KINDS, xs[b], geom[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert s in ("LFX", "LFXX") or np.max(np.abs(add[s])) > 0
            e = rel_err(got[True][s][b], ex)
            worst = max(worst, e)
            assert e <= 1e-12, (s, b, e)
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T + 1):
            key, k = ("LXX", t) if t < T else ("LFXX", 0)
            blk = got[True][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            off = got[False][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            gk, go = ("LX", t) if t < T else ("LFX", 0)
            gon, goff = got[True][gk][b][go * n:(go + 1) * n], got[False][gk][b][go * n:(go + 1) * n]
            rows = add["rows"][t]
            assert rows.any() == active[b, t] and not rows[nv:].any()
            assert np.array_equal(blk, blk.T)
            assert np.array_equal(blk[~rows, :], off[~rows, :]) and np.array_equal(blk[:, ~rows], off[:, ~rows])
            assert np.array_equal(gon[~rows], goff[~rows])
            if active[b, t]:
                assert not np.array_equal(blk, off) and not np.array_equal(gon, goff)
            else:
                assert np.array_equal(blk, off) and np.array_equal(gon, goff)
    print("linearize", name, flags, stages, "worst", worst, "active blocks", int(active.sum()), "of", active.size)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None), ("tree38_frame", 0, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo_):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the flag-off context's values plus the numpy obstacle terms, lf included;
    a block without an active pair keeps the flag-off value bit for bit"""
    capi = gpu
    T, B, mu = 6, 3, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    pts = pick_points(model)
    geom, w = random_task(o, pts, KINDS, xs, B, 52)
    w[1, 3, 0] = 0.0
    active = check_task(o, pts, KINDS, xs, geom, w)
    active2 = check_task(o, pts, KINDS, xs2, geom, w, fractions=False)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (capi.FLAG_OBSTACLE_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                set_task(ctx, pts, KINDS, geom, w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, X, act in ((0, xs, active), (1, xs2, active2)):
        for b in range(B):
            add = ob_terms(o, pts, KINDS, X[b], geom[b], w[b])
            ex = got[False][which][b] + add
            assert np.any(add != 0.0) and np.array_equal(add != 0.0, act[b])
            e = rel_err(got[True][which][b], ex)
            print("cost_seq_aug", name, which, b, e)
            assert e <= 1e-12, (which, b, e)
            assert np.array_equal(got[True][which][b][~act[b]], got[False][which][b][~act[b]])


def _far_task(B, T):
    """two slots 10 m away from any robot here: a sphere and a half-space whose free side holds the robot"""
    geom = np.zeros((B, T + 1, 2, 4))
    geom[..., 0, :] = (10.0, -10.0, 10.0, 0.5)
    geom[..., 1, :] = (0.0, 0.0, 1.0, -10.0)
    return (SPHERE, HALFSPACE), geom, np.full((B, T + 1, 2), 50.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,extra,fwd_path", [
    ("tree38", 24, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("tree38", 24, 2, None, "box", 1),
])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "far"])
def test_untouched_obstacles_change_nothing(gpu, name, T, fd_mode, fo_, extra, fwd_path, mode):
    """flag on with nothing uploaded, with obstacles in the way but every weight 0, and with non-zero weights on obstacles 10 m
    away (the obstacle kernels run and find no active pair): linearise, both costs, sweep and forward are bit for bit what the
    flag-off context computes, on both forward paths"""
    capi = gpu
    mu, B = 10.0, 2
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    pts = pick_points(model)
    if mode == "far":
        kinds, geom, w = _far_task(B, T)
        assert np.min([ob_clearance(o, pts, kinds, xs[b], geom[b], w[b]) for b in range(B)]) > 5.0
    else:
        kinds = KINDS
        geom, w = random_task(o, pts, kinds, xs, B, 33)
        w[:] = 0.0
    base = capi.FLAG_TRACE | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_OBSTACLE_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if on and mode != "nothing":
                set_task(ctx, pts, kinds, geom, w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
            if on and mode == "far":
                assert np.min(ctx.obstacle_clearance(1)) > 5.0              # the accepted candidate stayed away as well
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
def test_solve_with_far_obstacles_changes_nothing(gpu):
    """ddp_hip_solve with non-zero weights on obstacles 10 m away: the log and the result are bit for bit the flag-off solve's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 4, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 101, held=True)
    pts = pick_points(model)
    kinds, geom, w = _far_task(B, T)
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST if on else 0) as ctx:
            _setup(ctx, xs, us)
            if on:
                set_task(ctx, pts, kinds, geom, w)
            log = solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
            res[on] = (log, ctx.download("X"), ctx.download("U"))
    assert not np.array_equal(res[True][1], xs)
    assert np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(res[False][0][k]), np.asarray(res[True][0][k])), k


def _emulate_forward(o, xs, us, mults, fb, mu, n_alpha, cost):
    """sequential halving with the full numpy cost: the first step 2^-k with sum_t (new - old) <= 0 (n_alpha = 0: the full step).
    Returns the step, the rollout, sum(new - old) and, of every candidate tried, |sum(new - old)| over the sum of the cost terms'
    magnitudes: how far each decision is from the rounding of another order of additions"""
    old = cost(xs, us)
    margins = []
    for k in range(34):
        step = 2.0 ** -k
        _, xn, un = o.forward_alpha(step, xs, us, mults, fb, mu)
        new = cost(xn, un)
        diff = new.sum() - old.sum()
        margins.append(abs(diff) / (np.sum(np.abs(new)) + np.sum(np.abs(old))))
        if n_alpha == 0 or diff <= 0:
            return step, xn, un, diff, margins
    return None


def blocking_task(o, pts, xs, us, mults, fb, mu):
    """Obstacles that the trajectory xs clears by 1 cm at every t and the full step's rollout enters: a half-space whose normal
    opposes the largest displacement of a point between xs and that rollout, and a sphere around where that point lands.  The
    weight makes the full step's obstacle terms five times what the step gains otherwise.  Returns (kinds, geom, w) of one
    instance and the full step's cost difference without the obstacles"""
    T = o.T
    _, x1, u1 = o.forward_alpha(1.0, xs, us, mults, fb, mu)
    gain = (o.cost_seq_aug(x1, u1, mults, mu) - o.cost_seq_aug(xs, us, mults, mu)).sum()
    Xo, Xn = xs.reshape(T + 1, o.nx), x1.reshape(T + 1, o.nx)
    Po = np.array([positions(o, pts, Xo[t][:o.nq]) for t in range(T + 1)])      # (T+1, K, 3)
    Pn = np.array([positions(o, pts, Xn[t][:o.nq]) for t in range(T + 1)])
    r = np.array([p[2] for p in pts])
    move = np.linalg.norm(Pn - Po, axis=2)
    t_, k_ = np.unravel_index(np.argmax(move), move.shape)
    n = (Po[t_, k_] - Pn[t_, k_]) / move[t_, k_]
    h = np.min(Po @ n - r[None, :]) - 0.01
    c = Pn[t_, k_]
    rho = np.min(np.linalg.norm(Po - c, axis=2) - r[None, :]) - 0.01
    kinds = (HALFSPACE, SPHERE) if rho > 0.0 else (HALFSPACE,)
    geom1 = np.array([np.concatenate([n, [h]]), np.concatenate([c, [max(rho, 0.0)]])])[:len(kinds)]
    geom = np.tile(geom1, (T + 1, 1, 1))
    unit = ob_terms(o, pts, kinds, x1, geom, np.ones((T + 1, len(kinds)))).sum()
    assert unit > 0.0
    return kinds, geom, np.full((T + 1, len(kinds)), 5.0 * abs(gain) / unit), gain


FORWARD_CASES = [(name, fo_, path, na) for name, fo_, path in (("tree38", None, 1), ("chain6ff", 0, 0), ("tree38_frame", None, 1))
                 for na in (1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path,n_alpha", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, n_alpha):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the obstacle terms
    included.  The obstacles (blocking_task) leave the old trajectory alone and stand where the full step lands: the test
    asserts on the emulation alone that the full step is accepted without them and rejected with them, and that every candidate
    tried decides by more than 1e-9 of the sum of the cost terms' magnitudes; only then are decisions compared"""
    capi = gpu
    T, mu = 16, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, 1, 81, held=True)
    mults = tc._mults(o, xs[0], 85)
    pts = pick_points(model)
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        kinds, geom, w, gain = blocking_task(o, pts, xs[0], us[0], mults, fb, mu_o[0])
        check_task(o, pts, kinds, xs, geom[None], w[None], fractions=False)
        set_task(ctx, pts, kinds, geom, w)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
        clear_old, clear_new = ctx.obstacle_clearance(0)[0], ctx.obstacle_clearance(1)[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + ob_terms(o, pts, kinds, X, geom, w)
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, n_alpha, "gain", gain, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins)
    assert gain < 0.0                                                          # without the obstacles the full step is accepted
    assert np.all(ob_terms(o, pts, kinds, xs[0], geom, w) == 0.0)              # the old trajectory touches nothing
    assert step_ref < 1.0 and len(margins) > 1                                 # with them it is rejected
    assert min(margins) > 1e-9, margins
    assert step[0] == step_ref, (step, step_ref)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)
    assert np.min(clear_old) > 0.0
    assert rel_err(clear_new, ob_clearance(o, pts, kinds, xn_ref, geom, w)) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with V_x != 0 from the obstacle terms, on the device's own derivatives against Oracle.backward:
    restarts, mu and reg identical, every step redone alone by the oracle from the device's V(t+1) to 1e-10
    (stepwise_backward_check).  Tree38 at T = 60 runs on K3h"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    pts = pick_points(model)
    geom, w = random_task(o, pts, KINDS, xs, 1, 72, wscale=10.0)
    check_task(o, pts, KINDS, xs, geom, w)
    mults = tc._mults(o, xs[0], 73)
    n, m = o.n, o.m
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, pts, KINDS, geom, w)
        ctx.linearize()
        if name == "tree38":
            assert ctx.bwd_stream_bytes() == tc._k3h_bytes(n, m)
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        d = o.alloc_derivs()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
        add = ob_derivs(o, model, pts, KINDS, xs[0], geom[0], w[0])
        assert np.max(np.abs(add["LX"])) > 0 and np.max(np.abs(d["lx"][:T * n])) > 0
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        print("sweep", name, "device restarts", int(restarts[0]), "oracle", ref_b["restarts"], "mu", mu_out[0], ref_b["mu"], "reg", reg[0], ref_b["reg"])
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0

    def one_step_oracle(t):
        e = int(o.ne[t])
        if not e:
            return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2, eq_kind=spec.eq_kind, eq_advance=2, ne=np.array([e], dtype=np.int64),
                      eq_target=np.zeros(e))
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < 1e-10, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo_, flags):
    """batch 3 through linearise, both costs, sweep, forward, twice: the second time instance 1 carries other obstacles.  Instance
    1's outputs change, those of instances 0 and 2 are bit for bit the same"""
    capi = gpu
    T, B, mu = 8, 3, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 91, held=True)
    pts = pick_points(model)
    geom, w = random_task(o, pts, KINDS, xs, B, 92, wscale=5.0)
    geom2, w2 = random_task(o, pts, KINDS, xs, B, 93, wscale=5.0)
    geom2[[0, 2]], w2[[0, 2]] = geom[[0, 2]], w[[0, 2]]
    check_task(o, pts, KINDS, xs, geom, w)
    check_task(o, pts, KINDS, xs, geom2, w2)
    out = []
    for g_, w_ in ((geom, w), (geom2, w2)):
        with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs, us)
            set_task(ctx, pts, KINDS, g_, w_)
            out.append(fc._run_all(ctx, mu, False))
    a, b = out
    assert not np.array_equal(a["LX"][1], b["LX"][1]) and not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
    assert not np.array_equal(a["FB_VAL"][1], b["FB_VAL"][1])
    for k in a:
        for i in (0, 2):
            if isinstance(a[k], tuple):
                for u, v in zip(a[k][1:], b[k][1:]):
                    assert np.array_equal(np.asarray(u)[i], np.asarray(v)[i]), (k, i)
            else:
                assert np.array_equal(a[k][i], b[k][i]), (k, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 5, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    xs, us = _trajs(o, model, B, 101, held=True)
    pts = pick_points(model)
    geom, w = random_task(o, pts, KINDS, xs, B, 102, wscale=10.0)
    check_task(o, pts, KINDS, xs, geom, w)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            set_task(ctx, pts, KINDS, geom, w)
            log = (solver.solve_stepwise if stepwise else solver.solve)(ctx, iters, thr, mu, 0.0, w_, n_)
            return log, ctx.download("X"), ctx.download("U")
    la, xa, ua = run(False)
    lb, xb, ub = run(True)
    assert np.all(np.isfinite(xa))
    assert not np.array_equal(xa, xs)
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(la[k]), np.asarray(lb[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("tree38", None), ("chain6ff", 0), ("table7", None)])
def test_clearance(gpu, name, fo_):
    """ddp_hip_obstacle_clearance against the yardstick to 1e-12 along X, +inf where no slot is live, before any weight is live
    (+inf everywhere), and which = 1 along X_NEW after a forward"""
    capi = gpu
    T, B, mu = 6, 3, 10.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 121, held=name != "table7")
    pts = pick_points(model)
    geom, w = random_task(o, pts, KINDS, xs, B, 124)
    w[1, 2, :] = 0.0; w[2, T, :] = 0.0; w[0, 1, 1] = 0.0
    check_task(o, pts, KINDS, xs, geom, w)
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_obstacle_points(points=pts, kinds=KINDS)
        assert np.all(ctx.obstacle_clearance(0) == np.inf)                  # points set, no live weight
        ctx.set_obstacle_cost(geom=geom, weight=w)
        got = ctx.obstacle_clearance(0)
        ex = np.stack([ob_clearance(o, pts, KINDS, xs[b], geom[b], w[b]) for b in range(B)])
        assert got[1, 2] == np.inf and got[2, T] == np.inf and np.array_equal(np.isinf(got), np.isinf(ex))
        fin = np.isfinite(ex)
        assert np.min(ex[fin]) < 0 < np.max(ex[fin])
        e = np.max(np.abs(got[fin] - ex[fin]) / np.maximum(1.0, np.abs(ex[fin])))
        print("clearance", name, e)
        assert e <= 1e-12, e
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        ctx.forward(mu_o, n_alpha=8)
        xn = ctx.download("X_NEW")
        got1 = ctx.obstacle_clearance(1)
        ex1 = np.stack([ob_clearance(o, pts, KINDS, xn[b], geom[b], w[b]) for b in range(B)])
        assert np.array_equal(np.isinf(got1), np.isinf(ex1))
        e1 = np.max(np.abs(got1[fin] - ex1[fin]) / np.maximum(1.0, np.abs(ex1[fin])))
        assert e1 <= 1e-12, e1
        assert np.array_equal(ctx.obstacle_clearance(0), got)               # X is where it was


@pytest.mark.gpu
def test_clearance_keeps_nan(gpu):
    """a non-finite configuration entry that only an early point depends on (the leaf joint's angle: the leaf's point is point 2 of
    5, the points after it stay finite) gives a NaN clearance at that (instance, t) and nowhere else"""
    capi = gpu
    T = 2
    model, spec, o = _reach_problem(T)
    xs, us = _trajs(o, model, 1, 151)
    pts = pick_points(model)
    leaf = max(j for j, _, _ in pts)
    assert [j for j, _, _ in pts].index(leaf) < len(pts) - 1 and pts[-1][0] < leaf
    geom, w = random_task(o, pts, KINDS, xs, 1, 152)
    bad = xs.copy()
    bad[0, 1 * o.nx + leaf] = np.nan
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        _setup(ctx, bad, us)
        set_task(ctx, pts, KINDS, geom, w)
        got = ctx.obstacle_clearance(0)[0]
    ex = ob_clearance(o, pts, KINDS, xs[0], geom[0], w[0])
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))
    assert rel_err(got[[0, 2]], ex[[0, 2]]) <= 1e-12


@pytest.mark.gpu
def test_degenerate_centre(gpu):
    """a sphere centred on a collision point: the pair contributes its value 1/2 w (r + rho)^2 and no derivative.  The centre has
    to be the device's own p_k bit for bit, so it is read back first: a point of radius 0 against the half-space (e_a, 0) has
    d = p_a exactly"""
    capi = gpu
    T, rho, wgt = 2, 0.1, 3.0
    model, spec, o = make("chain6", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 131)
    tip = (5, (0.0, 0.0, 0.0823), 0.0)
    kinds = (HALFSPACE, HALFSPACE, HALFSPACE, SPHERE)
    geom = np.zeros((T + 1, 4, 4))
    geom[:, :3, :3] = np.eye(3)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST if on else 0) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if on:
                ctx.set_obstacle_points(points=[tip], kinds=kinds)
                p = np.zeros((T + 1, 3))
                for a in range(3):
                    ctx.set_obstacle_cost(geom=geom, weight=np.eye(4)[a])
                    p[:, a] = ctx.obstacle_clearance(0)[0]
                X = xs[0].reshape(T + 1, o.nx)
                assert rel_err(p, np.array([o.frame_position(tip[0], tip[1], X[t][:o.nq]) for t in range(T + 1)])) <= 1e-12
                geom[:, 3, :3], geom[:, 3, 3] = p, rho
                geom[0, 3, :3] += 1.0                                       # t = 0: the sphere is elsewhere
                ctx.set_obstacle_cost(geom=geom, weight=wgt * np.eye(4)[3])
                clear = ctx.obstacle_clearance(0)[0]
                assert np.all(clear[1:] == -rho) and clear[0] > 0, clear    # |p - c| == 0 at t = 1 .. T
            ctx.linearize()
            ctx.cost_seq_aug(0, 1.0)
            got[on] = {s: ctx.download(s)[0] for s in DERIVS + ("COSTS_OLD",)}
    for s in DERIVS:
        assert np.array_equal(got[True][s], got[False][s]), s               # no derivative anywhere
    assert got[True]["COSTS_OLD"][0] == got[False]["COSTS_OLD"][0]
    extra = got[True]["COSTS_OLD"][1:] - got[False]["COSTS_OLD"][1:]
    assert np.max(np.abs(extra - 0.5 * wgt * rho * rho)) <= 1e-12 * max(1.0, np.max(np.abs(got[False]["COSTS_OLD"]))), extra


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    import ctypes as C
    capi = gpu
    T, B = 4, 3
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    L = capi.lib()
    dp = C.POINTER(C.c_double)
    pts = pick_points(model)
    no = len(KINDS)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_obstacle_points(points=pts, kinds=KINDS)) == capi.E_UNSUPPORTED
        with pytest.raises(ValueError):                              # the wrapper has no slot count to check shapes against
            ctx.set_obstacle_cost(weight=np.ones(no))
        z3 = np.ones(T + 1)
        assert L.ddp_hip_obstacle_upload(ctx._h, None, z3.ctypes.data_as(dp), 0, 1) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.obstacle_cost()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.obstacle_clearance()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_OBSTACLE_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        # before set_points: no upload, no clearance
        with pytest.raises(ValueError):
            ctx.set_obstacle_cost(weight=np.ones(no))
        z3 = np.ones(B * (T + 1) * no)
        assert L.ddp_hip_obstacle_upload(ctx._h, None, z3.ctypes.data_as(dp), 0, B) == capi.E_ARG
        assert code(lambda: ctx.obstacle_clearance()) == capi.E_ARG
        # set_points refusals
        many = [pts[k % len(pts)] for k in range(capi.MAX_COLLISION_POINTS + 1)]
        for bad_pts, bad_kinds in (([], KINDS), (many, KINDS), (pts, []), (pts, [SPHERE] * (capi.MAX_OBSTACLES + 1)),
                                   ([(model.nv, pts[0][1], 0.1)] + pts[1:], KINDS), ([(-1, pts[0][1], 0.1)] + pts[1:], KINDS),
                                   ([(0, (0.0, np.nan, 0.0), 0.1)], KINDS), ([(0, (0.0, np.inf, 0.0), 0.1)], KINDS),
                                   ([(0, pts[0][1], -1e-3)], KINDS), ([(0, pts[0][1], np.nan)], KINDS), ([(0, pts[0][1], np.inf)], KINDS),
                                   (pts, [SPHERE, 2, HALFSPACE]), (pts, [-1])):
            assert code(lambda: ctx.set_obstacle_points(points=bad_pts, kinds=bad_kinds)) == capi.E_ARG, (bad_pts, bad_kinds)
        assert code(lambda: ctx.obstacle_clearance()) == capi.E_ARG           # a refused set_points sets nothing
        ctx.set_obstacle_points(points=pts, kinds=KINDS)
        g0, w0 = ctx.obstacle_cost()                                          # defaults: geometry 0, weights 0
        assert g0.shape == (B, T + 1, no, 4) and w0.shape == (B, T + 1, no) and np.all(g0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        gg = rng.normal(size=(B, T + 1, no, 4))
        for s_, kind in enumerate(KINDS):
            if kind == SPHERE:
                gg[..., s_, 3] = np.abs(gg[..., s_, 3])
            else:
                gg[..., s_, :3] /= np.linalg.norm(gg[..., s_, :3], axis=-1, keepdims=True)
        wg = rng.uniform(0, 1, size=(B, T + 1, no))
        ctx.set_obstacle_cost(geom=gg, weight=wg)
        per_g, per_w = gg[0].copy(), wg[0].copy()
        for bad in (-1e-3, np.nan, np.inf):
            wb = per_w.copy(); wb[1, 2] = bad
            assert code(lambda: ctx.set_obstacle_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_obstacle_cost(geom=per_g, weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            for s_ in range(no):
                gb = per_g.copy(); gb[2, s_, 1] = bad
                assert code(lambda: ctx.set_obstacle_cost(geom=gb, weight=per_w)) == capi.E_ARG, (bad, s_)
                assert code(lambda: ctx.set_obstacle_cost(geom=gb)) == capi.E_ARG, (bad, s_)
        gb = per_g.copy(); gb[1, 0, 3] = -1e-3                               # a negative sphere radius
        assert code(lambda: ctx.set_obstacle_cost(geom=gb)) == capi.E_ARG
        gb = per_g.copy(); gb[1, 1, :3] *= 1.0 + 1e-9                        # a half-space normal off unit length
        assert code(lambda: ctx.set_obstacle_cost(geom=gb)) == capi.E_ARG
        gb = per_g.copy(); gb[3, 1, :3] = 0.0
        assert code(lambda: ctx.set_obstacle_cost(geom=gb, weight=per_w)) == capi.E_ARG
        gb = per_g.copy(); gb[1, 1, :3] *= 1.0 + 1e-12; gb[1, 1, 3] = -5.0   # within 1e-10: accepted below; an offset may be negative
        assert code(lambda: ctx.set_obstacle_cost(weight=per_w, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_obstacle_cost(weight=per_w, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_obstacle_cost(weight=per_w, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.obstacle_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros(B * (T + 1) * no * 4)
        assert L.ddp_hip_obstacle_upload(ctx._h, None, z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        assert L.ddp_hip_obstacle_clearance(ctx._h, 2, z.ctypes.data_as(dp)) == capi.E_ARG
        assert L.ddp_hip_obstacle_clearance(ctx._h, 0, None) == capi.E_ARG
        g1, w1 = ctx.obstacle_cost()
        assert np.array_equal(g1, gg) and np.array_equal(w1, wg)                # a refused upload leaves both sides as they were
        ctx.set_obstacle_cost(geom=gb, first=1, count=1)                        # one side, one instance; the weights stay
        g1, w1 = ctx.obstacle_cost()
        assert np.array_equal(g1[0], gg[0]) and np.array_equal(g1[1], gb) and np.array_equal(g1[2], gg[2]) and np.array_equal(w1, wg)
        g2, w2 = ctx.obstacle_cost(first=1, count=2)                            # the round trip of a range of instances
        assert np.array_equal(g2, g1[1:]) and np.array_equal(w2, wg[1:])
        ctx.set_obstacle_cost(weight=np.array([1.0, 2.0, 0.0]), first=1, count=2)   # broadcast: (n_obs,)
        assert np.array_equal(ctx.obstacle_cost()[1][1:], np.broadcast_to([1.0, 2.0, 0.0], (2, T + 1, no)))
        assert np.array_equal(ctx.obstacle_cost()[1][0], wg[0])
        ctx.set_obstacle_cost(geom=per_g[0])                                    # broadcast: (n_obs, 4)
        assert np.array_equal(ctx.obstacle_cost()[0], np.broadcast_to(per_g[0], (B, T + 1, no, 4)))
        # set_points again: the same counts and kinds keep the data (the points may move), other counts or kinds reset it
        moved = [(j, tuple(0.5 * np.asarray(off)), 2.0 * r) for j, off, r in pts]
        ctx.set_obstacle_points(points=moved, kinds=KINDS)
        g3, w3 = ctx.obstacle_cost()
        assert np.array_equal(g3, np.broadcast_to(per_g[0], (B, T + 1, no, 4))) and np.any(w3 != 0.0)
        ctx.set_obstacle_points(points=pts[:4], kinds=KINDS)
        g4, w4 = ctx.obstacle_cost()
        assert np.all(g4 == 0.0) and np.all(w4 == 0.0)
        ctx.set_obstacle_cost(weight=np.ones(no))
        ctx.set_obstacle_points(points=pts[:4], kinds=KINDS[:2])
        g5, w5 = ctx.obstacle_cost()
        assert g5.shape == (B, T + 1, 2, 4) and np.all(g5 == 0.0) and np.all(w5 == 0.0)
        ctx.set_obstacle_cost(weight=np.ones(2))
        ctx.set_obstacle_points(points=pts[:4], kinds=(HALFSPACE, SPHERE))
        assert np.all(ctx.obstacle_cost()[1] == 0.0)


def _reach_problem(T):
    """the UR5-like chain without its configuration constraint"""
    from ddp_pinocchio_amd import capi
    from oracle.binding import Oracle
    model = capi.BuiltinModel(capi.BUILTIN_CHAIN6)
    kw = dict(dt=0.01, c=1.0, fd_mode=0, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    return model, capi.ProblemSpec(model, T, batch=1, **kw), Oracle(model, T, **kw)


@pytest.mark.gpu
def test_reach_around_obstacle(gpu):
    """chain6, T = 40, no constraint: a tracking cost pulls the arm (and so its tip) to a goal posture.  The flag-off solve's tip
    path is taken first; a sphere is then put on that path, halfway.  With the obstacle weight on, from the same start: every
    iteration is accepted, the total cost never increases from one iterate to the next (the last one included), and the final
    worst penetration (-min clearance) is strictly smaller than that of the flag-off solution"""
    capi = gpu
    T, mu, iters = 40, 1.0, 12
    model, spec, o = _reach_problem(T)
    xs, us = _trajs(o, model, 1, 141, held=True)
    tip = (5, (0.0, 0.0, 0.0823), 0.03)
    rng = np.random.default_rng(142)
    goal = np.concatenate([xs[0][:o.nq] + 0.6 * rng.choice([-1.0, 1.0], size=o.nv), np.zeros(o.nv)])
    xref = np.tile(goal, (T + 1, 1))
    wx = np.tile(np.concatenate([np.full(o.nv, 200.0), np.full(o.nv, 1.0)]), (T + 1, 1))
    wx[T] *= 10.0

    def solve(ctx):
        costs, steps = [], []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            steps.append(step[0])
            assert step[0] > 0.0, steps                                    # the iteration was accepted: X_NEW is the iterate
            ctx.swap_traj()
        ctx.cost_seq_aug(0, mu)                                            # ... and the cost of the last one
        costs.append(ctx.download("COSTS_OLD")[0].sum())
        return costs, steps, ctx.download("X")
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_tracking_cost(xref=xref, wx=wx)
        costs_off, _, x_off = solve(ctx)
    Xo = x_off[0].reshape(T + 1, o.nx)
    path = np.array([o.frame_position(tip[0], tip[1], Xo[t][:o.nq]) for t in range(T + 1)])
    assert np.linalg.norm(path[T] - path[0]) > 0.1                          # the tip travels
    geom = np.concatenate([path[T // 2], [0.05]])[None, :]                  # a sphere on the unobstructed path, at every t
    start = pair(SPHERE, geom[0], path[0], tip[2])[0]
    assert start > 0.0, start                                               # the arm starts clear of it
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS) as ctx:
        ctx.set_tracking_cost(xref=xref, wx=wx)
        ctx.set_obstacle_points(points=[tip], kinds=[SPHERE])
        ctx.set_obstacle_cost(geom=geom, weight=np.full(1, 1e5))
        _setup(ctx, x_off, us)
        pen_off = -np.min(ctx.obstacle_clearance(0))
        _setup(ctx, xs, us)
        costs, steps, x_on = solve(ctx)
        ctx.upload("X", x_on)
        pen_on = -np.min(ctx.obstacle_clearance(0))
    print("reach around: costs", costs, "steps", steps, "penetration off", pen_off, "on", pen_on)
    assert abs(pen_off - (tip[2] + 0.05)) <= 1e-9                           # the flag-off path goes through the centre
    assert len(costs) == iters + 1 and all(s > 0.0 for s in steps), steps
    for a, b in zip(costs, costs[1:]):
        assert b <= a, costs
    assert pen_on < pen_off, (pen_on, pen_off)
