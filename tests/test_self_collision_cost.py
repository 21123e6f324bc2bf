"""Per-instance self-collision costs (DDP_HIP_FLAG_SELF_COLLISION_COST, include/ddp_hip/ddp_hip.h): spheres on the robot (sphere k:
off_k fixed in joint_k, radius r_k, world position p_k(q)) in pairs i = (a_i, b_i), with a margin and a weight per (instance, t, pair),

    D_i = |p_a - p_b|,   d_i = D_i - (r_a + r_b + m_i),   u_i = (p_a - p_b) / D_i,   e_i = d_i < 0 ? d_i : 0
    l(t, x, u) += 1/2 sum_i w[b][t][i] e_i^2,   lf alike at T

The oracle has no such cost, so the yardstick is the numpy restatement below, built on Oracle.frame_position and
Oracle.frame_jacobian(world_aligned=True): z_i = + P_a^T u_i on the tangent columns of path(a_i) alone, - P_b^T u_i on those of
path(b_i) alone and exact zero on the columns of both (the distance does not change when a common ancestor moves); lx += w e z,
lxx += w z z^T over the pairs with w != 0, e != 0 and D != 0.  The helpers of test_obstacle_cost.py, test_frame_cost.py,
test_tracking_cost.py and the others are reused by import; tolerances are theirs.

The robot's geometry along a trajectory is given, so the task generator sets activity through the margins: m = D - r_a - r_b
+- depth with depth in 0.01 .. 0.1.  check_task asserts on the yardstick alone that no live pair sits within 1e-6 of its margin or
has its centres within 1e-3 of each other, so that device and numpy cannot disagree about which pairs are active."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_com_cost as cm
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_frame_vel_cost as fv
import test_obstacle_cost as ob
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = ob.H
W5 = ob.W5
DERIVS = fc.DERIVS
NAMES = fc.NAMES
make_any = cm.make_any
_trajs, _setup = tc._trajs, tc._setup
pick_points = ob.pick_points
_emulate_forward = ob._emulate_forward
_reach_problem = ob._reach_problem


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def all_pairs(pts):
    """every pair of spheres that is not on one joint, a < b (the five of pick_points: 9 pairs)"""
    return [(a, b) for a in range(len(pts)) for b in range(a + 1, len(pts)) if pts[a][0] != pts[b][0]]


def more_points(model, pts):
    """two more spheres on joints that carry none yet: 7 spheres, 20 pairs -- more than the 16 lanes a state has"""
    used = {j for j, _, _ in pts}
    free = [j for j in range(len(model.parent)) if j not in used]
    return list(pts) + [(free[len(free) // 3], (0.04, 0.03, -0.06), 0.04), (free[(2 * len(free)) // 3], (-0.05, 0.02, 0.09), 0.07)]


def sym_cols(model, ja, jb):
    """the tangent columns of path(ja) that are not on path(jb), and of path(jb) that are not on path(ja)"""
    pa, pb = fv.path_of(model, ja), fv.path_of(model, jb)
    only_a = [c for i in pa if i not in pb for c in fv.cols_of(model, i)]
    only_b = [c for i in pb if i not in pa for c in fv.cols_of(model, i)]
    return only_a, only_b


def centres(o, pts, q):
    return [o.frame_position(j, off, q) for j, off, _ in pts]


def pair_d(pts, P, a, b, margin):
    """(D_i, d_i, u_i) of one pair from the spheres' centres P; u is None where the centres coincide"""
    diff = P[a] - P[b]
    D = float(np.sqrt(diff @ diff))
    return D, D - (pts[a][2] + pts[b][2] + margin), (diff / D if D != 0.0 else None)


def sc_term(o, pts, pairs, q, m_t, w_t):
    """1/2 sum_i w e^2 at one configuration, the pairs in ascending order; and whether a pair is active"""
    P = centres(o, pts, q)
    s, act = 0.0, False
    for i, (a, b) in enumerate(pairs):
        if w_t[i] == 0.0:
            continue
        _, d, _ = pair_d(pts, P, a, b, m_t[i])
        if d < 0:
            s += w_t[i] * d * d
            act = True
    return 0.5 * s, act


def sc_terms(o, pts, pairs, xs, m, w):
    """the self-collision terms of one instance per t (T+1 values; the last belongs to lf); m, w: (T+1, n_pairs)"""
    X = xs.reshape(o.T + 1, o.nx)
    return np.array([sc_term(o, pts, pairs, X[t][:o.nq], m[t], w[t])[0] for t in range(o.T + 1)])


def sc_clearance(o, pts, pairs, xs, m, w):
    """min over the pairs with w != 0 of d_i per t; +inf where no pair is live"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.full(o.T + 1, np.inf)
    for t in range(o.T + 1):
        P = centres(o, pts, X[t][:o.nq])
        for i, (a, b) in enumerate(pairs):
            if w[t][i] != 0.0:
                out[t] = min(out[t], pair_d(pts, P, a, b, m[t][i])[1])
    return out


def sc_z(o, model, pts, a, b, q, u):
    """z_i over the nv tangent columns, the common columns and the columns off both paths exact zero; and the symmetric difference"""
    (ja, offa, _), (jb, offb, _) = pts[a], pts[b]
    ca, cb = sym_cols(model, ja, jb)
    z = np.zeros(o.nv)
    if ca:
        z[ca] = o.frame_jacobian(ja, offa, q, world_aligned=True)[:, ca].T @ u
    if cb:
        z[cb] = -(o.frame_jacobian(jb, offb, q, world_aligned=True)[:, cb].T @ u)
    return z, ca + cb


def sc_grad_hess(o, model, pts, pairs, x, m_t, w_t):
    """(lx, lxx) contributions at one state, n and n x n, and the tangent rows of the active pairs' symmetric differences (a mask
    over n): sum w e z and the Gauss-Newton sum w z z^T on the q rows, over the pairs with w != 0, e != 0 and D != 0"""
    nv, n = o.nv, o.n
    g, Hm, rows = np.zeros(n), np.zeros((n, n)), np.zeros(n, dtype=bool)
    q = x[:o.nq]
    P = centres(o, pts, q)
    for i, (a, b) in enumerate(pairs):
        if w_t[i] == 0.0:
            continue
        _, d, u = pair_d(pts, P, a, b, m_t[i])
        if not d < 0 or u is None:
            continue
        z, cols = sc_z(o, model, pts, a, b, q, u)
        rows[cols] = True
        g[:nv] += w_t[i] * d * z
        Hm[:nv, :nv] += w_t[i] * np.outer(z, z)          # entry (r, c) and (c, r) alike: symmetric bit for bit
    return g, Hm, rows


def sc_derivs(o, model, pts, pairs, xs, m, w):
    """what the terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout, and the active rows
    per t"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": [], "rows": []}
    for t in range(o.T + 1):
        g, Hm, rows = sc_grad_hess(o, model, pts, pairs, X[t], m[t], w[t])
        out["rows"].append(rows)
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, pts, pairs, xs, B, seed, wscale=1.0, p_clear=0.5):
    """margins and weights (B, T+1, n_pairs) each.  Per (instance, t): with probability p_clear a block in which every pair is
    clear of its margin by 0.01 .. 0.1, else a block in which each pair penetrates by 0.01 .. 0.1 (at least one pair) or stays
    clear by as much: m = D - r_a - r_b +- depth"""
    rng = np.random.default_rng(seed)
    T, npair = o.T, len(pairs)
    m, w = np.zeros((B, T + 1, npair)), wscale * rng.uniform(0.5, 5.0, size=(B, T + 1, npair))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            P = centres(o, pts, X[t][:o.nq])
            clear_block = rng.uniform() < p_clear
            forced = int(rng.integers(npair))
            for i, (a, c) in enumerate(pairs):
                depth = rng.uniform(0.01, 0.1)
                inside = (not clear_block) and (i == forced or rng.uniform() < 0.6)
                D = pair_d(pts, P, a, c, 0.0)[0]
                m[b, t, i] = D - pts[a][2] - pts[c][2] + (depth if inside else -depth)
    return m, w


def check_task(o, pts, pairs, xs, m, w, fractions=True):
    """the conditions on the inputs, on the yardstick alone: no live pair has |d| < 1e-6 or D < 1e-3; at least a quarter of the
    (instance, t) blocks have an active pair and at least a quarter have none.  Returns the blocks' activity (B, T+1)"""
    B, T = xs.shape[0], o.T
    active = np.zeros((B, T + 1), dtype=bool)
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            P = centres(o, pts, X[t][:o.nq])
            for i, (a, c) in enumerate(pairs):
                if w[b, t, i] == 0.0:
                    continue
                D, d, _ = pair_d(pts, P, a, c, m[b, t, i])
                assert abs(d) >= 1e-6, (b, t, i, d)
                assert D >= 1e-3, (b, t, i, D)
                active[b, t] |= d < 0
    if fractions:
        assert 4 * active.sum() >= active.size and 4 * (~active).sum() >= active.size, (active.sum(), active.size)
    return active


def set_task(ctx, pts, pairs, margin=None, weight=None):
    ctx.set_self_collision_pairs(points=pts, pairs=pairs)
    if margin is not None or weight is not None:
        ctx.set_self_collision_cost(margin=margin, weight=weight)


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff", "table7"])
def test_yardstick_gradient(name):
    """z_i (common columns left out) against the 5-point central difference of D_i along x (+) (+-h e_c) over all nv columns --
    the common columns come out 0 within the tolerance --; lx against the central difference of the term at states with active
    pairs; lxx symmetric bit for bit and positive semidefinite, with zero velocity rows and columns, zero rows outside the
    symmetric differences and, behind a free-flyer root, zero root rows"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    assert len(pairs) == 9
    xs, us = _trajs(o, model, 1, 3)
    m, w = random_task(o, pts, pairs, xs, 1, 4, p_clear=0.0)
    check_task(o, pts, pairs, xs, m, w, fractions=False)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    for t in (1, T):
        q = X[t][:o.nq]
        P = centres(o, pts, q)
        for i, (a, b) in enumerate(pairs):
            _, _, u = pair_d(pts, P, a, b, 0.0)
            z, cols = sc_z(o, model, pts, a, b, q, u)
            assert cols and np.all(z[[c for c in range(nv) if c not in cols]] == 0.0)
            fd = np.zeros(nv)
            for c in range(nv):
                e = np.zeros(nv); e[c] = H
                fd[c] = sum(cw * pair_d(pts, centres(o, pts, o.integrate(q, s * e)), a, b, 0.0)[0] for s, cw in W5) / H
            assert np.max(np.abs(fd - z)) <= 1e-8 * max(1.0, np.max(np.abs(z))), (i, np.max(np.abs(fd - z)))
        g, Hm, rows = sc_grad_hess(o, model, pts, pairs, X[t], m[0, t], w[0, t])
        assert np.max(np.abs(g[:nv])) > 0 and rows.any()

        def cost_at(dx):
            return sc_term(o, pts, pairs, tc._integrate_x(o, X[t], dx)[:o.nq], m[0, t], w[0, t])[0]
        fd = np.zeros(n)
        for c in range(n):
            e = np.zeros(n); e[c] = H
            fd[c] = sum(cw * cost_at(s * e) for s, cw in W5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        assert np.array_equal(Hm, Hm.T)
        assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(g[nv:] == 0.0)
        assert np.all(g[~rows] == 0.0) and np.all(Hm[~rows, :] == 0.0)
        if model.ff:
            assert not rows[:6].any() and np.all(g[:6] == 0.0) and np.all(Hm[:6, :] == 0.0) and np.all(Hm[:, :6] == 0.0)
        assert np.min(np.linalg.eigvalsh(Hm)) >= -1e-12 * np.max(np.abs(Hm))


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_SELF_COLLISION_COST == 1024 and re.search(r"#define\s+DDP_HIP_FLAG_SELF_COLLISION_COST\s+1024u", header)
    assert capi.MAX_COLLISION_PAIRS == 32 and re.search(r"#define\s+DDP_HIP_MAX_COLLISION_PAIRS\s+32\b", header)
    assert capi.MAX_COLLISION_POINTS == 16
    L = capi.lib()
    for name in ("ddp_hip_self_collision_set_pairs", "ddp_hip_self_collision_upload", "ddp_hip_self_collision_download",
                 "ddp_hip_self_collision_clearance"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    for name in ("set_self_collision_pairs", "set_self_collision_cost", "self_collision_cost", "self_collision_clearance"):
        assert hasattr(capi.Context, name), name
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B, npair = 5, 2, 3
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h, ctx.n_collision_pairs = spec, B, None, 0
    with pytest.raises(ValueError, match="set_self_collision_pairs"):
        ctx.set_self_collision_cost(weight=np.zeros(npair))
    ctx.n_collision_pairs = npair
    for kw in (dict(margin=np.zeros(npair + 1)), dict(margin=0.0), dict(margin=np.zeros((T, npair))),
               dict(margin=np.zeros((B + 1, T + 1, npair))), dict(margin=np.zeros((T + 1, npair + 1))), dict(margin=np.zeros((npair, 1))),
               dict(weight=np.zeros(npair - 1)), dict(weight=0.0), dict(weight=np.zeros((T, npair))),
               dict(weight=np.zeros((B, T + 1, npair)), count=1), dict(weight=np.zeros((T + 1, npair, 1))),
               dict(margin=np.zeros(npair), weight=np.zeros((T + 1, npair + 1)))):
        with pytest.raises(ValueError):
            ctx.set_self_collision_cost(**kw)
    for bad_pts, bad_pairs in (([(0, (0.0, 0.0), 0.1), (1, (0.0, 0.0, 0.0), 0.1)], [(0, 1)]),
                               ([(0, (0.0, 0.0, 0.0)), (1, (0.0, 0.0, 0.0), 0.1)], [(0, 1)]),
                               ([(0, (0.0, 0.0, 0.0), 0.1), (1, (0.0, 0.0, 0.0), 0.1)], [(0, 1, 1)])):
        with pytest.raises(ValueError):
            ctx.set_self_collision_pairs(points=bad_pts, pairs=bad_pairs)


def test_self_collision_block_host_logic():
    """host/test_self_collision_block.cpp: the term's record, the pair-list rules and what an upload of margins and weights
    decides (csrc/cost_block.h), which need no device"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_self_collision_block"])
    out = subprocess.run([os.path.join(host, "test_self_collision_block")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------
LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("table7", 2, None, ""), ("tree38", 2, None, "all"), ("tree38", 2, None, "many")]


def _lin_task(o, model, xs, B, T, many=False):
    pts = more_points(model, pick_points(model)) if many else pick_points(model)
    pairs = all_pairs(pts)
    assert len(pairs) == (20 if many else 9)
    m, w = random_task(o, pts, pairs, xs, B, 43)
    w[1, 2, 1] = 0.0; w[0, T, 2] = 0.0; w[2, 3, 0] = 0.0   # one pair's weight off at single (instance, t) entries
    return pts, pairs, m, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different margins per instance,
    5 spheres in 9 pairs, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU,
    LUU, LUX, every velocity row and column and the q rows outside the active pairs' symmetric differences (a free-flyer root's
    rows always) bit for bit the flag-off values; blocks without an active pair bit for bit flag-off, blocks with one differ.
    "all": tracking, frame positions, orientations and velocities, state limits, the CoM cost and obstacles live beside it;
    "many": 7 spheres in 20 pairs"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    pts, pairs, m, w = _lin_task(o, model, xs, B, T, many=flags == "many")
    active = check_task(o, pts, pairs, xs, m, w)
    frames = fc.pick_frames(model, 3)
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "all":
        base |= (capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_FRAME_VEL_COST
                 | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST | capi.FLAG_OBSTACLE_COST)
        ref = tc.random_ref(o, model, xs, us, B, 44)
        ftask = fc.random_task(o, xs, frames, B, 45)
        otask = fo.random_orient(o, xs, frames, B, 47)
        vtask = fv.random_task(o, xs, frames, B, 49)
        lim = sl.random_limits(o, xs, B, 46)
        ctask = cm.random_task(o, model, xs, B, 48)
        opts = pick_points(model)
        obtask = ob.random_task(o, opts, ob.KINDS, xs, B, 50)
        assert ob.check_task(o, opts, ob.KINDS, xs, *obtask).any()
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_SELF_COLLISION_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "all":
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(frames=frames, target=ftask[0], weight=ftask[1])
                ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
                ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
                ob.set_task(ctx, opts, ob.KINDS, *obtask)
            if on:
                set_task(ctx, pts, pairs, m, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = sc_derivs(o, model, pts, pairs, xs[b], m[b], w[b])
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
            assert not (model.ff and rows[:6].any())
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
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the flag-off context's values plus the numpy terms, lf included; a block
    without an active pair keeps the flag-off value bit for bit.  tree38 carries the 20-pair list: two pairs per lane"""
    capi = gpu
    T, B, mu = 6, 3, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    pts = more_points(model, pick_points(model)) if name == "tree38" else pick_points(model)
    pairs = all_pairs(pts)
    m, w = random_task(o, pts, pairs, xs, B, 52)
    w[1, 3, 0] = 0.0
    active = check_task(o, pts, pairs, xs, m, w)
    active2 = check_task(o, pts, pairs, xs2, m, w, fractions=False)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (capi.FLAG_SELF_COLLISION_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                set_task(ctx, pts, pairs, m, w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, X, act in ((0, xs, active), (1, xs2, active2)):
        for b in range(B):
            add = sc_terms(o, pts, pairs, X[b], m[b], w[b])
            ex = got[False][which][b] + add
            assert np.any(add != 0.0) and np.array_equal(add != 0.0, act[b])
            e = rel_err(got[True][which][b], ex)
            print("cost_seq_aug", name, which, b, e)
            assert e <= 1e-12, (which, b, e)
            assert np.array_equal(got[True][which][b][~act[b]], got[False][which][b][~act[b]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,extra,fwd_path", [
    ("tree38", 24, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("tree38", 24, 2, None, "box", 1),
])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "never"])
def test_untouched_pairs_change_nothing(gpu, name, T, fd_mode, fo_, extra, fwd_path, mode):
    """flag on with nothing uploaded, with pairs within their margins but every weight 0, and with non-zero weights on margins of
    -10 (the kernels run and find no active pair): linearise, both costs, sweep and forward are bit for bit what the flag-off
    context computes, on both forward paths"""
    capi = gpu
    mu, B = 10.0, 2
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    m, w = random_task(o, pts, pairs, xs, B, 33)
    if mode == "never":
        m[:] = -10.0
        assert np.min([sc_clearance(o, pts, pairs, xs[b], m[b], w[b]) for b in range(B)]) > 5.0
    else:
        w[:] = 0.0
    base = capi.FLAG_TRACE | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_SELF_COLLISION_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if on and mode != "nothing":
                set_task(ctx, pts, pairs, m, w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
            if on and mode == "never":
                assert np.min(ctx.self_collision_clearance(1)) > 5.0        # the accepted candidate stayed clear as well
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
def test_solve_with_untouched_pairs_changes_nothing(gpu):
    """ddp_hip_solve with non-zero weights on margins of -10: the log and the result are bit for bit the flag-off solve's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 4, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 101, held=True)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST if on else 0) as ctx:
            _setup(ctx, xs, us)
            if on:
                set_task(ctx, pts, pairs, np.full(len(pairs), -10.0), np.full(len(pairs), 50.0))
            log = solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
            res[on] = (log, ctx.download("X"), ctx.download("U"))
    assert not np.array_equal(res[True][1], xs)
    assert np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(res[False][0][k]), np.asarray(res[True][0][k])), k


def blocking_task(o, pts, pairs, xs, us, mults, fb, mu):
    """Margins that leave the trajectory xs clear by exactly 1 cm at every t, per t and pair, and a weight on the one pair whose
    distance shrinks most under the full step: five times what the step gains otherwise.  Returns (margins, weights) of one
    instance, (T+1, n_pairs) each, the full step's cost difference without the term, and by how much that pair approaches"""
    T = o.T
    _, x1, u1 = o.forward_alpha(1.0, xs, us, mults, fb, mu)
    gain = (o.cost_seq_aug(x1, u1, mults, mu) - o.cost_seq_aug(xs, us, mults, mu)).sum()
    Xo, Xn = xs.reshape(T + 1, o.nx), x1.reshape(T + 1, o.nx)
    Do = np.array([[pair_d(pts, centres(o, pts, Xo[t][:o.nq]), a, b, 0.0)[0] for a, b in pairs] for t in range(T + 1)])
    Dn = np.array([[pair_d(pts, centres(o, pts, Xn[t][:o.nq]), a, b, 0.0)[0] for a, b in pairs] for t in range(T + 1)])
    rsum = np.array([pts[a][2] + pts[b][2] for a, b in pairs])
    m = Do - rsum[None, :] - 0.01
    shrink = np.max(Do - Dn, axis=0)
    i_ = int(np.argmax(shrink))
    sel = np.zeros((T + 1, len(pairs)))
    sel[:, i_] = 1.0
    unit = sc_terms(o, pts, pairs, x1, m, sel).sum()
    return m, sel * (5.0 * abs(gain) / unit if unit > 0.0 else 0.0), gain, float(shrink[i_])


FORWARD_CASES = [(name, fo_, path, na) for name, fo_, path in (("tree38", None, 1), ("chain6ff", 0, 0), ("tree38_frame", None, 1))
                 for na in (1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path,n_alpha", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, n_alpha):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the self-collision terms
    included.  The margins (blocking_task) leave the old trajectory clear by 1 cm at every t and weigh the pair that the full step
    brings closest: the test asserts on the emulation alone that the full step is accepted without the term and rejected with it,
    and that every candidate tried decides by more than 1e-9 of the sum of the cost terms' magnitudes; only then are decisions
    compared.  A seed whose full step brings no pair closer by more than 1 cm is passed over"""
    capi = gpu
    T, mu = 16, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        for seed in range(81, 97):                                             # (chain6ff's held trajectories barely move: seed 90)
            xs, us = _trajs(o, model, 1, seed, held=True)
            mults = tc._mults(o, xs[0], 85)
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
            m, w, gain, shrink = blocking_task(o, pts, pairs, xs[0], us[0], mults, fb, mu_o[0])
            if shrink > 0.01:
                break
        assert shrink > 0.01, shrink
        check_task(o, pts, pairs, xs, m[None], w[None], fractions=False)
        set_task(ctx, pts, pairs, m, w)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
        clear_old, clear_new = ctx.self_collision_clearance(0)[0], ctx.self_collision_clearance(1)[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + sc_terms(o, pts, pairs, X, m, w)
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, n_alpha, "seed", seed, "shrink", shrink, "gain", gain, "step", step[0], step_ref, "dcost", dcost[0], new,
          "margins", margins)
    assert gain < 0.0                                                          # without the term the full step is accepted
    assert np.all(sc_terms(o, pts, pairs, xs[0], m, w) == 0.0)                 # the old trajectory is clear
    assert step_ref < 1.0 and len(margins) > 1                                 # with it the full step is rejected
    assert min(margins) > 1e-9, margins
    assert step[0] == step_ref, (step, step_ref)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)
    assert rel_err(clear_old, np.full(T + 1, 0.01)) < 1e-9
    assert rel_err(clear_new, sc_clearance(o, pts, pairs, xn_ref, m, w)) < 1e-9


@pytest.mark.gpu
def test_sweep_matches_oracle(gpu):
    """the backward sweep with the device's LX / LXX carrying the term against Oracle.backward, tree38 at T = 60 (K3h): restarts,
    mu and reg identical, every step redone alone by the oracle from the device's V(t+1) to 1e-10 (stepwise_backward_check)"""
    from oracle.binding import Oracle
    capi = gpu
    name, T, mu = "tree38", 60, 1.0
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    m, w = random_task(o, pts, pairs, xs, 1, 72, wscale=10.0)
    check_task(o, pts, pairs, xs, m, w)
    mults = tc._mults(o, xs[0], 73)
    n, mm = o.n, o.m
    with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, pts, pairs, m, w)
        ctx.linearize()
        assert ctx.bwd_stream_bytes() == tc._k3h_bytes(n, mm)
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        d = o.alloc_derivs()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
        add = sc_derivs(o, model, pts, pairs, xs[0], m[0], w[0])
        assert np.max(np.abs(add["LX"])) > 0 and np.max(np.abs(d["lx"][:T * n])) > 0
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        print("sweep", name, "device restarts", int(restarts[0]), "oracle", ref_b["restarts"], "mu", mu_out[0], ref_b["mu"], "reg", reg[0], ref_b["reg"])
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0

    def one_step_oracle(t):
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
    assert not o.Etot
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < 1e-10, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("tree38", None), ("chain6ff", 0), ("table7", None)])
def test_clearance(gpu, name, fo_):
    """ddp_hip_self_collision_clearance against the yardstick to 1e-12 along X, +inf where no pair is live, E_ARG before
    set_self_collision_pairs, +inf everywhere before any weight is live, and which = 1 along X_NEW after a forward"""
    capi = gpu
    T, B, mu = 6, 3, 10.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 121, held=name != "table7")
    pts = pick_points(model)
    pairs = all_pairs(pts)
    m, w = random_task(o, pts, pairs, xs, B, 124)
    w[1, 2, :] = 0.0; w[2, T, :] = 0.0; w[0, 1, 1] = 0.0
    check_task(o, pts, pairs, xs, m, w)
    with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        with pytest.raises(capi.DdpHipError) as exc:
            ctx.self_collision_clearance(0)
        assert exc.value.code == capi.E_ARG
        ctx.set_self_collision_pairs(points=pts, pairs=pairs)
        assert np.all(ctx.self_collision_clearance(0) == np.inf)            # pairs set, no live weight
        ctx.set_self_collision_cost(margin=m, weight=w)
        got = ctx.self_collision_clearance(0)
        ex = np.stack([sc_clearance(o, pts, pairs, xs[b], m[b], w[b]) for b in range(B)])
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
        got1 = ctx.self_collision_clearance(1)
        ex1 = np.stack([sc_clearance(o, pts, pairs, xn[b], m[b], w[b]) for b in range(B)])
        assert np.array_equal(np.isinf(got1), np.isinf(ex1))
        e1 = np.max(np.abs(got1[fin] - ex1[fin]) / np.maximum(1.0, np.abs(ex1[fin])))
        assert e1 <= 1e-12, e1
        assert np.array_equal(ctx.self_collision_clearance(0), got)         # X is where it was


@pytest.mark.gpu
def test_clearance_keeps_nan(gpu):
    """a non-finite configuration entry that only the leaf's sphere depends on (the leaf joint's angle) gives a NaN clearance at
    that (instance, t), whichever place its pairs have in the list, and nowhere else"""
    capi = gpu
    T = 2
    model, spec, o = _reach_problem(T)
    xs, us = _trajs(o, model, 1, 151)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    leaf = max(j for j, _, _ in pts)
    k_leaf = [j for j, _, _ in pts].index(leaf)
    assert any(k_leaf in p for p in pairs[:-1]) and k_leaf not in pairs[-1]     # finite pairs are folded after a NaN one
    m, w = random_task(o, pts, pairs, xs, 1, 152)
    bad = xs.copy()
    bad[0, 1 * o.nx + leaf] = np.nan
    with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST) as ctx:
        _setup(ctx, bad, us)
        set_task(ctx, pts, pairs, m, w)
        got = ctx.self_collision_clearance(0)[0]
    ex = sc_clearance(o, pts, pairs, xs[0], m[0], w[0])
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))
    assert rel_err(got[[0, 2]], ex[[0, 2]]) <= 1e-12


@pytest.mark.gpu
def test_degenerate_and_rules(gpu):
    """A pair at D == 0: at the neutral configuration (q = 0) every joint rotation is the identity, so a sphere at the origin of
    joint 5 and a sphere of joint 4 whose offset is joint 5's placement in joint 4 coincide exactly.  That pair gives its value
    1/2 w (r_a + r_b + m)^2 and no derivative.  Then every refusal of the interface, set_pairs again (the same list keeps the
    data, another resets it) and the live rule on half-batch uploads of zeros"""
    import ctypes as C
    capi = gpu
    T, B = 2, 2
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)
    pp5 = tuple(float(v) for v in np.asarray(model.pp).reshape(-1, 3)[5])
    pts = [(5, (0.0, 0.0, 0.0), 0.03), (4, pp5, 0.05), (0, (0.1, 0.0, 0.05), 0.04)]
    pairs = [(0, 1), (0, 2)]
    xs = np.zeros((B, (T + 1) * o.nx))
    us = np.zeros((B, T * o.m))
    assert np.array_equal(o.frame_position(5, pts[0][1], xs[0][:o.nq]), o.frame_position(4, pp5, xs[0][:o.nq]))
    margin, wgt = np.array([0.02, -10.0]), np.array([3.0, 7.0])
    value = 0.5 * wgt[0] * (0.03 + 0.05 + 0.02) ** 2
    mults = tc._mults(o, xs[0], 43)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST if on else 0) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if on:
                set_task(ctx, pts, pairs, margin, wgt)
                assert np.all(ctx.self_collision_clearance(0) == -(0.03 + 0.05 + 0.02))
            ctx.linearize()
            ctx.cost_seq_aug(0, 1.0)
            got[on] = {s: ctx.download(s) for s in DERIVS + ("COSTS_OLD",)}
    for s in DERIVS:
        assert np.array_equal(got[True][s], got[False][s]), s               # no derivative anywhere
    extra = got[True]["COSTS_OLD"] - got[False]["COSTS_OLD"]
    assert np.max(np.abs(extra - value)) <= 1e-12 * max(1.0, np.max(np.abs(got[False]["COSTS_OLD"]))), extra

    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    T, B = 4, 4
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    pts = pick_points(model)
    pairs = all_pairs(pts)
    npair = len(pairs)
    same_joint = next((a, b) for a in range(len(pts)) for b in range(a + 1, len(pts)) if pts[a][0] == pts[b][0])
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_self_collision_pairs(points=pts, pairs=pairs)) == capi.E_UNSUPPORTED
        with pytest.raises(ValueError):                              # the wrapper has no pair count to check shapes against
            ctx.set_self_collision_cost(weight=np.ones(npair))
        z = np.ones(B * (T + 1) * npair)
        assert L.ddp_hip_self_collision_upload(ctx._h, None, z.ctypes.data_as(dp), 0, 1) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.self_collision_cost()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.self_collision_clearance()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_SELF_COLLISION_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST) as ctx:   # the flag stands alone: no obstacle flag beside it
        with pytest.raises(ValueError):
            ctx.set_self_collision_cost(weight=np.ones(npair))
        z = np.ones(B * (T + 1) * npair)
        assert L.ddp_hip_self_collision_upload(ctx._h, None, z.ctypes.data_as(dp), 0, B) == capi.E_ARG   # before set_pairs
        assert code(lambda: ctx.self_collision_clearance()) == capi.E_ARG
        many_pts = [(k % (model.nv - 5), pts[0][1], 0.01) for k in range(capi.MAX_COLLISION_POINTS + 1)]
        many_pairs = [pairs[k % npair] for k in range(capi.MAX_COLLISION_PAIRS + 1)]
        for bad_pts, bad_pairs in (([], pairs), (pts[:1], [(0, 0)]), (many_pts, [(0, 1)]), (pts, []), (pts, many_pairs),
                                   ([(model.nv - 5, pts[0][1], 0.1)] + pts[1:], pairs), ([(-1, pts[0][1], 0.1)] + pts[1:], pairs),
                                   ([(0, (0.0, np.nan, 0.0), 0.1)] + pts[1:], pairs), ([(0, (0.0, np.inf, 0.0), 0.1)] + pts[1:], pairs),
                                   ([(0, pts[0][1], -1e-3)] + pts[1:], pairs), ([(0, pts[0][1], np.nan)] + pts[1:], pairs),
                                   ([(0, pts[0][1], np.inf)] + pts[1:], pairs),
                                   (pts, [(0, len(pts))]), (pts, [(len(pts), 0)]), (pts, [(-1, 0)]), (pts, [(0, -1)]),
                                   (pts, [(2, 2)]), (pts, [same_joint]), (pts, [same_joint[::-1]]), (pts, pairs + [same_joint])):
            assert code(lambda: ctx.set_self_collision_pairs(points=bad_pts, pairs=bad_pairs)) == capi.E_ARG, (bad_pts, bad_pairs)
        assert code(lambda: ctx.self_collision_clearance()) == capi.E_ARG     # a refused set_pairs sets nothing
        ctx.set_self_collision_pairs(points=pts, pairs=pairs + [pairs[0], pairs[0][::-1]])   # duplicates are allowed
        ctx.set_self_collision_pairs(points=pts, pairs=pairs)
        m0, w0 = ctx.self_collision_cost()                                    # defaults: margins 0, weights 0
        assert m0.shape == (B, T + 1, npair) and w0.shape == (B, T + 1, npair) and np.all(m0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        mg, wg = rng.normal(size=(B, T + 1, npair)), rng.uniform(0, 1, size=(B, T + 1, npair))
        ctx.set_self_collision_cost(margin=mg, weight=wg)
        per_m, per_w = mg[0].copy(), wg[0].copy()
        for bad in (-1e-3, np.nan, np.inf):
            wb = per_w.copy(); wb[1, 2] = bad
            assert code(lambda: ctx.set_self_collision_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_self_collision_cost(margin=per_m, weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, np.inf, -np.inf):
            mb = per_m.copy(); mb[2, 1] = bad
            assert code(lambda: ctx.set_self_collision_cost(margin=mb, weight=per_w)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_self_collision_cost(margin=mb)) == capi.E_ARG, bad
        assert code(lambda: ctx.set_self_collision_cost(weight=per_w, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_self_collision_cost(weight=per_w, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_self_collision_cost(weight=per_w, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.self_collision_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros((B + 1) * (T + 1) * npair)
        assert L.ddp_hip_self_collision_upload(ctx._h, None, z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        assert L.ddp_hip_self_collision_clearance(ctx._h, 2, z.ctypes.data_as(dp)) == capi.E_ARG
        assert L.ddp_hip_self_collision_clearance(ctx._h, 0, None) == capi.E_ARG
        m1, w1 = ctx.self_collision_cost()
        assert np.array_equal(m1, mg) and np.array_equal(w1, wg)                # a refused upload leaves both sides as they were
        mneg = -np.abs(per_m) - 1.0
        ctx.set_self_collision_cost(margin=mneg, first=1, count=1)              # one side, one instance (a negative margin); the weights stay
        m1, w1 = ctx.self_collision_cost()
        assert np.array_equal(m1[0], mg[0]) and np.array_equal(m1[1], mneg) and np.array_equal(m1[2:], mg[2:]) and np.array_equal(w1, wg)
        m2, w2 = ctx.self_collision_cost(first=1, count=2)                      # the round trip of a range of instances
        assert np.array_equal(m2, m1[1:3]) and np.array_equal(w2, wg[1:3])
        bw = np.arange(npair, dtype=float)
        ctx.set_self_collision_cost(weight=bw, first=1, count=2)                # broadcast: (n_pairs,)
        assert np.array_equal(ctx.self_collision_cost()[1][1:3], np.broadcast_to(bw, (2, T + 1, npair)))
        assert np.array_equal(ctx.self_collision_cost()[1][0], wg[0])
        ctx.set_self_collision_cost(margin=per_m[0])
        assert np.array_equal(ctx.self_collision_cost()[0], np.broadcast_to(per_m[0], (B, T + 1, npair)))
        # set_pairs again: the same list keeps the data (the points may move, the radii change), another list resets it
        moved = [(j, tuple(0.5 * np.asarray(off)), 2.0 * r) for j, off, r in pts]
        ctx.set_self_collision_pairs(points=moved, pairs=pairs)
        m3, w3 = ctx.self_collision_cost()
        assert np.array_equal(m3, np.broadcast_to(per_m[0], (B, T + 1, npair))) and np.any(w3 != 0.0)
        ctx.set_self_collision_pairs(points=pts, pairs=pairs[:-1] + [pairs[-1][::-1]])   # the same count, one pair the other way round
        m4, w4 = ctx.self_collision_cost()
        assert np.all(m4 == 0.0) and np.all(w4 == 0.0)
        ctx.set_self_collision_cost(weight=np.ones(npair))
        ctx.set_self_collision_pairs(points=pts, pairs=pairs[:4])
        m5, w5 = ctx.self_collision_cost()
        assert m5.shape == (B, T + 1, 4) and np.all(m5 == 0.0) and np.all(w5 == 0.0)
        # the live rule: zeros that arrive half-batch by half-batch leave the kernels launched, with the flag-off bits
        xs, us = _trajs(o, model, B, 161)
        _setup(ctx, xs, us)
        ctx.set_self_collision_pairs(points=pts, pairs=pairs)
        ctx.linearize()
        off = {s: ctx.download(s) for s in DERIVS}
        m, w = random_task(o, pts, pairs, xs, B, 162, p_clear=0.0)
        ctx.set_self_collision_cost(margin=m, weight=w)
        ctx.linearize()
        assert not np.array_equal(ctx.download("LX"), off["LX"])
        ctx.set_self_collision_cost(weight=np.zeros(npair), first=0, count=B // 2)
        ctx.linearize()
        lx = ctx.download("LX")
        assert np.array_equal(lx[:B // 2], off["LX"][:B // 2]) and not np.array_equal(lx[B // 2:], off["LX"][B // 2:])
        ctx.set_self_collision_cost(weight=np.zeros(npair), first=B // 2, count=B - B // 2)
        ctx.linearize()
        for s in DERIVS:
            assert np.array_equal(ctx.download(s), off[s]), s
        assert np.all(ctx.self_collision_clearance(0) == np.inf)


FOLD_WEIGHT = 2e4


def fold_task(o, model, xs0):
    """chain6: a sphere on the base joint and one on the last joint, and the posture within 1 rad per joint of the start that brings
    them closest (a coordinate search on the yardstick).  The radii make that posture penetrate by 10 cm"""
    base, end = (0, (0.0, 0.0, 0.05), 0.0), (5, (0.0, 0.0, 0.0823), 0.0)
    q0 = xs0[:o.nq].copy()

    def dist(q):
        return float(np.linalg.norm(o.frame_position(end[0], end[1], q) - o.frame_position(base[0], base[1], q)))
    q = q0.copy()
    for _ in range(4):
        for j in range(1, o.nv):
            cand = q0[j] + np.linspace(-1.0, 1.0, 41)
            vals = []
            for c in cand:
                qq = q.copy(); qq[j] = c
                vals.append(dist(qq))
            q[j] = cand[int(np.argmin(vals))]
    r = 0.5 * (dist(q) + 0.10)
    pts = [(base[0], base[1], r), (end[0], end[1], r)]
    return pts, [(0, 1)], q, dist(q0) - 2 * r


@pytest.mark.gpu
def test_fold_task(gpu):
    """chain6, T = 40, no constraint: a tracking cost pulls the arm to a posture that folds the end sphere into the base sphere.
    The flag-off solve penetrates by more than 1 cm (asserted on the yardstick).  With the term on, from the same start, the least
    clearance of the result is strictly larger, and its full cost -- tracking and self-collision, evaluated with numpy -- is no
    larger than the initial trajectory's.  Measured on an MI355X with weight 2e4: least clearance -2.76 cm without the flag,
    -1.35 cm with it"""
    capi = gpu
    T, mu, iters = 40, 1.0, 12
    model, spec, o = _reach_problem(T)
    xs, us = _trajs(o, model, 1, 141, held=True)
    pts, pairs, q_goal, start = fold_task(o, model, xs[0])
    goal = np.concatenate([q_goal, np.zeros(o.nv)])
    xref = np.tile(goal, (T + 1, 1))
    wx = np.tile(np.concatenate([np.full(o.nv, 200.0), np.full(o.nv, 1.0)]), (T + 1, 1))
    wx[T] *= 10.0
    ref = {"xref": xref[None], "wx": wx[None], "uref": np.zeros((1, T, o.m)), "wu": np.zeros((1, T, o.m))}
    margin, weight = np.zeros((T + 1, 1)), np.full((T + 1, 1), FOLD_WEIGHT)

    def full_cost(X, U):
        return float(tc.full_cost(o, 1.0, X, U, ref).sum() + sc_terms(o, pts, pairs, X, margin, weight).sum())

    def solve(ctx):
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            if step[0] > 0.0:
                ctx.swap_traj()
        return ctx.download("X"), ctx.download("U")
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS | (capi.FLAG_SELF_COLLISION_COST if on else 0)) as ctx:
            _setup(ctx, xs, us)
            ctx.set_tracking_cost(xref=xref, wx=wx)
            if on:
                set_task(ctx, pts, pairs, margin, weight)
            res[on] = solve(ctx)
    clear_off = float(np.min(sc_clearance(o, pts, pairs, res[False][0][0], margin, weight)))
    clear_on = float(np.min(sc_clearance(o, pts, pairs, res[True][0][0], margin, weight)))
    c0, c1 = full_cost(xs[0], us[0]), full_cost(res[True][0][0], res[True][1][0])
    print("fold: clearance at the start", start, "flag off", clear_off, "flag on", clear_on, "weight", FOLD_WEIGHT, "cost", c0, "->", c1)
    assert clear_off < -0.01, clear_off                                     # the flag-off solve folds through
    assert clear_on > clear_off, (clear_on, clear_off)
    assert c1 <= c0, (c0, c1)
