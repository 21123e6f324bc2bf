"""Per-instance capsule collision costs (DDP_HIP_FLAG_CAPSULE_COST, include/ddp_hip/ddp_hip.h): capsules on the robot (capsule k: the
segment end0_k .. end1_k fixed in joint_k, radius r_k) in pairs i, body A robot capsule a_i and body B another robot capsule
(VS_ROBOT), a world capsule (VS_CAPSULE) or a half-space (VS_HALFSPACE) of the pair's own eight doubles per (instance, t),

    D_i = |c_a - c_b|,   d_i = D_i - (r_a + r_b + m_i),   u_i = (c_a - c_b) / D_i,   e_i = d_i < 0 ? d_i : 0
    half-space:  d_i = min_end(n . p_end) - h - r_a - m_i,   u_i = n
    l(t, x, u) += 1/2 sum_i w[b][t][i] e_i^2,   lf alike at T

with c_a, c_b the closest points of the two segments by the rule the header pins.  The oracle has no such cost, so the yardstick is
the numpy restatement below, built on Oracle.frame_position and Oracle.frame_jacobian(world_aligned=True): the closest points are
frozen in their joints with s and t held, z_i = + P_ca^T u_i on the tangent columns of path(A) alone, - P_cb^T u_i on those of
path(B) alone (a world body has no path: all of path(A)), lx += w e z, lxx += w z z^T over the pairs with w != 0, e != 0 and
(segments) D != 0.  The helpers of test_self_collision_cost.py, test_obstacle_cost.py and the others are reused by import;
tolerances are theirs.

The task generator sets activity through the margins: m = (what d is with m = 0) +- depth with depth in 0.01 .. 0.1.  check_task
asserts on the yardstick alone that no live pair sits within 1e-6 of its margin, has D < 1e-3, has den / (A E) < 1e-3 where both
segments have length, or has a closest-point parameter whose unclamped value lies within 1e-6 of 0 or 1 (the generator also keeps
a half-space's two ends 1e-3 apart along the normal): device and numpy then cannot disagree about activity or branch.  The
generator drops the pairs that miss the condition (weight 0) and asserts that these are at most a quarter."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_advance as adv
import test_frame_cost as fc
import test_frame_vel_cost as fv
import test_obstacle_cost as ob
import test_self_collision_cost as sc
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W5 = ob.H, ob.W5
DERIVS, NAMES = fc.DERIVS, fc.NAMES
make_any = sc.make_any
_trajs, _setup = tc._trajs, tc._setup
_emulate_forward, _reach_problem = ob._emulate_forward, ob._reach_problem
ROBOT, WORLD, HALF = 0, 1, 2


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _clamp(x):
    return 0.0 if x < 0.0 else (1.0 if x > 1.0 else x)


def closest_params(a0, a1, b0, b1):
    """(s, t, info) by the header's rule, every product rounded on its own.  info: A, E, den (None in the degenerate branches) and
    the unclamped values of every parameter that went through a clamp"""
    a0, a1, b0, b1 = ([float(v) for v in p] for p in (a0, a1, b0, b1))
    d1 = [a1[k] - a0[k] for k in range(3)]
    d2 = [b1[k] - b0[k] for k in range(3)]
    r = [a0[k] - b0[k] for k in range(3)]
    A, E, F, C = _dot(d1, d1), _dot(d2, d2), _dot(d2, r), _dot(d1, r)
    info = {"A": A, "E": E, "den": None, "raw": []}
    if A == 0.0 and E == 0.0:
        return 0.0, 0.0, info
    if A == 0.0:
        info["raw"].append(F / E)
        return 0.0, _clamp(F / E), info
    if E == 0.0:
        info["raw"].append(-C / A)
        return _clamp(-C / A), 0.0, info
    Bv = _dot(d1, d2)
    den = A * E - Bv * Bv
    info["den"] = den
    s = 0.0
    if den > 0.0:
        info["raw"].append((Bv * F - C * E) / den)
        s = _clamp((Bv * F - C * E) / den)
    t = (Bv * s + F) / E
    info["raw"].append(t)
    if t < 0.0:
        t = 0.0
        info["raw"].append(-C / A)
        s = _clamp(-C / A)
    elif t > 1.0:
        t = 1.0
        info["raw"].append((Bv - C) / A)
        s = _clamp((Bv - C) / A)
    return s, t, info


def pick_capsules(model):
    """five capsules on the joints of ob.pick_points (a root-side joint, a mid-tree joint twice, two leaves): four segments of
    8 .. 20 cm and one sphere (end0 == end1); one radius is 0"""
    pts = ob.pick_points(model)
    delta = [(0.12, 0.02, -0.05), (-0.03, 0.2, 0.04), (0.05, -0.06, 0.15), (0.0, 0.0, 0.0), (0.02, 0.08, -0.03)]
    return [(j, tuple(off), tuple(np.asarray(off) + np.asarray(dl)), r) for (j, off, r), dl in zip(pts, delta)]


def pick_pairs(caps):
    """every pair of robot capsules on different joints (9), every capsule against a world capsule (5) and against a half-space
    (5): 19 pairs, more than the 16 lanes a state has in the value kernels"""
    n = len(caps)
    rob = [(a, ROBOT, b) for a in range(n) for b in range(a + 1, n) if caps[a][0] != caps[b][0]]
    return rob + [(a, WORLD, 0) for a in range(n)] + [(a, HALF, 0) for a in range(n)]


def ends(o, caps, q):
    return [(o.frame_position(j, e0, q), o.frame_position(j, e1, q)) for j, e0, e1, _ in caps]


def pair_eval(caps, E, pair, g):
    """one pair from the capsules' world ends E and its eight doubles g (margin included): a dict with D (None for a half-space),
    d, u (None where the closest points coincide), the closest-point parameters s (body A) and t (body B), and info"""
    a, kind, b = pair
    a0, a1 = E[a]
    ra = caps[a][3]
    if kind == HALF:
        n = np.asarray(g[:3], dtype=float)
        p0, p1 = _dot(n, a0), _dot(n, a1)
        second = p1 < p0
        return {"D": None, "d": (p1 if second else p0) - g[3] - ra - g[7], "u": n, "s": 1.0 if second else 0.0, "t": None,
                "info": {"gap": abs(p1 - p0), "sphere": bool(np.array_equal(a0, a1))}}
    b0, b1 = E[b] if kind == ROBOT else (np.asarray(g[0:3], dtype=float), np.asarray(g[3:6], dtype=float))
    rb = caps[b][3] if kind == ROBOT else g[6]
    s, t, info = closest_params(a0, a1, b0, b1)
    ca = np.array([a0[k] + s * (a1[k] - a0[k]) for k in range(3)])
    cb = np.array([b0[k] + t * (b1[k] - b0[k]) for k in range(3)])
    diff = ca - cb
    D = float(np.sqrt(_dot(diff, diff)))
    return {"D": D, "d": D - (ra + rb + g[7]), "u": diff / D if D != 0.0 else None, "s": s, "t": t, "info": info, "ca": ca, "cb": cb}


def cp_term(o, caps, pairs, q, g_t, w_t):
    """1/2 sum_i w e^2 at one configuration, the pairs in ascending order; and whether a pair is active"""
    E = ends(o, caps, q)
    s, act = 0.0, False
    for i, pair in enumerate(pairs):
        if w_t[i] == 0.0:
            continue
        d = pair_eval(caps, E, pair, g_t[i])["d"]
        if not d >= 0:
            s += w_t[i] * d * d
            act = True
    return 0.5 * s, act


def cp_terms(o, caps, pairs, xs, g, w):
    """the capsule terms of one instance per t (T+1 values; the last belongs to lf); g: (T+1, n_pairs, 8), w: (T+1, n_pairs)"""
    X = xs.reshape(o.T + 1, o.nx)
    return np.array([cp_term(o, caps, pairs, X[t][:o.nq], g[t], w[t])[0] for t in range(o.T + 1)])


def cp_clearance(o, caps, pairs, xs, g, w):
    """min over the pairs with w != 0 of d_i per t; +inf where no pair is live"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.full(o.T + 1, np.inf)
    for t in range(o.T + 1):
        E = ends(o, caps, X[t][:o.nq])
        for i, pair in enumerate(pairs):
            if w[t][i] != 0.0:
                out[t] = min(out[t], pair_eval(caps, E, pair, g[t][i])["d"])
    return out


def _path_cols(model, j):
    return [c for i in fv.path_of(model, j) for c in fv.cols_of(model, i)]


def cp_z(o, model, caps, pair, q, ev):
    """z_i over the nv tangent columns, exact zero off the pair's column set; and the column set.  The closest points are points
    of their joints: end0 + s (end1 - end0) with s held"""
    a, kind, b = pair
    ja, e0, e1, _ = caps[a]
    offa = np.asarray(e0) + ev["s"] * (np.asarray(e1) - np.asarray(e0))
    if kind == ROBOT:
        jb, f0, f1, _ = caps[b]
        offb = np.asarray(f0) + ev["t"] * (np.asarray(f1) - np.asarray(f0))
        ca, cb = sc.sym_cols(model, ja, jb)
    else:
        ca, cb = _path_cols(model, ja), []
    z = np.zeros(o.nv)
    if ca:
        z[ca] = o.frame_jacobian(ja, offa, q, world_aligned=True)[:, ca].T @ ev["u"]
    if cb:
        z[cb] = -(o.frame_jacobian(jb, offb, q, world_aligned=True)[:, cb].T @ ev["u"])
    return z, ca + cb


def cp_grad_hess(o, model, caps, pairs, x, g_t, w_t):
    """(lx, lxx) contributions at one state, n and n x n, and the tangent rows of the active pairs' column sets (a mask over n)"""
    nv, n = o.nv, o.n
    g, Hm, rows = np.zeros(n), np.zeros((n, n)), np.zeros(n, dtype=bool)
    q = x[:o.nq]
    E = ends(o, caps, q)
    for i, pair in enumerate(pairs):
        if w_t[i] == 0.0:
            continue
        ev = pair_eval(caps, E, pair, g_t[i])
        if not ev["d"] < 0 or ev["u"] is None:
            continue
        z, cols = cp_z(o, model, caps, pair, q, ev)
        rows[cols] = True
        g[:nv] += w_t[i] * ev["d"] * z
        Hm[:nv, :nv] += w_t[i] * np.outer(z, z)          # entry (r, c) and (c, r) alike: symmetric bit for bit
    return g, Hm, rows


def cp_derivs(o, model, caps, pairs, xs, g, w):
    """what the terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout, and the active rows
    per t"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": [], "rows": []}
    for t in range(o.T + 1):
        gr, Hm, rows = cp_grad_hess(o, model, caps, pairs, X[t], g[t], w[t])
        out["rows"].append(rows)
        if t == o.T:
            out["LFX"], out["LFXX"] = gr, Hm.ravel(order="F")
        else:
            out["LX"].append(gr); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.sqrt(v @ v)


def pair_ok(ev, guard=1e-6):
    """the generator's condition on one live pair (module docstring); guard: how far an unclamped parameter stays from 0 and 1"""
    if abs(ev["d"]) < 1e-6:
        return False
    if ev["D"] is None:
        return ev["info"]["sphere"] or ev["info"]["gap"] >= 1e-3
    info = ev["info"]
    if ev["D"] < 1e-3:
        return False
    if info["den"] is not None and info["den"] / (info["A"] * info["E"]) < 1e-3:
        return False
    return all(min(abs(r), abs(r - 1.0)) >= guard for r in info["raw"])


def random_task(o, caps, pairs, xs, B, seed, wscale=1.0, p_clear=0.5, guard=1e-6):
    """geom (B, T+1, n_pairs, 8) and weights (B, T+1, n_pairs), every instance and t its own.  A world capsule: a segment of
    0 .. 40 cm (one in five a sphere) some 10 .. 40 cm from body A, rho in 0 .. 8 cm; a half-space: a random unit normal.  Per
    (instance, t): with probability p_clear a block in which every pair is clear of its margin by 0.01 .. 0.1, else a block in
    which each pair penetrates by 0.01 .. 0.1 (at least one pair) or stays clear by as much.  A pair that misses the generator's
    condition is dropped (weight 0); at most a quarter may be"""
    rng = np.random.default_rng(seed)
    T, npair = o.T, len(pairs)
    g = np.zeros((B, T + 1, npair, 8))
    w = wscale * rng.uniform(0.5, 5.0, size=(B, T + 1, npair))
    dropped = 0
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            E = ends(o, caps, X[t][:o.nq])
            clear_block = rng.uniform() < p_clear
            forced = int(rng.integers(npair))
            for i, pair in enumerate(pairs):
                a, kind, _ = pair
                mid = 0.5 * (E[a][0] + E[a][1])
                if kind == WORLD:
                    c = mid + rng.uniform(0.1, 0.4) * _unit(rng)
                    half = (0.0 if rng.uniform() < 0.2 else rng.uniform(0.02, 0.2)) * _unit(rng)
                    g[b, t, i, 0:3], g[b, t, i, 3:6], g[b, t, i, 6] = c - half, c + half, rng.uniform(0.0, 0.08)
                elif kind == HALF:
                    n = _unit(rng)
                    g[b, t, i, 0:3], g[b, t, i, 3] = n, float(n @ mid) - rng.uniform(0.0, 0.3)
                    g[b, t, i, 4:7] = rng.normal(size=3)           # ignored entries: finite, not zero
                else:
                    g[b, t, i, 0:7] = rng.normal(size=7)
                depth = rng.uniform(0.01, 0.1)
                inside = (not clear_block) and (i == forced or rng.uniform() < 0.6)
                d0 = pair_eval(caps, E, pair, g[b, t, i])["d"]            # (the margin is still 0)
                g[b, t, i, 7] = d0 + (depth if inside else -depth)
                if not pair_ok(pair_eval(caps, E, pair, g[b, t, i]), guard):
                    w[b, t, i] = 0.0
                    dropped += 1
    assert 4 * dropped <= B * (T + 1) * npair, (dropped, B * (T + 1) * npair)
    return g, w


def check_task(o, caps, pairs, xs, g, w, fractions=True):
    """the conditions on the inputs, on the yardstick alone (module docstring); at least a quarter of the (instance, t) blocks have
    an active pair and at least a quarter have none.  Returns the blocks' activity (B, T+1)"""
    B, T = xs.shape[0], o.T
    active = np.zeros((B, T + 1), dtype=bool)
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            E = ends(o, caps, X[t][:o.nq])
            for i, pair in enumerate(pairs):
                if w[b, t, i] == 0.0:
                    continue
                ev = pair_eval(caps, E, pair, g[b, t, i])
                assert pair_ok(ev), (b, t, i, ev)
                active[b, t] |= ev["d"] < 0
    if fractions:
        assert 4 * active.sum() >= active.size and 4 * (~active).sum() >= active.size, (active.sum(), active.size)
    return active


def set_task(ctx, caps, pairs, geom=None, weight=None):
    ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
    if geom is not None or weight is not None:
        ctx.set_capsule_cost(geom=geom, weight=weight)


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff", "table7"])
def test_yardstick_gradient(name):
    """lx against the 5-point central difference of the term's own value (closest points re-formed at every point of the stencil:
    the envelope theorem) at states with active pairs, at the siblings' tolerance; lxx symmetric bit for bit and positive
    semidefinite, with zero velocity rows and columns and zero rows outside the active pairs' column sets; a robot pair leaves a
    free-flyer root's rows alone, a world pair does not.  The stencil spans +-2e-3 per coordinate, so this test's generator keeps
    every unclamped parameter 0.05 away from 0 and 1: the distance is C1 across a clamp but not C2"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    assert len(pairs) == 19 and any(c[1] == c[2] for c in caps)
    xs, us = _trajs(o, model, 1, 3)
    g, w = random_task(o, caps, pairs, xs, 1, 4, p_clear=0.0, guard=0.05)
    for t in range(T + 1):                                   # a half-space's lower end must not change within the stencil
        E = ends(o, caps, xs[0].reshape(T + 1, o.nx)[t][:o.nq])
        for i, pair in enumerate(pairs):
            ev = pair_eval(caps, E, pair, g[0, t, i])
            if pair[1] == HALF and not ev["info"]["sphere"] and ev["info"]["gap"] < 0.02:
                w[0, t, i] = 0.0
    check_task(o, caps, pairs, xs, g, w, fractions=False)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    for t in (1, T):
        gr, Hm, rows = cp_grad_hess(o, model, caps, pairs, X[t], g[0, t], w[0, t])
        assert np.max(np.abs(gr[:nv])) > 0 and rows.any()

        def cost_at(dx):
            return cp_term(o, caps, pairs, tc._integrate_x(o, X[t], dx)[:o.nq], g[0, t], w[0, t])[0]
        fd = np.zeros(n)
        for c in range(n):
            e = np.zeros(n); e[c] = H
            fd[c] = sum(cw * cost_at(s * e) for s, cw in W5) / H
        assert np.max(np.abs(fd - gr)) <= 1e-8 * max(1.0, np.max(np.abs(gr))), (t, np.max(np.abs(fd - gr)))
        assert np.array_equal(Hm, Hm.T)
        assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(gr[nv:] == 0.0)
        assert np.all(gr[~rows] == 0.0) and np.all(Hm[~rows, :] == 0.0)
        assert np.min(np.linalg.eigvalsh(Hm)) >= -1e-12 * np.max(np.abs(Hm))
        if model.ff:
            rob = [k for k, p in enumerate(pairs) if p[1] == ROBOT]
            gr_r, Hm_r, rows_r = cp_grad_hess(o, model, caps, [pairs[k] for k in rob], X[t], g[0, t][rob], w[0, t][rob])
            assert rows_r.any() and not rows_r[:6].any() and np.all(gr_r[:6] == 0.0) and np.all(Hm_r[:6, :] == 0.0)
            assert rows[:6].all()


def test_closest_points_are_closest():
    """the restated rule against a 201 x 201 scan of (s, t), as host/test_capsule_block.cpp holds the library's routine"""
    rng = np.random.default_rng(11)
    grid = np.linspace(0.0, 1.0, 201)
    for trial in range(40):
        a0, a1, b0, b1 = rng.uniform(-1, 1, size=(4, 3))
        if trial % 5 == 1:
            a1 = a0.copy()
        if trial % 7 == 2:
            b1 = b0 + 0.6 * (a1 - a0)
        s, t, _ = closest_params(a0, a1, b0, b1)
        D = np.linalg.norm(a0 + s * (a1 - a0) - b0 - t * (b1 - b0))
        pa = a0[None, :] + grid[:, None] * (a1 - a0)[None, :]
        pb = b0[None, :] + grid[:, None] * (b1 - b0)[None, :]
        best = np.min(np.linalg.norm(pa[:, None, :] - pb[None, :, :], axis=2))
        assert 0.0 <= s <= 1.0 and 0.0 <= t <= 1.0
        assert best - (np.linalg.norm(a1 - a0) + np.linalg.norm(b1 - b0)) / 400 - 1e-12 <= D <= best + 1e-12, (trial, D, best)


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_CAPSULE_COST == 131072 and re.search(r"#define\s+DDP_HIP_FLAG_CAPSULE_COST\s+131072u", header)
    assert capi.MAX_CAPSULES == 16 and re.search(r"#define\s+DDP_HIP_MAX_CAPSULES\s+16\b", header)
    assert capi.MAX_CAPSULE_PAIRS == 32 and re.search(r"#define\s+DDP_HIP_MAX_CAPSULE_PAIRS\s+32\b", header)
    for k, name in enumerate(("ROBOT", "CAPSULE", "HALFSPACE")):
        assert getattr(capi, "CAPSULE_VS_" + name) == k and re.search(r"#define\s+DDP_HIP_CAPSULE_VS_%s\s+%d\b" % (name, k), header)
    L = capi.lib()
    for name in ("ddp_hip_capsule_set_pairs", "ddp_hip_capsule_upload", "ddp_hip_capsule_download", "ddp_hip_capsule_clearance",
                 "ddp_hip_model_capsule_pair"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    for name in ("set_capsule_pairs", "set_capsule_cost", "capsule_cost", "capsule_clearance"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.ModelHandle, "capsule_pair")
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B, npair = 5, 2, 3
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h, ctx.n_capsule_pairs = spec, B, None, 0
    with pytest.raises(ValueError, match="set_capsule_pairs"):
        ctx.set_capsule_cost(weight=np.zeros(npair))
    ctx.n_capsule_pairs = npair
    for kw in (dict(geom=np.zeros((npair, 7))), dict(geom=np.zeros(8)), dict(geom=np.zeros((T, npair, 8))),
               dict(geom=np.zeros((B + 1, T + 1, npair, 8))), dict(weight=np.zeros(npair - 1)), dict(weight=0.0),
               dict(weight=np.zeros((T, npair))), dict(weight=np.zeros((B, T + 1, npair)), count=1),
               dict(geom=np.zeros((npair, 8)), weight=np.zeros((T + 1, npair + 1)))):
        with pytest.raises(ValueError):
            ctx.set_capsule_cost(**kw)
    for bad_caps, bad_pairs in (([(0, (0.0, 0.0), (0.0, 0.0, 0.0), 0.1)], [(0, HALF)]), ([(0, (0.0, 0.0, 0.0), 0.1)], [(0, HALF)]),
                                ([(0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.1), 0.1)], [(0,)])):
        with pytest.raises(ValueError):
            ctx.set_capsule_pairs(capsules=bad_caps, pairs=bad_pairs)


def test_capsule_block_host_logic():
    """host/test_capsule_block.cpp: the term's record and index, the geometry validator by kind, the pair-list rules, what an
    upload decides, and the library's closest-point routine against a scan (csrc/cost_block.h, csrc/capsule_cost.h), which need
    no device"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_capsule_block"])
    out = subprocess.run([os.path.join(host, "test_capsule_block")], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------
LIN_CASES = [("chain6", 2, None, ""), ("tree38", 0, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("table7", 2, None, ""), ("tree38", 2, None, "both")]


def _lin_task(o, model, xs, B, T):
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    g, w = random_task(o, caps, pairs, xs, B, 43)
    w[1, 2, 1] = 0.0; w[0, T, 2] = 0.0; w[2, 1, 0] = 0.0   # one pair's weight off at single (instance, t) entries
    return caps, pairs, g, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different geometry per instance,
    5 capsules (one a sphere) in 19 pairs of all three kinds, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST);
    LXX / LFXX symmetric bit for bit; LU, LUU, LUX, every velocity row and column and the q rows outside the active pairs' column
    sets bit for bit the flag-off values; blocks without an active pair bit for bit flag-off, blocks with one differ.  "both":
    self-collision and obstacles live beside it (the capsules' additions come last)"""
    capi = gpu
    T, B = 3, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    caps, pairs, g, w = _lin_task(o, model, xs, B, T)
    active = check_task(o, caps, pairs, xs, g, w)
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "both":
        base |= capi.FLAG_SELF_COLLISION_COST | capi.FLAG_OBSTACLE_COST
        pts = ob.pick_points(model)
        spairs = sc.all_pairs(pts)
        stask = sc.random_task(o, pts, spairs, xs, B, 44)
        otask = ob.random_task(o, pts, ob.KINDS, xs, B, 50)
        assert sc.check_task(o, pts, spairs, xs, *stask, fractions=False).any() and ob.check_task(o, pts, ob.KINDS, xs, *otask).any()
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_CAPSULE_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "both":
                sc.set_task(ctx, pts, spairs, *stask)
                ob.set_task(ctx, pts, ob.KINDS, *otask)
            if on:
                set_task(ctx, caps, pairs, g, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = cp_derivs(o, model, caps, pairs, xs[b], g[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert s in ("LFX", "LFXX") or np.max(np.abs(add[s])) > 0
            e = rel_err(got[True][s][b], ex)
            worst = max(worst, e)
            print("linearize", name, flags, stages, s, b, e)
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
@pytest.mark.parametrize("name,fd_mode,fo_", [("tree38", 0, None), ("chain6ff", 0, 0), ("table7", 2, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo_):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the flag-off context's values plus the numpy terms, lf included; a block
    without an active pair keeps the flag-off value bit for bit.  19 pairs: two pairs per lane"""
    capi = gpu
    T, B, mu = 4, 3, 30.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    g, w = random_task(o, caps, pairs, xs, B, 52)
    w[1, 3, 0] = 0.0
    active = check_task(o, caps, pairs, xs, g, w)
    xs2 = xs[::-1].copy()                                   # X_NEW: the instances' trajectories in the other order
    us2 = us[::-1].copy()
    g2, w2 = g[::-1].copy(), w[::-1].copy()
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (capi.FLAG_CAPSULE_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if on:
                set_task(ctx, caps, pairs, g, w)
            ctx.cost_seq_aug(0, mu)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                ctx.set_capsule_cost(geom=g2, weight=w2)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, X, gg, ww, act in ((0, xs, g, w, active), (1, xs2, g2, w2, active[::-1])):
        for b in range(B):
            add = cp_terms(o, caps, pairs, X[b], gg[b], ww[b])
            ex = got[False][which][b] + add
            assert np.any(add != 0.0) and np.array_equal(add != 0.0, act[b])
            e = rel_err(got[True][which][b], ex)
            print("cost_seq_aug", name, which, b, e)
            assert e <= 1e-12, (which, b, e)
            assert np.array_equal(got[True][which][b][~act[b]], got[False][which][b][~act[b]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [("tree38", 4, 2, None, 1), ("chain6ff", 4, 2, 0, 0)])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "never"])
def test_untouched_pairs_change_nothing(gpu, name, T, fd_mode, fo_, fwd_path, mode):
    """flag on with nothing uploaded, with pairs within their margins but every weight 0, and with non-zero weights on margins of
    -10 (the kernels run and find no active pair): linearise, both costs, sweep and forward are bit for bit what the flag-off
    context computes, on both forward paths"""
    capi = gpu
    mu, B = 10.0, 2
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    g, w = random_task(o, caps, pairs, xs, B, 33)
    if mode == "never":
        g[..., 7] = -10.0
        assert np.min([cp_clearance(o, caps, pairs, xs[b], g[b], w[b]) for b in range(B)]) > 5.0
    else:
        w[:] = 0.0
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (capi.FLAG_CAPSULE_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on and mode != "nothing":
                set_task(ctx, caps, pairs, g, w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
            if on and mode == "never":
                assert np.min(ctx.capsule_clearance(1)) > 5.0                # the accepted candidate stayed clear as well
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
def test_solve_with_untouched_pairs_changes_nothing(gpu):
    """ddp_hip_solve with non-zero weights on margins of -10: the log and the result are bit for bit the flag-off solve's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 4, 2, 3, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 101, held=True)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    g, w = random_task(o, caps, pairs, xs, B, 102)
    g[..., 7] = -10.0
    w[:] = 50.0
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST if on else 0) as ctx:
            _setup(ctx, xs, us)
            if on:
                set_task(ctx, caps, pairs, g, w)
            log = solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
            res[on] = (log, ctx.download("X"), ctx.download("U"))
    assert not np.array_equal(res[True][1], xs)
    assert np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(res[False][0][k]), np.asarray(res[True][0][k])), k


def blocking_task(o, caps, pairs, geom, xs, us, mults, fb, mu):
    """Margins that leave the trajectory xs clear by exactly 1 cm at every t, per t and pair (the world bodies of `geom` as they
    are), and a weight on the one pair whose distance shrinks most under the full step: five times what the step gains otherwise.
    Returns (geom, weights) of one instance, the full step's cost difference without the term, and by how much that pair approaches"""
    T = o.T
    _, x1, u1 = o.forward_alpha(1.0, xs, us, mults, fb, mu)
    gain = (o.cost_seq_aug(x1, u1, mults, mu) - o.cost_seq_aug(xs, us, mults, mu)).sum()
    Xo, Xn = xs.reshape(T + 1, o.nx), x1.reshape(T + 1, o.nx)
    g = geom.copy()
    g[..., 7] = 0.0

    def d0(X):
        return np.array([[pair_eval(caps, ends(o, caps, X[t][:o.nq]), pair, g[t, i])["d"] for i, pair in enumerate(pairs)]
                         for t in range(T + 1)])
    Do, Dn = d0(Xo), d0(Xn)
    g[..., 7] = Do - 0.01
    shrink = np.max(Do - Dn, axis=0)
    i_ = int(np.argmax(shrink))
    sel = np.zeros((T + 1, len(pairs)))
    sel[:, i_] = 1.0
    unit = cp_terms(o, caps, pairs, x1, g, sel).sum()
    return g, sel * (5.0 * abs(gain) / unit if unit > 0.0 else 0.0), gain, float(shrink[i_])


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path", [("tree38", None, 1), ("chain6ff", 0, 0)])
@pytest.mark.parametrize("n_alpha", [1, 4])
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, n_alpha):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the capsule terms included
    (the siblings' emulation).  The margins (blocking_task) leave the old trajectory clear by 1 cm at every t and weigh the pair
    that the full step brings closest: the test asserts on the emulation alone that the full step is accepted without the term and
    rejected with it, and that every candidate tried decides by more than 1e-9 of the sum of the cost terms' magnitudes; only then
    are decisions compared.  A seed whose full step brings no pair closer by more than 1 cm is passed over"""
    capi = gpu
    T, mu = 16, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        for seed in range(81, 97):
            xs, us = _trajs(o, model, 1, seed, held=True)
            mults = tc._mults(o, xs[0], 85)
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
            geom, _ = random_task(o, caps, pairs, xs, 1, seed + 100)
            g, w, gain, shrink = blocking_task(o, caps, pairs, geom[0], xs[0], us[0], mults, fb, mu_o[0])
            if shrink > 0.01:
                break
        assert shrink > 0.01, shrink
        set_task(ctx, caps, pairs, g, w)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
        clear_old, clear_new = ctx.capsule_clearance(0)[0], ctx.capsule_clearance(1)[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + cp_terms(o, caps, pairs, X, g, w)
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, n_alpha, "seed", seed, "shrink", shrink, "gain", gain, "step", step[0], step_ref, "dcost", dcost[0], new,
          "margins", margins)
    assert gain < 0.0                                                          # without the term the full step is accepted
    assert np.all(cp_terms(o, caps, pairs, xs[0], g, w) == 0.0)                # the old trajectory is clear
    assert step_ref < 1.0 and len(margins) > 1                                 # with it the full step is rejected
    assert min(margins) > 1e-9, margins
    assert step[0] == step_ref, (step, step_ref)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)
    assert rel_err(clear_old, np.full(T + 1, 0.01)) < 1e-9
    assert rel_err(clear_new, cp_clearance(o, caps, pairs, xn_ref, g, w)) < 1e-9


@pytest.mark.gpu
def test_sweep_matches_oracle(gpu):
    """the backward sweep with the device's LX / LXX carrying the term against Oracle.backward: restarts, mu and reg identical,
    every step redone alone by the oracle from the device's V(t+1) to 1e-10 (stepwise_backward_check)"""
    from oracle.binding import Oracle
    capi = gpu
    name, T, mu = "tree38", 4, 1.0
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    g, w = random_task(o, caps, pairs, xs, 1, 72, wscale=10.0, p_clear=0.0)
    check_task(o, caps, pairs, xs, g, w, fractions=False)
    mults = tc._mults(o, xs[0], 73)
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, caps, pairs, g, w)
        ctx.linearize()
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        d = o.alloc_derivs()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
        add = cp_derivs(o, model, caps, pairs, xs[0], g[0], w[0])
        assert np.max(np.abs(add["LX"])) > 0 and np.max(np.abs(d["lx"][:T * o.n])) > 0
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0 and not o.Etot

    def one_step_oracle(t):
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < 1e-10, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("tree38", None), ("chain6ff", 0), ("table7", None)])
def test_clearance(gpu, name, fo_):
    """ddp_hip_capsule_clearance against the yardstick to 1e-12 along X and X_NEW, +inf where no pair is live, E_ARG before
    set_capsule_pairs, +inf everywhere before any weight is live"""
    capi = gpu
    T, B = 4, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 121)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    g, w = random_task(o, caps, pairs, xs, B, 124)
    w[1, 2, :] = 0.0; w[2, T, :] = 0.0; w[0, 1, 1] = 0.0
    check_task(o, caps, pairs, xs, g, w)
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        with pytest.raises(capi.DdpHipError) as exc:
            ctx.capsule_clearance(0)
        assert exc.value.code == capi.E_ARG
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        assert np.all(ctx.capsule_clearance(0) == np.inf)                   # pairs set, no live weight
        ctx.set_capsule_cost(geom=g, weight=w)
        got = ctx.capsule_clearance(0)
        ex = np.stack([cp_clearance(o, caps, pairs, xs[b], g[b], w[b]) for b in range(B)])
        assert got[1, 2] == np.inf and got[2, T] == np.inf and np.array_equal(np.isinf(got), np.isinf(ex))
        fin = np.isfinite(ex)
        assert np.min(ex[fin]) < 0 < np.max(ex[fin])
        e = np.max(np.abs(got[fin] - ex[fin]) / np.maximum(1.0, np.abs(ex[fin])))
        print("clearance", name, e)
        assert e <= 1e-12, e
        xn = np.roll(xs, 1, axis=0)
        ctx.upload("X_NEW", xn)
        got1 = ctx.capsule_clearance(1)
        ex1 = np.stack([cp_clearance(o, caps, pairs, xn[b], g[b], w[b]) for b in range(B)])
        assert np.array_equal(np.isinf(got1), np.isinf(ex1))
        e1 = np.max(np.abs(got1[fin] - ex1[fin]) / np.maximum(1.0, np.abs(ex1[fin])))
        assert e1 <= 1e-12, e1
        assert np.array_equal(ctx.capsule_clearance(0), got)                # X is where it was


@pytest.mark.gpu
def test_clearance_keeps_nan(gpu):
    """a non-finite configuration entry that only the leaf's capsule depends on (the leaf joint's angle) gives a NaN clearance at
    that (instance, t), whichever place its pairs have in the list, and nowhere else"""
    capi = gpu
    T = 2
    model, spec, o = _reach_problem(T)
    xs, us = _trajs(o, model, 1, 151)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    leaf = max(c[0] for c in caps)
    k_leaf = [c[0] for c in caps].index(leaf)
    assert any(p[0] == k_leaf for p in pairs[:-1]) and pairs[-1][0] != k_leaf    # finite pairs are folded after a NaN one
    g, w = random_task(o, caps, pairs, xs, 1, 152)
    bad = xs.copy()
    bad[0, 1 * o.nx + leaf] = np.nan
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as ctx:
        _setup(ctx, bad, us)
        set_task(ctx, caps, pairs, g, w)
        got = ctx.capsule_clearance(0)[0]
    ex = cp_clearance(o, caps, pairs, xs[0], g[0], w[0])
    assert np.isnan(got[1]) and np.all(np.isfinite(got[[0, 2]]))
    assert rel_err(got[[0, 2]], ex[[0, 2]]) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree38", "chain6ff", "table7"])
def test_model_capsule_pair(gpu, name):
    """ModelHandle.capsule_pair against the yardstick to 1e-12: D, both closest points and dD/dq = z (exact zeros off the
    symmetric difference of the two paths), for every robot pair, a sphere among the capsules"""
    capi = gpu
    model, _, o = make_any(name, 2, fd_mode=0)
    caps = pick_capsules(model)
    xs, _ = _trajs(o, model, 1, 171)
    q = xs[0].reshape(3, o.nx)[1][:o.nq]
    E = ends(o, caps, q)
    worst = 0.0
    with capi.ModelHandle(model) as h:
        for pair in [p for p in pick_pairs(caps) if p[1] == ROBOT]:
            a, _, b = pair
            ev = pair_eval(caps, E, pair, np.zeros(8))
            assert pair_ok(dict(ev, d=1.0))
            z, cols = cp_z(o, model, caps, pair, q, ev)
            D, ca, cb, J = h.capsule_pair(caps[a][0], caps[a][1], caps[a][2], caps[b][0], caps[b][1], caps[b][2], q, jacobian=True)
            D2, ca2, cb2 = h.capsule_pair(caps[a][0], caps[a][1], caps[a][2], caps[b][0], caps[b][1], caps[b][2], q)
            assert D2 == D and np.array_equal(ca2, ca) and np.array_equal(cb2, cb)
            worst = max(worst, abs(D - ev["D"]) / max(1.0, ev["D"]), rel_err(ca, ev["ca"]), rel_err(cb, ev["cb"]), rel_err(J, z))
            assert np.all(J[[c for c in range(o.nv) if c not in cols]] == 0.0)
        with pytest.raises(capi.DdpHipError) as exc:                          # both capsules on one joint
            h.capsule_pair(caps[1][0], caps[1][1], caps[1][2], caps[1][0], caps[0][1], caps[0][2], q)
        assert exc.value.code == capi.E_ARG
    print("capsule_pair", name, worst)
    assert worst <= 1e-12, worst


@pytest.mark.gpu
def test_degenerate_and_pinned_rules(gpu):
    """A pair at D == 0: at the neutral configuration (q = 0) a sphere at the origin of joint 5 and a sphere of joint 4 at joint
    5's placement coincide exactly; the pair gives its value 1/2 w (r_a + r_b + m)^2 and no derivative, and so does a world sphere
    at that point.  A world capsule parallel to a robot capsule and a half-space whose normal is perpendicular to one (a tie of
    the two ends up to rounding) follow the pinned rule: values only, against the yardstick"""
    capi = gpu
    T, B = 2, 2
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)
    pp5 = tuple(float(v) for v in np.asarray(model.pp).reshape(-1, 3)[5])
    z3 = (0.0, 0.0, 0.0)
    caps = [(5, z3, z3, 0.03), (4, pp5, pp5, 0.05), (0, (0.1, 0.0, 0.05), (0.1, 0.0, 0.25), 0.04)]
    xs = np.zeros((B, (T + 1) * o.nx))
    us = np.zeros((B, T * o.m))
    q0 = xs[0][:o.nq]
    E = ends(o, caps, q0)
    assert np.array_equal(E[0][0], E[1][0])
    a0, a1 = E[2]
    axis = (a1 - a0) / np.linalg.norm(a1 - a0)
    perp = np.cross(axis, [1.0, 0.0, 0.0]) if abs(axis[0]) < 0.9 else np.cross(axis, [0.0, 1.0, 0.0])
    perp /= np.linalg.norm(perp)
    pairs = [(0, ROBOT, 1), (0, WORLD, 0), (0, ROBOT, 2), (2, WORLD, 0), (2, HALF, 0)]
    g = np.zeros((len(pairs), 8))
    g[0, :7], g[0, 7] = 1.0, 0.02
    g[1, 0:3], g[1, 3:6], g[1, 6], g[1, 7] = E[0][0], E[0][0], 0.01, 0.03
    g[2, 7] = -10.0
    g[3, 0:3], g[3, 3:6], g[3, 6], g[3, 7] = a0 + 0.1 * perp - 0.05 * axis, a1 + 0.1 * perp + 0.3 * axis, 0.02, 0.1   # parallel, active
    g[4, 0:3], g[4, 3], g[4, 7] = perp, float(perp @ a0) - 0.1, 0.2                                                   # a tie, active
    wgt = np.array([3.0, 7.0, 5.0, 2.0, 4.0])
    value01 = 0.5 * wgt[0] * (0.03 + 0.05 + 0.02) ** 2 + 0.5 * wgt[1] * (0.03 + 0.01 + 0.03) ** 2
    mults = tc._mults(o, xs[0], 43)
    got = {}
    for on, npair in ((False, 0), (True, 3), (True, 5)):
        with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST if on else 0) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if on:
                set_task(ctx, caps, pairs[:npair], g[:npair], wgt[:npair])
                got["clear", npair] = ctx.capsule_clearance(0)
            ctx.linearize()
            ctx.cost_seq_aug(0, 1.0)
            got[npair] = {s: ctx.download(s) for s in DERIVS + ("COSTS_OLD",)}
    for s in DERIVS:
        assert np.array_equal(got[3][s], got[0][s]), s                         # D == 0: no derivative anywhere
    scale = max(1.0, np.max(np.abs(got[0]["COSTS_OLD"])))
    extra = got[3]["COSTS_OLD"] - got[0]["COSTS_OLD"]
    assert np.max(np.abs(extra - value01)) <= 1e-12 * scale, extra
    assert np.all(got["clear", 3] == -(0.03 + 0.05 + 0.02))
    ex = cp_terms(o, caps, pairs, xs[0], np.broadcast_to(g, (T + 1, 5, 8)), np.broadcast_to(wgt, (T + 1, 5)))
    ex3 = cp_terms(o, caps, pairs[:3], xs[0], np.broadcast_to(g[:3], (T + 1, 3, 8)), np.broadcast_to(wgt[:3], (T + 1, 3)))
    assert np.all(ex - ex3 > 1e-4)                                             # the parallel pair and the tie are active
    extra5 = got[5]["COSTS_OLD"] - got[0]["COSTS_OLD"]
    assert np.max(np.abs(extra5 - ex[None, :])) <= 1e-12 * scale, (extra5, ex)
    exc = cp_clearance(o, caps, pairs, xs[0], np.broadcast_to(g, (T + 1, 5, 8)), np.broadcast_to(wgt, (T + 1, 5)))
    assert np.max(np.abs(got["clear", 5] - exc[None, :])) <= 1e-12


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    """every refusal of the interface with nothing written, set_pairs again (the same counts and kinds keep the data, others reset
    it) and the live rule on half-batch uploads of zeros"""
    import ctypes as C
    capi = gpu
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    T, B = 3, 4
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    npair = len(pairs)
    same_joint = next((a, ROBOT, b) for a in range(len(caps)) for b in range(a + 1, len(caps)) if caps[a][0] == caps[b][0])
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_capsule_pairs(capsules=caps, pairs=pairs)) == capi.E_UNSUPPORTED
        with pytest.raises(ValueError):                              # the wrapper has no pair count to check shapes against
            ctx.set_capsule_cost(weight=np.ones(npair))
        z = np.ones(B * (T + 1) * npair)
        assert L.ddp_hip_capsule_upload(ctx._h, None, z.ctypes.data_as(dp), 0, 1) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.capsule_cost()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.capsule_clearance()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_CAPSULE_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as ctx:     # the flag stands alone
        z = np.ones(B * (T + 1) * npair)
        assert L.ddp_hip_capsule_upload(ctx._h, None, z.ctypes.data_as(dp), 0, B) == capi.E_ARG   # before set_pairs
        assert code(lambda: ctx.capsule_clearance()) == capi.E_ARG
        j0, e0, e1, r0 = caps[0]
        nj = model.nv - 5
        many_caps = [(k % nj, e0, e1, 0.01) for k in range(capi.MAX_CAPSULES + 1)]
        many_pairs = [pairs[k % npair] for k in range(capi.MAX_CAPSULE_PAIRS + 1)]
        rest = caps[1:]
        for bad_caps, bad_pairs in (([], pairs), (many_caps, [(0, HALF, 0)]), (caps, []), (caps, many_pairs),
                                    ([(nj, e0, e1, r0)] + rest, pairs), ([(-1, e0, e1, r0)] + rest, pairs),
                                    ([(j0, (0.0, np.nan, 0.0), e1, r0)] + rest, pairs), ([(j0, e0, (0.0, np.inf, 0.0), r0)] + rest, pairs),
                                    ([(j0, e0, e1, -1e-3)] + rest, pairs), ([(j0, e0, e1, np.nan)] + rest, pairs),
                                    ([(j0, e0, e1, np.inf)] + rest, pairs),
                                    (caps, [(0, ROBOT, len(caps))]), (caps, [(len(caps), ROBOT, 0)]), (caps, [(-1, ROBOT, 0)]),
                                    (caps, [(0, ROBOT, -1)]), (caps, [(len(caps), WORLD, 0)]), (caps, [(-1, HALF, 0)]),
                                    (caps, [(0, 3, 1)]), (caps, [(0, -1, 1)]),
                                    (caps, [(2, ROBOT, 2)]), (caps, [same_joint]), (caps, [same_joint[::-1]]), (caps, pairs + [same_joint])):
            assert code(lambda: ctx.set_capsule_pairs(capsules=bad_caps, pairs=bad_pairs)) == capi.E_ARG, (bad_caps, bad_pairs)
        assert code(lambda: ctx.capsule_clearance()) == capi.E_ARG            # a refused set_pairs sets nothing
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs + [pairs[0], (pairs[0][2], ROBOT, pairs[0][0])])   # duplicates are allowed
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        g0, w0 = ctx.capsule_cost()                                           # defaults: geometry 0, weights 0
        assert g0.shape == (B, T + 1, npair, 8) and w0.shape == (B, T + 1, npair) and np.all(g0 == 0.0) and np.all(w0 == 0.0)
        xs, us = _trajs(o, model, B, 161)
        gg, wg = random_task(o, caps, pairs, xs, B, 162, p_clear=0.0)
        ctx.set_capsule_cost(geom=gg, weight=wg)
        per_g, per_w = gg[0].copy(), wg[0].copy()
        i_w = next(i for i, p in enumerate(pairs) if p[1] == WORLD)
        i_h = next(i for i, p in enumerate(pairs) if p[1] == HALF)
        for bad in (-1e-3, np.nan, np.inf):
            wb = per_w.copy(); wb[1, 2] = bad
            assert code(lambda: ctx.set_capsule_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_capsule_cost(geom=per_g, weight=wb)) == capi.E_ARG, bad
        for i, a in ((0, 3), (0, 7), (i_w, 0), (i_w, 6), (i_w, 7), (i_h, 1), (i_h, 3), (i_h, 5), (i_h, 7)):
            for bad in (np.nan, np.inf, -np.inf):                             # a non-finite entry, the ignored ones included
                gb = per_g.copy(); gb[T, i, a] = bad
                assert code(lambda: ctx.set_capsule_cost(geom=gb, weight=per_w)) == capi.E_ARG, (i, a, bad)
                assert code(lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG, (i, a, bad)
        gb = per_g.copy(); gb[1, i_w, 6] = -1e-3                              # rho < 0
        assert code(lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG
        gb = per_g.copy(); gb[1, i_h, 0:3] *= 1.0 + 1e-9                      # a normal off unit length
        assert code(lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG
        gb = per_g.copy(); gb[1, 0, 6] = -1.0; gb[1, i_h, 6] = -1.0           # ... but an ignored entry may be negative
        ctx.set_capsule_cost(geom=gb, first=0, count=1)
        ctx.set_capsule_cost(geom=per_g, first=0, count=1)
        assert code(lambda: ctx.set_capsule_cost(weight=per_w, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_capsule_cost(weight=per_w, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_capsule_cost(weight=per_w, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.capsule_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros((B + 1) * (T + 1) * npair)
        assert L.ddp_hip_capsule_upload(ctx._h, None, z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        assert L.ddp_hip_capsule_clearance(ctx._h, 2, z.ctypes.data_as(dp)) == capi.E_ARG
        assert L.ddp_hip_capsule_clearance(ctx._h, 0, None) == capi.E_ARG
        g1, w1 = ctx.capsule_cost()
        assert np.array_equal(g1, gg) and np.array_equal(w1, wg)              # a refused upload leaves both sides as they were
        g2, w2 = ctx.capsule_cost(first=1, count=2)                           # the round trip of a range of instances
        assert np.array_equal(g2, gg[1:3]) and np.array_equal(w2, wg[1:3])
        bw = np.arange(npair, dtype=float)
        ctx.set_capsule_cost(weight=bw, first=1, count=2)                     # broadcast: (n_pairs,); the geometry stays
        assert np.array_equal(ctx.capsule_cost()[1][1:3], np.broadcast_to(bw, (2, T + 1, npair)))
        assert np.array_equal(ctx.capsule_cost()[1][0], wg[0]) and np.array_equal(ctx.capsule_cost()[0], gg)
        # set_pairs again: the same counts and kinds keep the data (capsules may move, radii change, a pair name other capsules)
        moved = [(j, tuple(0.5 * np.asarray(a)), tuple(0.5 * np.asarray(b)), 2.0 * r) for j, a, b, r in caps]
        swapped = [(pairs[0][2], ROBOT, pairs[0][0])] + pairs[1:]
        ctx.set_capsule_pairs(capsules=moved, pairs=swapped)
        g3, w3 = ctx.capsule_cost()
        assert np.array_equal(g3, gg) and np.any(w3 != 0.0)
        other = [(p[0], HALF if k == i_w else p[1], p[2]) for k, p in enumerate(pairs)]   # the same count, one kind changed
        ctx.set_capsule_pairs(capsules=caps, pairs=other)
        g4, w4 = ctx.capsule_cost()
        assert np.all(g4 == 0.0) and np.all(w4 == 0.0)
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        ctx.set_capsule_cost(weight=np.ones(npair))
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs[:4])
        g5, w5 = ctx.capsule_cost()
        assert g5.shape == (B, T + 1, 4, 8) and np.all(g5 == 0.0) and np.all(w5 == 0.0)
        # the live rule: zeros that arrive half-batch by half-batch leave the kernels launched, with the flag-off bits
        _setup(ctx, xs, us)
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        ctx.linearize()
        off = {s: ctx.download(s) for s in DERIVS}
        ctx.set_capsule_cost(geom=gg, weight=wg)
        ctx.linearize()
        assert not np.array_equal(ctx.download("LX"), off["LX"])
        ctx.set_capsule_cost(weight=np.zeros(npair), first=0, count=B // 2)
        ctx.linearize()
        lx = ctx.download("LX")
        assert np.array_equal(lx[:B // 2], off["LX"][:B // 2]) and not np.array_equal(lx[B // 2:], off["LX"][B // 2:])
        ctx.set_capsule_cost(weight=np.zeros(npair), first=B // 2, count=B - B // 2)
        ctx.linearize()
        for s in DERIVS:
            assert np.array_equal(ctx.download(s), off[s]), s
        assert np.all(ctx.capsule_clearance(0) == np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 2])
def test_advance_shifts_both_sides(gpu, shift):
    """ddp_hip_advance on a context with the flag: geometry and weights downloaded afterwards equal the numpy shift of the old ones
    bit for bit -- rows 0 .. T-1 by the hold rule, row T untouched"""
    capi = gpu
    T, B = 4, 2
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    caps = pick_capsules(model)
    pairs = pick_pairs(caps)
    xs, us = _trajs(o, model, B, 181)
    g, w = random_task(o, caps, pairs, xs, B, 182)
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as ctx:
        _setup(ctx, xs, us)
        set_task(ctx, caps, pairs, g, w)
        ctx.advance(shift, None, capi.ADVANCE_NO_ROLL)
        g1, w1 = ctx.capsule_cost()
    assert np.array_equal(g1, adv.np_advance(g, shift, terminal=True)) and np.array_equal(w1, adv.np_advance(w, shift, terminal=True))
    assert np.array_equal(g1[:, T], g[:, T]) and np.array_equal(w1[:, T], w[:, T]) and not np.array_equal(g1, g)
    assert np.array_equal(g1[:, T - 1], g[:, T - 1]) and np.array_equal(g1[:, 0], g[:, shift])


REACH_WEIGHT = 1e6
DEPTH_TOL = 0.01


@pytest.mark.gpu
def test_reach_past_world_capsule(gpu):
    """chain6, T = 40, no constraint: a tracking cost pulls the arm to a goal posture; the last link carries a capsule.  The
    flag-off ddp_hip_solve's tip path is taken first; a world capsule (a pole across the path) is then put on it, halfway.  The
    same solve without the term ends with a clearance below -DEPTH_TOL, the solve with it -- from the same start -- at or above
    -DEPTH_TOL (1 cm: the depth the siblings' fold test calls folding through).  The penalty is soft: the depth at which it
    balances the pull of the tracking cost on a tip that passes the pole at some 3 cm per step goes with 1 / weight.  Measured on
    an MI355X, least clearance after 30 iterations: -7.0 cm without the term, -4.6 cm at weight 1e5, -0.62 cm at 1e6, -0.06 cm at
    1e7; the weight here is 1e6"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, iters, thr, mu, w_, n_ = 40, 30, 1e-9, 1.0, 1e-1, 10.0
    model, spec, o = _reach_problem(T)
    xs, us = _trajs(o, model, 1, 141, held=True)
    link = (5, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0823), 0.03)
    rng = np.random.default_rng(142)
    goal = np.concatenate([xs[0][:o.nq] + 0.6 * rng.choice([-1.0, 1.0], size=o.nv), np.zeros(o.nv)])
    xref = np.tile(goal, (T + 1, 1))
    wx = np.tile(np.concatenate([np.full(o.nv, 200.0), np.full(o.nv, 1.0)]), (T + 1, 1))
    wx[T] *= 10.0
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_tracking_cost(xref=xref, wx=wx)
        solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
        x_off = ctx.download("X")
    Xo = x_off[0].reshape(T + 1, o.nx)
    path = np.array([o.frame_position(link[0], link[2], Xo[t][:o.nq]) for t in range(T + 1)])
    travel = path[T] - path[0]
    assert np.linalg.norm(travel) > 0.1                                      # the tip travels
    across = np.cross(travel, [0.0, 0.0, 1.0])
    across /= np.linalg.norm(across)
    geom = np.concatenate([path[T // 2] - 0.15 * across, path[T // 2] + 0.15 * across, [0.04, 0.0]])[None, :]
    pairs = [(0, WORLD, 0)]
    weight = np.full(1, REACH_WEIGHT)
    gT, wT = np.broadcast_to(geom, (T + 1, 1, 8)), np.broadcast_to(weight, (T + 1, 1))
    assert np.min(cp_clearance(o, [link], pairs, xs[0], gT, wT)[0]) > 0.0    # the arm starts clear of it
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        ctx.set_tracking_cost(xref=xref, wx=wx)
        set_task(ctx, [link], pairs, geom, weight)
        _setup(ctx, x_off, us)
        clear_off = float(np.min(ctx.capsule_clearance(0)))
        _setup(ctx, xs, us)
        solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
        clear_on = float(np.min(ctx.capsule_clearance(0)))
        x_on = ctx.download("X")
    print("reach past capsule: clearance without the term", clear_off, "with it", clear_on, "weight", REACH_WEIGHT)
    assert abs(clear_on - np.min(cp_clearance(o, [link], pairs, x_on[0], gT, wT))) <= 1e-9
    assert clear_off < -DEPTH_TOL, clear_off
    assert clear_on >= -DEPTH_TOL, clear_on
