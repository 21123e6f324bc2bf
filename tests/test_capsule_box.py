"""Capsule pairs of kind CAPSULE_VS_BOX (ddp_hip.h): body B is an oriented box, its shape (half extents) shared by the batch, its
pose (centre, unit quaternion x y z w) and a margin the pair's own eight doubles per (instance, t).

The yardstick is the siblings' (test_capsule_cost.py, test_capsule_grid.py) with a fifth branch in pair_eval: box_rule below, the
header's pinned search restated literally in Python floats (no fused product, the breakpoints sorted, every candidate in the order
the header gives).  It is checked here against a dense scan of the segment parameter and against central differences.  Tolerances
are the siblings': 1e-12 relative for values, clearances and derivatives.

Stability guard.  A case with |f*| < 1e-6 (f == 0 is where the pair loses its derivative), or whose best candidates of two
different sub-intervals differ in s by more than 1e-9 while their values differ by less than 1e-9 (the argmin may flip on the last
bit of the device's own forward kinematics), has weight 0 or is left out of the comparison; every test that excludes asserts that
the excluded share is at most 5 %.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import test_advance as adv
import test_capsule_cost as cc
import test_capsule_grid as cg
import test_frame_cost as fc
import test_tracking_cost as tc
from problems import make
from synth import rel_err

ROOT = cc.ROOT
TOL = 1e-12
ROBOT, WORLD, HALF, GRID, BOX = 0, 1, 2, 3, 4
DERIVS = cc.DERIVS
_trajs, _setup = tc._trajs, tc._setup
MODELS = [("chain6", None), ("chain6ff", 0), ("tree38", None)]
SHAPES = np.array([[0.12, 0.3, 0.05], [0.4, 0.07, 0.21], [0.06, 0.09, 0.45]])      # the box shapes of the mixed tasks
SHAPES.setflags(write=False)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def quat_R(q):
    """lie.h's quat_to_R (x y z w, world = R box), every product rounded on its own"""
    x, y, z, w = (float(v) for v in q)
    return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
            [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
            [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]]


def box_phi(p, h):
    q = [abs(p[k]) - h[k] for k in range(3)]
    if any(v != v for v in q):
        return math.nan
    e = [v if v > 0.0 else 0.0 for v in q]
    o = math.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])
    if o > 0.0:
        return o
    m = q[0]
    if q[1] > m:
        m = q[1]
    if q[2] > m:
        m = q[2]
    return m


def _better(f, best, first):
    if first:
        return True
    if best != best:
        return False
    return f != f or f < best


def box_rule(a0, a1, half, pose):
    """the header's rule on one world segment: a dict with f (the least signed distance), s, ca, u (None where f == 0), kink, and
    `split`: the least gap in value between the winner and a candidate of another sub-interval more than 1e-9 away in s (inf:
    none)"""
    a0, a1, h = [float(v) for v in a0], [float(v) for v in a1], [float(v) for v in half]
    c = [float(v) for v in pose[:3]]
    R = quat_R(pose[3:7])
    ra, rb = [a0[k] - c[k] for k in range(3)], [a1[k] - c[k] for k in range(3)]
    a = [R[0][k] * ra[0] + R[1][k] * ra[1] + R[2][k] * ra[2] for k in range(3)]
    b = [R[0][k] * rb[0] + R[1][k] * rb[1] + R[2][k] * rb[2] for k in range(3)]
    dl = [b[k] - a[k] for k in range(3)]
    bps = [0.0, 1.0]
    for k in range(3):
        if dl[k] != 0.0:
            for s in ((h[k] - a[k]) / dl[k], (-h[k] - a[k]) / dl[k]):
                if 0.0 < s < 1.0:
                    bps.append(s)
    bps.sort()
    c0 = [a[0] - h[0], -a[0] - h[0], a[1] - h[1], -a[1] - h[1], a[2] - h[2], -a[2] - h[2]]
    m0 = [dl[0], -dl[0], dl[1], -dl[1], dl[2], -dl[2]]

    def f_at(s):
        return box_phi([a[k] + s * dl[k] for k in range(3)], h)
    best = {"f": 0.0, "s": 0.0, "ij": None, "iv": -1}
    first = True
    per_interval = []
    for iv in range(len(bps) - 1):
        lo, hi = bps[iv], bps[iv + 1]
        mid = 0.5 * (lo + hi)
        cands = [(lo, None)]
        A = C = 0.0
        outside = False
        for k in range(3):
            pm = a[k] + mid * dl[k]
            sg = 1.0 if pm > h[k] else (-1.0 if pm < -h[k] else 0.0)
            if sg != 0.0:
                outside = True
                A = A + dl[k] * dl[k]
                C = C + dl[k] * (a[k] - sg * h[k])
        if outside:
            if A > 0.0:
                s = -C / A
                if lo < s < hi:
                    cands.append((s, None))
        else:
            for i in range(5):
                for j in range(i + 1, 6):
                    if m0[i] == m0[j]:
                        continue
                    s = (c0[j] - c0[i]) / (m0[i] - m0[j])
                    if lo < s < hi:
                        cands.append((s, (i, j)))
        cands.append((hi, None))
        loc = None
        for s, ij in cands:
            f = f_at(s)
            if loc is None or f < loc[0]:
                loc = (f, s)
            if _better(f, best["f"], first):
                best = {"f": f, "s": s, "ij": ij, "iv": iv}
            first = False
        per_interval.append(loc)
    fb, sb = best["f"], best["s"]
    split = math.inf
    for iv, (f, s) in enumerate(per_interval):
        if iv != best["iv"] and abs(s - sb) > 1e-9:
            split = min(split, abs(f - fb))
    p = [a[k] + sb * dl[k] for k in range(3)]
    n = [0.0, 0.0, 0.0]
    kink = False
    if not fb > 0.0 and best["ij"] is not None:
        i, j = best["ij"]
        mi, mj = m0[i], m0[j]
        if (mi > 0.0 and mj < 0.0) or (mi < 0.0 and mj > 0.0):
            kink = True
            ai, aj = abs(mi), abs(mj)
            den = ai + aj
            for l in range(6):
                sgn = -1.0 if l & 1 else 1.0
                if l == i:
                    n[l >> 1] = n[l >> 1] + sgn * aj
                if l == j:
                    n[l >> 1] = n[l >> 1] + sgn * ai
            n = [v / den for v in n]
    if fb > 0.0:
        for k in range(3):
            cl = -h[k] if p[k] < -h[k] else (h[k] if p[k] > h[k] else p[k])
            n[k] = (p[k] - cl) / fb
    elif not kink:
        l = [p[0] - h[0], -p[0] - h[0], p[1] - h[1], -p[1] - h[1], p[2] - h[2], -p[2] - h[2]]
        bi = 0
        for i in range(1, 6):
            if l[i] > l[bi]:
                bi = i
        n[bi >> 1] = -1.0 if bi & 1 else 1.0
    ca = np.array([a0[k] + sb * (a1[k] - a0[k]) for k in range(3)])
    u = np.array([R[k][0] * n[0] + R[k][1] * n[1] + R[k][2] * n[2] for k in range(3)])
    return {"f": fb, "s": sb, "ca": ca, "u": (u if fb != 0.0 else None), "kink": kink, "split": split, "inside": not fb > 0.0}


def stable(r):
    return abs(r["f"]) >= 1e-6 and r["split"] >= 1e-9


def box_eval(shapes, base):
    """the siblings' pair_eval(caps, E, pair, g) with the fifth kind: g = (centre, quaternion, margin), pair[2] the shape"""
    def pair_eval(caps, E, pair, g):
        if pair[1] != BOX:
            return base(caps, E, pair, g)
        a = pair[0]
        r = box_rule(E[a][0], E[a][1], shapes[pair[2]], g[:7])
        return {"D": None, "d": r["f"] - caps[a][3] - g[7], "u": r["u"], "s": r["s"], "t": None, "ca": r["ca"],
                "info": {"sphere": True, "gap": np.inf, "rule": r}}
    return pair_eval


def random_case(rng, parallel=False, scale=1.0):
    """the generator of the rule's own checks: extents U(0.05, 0.5), ends N(0, 0.5^2) and N(0, 0.4^2) about them, a random pose;
    scale < 1 draws the segment nearer the box's middle (more of it inside)"""
    half = rng.uniform(0.05, 0.5, 3)
    a0 = rng.normal(0.0, 0.5 * scale, 3)
    a1 = a0 + rng.normal(0.0, 0.4 * scale, 3)
    q = rng.normal(size=4)
    pose = np.concatenate([rng.normal(0.0, 0.2, 3), q / np.sqrt(q @ q)])
    if parallel:                                                        # the segment parallel to a face pair, in world axes
        pose[3:] = (0.0, 0.0, 0.0, 1.0)
        k = int(rng.integers(3))
        a1[k] = a0[k]
    return a0, a1, half, pose


def phi_many(P, half, pose):
    """the box's signed distance at many world points, in array arithmetic (an independent statement of phi)"""
    R = np.array(quat_R(pose[3:7]))
    p = (P - pose[:3]) @ R
    q = np.abs(p) - half
    out = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    return np.where(out > 0.0, out, np.max(q, axis=1))


def mixed_pairs(caps):
    """the grid sibling's 23 pairs of four kinds and, before, between and behind them, 4 box pairs on 3 shapes (two pairs on one
    shape, a sphere's among them): 27"""
    p = cg.mixed_pairs(caps)
    return [(1, BOX, 0)] + p[:12] + [(3, BOX, 2)] + p[12:] + [(0, BOX, 1), (4, BOX, 0)]


def box_task(o, caps, pairs, xs, B, seed, grid, shapes=SHAPES):
    """geom (B, T+1, n_pairs, 8), weights and the excluded share of the box pairs.  The older kinds by the grid sibling's generator
    (which sees a half-space in a box pair's place).  A box pair, per (instance, t): a random orientation, the centre within 0 ..
    0.45 m of the capsule's middle (so that inside, straddling and outside cases all occur); the margin makes the pair penetrate by
    0.01 .. 0.1 -- only in a block that an older pair already makes active, so that clear blocks remain -- or stay clear by as
    much.  The first box pair is active and inside its box at t = 0 and clear at t = 1.  A case the stability guard (module
    docstring) leaves out has weight 0"""
    plain = [(p[0], HALF, 0) if p[1] == BOX else p for p in pairs]
    if any(p[1] == GRID for p in pairs):
        g, w, _ = cg.grid_task(o, caps, plain, xs, B, seed, grid)
    else:
        g, w = cc.random_task(o, caps, plain, xs, B, seed + 1)
    rng = np.random.default_rng(seed + 7)
    bi = [i for i, p in enumerate(pairs) if p[1] == BOX]
    older = cg.grid_eval(grid) if grid is not None else cg._SIBLING_EVAL
    excluded = total = 0
    for b in range(B):
        X = xs[b].reshape(o.T + 1, o.nx)
        for t in range(o.T + 1):
            E = cc.ends(o, caps, X[t][:o.nq])
            busy = any(w[b, t, i] != 0.0 and older(caps, E, p, g[b, t, i])["d"] < 0 for i, p in enumerate(pairs) if p[1] != BOX)
            for i in bi:
                a = pairs[i][0]
                mid = 0.5 * (E[a][0] + E[a][1])
                q = rng.normal(size=4)
                inside = rng.uniform() < 0.5 and busy
                off = rng.uniform(0.0, 0.45) * cc._unit(rng)
                if i == bi[0] and t < 2:
                    inside, off = t == 0, (0.02 * cc._unit(rng) if t == 0 else off)
                g[b, t, i, :3], g[b, t, i, 3:7], g[b, t, i, 7] = mid + off, q / np.sqrt(q @ q), 0.0
                w[b, t, i] = rng.uniform(0.5, 5.0)
                r = box_rule(E[a][0], E[a][1], shapes[pairs[i][2]], g[b, t, i, :7])
                depth = rng.uniform(0.01, 0.1)
                g[b, t, i, 7] = r["f"] - caps[a][3] + (depth if inside else -depth)
                total += 1
                if not stable(r):
                    w[b, t, i] = 0.0
                    excluded += 1
    return g, w, (excluded / total if total else 0.0)


def five_eval(grid, shapes=SHAPES):
    return box_eval(shapes, cg.grid_eval(grid) if grid is not None else cg._SIBLING_EVAL)


def check_box_task(monkeypatch, o, caps, pairs, xs, g, w, grid, share, need=True, shapes=SHAPES):
    """cc.pair_eval becomes the five-kind one from here on; the conditions on the inputs, on the yardstick alone: the siblings', the
    excluded share, and with `need` live box pairs that are active, that are clear, whose segment is inside the box (f* < 0) and
    outside it.  Returns the blocks' activity"""
    monkeypatch.setattr(cc, "pair_eval", five_eval(grid, shapes))
    assert share <= 0.05, share
    active = cc.check_task(o, caps, pairs, xs, g, w, fractions=False)
    n_act = n_clear = n_in = n_out = 0
    for b in range(xs.shape[0]):
        X = xs[b].reshape(o.T + 1, o.nx)
        for t in range(o.T + 1):
            E = cc.ends(o, caps, X[t][:o.nq])
            for i, p in enumerate(pairs):
                if p[1] != BOX or w[b, t, i] == 0.0:
                    continue
                ev = cc.pair_eval(caps, E, p, g[b, t, i])
                n_act += ev["d"] < 0
                n_clear += ev["d"] > 0
                n_in += ev["info"]["rule"]["inside"]
                n_out += not ev["info"]["rule"]["inside"]
    assert not need or (n_act >= 1 and n_clear >= 1 and n_in >= 1 and n_out >= 1), (n_act, n_clear, n_in, n_out)
    return active


def set_task(ctx, grid, caps, pairs, geom=None, weight=None, shapes=SHAPES):
    if grid is not None:
        ctx.set_obstacle_grid(*grid)
    ctx.set_capsule_boxes(shapes)
    cc.set_task(ctx, caps, pairs, geom, weight)


def blocking_task(o, caps, pairs, geom, xs, us, mults, fb, mu):
    """the siblings', for a horizon of a few steps: the pair whose distance shrinks most under the full step is found first; the
    margins then leave the trajectory xs clear, at every t and for every pair, by a quarter of that shrink (not by a fixed 1 cm,
    which three steps do not cover), and that pair is weighted at five times what the step gains otherwise.  Returns (geom,
    weights) of one instance, the full step's cost difference without the term, the shrink and the clearance left"""
    T = o.T
    _, x1, u1 = o.forward_alpha(1.0, xs, us, mults, fb, mu)
    gain = (o.cost_seq_aug(x1, u1, mults, mu) - o.cost_seq_aug(xs, us, mults, mu)).sum()
    Xo, Xn = xs.reshape(T + 1, o.nx), x1.reshape(T + 1, o.nx)
    g = geom.copy()
    g[..., 7] = 0.0

    def d0(X):
        return np.array([[cc.pair_eval(caps, cc.ends(o, caps, X[t][:o.nq]), pair, g[t, i])["d"] for i, pair in enumerate(pairs)]
                         for t in range(T + 1)])
    Do, Dn = d0(Xo), d0(Xn)
    shrink = np.max(Do - Dn, axis=0)
    i_ = int(np.argmax(shrink))
    clear = 0.25 * float(shrink[i_])
    g[..., 7] = Do - clear
    sel = np.zeros((T + 1, len(pairs)))
    sel[:, i_] = 1.0
    unit = cc.cp_terms(o, caps, pairs, x1, g, sel).sum()
    return g, sel * (5.0 * abs(gain) / unit if unit > 0.0 else 0.0), gain, float(shrink[i_]), clear


def code(capi, fn):
    with pytest.raises(capi.DdpHipError) as exc:
        fn()
    return exc.value.code


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_yardstick_against_dense_scan():
    """the restated rule against a 4 001-point scan of s on 1 000 random cases, a seventh of them parallel to a face pair: never
    above the scan's minimum, never below it by more than the scan's Lipschitz slack (phi is 1-Lipschitz, the scan's spacing is
    |delta| / 4000); and how rare the guarded cases are with this generator"""
    rng = np.random.default_rng(1)
    sig = np.linspace(0.0, 1.0, 4001)
    n_in = n_kink = n_unstable = 0
    N = 1000
    for trial in range(N):
        a0, a1, half, pose = random_case(rng, parallel=trial % 7 == 3)
        r = box_rule(a0, a1, half, pose)
        scan = float(np.min(phi_many(a0[None, :] + sig[:, None] * (a1 - a0)[None, :], half, pose)))
        assert 0.0 <= r["s"] <= 1.0
        assert r["f"] <= scan + 1e-12, (trial, r["f"], scan)
        assert r["f"] >= scan - np.linalg.norm(a1 - a0) / 8000 - 1e-12, (trial, r["f"], scan)
        assert abs(r["f"] - float(phi_many(r["ca"][None, :], half, pose)[0])) <= 1e-12
        n_in += r["inside"]
        n_kink += r["kink"]
        n_unstable += not stable(r)
    assert n_in >= 80 and n_kink >= 40, (n_in, n_kink)
    assert n_unstable <= 0.05 * N, n_unstable


def test_yardstick_gradient():
    """central differences of f* in both ends (a random direction of the six coordinates, step 1e-6) against the frozen-point
    derivative (1 - s*) u . da0 + s* u . da1, to 1e-6 as the sibling's _fd_check; outside, inside and kink cases; a pinned kink"""
    rng = np.random.default_rng(2)
    h = 1e-6
    n_out = n_in = n_kink = n_skip = 0
    N = 600
    for trial in range(N):
        a0, a1, half, pose = random_case(rng, scale=1.0 if trial % 2 else 0.4)
        r = box_rule(a0, a1, half, pose)
        if not stable(r):
            n_skip += 1
            continue
        d0, d1 = cc._unit(rng), cc._unit(rng)
        fp = box_rule(a0 + h * d0, a1 + h * d1, half, pose)["f"]
        fm = box_rule(a0 - h * d0, a1 - h * d1, half, pose)["f"]
        an = (1.0 - r["s"]) * float(r["u"] @ d0) + r["s"] * float(r["u"] @ d1)
        assert abs((fp - fm) / (2 * h) - an) <= 1e-6, (trial, (fp - fm) / (2 * h), an, r)
        n_out += not r["inside"]
        n_in += r["inside"] and not r["kink"]
        n_kink += r["kink"]
    assert n_skip <= 0.05 * N and n_out >= 200 and n_in >= 40 and n_kink >= 40, (n_skip, n_out, n_in, n_kink)
    # the kink worked out by hand in host/test_capsule_box_block.cpp
    r = box_rule([0.9, 0.0, 0.0], [-0.1, 1.9, 0.0], [1.0, 2.0, 3.0], [0, 0, 0, 0, 0, 0, 1.0])
    assert r["kink"] and abs(r["s"] - 1.9 / 2.9) <= 1e-15 and np.max(np.abs(r["u"] - np.array([1.9, 1.0, 0.0]) / 2.9)) <= 1e-15
    # a zero quaternion is the identity by the formula
    r0 = box_rule([3.0, 0.5, -1.0], [3.0, 0.5, -1.0], [1.0, 2.0, 3.0], np.zeros(7))
    assert r0["f"] == 2.0 and np.array_equal(r0["u"], [1.0, 0.0, 0.0])


def test_capsule_box_block_host_logic():
    """host/test_capsule_box_block.cpp: the library's routine compiled for the host against a dense scan and against cases worked
    out by hand, the geometry validator per kind, the pair-list rule with a box count"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_capsule_box_block"])
    out = subprocess.run([os.path.join(host, "test_capsule_box_block")], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.CAPSULE_VS_BOX == 4 and re.search(r"#define\s+DDP_HIP_CAPSULE_VS_BOX\s+4\b", header)
    assert capi.MAX_CAPSULE_BOXES == 8 and re.search(r"#define\s+DDP_HIP_MAX_CAPSULE_BOXES\s+8\b", header)
    L = capi.lib()
    for name in ("ddp_hip_capsule_set_boxes", "ddp_hip_model_capsule_box"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert hasattr(capi.Context, "set_capsule_boxes") and hasattr(capi.ModelHandle, "capsule_box")
    assert "CAPSULE_VS_BOX" in capi.Context.set_capsule_pairs.__doc__ and "box pair" in capi.Context.set_capsule_cost.__doc__
    h = capi.ModelHandle.__new__(capi.ModelHandle)
    h.nv, h._h = 6, None
    for bad in (dict(a0=np.zeros(2)), dict(half=np.zeros(4)), dict(pose=np.zeros(6))):
        kw = dict(a0=np.zeros(3), a1=np.zeros(3), half=np.ones(3), pose=np.array([0, 0, 0, 0, 0, 0, 1.0]))
        kw.update(bad)
        with pytest.raises(ValueError, match="capsule_box"):
            h.capsule_box(0, kw["a0"], kw["a1"], 0.01, kw["half"], kw["pose"], np.zeros(6))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", MODELS)
def test_values_and_clearance(gpu, monkeypatch, name, fo_):
    """COSTS_OLD (ddp_hip_cost_seq_aug) against the flag-off context's values plus the numpy terms, and ddp_hip_capsule_clearance
    against the yardstick, to 1e-12: all five kinds in one context, 23 + 4 pairs on three shapes, batch 3, every instance and t its
    own geometry.  A block without an active pair keeps the flag-off value bit for bit"""
    capi = gpu
    T, B, mu = 3, 3, 30.0
    grid = cg.sphere_scene()
    model, spec, o = cc.make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    caps = cc.pick_capsules(model)
    pairs = mixed_pairs(caps)
    assert len(pairs) == 27 and sorted({p[1] for p in pairs}) == [0, 1, 2, 3, 4]
    g, w, share = box_task(o, caps, pairs, xs, B, 52, grid)
    active = check_box_task(monkeypatch, o, caps, pairs, xs, g, w, grid, share)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (capi.FLAG_CAPSULE_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if on:
                set_task(ctx, grid, caps, pairs, g, w)
                clear = ctx.capsule_clearance(0)
            ctx.cost_seq_aug(0, mu)
            got[on] = ctx.download("COSTS_OLD")
    box_only = w * np.array([p[1] == BOX for p in pairs])
    for b in range(B):
        add = cc.cp_terms(o, caps, pairs, xs[b], g[b], w[b])
        assert np.any(add != 0.0) and np.array_equal(add != 0.0, active[b])
        assert np.any(cc.cp_terms(o, caps, pairs, xs[b], g[b], box_only[b]) != 0.0)      # the box pairs contribute
        e = rel_err(got[True][b], got[False][b] + add)
        print("values", name, b, e)
        assert e <= TOL, (b, e)
        assert np.array_equal(got[True][b][~active[b]], got[False][b][~active[b]])
    ex = np.stack([cc.cp_clearance(o, caps, pairs, xs[b], g[b], w[b]) for b in range(B)])
    assert np.array_equal(np.isinf(clear), np.isinf(ex))
    fin = np.isfinite(ex)
    assert np.min(ex[fin]) < 0
    e = np.max(np.abs(clear[fin] - ex[fin]) / np.maximum(1.0, np.abs(ex[fin])))
    print("clearance", name, e)
    assert e <= TOL, e


LIN_CASES = [("chain6", 2, None), ("chain6", 0, None), ("chain6ff", 2, 0), ("tree38", 0, None), ("tree38", 2, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, monkeypatch, name, fd_mode, fo_, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the restatement's frozen-point terms, T = 2, batch 2, 23 + 4 pairs of all
    five kinds, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU, LUU, LUX
    and every row and column outside the active pairs' column sets bit for bit the flag-off values; a box pair is a world pair: a
    free-flyer root's six columns carry it"""
    capi = gpu
    T, B = 2, 2
    grid = cg.sphere_scene()
    model, spec, o = cc.make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    caps = cc.pick_capsules(model)
    pairs = mixed_pairs(caps)
    g, w, share = box_task(o, caps, pairs, xs, B, 43, grid)
    active = check_box_task(monkeypatch, o, caps, pairs, xs, g, w, grid, share)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST if on else 0) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if on:
                set_task(ctx, grid, caps, pairs, g, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    n_box_blocks = 0
    for b in range(B):
        add = cc.cp_derivs(o, model, caps, pairs, xs[b], g[b], w[b])
        bonly = cc.cp_derivs(o, model, caps, pairs, xs[b], g[b], w[b] * np.array([p[1] == BOX for p in pairs]))
        for s in ("LX", "LXX", "LFX", "LFXX"):
            e = rel_err(got[True][s][b], got[False][s][b] + add[s])
            worst = max(worst, e)
            assert e <= TOL, (s, b, e)
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
            if bonly["rows"][t].any():
                n_box_blocks += 1
                if model.ff:
                    assert bonly["rows"][t][:6].all()
    assert n_box_blocks >= 1                                                # the box pairs contribute
    print("linearize", name, fd_mode, stages, "worst", worst, "active blocks", int(active.sum()), "of", active.size)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path", [("tree38", None, 1), ("chain6ff", 0, 0)])
@pytest.mark.parametrize("n_alpha", [1, 4])
def test_forward_matches_emulation(gpu, monkeypatch, name, fo_, fwd_path, n_alpha):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the box pairs' terms included
    (the siblings' emulation), T = 3: five box pairs, the old trajectory clear by a quarter of what the full step closes, the pair the full step brings closest
    weighted so that the full step is rejected (blocking_task above); decisions are compared only where every candidate decides by more than 1e-9"""
    capi = gpu
    T, mu = 3, 1.0
    monkeypatch.setattr(cc, "pair_eval", five_eval(None))
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    caps = cc.pick_capsules(model)
    pairs = [(a, BOX, a % 3) for a in range(len(caps))]
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        shrink = -np.inf
        for seed in range(81, 97):
            xs, us = _trajs(o, model, 1, seed, held=True)
            mults = tc._mults(o, xs[0], 85)
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
            geom, _, share = box_task(o, caps, pairs, xs, 1, seed + 100, None)
            g, w, gain, shrink, clear = blocking_task(o, caps, pairs, geom[0], xs[0], us[0], mults, fb, mu_o[0])
            if shrink > 1e-4 and share <= 0.05:
                break
        assert shrink > 1e-4, shrink
        set_task(ctx, None, caps, pairs, g, w)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
        clear_old, clear_new = ctx.capsule_clearance(0)[0], ctx.capsule_clearance(1)[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + cc.cp_terms(o, caps, pairs, X, g, w)
    em = cc._emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, n_alpha, "seed", seed, "shrink", shrink, "gain", gain, "step", step[0], step_ref, "dcost", dcost[0], new,
          "margins", margins)
    assert gain < 0.0                                                          # without the term the full step is accepted
    assert np.all(cc.cp_terms(o, caps, pairs, xs[0], g, w) == 0.0)             # the old trajectory is clear
    assert step_ref < 1.0 and len(margins) > 1                                 # with it the full step is rejected
    assert min(margins) > 1e-9, margins
    assert step[0] == step_ref, (step, step_ref)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)
    assert np.max(np.abs(clear_old - clear)) < 1e-9
    assert rel_err(clear_new, cc.cp_clearance(o, caps, pairs, xn_ref, g, w)) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree38", "chain6ff"])
def test_model_capsule_box(gpu, name):
    """ModelHandle.capsule_box against the yardstick to 1e-12: d, s, c_a, u and grad = P_ca^T u (exact zeros off the capsule's
    path), for every capsule against boxes placed so that outside, inside and kink cases all occur"""
    capi = gpu
    model, _, o = cc.make_any(name, 2, fd_mode=0)
    caps = cc.pick_capsules(model)
    xs, _ = _trajs(o, model, 1, 171)
    q = xs[0].reshape(3, o.nx)[1][:o.nq]
    E = cc.ends(o, caps, q)
    rng = np.random.default_rng(172)
    worst, seen, skipped, total = 0.0, {"out": 0, "in": 0, "kink": 0}, 0, 0
    with capi.ModelHandle(model) as h:
        for trial in range(40):
            k = trial % len(caps)
            j, e0, e1, rad = caps[k]
            half = rng.uniform(0.05, 0.5, 3)
            qt = rng.normal(size=4)
            pose = np.concatenate([0.5 * (E[k][0] + E[k][1]) + rng.uniform(0.0, 0.45) * cc._unit(rng), qt / np.sqrt(qt @ qt)])
            r = box_rule(E[k][0], E[k][1], half, pose)
            total += 1
            if not stable(r):
                skipped += 1
                continue
            ev = {"s": r["s"], "u": r["u"], "t": None}
            z, cols = cc.cp_z(o, model, caps, (k, BOX, 0), q, ev)
            d, s, ca, u, grad = h.capsule_box(j, e0, e1, rad, half, pose, q, gradient=True)
            d2, s2, ca2, u2 = h.capsule_box(j, e0, e1, rad, half, pose, q)
            assert d2 == d and s2 == s and np.array_equal(ca2, ca) and np.array_equal(u2, u)
            ex = r["f"] - rad
            worst = max(worst, abs(d - ex) / max(1.0, abs(ex)), abs(s - r["s"]), rel_err(ca, r["ca"]), float(np.max(np.abs(u - r["u"]))),
                        rel_err(grad, z))
            assert np.all(grad[[c for c in range(o.nv) if c not in cols]] == 0.0)
            seen["kink" if r["kink"] else ("in" if r["inside"] else "out")] += 1
        unit = np.array([0, 0, 0, 0, 0, 0, 1.0])
        for bad in (dict(half=[0.1, 0.0, 0.1]), dict(half=[0.1, np.inf, 0.1]), dict(pose=np.array([0, 0, 0, 0, 0, 0, 1.1])),
                    dict(pose=np.array([np.nan, 0, 0, 0, 0, 0, 1.0])), dict(joint=999), dict(radius=-0.1)):
            kw = dict(joint=caps[0][0], half=[0.1, 0.1, 0.1], pose=unit, radius=0.01)
            kw.update(bad)
            assert code(capi, lambda: h.capsule_box(kw["joint"], caps[0][1], caps[0][2], kw["radius"], kw["half"], kw["pose"], q)) == capi.E_ARG
    print("capsule_box", name, worst, seen, "skipped", skipped)
    assert skipped <= 0.05 * total and seen["out"] >= 5 and seen["in"] >= 3 and seen["kink"] >= 1, (seen, skipped)
    assert worst <= 1e-12, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [("tree38", 4, 2, None, 1), ("chain6ff", 4, 2, 0, 0)])
@pytest.mark.parametrize("mode", ["no_box_pair", "zero_weights", "never"])
def test_neutrality(gpu, monkeypatch, name, T, fd_mode, fo_, fwd_path, mode):
    """linearise, both costs, sweep and forward at T = 4, bit for bit: a capsule context with live pairs of the four older kinds
    computes the same whether or not box shapes are set ("no_box_pair"); with box pairs whose weights are all 0, and with non-zero
    weights on box pairs that nothing comes near (margin -10), a context computes what the flag-off context computes"""
    capi = gpu
    mu, B = 10.0, 2
    grid = cg.sphere_scene()
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    caps = cc.pick_capsules(model)
    if mode == "no_box_pair":
        pairs = cg.mixed_pairs(caps)
        g, w, _ = cg.grid_task(o, caps, pairs, xs, B, 33, grid, p_out=0.0)
        monkeypatch.setattr(cc, "pair_eval", cg.grid_eval(grid))
        assert cc.check_task(o, caps, pairs, xs, g, w, fractions=False).any()
    else:
        pairs = mixed_pairs(caps)
        g, w, _ = box_task(o, caps, pairs, xs, B, 33, grid)
        monkeypatch.setattr(cc, "pair_eval", five_eval(grid))
        if mode == "never":
            g[..., 7] = -10.0
            assert np.min([cc.cp_clearance(o, caps, pairs, xs[b], g[b], w[b]) for b in range(B)]) > 5.0
        else:
            w[:] = 0.0
    out = {}
    for on in (False, True):
        flags = capi.FLAG_TRACE | (capi.FLAG_CAPSULE_COST if on or mode == "no_box_pair" else 0)
        with capi.Context(spec, flags=flags) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if mode == "no_box_pair":
                if on:
                    ctx.set_capsule_boxes(SHAPES)
                cg.set_task(ctx, grid, caps, pairs, g, w)
            elif on:
                set_task(ctx, grid, caps, pairs, g, w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
            if on and mode == "never":
                assert 5.0 < np.min(ctx.capsule_clearance(1)) < np.inf
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
def test_neutrality_solve(gpu):
    """a 3-iteration ddp_hip_solve with non-zero weights on box pairs that nothing comes near: log and result bit for bit the
    flag-off solve's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 4, 2, 3, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 101, held=True)
    caps = cc.pick_capsules(model)
    pairs = [(a, BOX, a % 3) for a in range(len(caps))]
    g, w, _ = box_task(o, caps, pairs, xs, B, 102, None)
    g[..., 7] = -10.0
    w[:] = 50.0
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST if on else 0) as ctx:
            _setup(ctx, xs, us)
            if on:
                set_task(ctx, None, caps, pairs, g, w)
            log = solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
            res[on] = (log, ctx.download("X"), ctx.download("U"))
    assert not np.array_equal(res[True][1], xs)
    assert np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(res[False][0][k]), np.asarray(res[True][0][k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("chain6ff", 0), ("tree38", None)])
def test_equivalences(gpu, name, fo_):
    """two checks that do not go through the yardstick, to 1e-12.  (a) a 4 m cube, turned at random, with one face near the robot
    is a CAPSULE_VS_HALFSPACE pair with that face's plane: costs, LX, LXX, LFX, LFXX and clearances agree.  (b) a sphere capsule
    (end0 == end1) outside a box: the clearance is the closed form | max(|p| - h, 0) | - r - m in array arithmetic"""
    capi = gpu
    T, B, mu = 2, 2, 30.0
    model, spec, o = cc.make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 61)
    mults = tc._mults(o, xs[0], 62)
    rng = np.random.default_rng(63)
    caps = cc.pick_capsules(model)
    segs = [c for c in caps if c[1] != c[2]]
    big = np.array([[2.0, 2.0, 2.0]])

    def run(flags, prepare):
        with capi.Context(spec, flags=flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            prepare(ctx)
            ctx.linearize(capi.LIN_COST)
            r = {s: ctx.download(s) for s in ("LX", "LXX", "LFX", "LFXX")}
            ctx.cost_seq_aug(0, mu)
            r["COSTS_OLD"] = ctx.download("COSTS_OLD")
            r["clear"] = ctx.capsule_clearance(0) if flags else None
            return r
    off = run(0, lambda ctx: None)
    gb, gh = np.zeros((B, T + 1, len(segs), 8)), np.zeros((B, T + 1, len(segs), 8))
    wgt = rng.uniform(0.5, 5.0, size=(B, T + 1, len(segs)))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            E = cc.ends(o, segs, X[t][:o.nq])
            for a in range(len(segs)):
                qt = rng.normal(size=4)
                qt /= np.sqrt(qt @ qt)
                R = np.array(quat_R(qt))
                k, sgn = int(rng.integers(3)), float(rng.choice([-1.0, 1.0]))
                n = sgn * R[:, k]                                        # the outward normal of the face in the world
                p0, p1 = float(n @ E[a][0]), float(n @ E[a][1])
                assert abs(p0 - p1) > 1e-6
                m = rng.uniform(0.01, 0.1)                               # penetrates the margin by 1 .. 10 cm, 5 cm off the face
                hs = min(p0, p1) - 0.05
                mid = 0.5 * (E[a][0] + E[a][1])
                centre = mid - n * (float(n @ mid) - hs) - 2.0 * n      # the face's plane n . p = hs, the cube behind it
                gb[b, t, a, :3], gb[b, t, a, 3:7], gb[b, t, a, 7] = centre, qt, 0.05 - segs[a][3] + m
                gh[b, t, a, :3], gh[b, t, a, 3], gh[b, t, a, 7] = n, hs, 0.05 - segs[a][3] + m
    pb, ph = [(a, BOX, 0) for a in range(len(segs))], [(a, HALF, 0) for a in range(len(segs))]
    ra = run(capi.FLAG_CAPSULE_COST, lambda ctx: set_task(ctx, None, segs, pb, gb, wgt, shapes=big))
    rb = run(capi.FLAG_CAPSULE_COST, lambda ctx: cc.set_task(ctx, segs, ph, gh, wgt))
    for s in ("LX", "LXX", "LFX", "LFXX", "COSTS_OLD"):
        assert not np.array_equal(ra[s], off[s]), s                       # the term is there
        e = rel_err(ra[s], rb[s])
        print("equivalence half-space", name, s, e)
        assert e <= TOL, (s, e)
    assert np.min(ra["clear"]) < 0
    assert np.max(np.abs(ra["clear"] - rb["clear"]) / np.maximum(1.0, np.abs(rb["clear"]))) <= TOL
    # (b) the sphere of the sibling's capsules
    k = next(i for i, c in enumerate(caps) if c[1] == c[2])
    j, e0, _, rad = caps[k]
    gs = np.zeros((B, T + 1, 1, 8))
    ex = np.zeros((B, T + 1))
    half = SHAPES[1]
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            P = o.frame_position(j, e0, X[t][:o.nq])
            qt = rng.normal(size=4)
            qt /= np.sqrt(qt @ qt)
            centre = P + rng.uniform(0.6, 0.9) * cc._unit(rng)            # farther than the box's half diagonal: outside
            m = rng.uniform(-0.05, 0.05)
            gs[b, t, 0, :3], gs[b, t, 0, 3:7], gs[b, t, 0, 7] = centre, qt, m
            p = np.array(quat_R(qt)).T @ (P - centre)
            ex[b, t] = np.linalg.norm(np.maximum(np.abs(p) - half, 0.0)) - rad - m
    assert np.min(ex + rad) > 0
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, None, [caps[k]], [(0, BOX, 1)], gs, np.ones(1))
        clear = ctx.capsule_clearance(0)
    e = np.max(np.abs(clear - ex) / np.maximum(1.0, np.abs(ex)))
    print("equivalence sphere", name, e)
    assert e <= TOL, e


@pytest.mark.gpu
def test_refusals(gpu):
    """each refused with nothing written: kind 4 before set_boxes; pair_b out of range; an extent <= 0 or non-finite; n_boxes = 9; a
    non-unit or non-finite quaternion; a non-finite centre or margin; set_boxes shrinking under a live pair; set_boxes on a context
    without the flag.  set_pairs again with the same counts and kinds keeps the data; extents may change while the pairs stand"""
    capi = gpu
    T, B, mu = 2, 2, 30.0
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 71)
    caps = cc.pick_capsules(model)
    pairs = [(0, BOX, 0), (1, HALF, 0), (2, BOX, 2), (3, BOX, 1)]
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        assert code(capi, lambda: ctx.set_capsule_boxes(SHAPES)) == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        assert code(capi, lambda: ctx.set_capsule_pairs(capsules=caps, pairs=pairs)) == capi.E_ARG          # no boxes yet
        ctx.set_capsule_boxes(SHAPES[:2])
        assert code(capi, lambda: ctx.set_capsule_pairs(capsules=caps, pairs=pairs)) == capi.E_ARG          # shape 2 of 2
        assert code(capi, lambda: ctx.set_capsule_pairs(capsules=caps, pairs=[(0, BOX, -1)])) == capi.E_ARG
        for bad in (0.0, -0.1, np.inf, np.nan):
            hb = SHAPES.copy()
            hb[1, 2] = bad
            assert code(capi, lambda: ctx.set_capsule_boxes(hb)) == capi.E_ARG, bad
        assert code(capi, lambda: ctx.set_capsule_boxes(np.ones((9, 3)))) == capi.E_ARG
        assert code(capi, lambda: ctx.set_capsule_pairs(capsules=caps, pairs=pairs)) == capi.E_ARG          # the refused calls changed nothing
        ctx.set_capsule_boxes(np.ones((8, 3)))
        ctx.set_capsule_boxes(SHAPES)
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        g, w, _ = box_task(o, caps, pairs, xs, B, 72, None)
        ctx.set_capsule_cost(geom=g, weight=w)
        for e in range(8):
            for bad in (np.nan, np.inf):
                gb = g.copy()
                gb[1, 2, 2, e] = bad
                assert code(capi, lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG, (e, bad)
        gb = g.copy()
        gb[0, 1, 3, 3:7] *= 1.0 + 1e-9                                   # not unit by the interface's rule
        assert code(capi, lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG
        gb = g.copy()
        gb[0, 1, 0, 3:7] = 0.0
        assert code(capi, lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG
        gb = g.copy()
        gb[0, 1, 1, 3:7] = 0.0                                           # a half-space's ignored entries may be anything finite
        ctx.set_capsule_cost(geom=gb)
        ctx.set_capsule_cost(geom=g)
        assert np.array_equal(ctx.capsule_cost()[0], g) and np.array_equal(ctx.capsule_cost()[1], w)
        assert code(capi, lambda: ctx.set_capsule_boxes(SHAPES[:2])) == capi.E_ARG                          # pair 2 names shape 2
        assert code(capi, lambda: ctx.set_capsule_boxes(np.zeros((0, 3)))) == capi.E_ARG
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)                                                 # same counts and kinds
        assert np.array_equal(ctx.capsule_cost()[0], g) and np.array_equal(ctx.capsule_cost()[1], w)
        ctx.set_capsule_pairs(capsules=caps, pairs=[(0, BOX, 1), (1, HALF, 0), (2, BOX, 0), (3, BOX, 1)])   # other shapes, same kinds
        assert np.array_equal(ctx.capsule_cost()[0], g)
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        # extents change while the pairs stand: the next launch reads the new ones
        clear0 = ctx.capsule_clearance(0)
        ctx.set_capsule_boxes(1.5 * SHAPES)
        clear1 = ctx.capsule_clearance(0)
        ev = box_eval(1.5 * SHAPES, cg._SIBLING_EVAL)
        for b in range(B):
            X = xs[b].reshape(T + 1, o.nx)
            for t in range(T + 1):
                E = cc.ends(o, caps, X[t][:o.nq])
                ds = [ev(caps, E, p, g[b, t, i])["d"] for i, p in enumerate(pairs) if w[b, t, i] != 0.0]
                assert abs(clear1[b, t] - min(ds)) <= 1e-9, (b, t)
        assert not np.array_equal(clear0, clear1)
        ctx.set_capsule_pairs(capsules=caps, pairs=[(0, HALF, 0), (1, HALF, 0), (2, BOX, 2), (3, BOX, 1)])  # another kind: reset
        assert np.all(ctx.capsule_cost()[0] == 0.0) and np.all(ctx.capsule_cost()[1] == 0.0)
        ctx.set_capsule_boxes(SHAPES)                                     # ... and zero geometry under zero weights is never evaluated
        ctx.cost_seq_aug(0, mu)
        assert np.all(np.isfinite(ctx.download("COSTS_OLD")))
        assert np.all(ctx.capsule_clearance(0) == np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 2])
def test_advance_shifts_rows(gpu, shift):
    """ddp_hip_advance: a box pair's geometry and weights move like the others' (rows 0 .. T-1 by the hold rule, row T untouched);
    the shapes are context state and stay"""
    capi = gpu
    T, B = 3, 2
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    xs, us = _trajs(o, model, B, 181)
    caps = cc.pick_capsules(model)
    pairs = [(0, BOX, 0), (1, WORLD, 0), (2, BOX, 2), (3, HALF, 0), (4, BOX, 1)]
    g, w, _ = box_task(o, caps, pairs, xs, B, 182, None)
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as ctx:
        _setup(ctx, xs, us)
        set_task(ctx, None, caps, pairs, g, w)
        ctx.advance(shift, None, capi.ADVANCE_NO_ROLL)
        g1, w1 = ctx.capsule_cost()
        assert code(capi, lambda: ctx.set_capsule_boxes(SHAPES[:2])) == capi.E_ARG      # the pairs and their shapes stand
    assert np.array_equal(g1, adv.np_advance(g, shift, terminal=True)) and np.array_equal(w1, adv.np_advance(w, shift, terminal=True))
    assert np.array_equal(g1[:, T], g[:, T]) and np.array_equal(w1[:, T], w[:, T]) and not np.array_equal(g1, g)
    assert np.array_equal(g1[:, 0], g[:, shift])


REACH_WEIGHT = 1e7          # the sibling's 1e6 leaves -1.9 cm in this scene: raised by a decade, the bound stays (reach_clearances)


def reach_clearances(capi, weight):
    """chain6, T = 40, 30 iterations of ddp_hip_solve (the sibling's reach task): a tracking cost pulls the arm to a goal posture,
    the last link carries a capsule.  The flag-off solve's tip path is taken first; a board (30 x 8 x 8 cm, its long axis across
    the path, turned with it) is then put on the path, halfway, so that the target lies on its far side.  Returns the least
    clearance of the flag-off solution and of the solve with the term at `weight`, from the same start"""
    from ddp_pinocchio_amd import solver
    T, iters, thr, mu, w_, n_ = 40, 30, 1e-9, 1.0, 1e-1, 10.0
    model, spec, o = cc._reach_problem(T)
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
    ex = np.cross(travel, [0.0, 0.0, 1.0])
    ex /= np.linalg.norm(ex)                                                 # the board's long axis: across the path
    ey = travel / np.linalg.norm(travel)
    ey = ey - (ey @ ex) * ex
    ey /= np.linalg.norm(ey)
    Rm = np.stack([ex, ey, np.cross(ex, ey)], axis=1)
    qw = 0.5 * math.sqrt(max(1e-12, 1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2]))
    quat = np.array([(Rm[2, 1] - Rm[1, 2]) / (4 * qw), (Rm[0, 2] - Rm[2, 0]) / (4 * qw), (Rm[1, 0] - Rm[0, 1]) / (4 * qw), qw])
    quat /= np.sqrt(quat @ quat)
    assert qw > 0.1 and np.max(np.abs(np.array(quat_R(quat)) - Rm)) < 1e-12
    shapes = np.array([[0.15, 0.04, 0.04]])
    geom = np.concatenate([path[T // 2], quat, [0.0]])[None, :]
    pairs = [(0, BOX, 0)]
    ev = box_eval(shapes, cg._SIBLING_EVAL)

    def clearance(x):
        X = x.reshape(T + 1, o.nx)
        return min(ev([link], cc.ends(o, [link], X[t][:o.nq]), pairs[0], geom[0])["d"] for t in range(T + 1))
    assert clearance(xs[0]) > 0.0                                            # the arm starts clear of it
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        ctx.set_tracking_cost(xref=xref, wx=wx)
        set_task(ctx, None, [link], pairs, geom, np.full(1, weight), shapes=shapes)
        _setup(ctx, x_off, us)
        clear_off = float(np.min(ctx.capsule_clearance(0)))
        _setup(ctx, xs, us)
        solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
        clear_on = float(np.min(ctx.capsule_clearance(0)))
        x_on = ctx.download("X")
    assert abs(clear_on - clearance(x_on[0])) <= 1e-9
    return clear_off, clear_on, link[3]


@pytest.mark.gpu
def test_reach_past_table_edge(gpu):
    """the tip must reach a target on the far side of a table edge (reach_clearances).  Without the term the link enters the box by
    more than 2 cm; with it, from the same start, the least clearance is at or above -DEPTH_TOL = -1 cm (the sibling's bound).  The
    penalty is soft and its depth goes with 1 / weight.  Measured on an MI355X, least clearance after 30 iterations: -7.0 cm
    without the term, -1.9 cm at the sibling's weight 1e6; the weight here is a decade above (DESIGN.md section 4ze has the depth
    per weight)"""
    clear_off, clear_on, radius = reach_clearances(gpu, REACH_WEIGHT)
    print("reach past table edge: clearance without the term", clear_off, "with it", clear_on, "weight", REACH_WEIGHT)
    assert clear_off + radius < -0.02, clear_off                             # the link's axis is more than 2 cm inside the box
    assert clear_on >= -cc.DEPTH_TOL, clear_on
