"""Capsule pairs of kind CAPSULE_VS_GRID (ddp_hip.h): body B is the context's resident signed distance field.

The yardstick is the sibling's (test_capsule_cost.py) with a fourth branch in pair_eval, restated here in numpy from the header:
the interval rule, the N + 1 material points, the trilinear lookup of test_obstacle_grid.py, the smallest j attaining the least
value, d = phi - r_a - m, u = grad phi at the selected sample, the point frozen in A's joint.  Tolerances are the siblings':
1e-12 relative for values, clearances and derivatives.

Stability of the argmin.  A case whose two smallest finite phi_j differ by less than 1e-9 (metres), or whose selected sample lies
within 1e-9 of a cell face (where the interpolant's gradient jumps), is excluded -- its weight is 0, or it is left out of a
comparison of j -- and every test that does so asserts that the excluded share is at most 5 %.
"""
import math
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import test_advance as adv
import test_capsule_cost as cc
import test_frame_cost as fc
import test_obstacle_cost as oc
import test_obstacle_grid as og
import test_tracking_cost as tc
from problems import make
from synth import rel_err

ROOT = cc.ROOT
TOL = 1e-12                  # what the sibling tests hold values, clearances and derivatives to
GAP = 1e-9                   # the exclusion rule's gap between the two smallest finite samples
ROBOT, WORLD, HALF, GRID = 0, 1, 2, 3
MAXN = 32
DERIVS = cc.DERIVS
_trajs, _setup = tc._trajs, tc._setup
_SIBLING_EVAL = cc.pair_eval
MODELS = [("chain6", None), ("chain6ff", 0), ("tree38", None)]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def intervals(e0, e1, cell):
    """N_k of the header: 0 for a sphere, else ceil(L / cell) within 1 .. 32; every product rounded on its own"""
    dx, dy, dz = (float(e1[k]) - float(e0[k]) for k in range(3))
    L = math.sqrt(dx * dx + dy * dy + dz * dz)
    if L == 0.0:
        return 0
    r = math.ceil(L / cell)
    return int(min(MAXN, max(1, r)))


def segment_rule(grid, a0, a1, shift, N):
    """the rule on one world segment: phi (the least sample, +inf: every sample outside), j (-1 then), the material point c, the
    gradient there (None outside), every sample's value, the gap between the two smallest finite ones (inf with fewer than
    two) and the selected sample's distance, in cells, to a cell face"""
    phi, origin, cell = grid
    a0, a1, shift = (np.asarray(v, dtype=float) for v in (a0, a1, shift))
    vals, pts = [], []
    for j in range(N + 1):
        sigma = j / N if N else 0.0
        c = a0 + sigma * (a1 - a0)
        pts.append(c)
        vals.append(og.lookup(phi, origin, cell, c - shift)[0])
    bj = 0
    for j in range(1, N + 1):
        if vals[j] < vals[bj]:
            bj = j
    fin = sorted(v for v in vals if np.isfinite(v))
    out = {"vals": vals, "gap": (fin[1] - fin[0]) if len(fin) > 1 else np.inf, "N": N}
    if not np.isfinite(vals[bj]):
        out.update(phi=np.inf, j=-1, c=a0, grad=None, edge=np.inf)
        return out
    val, grad = og.lookup(phi, origin, cell, pts[bj] - shift)
    s = (pts[bj] - shift - origin) / cell
    f = s - np.floor(s)
    inner = (s > 1e-9) & (s < np.array(phi.shape) - 1 - 1e-9)            # (on the grid's own boundary the cell is the only one)
    out.update(phi=val, j=bj, c=pts[bj], grad=grad, edge=float(np.min(np.where(inner, np.minimum(f, 1.0 - f), 0.5))))
    return out


def stable(r):
    return r["gap"] >= GAP and r["edge"] > 1e-9


def grid_eval(grid):
    """the sibling's pair_eval(caps, E, pair, g) with the fourth kind: g = (shift, ., ., ., ., margin)"""
    def pair_eval(caps, E, pair, g):
        if pair[1] != GRID:
            return _SIBLING_EVAL(caps, E, pair, g)
        a = pair[0]
        N = intervals(caps[a][1], caps[a][2], grid[2])
        r = segment_rule(grid, E[a][0], E[a][1], g[:3], N)
        info = {"sphere": True, "gap": r["gap"], "rule": r}
        if r["j"] < 0:
            return {"D": None, "d": np.inf, "u": None, "s": 0.0, "t": None, "info": info}
        u = r["grad"]
        return {"D": None, "d": r["phi"] - caps[a][3] - g[7], "u": (u if np.any(u != 0.0) else None), "s": (r["j"] / N if N else 0.0),
                "t": None, "info": info, "ca": r["c"]}
    return pair_eval


@functools.lru_cache(maxsize=None)
def sphere_scene(cell=0.05, shape=(12, 10, 8), origin=(-0.2, 0.1, 0.05), R=0.12):
    """the 12 x 10 x 8 scene: |p - c| - R sampled at the nodes, the centre a little off the grid's middle"""
    origin = np.array(origin, dtype=float)
    centre = origin + cell * (np.array(shape) - 1) * np.array([0.45, 0.55, 0.4])
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    phi = np.linalg.norm(origin + cell * idx - centre, axis=-1) - R
    phi.setflags(write=False)
    return phi, origin, cell


def plane_scene(n, h, cell=0.05, shape=(12, 10, 8), origin=(-0.2, 0.1, 0.05)):
    """n . p - h sampled at the nodes: the trilinear interpolant is the function itself"""
    origin = np.array(origin, dtype=float)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), -1)
    return (origin + cell * idx) @ np.asarray(n, dtype=float) - h, origin, cell


def extent(grid):
    return grid[1], grid[1] + grid[2] * (np.array(grid[0].shape) - 1)


def mixed_pairs(caps):
    """the sibling's 19 pairs of three kinds and, behind and between them, 4 grid pairs (a sphere's among them): 23"""
    p = cc.pick_pairs(caps)
    return [(1, GRID, 0)] + p[:10] + [(3, GRID, 0)] + p[10:] + [(0, GRID, 0), (2, GRID, 0)]


def grid_task(o, caps, pairs, xs, B, seed, grid, p_out=0.15):
    """geom (B, T+1, n_pairs, 8), weights (B, T+1, n_pairs) and the excluded share.  The pairs of the three older kinds by the
    sibling's generator.  A grid pair, per (instance, t): the shift brings the capsule's middle to a random place inside the
    grid (an end may stick out), with probability p_out the whole capsule far outside; the margin makes the pair penetrate by
    0.01 .. 0.1 or stay clear by as much.  The first grid pair is active at t = 0, its middle at the field's deepest node, and
    clear at t = 1, the last one outside at t = 0.  A pair that the exclusion rule (module docstring) leaves out has weight 0"""
    phi, origin, cell = grid
    rng = np.random.default_rng(seed)
    plain = [(p[0], HALF if p[1] == GRID else p[1], p[2] if len(p) > 2 else 0) for p in pairs]
    g, w = cc.random_task(o, caps, plain, xs, B, seed + 1)
    ev = grid_eval(grid)
    gi = [i for i, p in enumerate(pairs) if p[1] == GRID]
    excluded = total = 0
    for b in range(B):
        X = xs[b].reshape(o.T + 1, o.nx)
        for t in range(o.T + 1):
            E = cc.ends(o, caps, X[t][:o.nq])
            for i in gi:
                a = pairs[i][0]
                mid = 0.5 * (E[a][0] + E[a][1])
                out = rng.uniform() < p_out
                inside = rng.uniform() < 0.5
                if i == gi[0] and t < 2:
                    out, inside = False, t == 0
                if i == gi[-1] and t == 0:
                    out = True
                node = np.array([rng.integers(0, n - 1) for n in phi.shape])
                if i == gi[0] and t == 0:                               # across the field's deepest place: a middle sample wins
                    node = np.minimum(np.array(np.unravel_index(np.argmin(phi), phi.shape)), np.array(phi.shape) - 2)
                x = origin + cell * (node + rng.uniform(0.2, 0.8, 3)) - (np.array([3.0, 3.0, 3.0]) if out else 0.0)
                g[b, t, i, :3] = mid - x
                g[b, t, i, 3:7] = rng.normal(size=4)                    # ignored entries: finite, not zero
                g[b, t, i, 7] = 0.0
                w[b, t, i] = rng.uniform(0.5, 5.0)
                r = ev(caps, E, pairs[i], g[b, t, i])
                total += 1
                if r["d"] == np.inf:
                    assert out or i != gi[0]
                    continue
                assert not out
                depth = rng.uniform(0.01, 0.1)
                g[b, t, i, 7] = r["d"] + (depth if inside else -depth)
                if not stable(r["info"]["rule"]) or r["u"] is None:
                    w[b, t, i] = 0.0
                    excluded += 1
    return g, w, excluded / total


def check_grid_task(monkeypatch, o, caps, pairs, xs, g, w, grid, share, need=True):
    """the conditions on the inputs, on the yardstick alone, with cc.pair_eval the four-kind one from here on: the sibling's,
    the excluded share, and with `need` in every instance an active, a clear and an outside grid pair and, somewhere, one
    whose selected sample is neither end.  Returns the blocks' activity"""
    monkeypatch.setattr(cc, "pair_eval", grid_eval(grid))
    assert share <= 0.05, share
    active = cc.check_task(o, caps, pairs, xs, g, w, fractions=False)
    n_mid = 0
    for b in range(xs.shape[0]):
        X = xs[b].reshape(o.T + 1, o.nx)
        n_act = n_clear = n_out = 0
        for t in range(o.T + 1):
            E = cc.ends(o, caps, X[t][:o.nq])
            for i, p in enumerate(pairs):
                if p[1] != GRID or w[b, t, i] == 0.0:
                    continue
                r = cc.pair_eval(caps, E, p, g[b, t, i])
                n_out += r["d"] == np.inf
                n_act += r["d"] < 0
                n_clear += 0 < r["d"] < np.inf
                rule = r["info"]["rule"]
                n_mid += 0 < rule["j"] < rule["N"]
        if need:
            assert n_act >= 1 and n_clear >= 1 and n_out >= 1, (b, n_act, n_clear, n_out)
    assert n_mid >= 1 or not need
    return active


def set_task(ctx, grid, caps, pairs, geom=None, weight=None):
    ctx.set_obstacle_grid(*grid)
    cc.set_task(ctx, caps, pairs, geom, weight)


def code(capi, fn):
    with pytest.raises(capi.DdpHipError) as exc:
        fn()
    return exc.value.code


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def lookup_many(grid, P):
    """og.lookup's value at many points at once (inside ones; +inf outside)"""
    phi, origin, cell = grid
    n = np.array(phi.shape)
    s = (P - origin) / cell
    ok = np.all((s >= 0) & (s <= n - 1), axis=1)
    s = np.where(ok[:, None], s, 0.0)
    i = np.minimum(np.floor(s).astype(int), n - 2)
    f = s - i
    val = np.zeros(len(P))
    for c in range(8):
        cx, cy, cz = c >> 2, (c >> 1) & 1, c & 1
        wgt = (f[:, 0] if cx else 1 - f[:, 0]) * (f[:, 1] if cy else 1 - f[:, 1]) * (f[:, 2] if cz else 1 - f[:, 2])
        val += phi[i[:, 0] + cx, i[:, 1] + cy, i[:, 2] + cz] * wgt
    return np.where(ok, val, np.inf)


def test_yardstick_against_dense_scan():
    """the restated rule against a scan of 2 001 points per segment on the sphere scene: min_j phi_j is no smaller than the
    scan's minimum (N divides 2 000 here, so every sample is a scan point) and, for a segment that lies inside the grid, no
    larger than it plus L / (2 N) times a bound of the interpolant's gradient norm (each component is a convex combination of
    the cell's edge differences over the cell)"""
    grid = sphere_scene()
    phi, origin, cell = grid
    lo, hi = extent(grid)
    rng = np.random.default_rng(5)
    P = lo + rng.uniform(size=(50, 3)) * (hi - lo)
    assert np.max(np.abs(lookup_many(grid, P) - np.array([og.lookup(phi, origin, cell, p)[0] for p in P]))) <= 1e-15
    G = math.sqrt(sum(float(np.max(np.abs(np.diff(phi, axis=a)))) ** 2 for a in range(3))) / cell
    assert 1.0 <= G <= 1.8                                              # (a distance field: about 1 per axis at the worst)
    sig = np.linspace(0.0, 1.0, 2001)
    n_in = 0
    for trial in range(60):
        N = (1, 2, 4, 5, 8, 10)[trial % 6]
        mid = lo + rng.uniform(0.2, 0.8, 3) * (hi - lo)
        half = 0.5 * rng.uniform((N - 1) * cell, N * cell) * cc._unit(rng)
        a0, a1 = mid - half, mid + half
        assert intervals(a0, a1, cell) == N
        r = segment_rule(grid, a0, a1, np.zeros(3), N)
        scan = np.min(lookup_many(grid, a0[None, :] + sig[:, None] * (a1 - a0)[None, :]))
        assert r["phi"] >= scan - 1e-12, (trial, r["phi"], scan)
        if np.all(np.isfinite(r["vals"])) and np.all((np.minimum(a0, a1) >= lo) & (np.maximum(a0, a1) <= hi)):
            n_in += 1
            assert r["phi"] <= scan + np.linalg.norm(a1 - a0) / (2 * N) * G + 1e-12, (trial, r["phi"], scan)
    assert n_in >= 30, n_in


def test_yardstick_plane_and_point():
    """on a field sampled from a plane n . p - h the interpolant is exact: the rule's d is capsule_halfspace_point's, to 1e-12,
    for 200 random segments; with end0 == end1 the rule is the point lookup, exactly"""
    rng = np.random.default_rng(6)
    n = cc._unit(rng)
    grid = plane_scene(n, 0.17)
    phi, origin, cell = grid
    lo, hi = extent(grid)
    for trial in range(200):
        a0, a1 = (lo + rng.uniform(size=3) * (hi - lo) for _ in range(2))
        ra, m = rng.uniform(0.0, 0.05), rng.uniform(-0.05, 0.05)
        N = intervals(a0, a1, cell)
        assert 1 <= N <= 15
        r = segment_rule(grid, a0, a1, np.zeros(3), N)
        d = r["phi"] - ra - m
        p0, p1 = cc._dot(n, a0), cc._dot(n, a1)
        ex = min(p0, p1) - 0.17 - ra - m
        assert abs(d - ex) <= 1e-12 * max(1.0, abs(ex)), (trial, d, ex)
        assert r["j"] == (N if p1 < p0 else 0) or r["gap"] < GAP
        assert np.max(np.abs(r["grad"] - n)) <= 1e-12
    sgrid = sphere_scene()
    lo, hi = extent(sgrid)
    for trial in range(20):
        p = lo + rng.uniform(size=3) * (hi - lo)
        assert intervals(p, p, sgrid[2]) == 0
        r = segment_rule(sgrid, p, p, np.zeros(3), 0)
        val, grad = og.lookup(*sgrid, p)
        assert r["phi"] == val and r["j"] == 0 and np.array_equal(r["grad"], grad) and np.array_equal(r["c"], p)


def test_capsule_grid_block_host_logic():
    """host/test_capsule_grid_block.cpp: the interval rule, the library's sampling routine compiled for the host against values
    worked out by hand, the dealt scan against the scan on one lane, the pair-list rule with and without a resident grid"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_capsule_grid_block"])
    out = subprocess.run([os.path.join(host, "test_capsule_grid_block")], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.CAPSULE_VS_GRID == 3 and re.search(r"#define\s+DDP_HIP_CAPSULE_VS_GRID\s+3\b", header)
    assert capi.CAPSULE_GRID_MAX_INTERVALS == 32 and re.search(r"#define\s+DDP_HIP_CAPSULE_GRID_MAX_INTERVALS\s+32\b", header)
    L = capi.lib()
    name = "ddp_hip_obstacle_grid_segment_query"
    assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name)
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert hasattr(capi.Context, "obstacle_grid_segment_query")
    # shapes are checked before anything reaches the library: a context object without a device will do
    model, spec, _ = make("chain6", 3, batch=1, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, 1, None
    for seg, n in ((np.zeros((4, 5)), 1), (np.zeros(6), 1), (np.zeros((4, 6)), np.zeros(3)), (np.zeros((4, 6)), np.zeros((4, 1)))):
        with pytest.raises(ValueError, match="obstacle_grid_segment_query"):
            ctx.obstacle_grid_segment_query(seg, n)
    doc = capi.Context.set_capsule_cost.__doc__
    assert "grid pair" in doc and "CAPSULE_VS_GRID" in capi.Context.set_capsule_pairs.__doc__


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _capsule_ctx(capi, T=1, batch=1):
    model, spec, o = make("chain6", T, batch=batch, fd_mode=0)
    return capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS)


def _query_segments(grid, rng):
    """300 segments and interval counts: inside, straddling a face, outside, degenerate, through the last cell of each axis"""
    lo, hi = extent(grid)
    span = hi - lo
    seg, nint = [], []
    for k in range(300):
        kind = k % 5
        a0 = lo + rng.uniform(0.05, 0.95, 3) * span
        a1 = lo + rng.uniform(0.05, 0.95, 3) * span
        N = int(rng.integers(1, MAXN + 1))
        if kind == 1:                                                   # one end beyond a face
            ax = int(rng.integers(3))
            a1[ax] = (hi[ax] + rng.uniform(0.01, 0.3)) if rng.uniform() < 0.5 else (lo[ax] - rng.uniform(0.01, 0.3))
        elif kind == 2:                                                 # both beyond the same face
            ax = int(rng.integers(3))
            a0[ax], a1[ax] = hi[ax] + rng.uniform(0.01, 0.3), hi[ax] + rng.uniform(0.01, 0.3)
        elif kind == 3:                                                 # a point: one sample
            a1, N = a0.copy(), 0
        elif kind == 4:                                                 # an end on the last node of an axis, through its last cell
            ax = k // 5 % 3
            a1[ax] = hi[ax]
            a0[ax] = hi[ax] - rng.uniform(0.2, 1.5) * grid[2]
        if k in (7, 8):
            N = MAXN
        seg.append(np.concatenate([a0, a1])); nint.append(N)
    return np.array(seg), np.array(nint, dtype=np.int32)


@pytest.mark.gpu
def test_segment_query(gpu):
    """ddp_hip_obstacle_grid_segment_query on 300 segments of the sphere scene and on the 2 x 2 x 2 edge grid: j against the
    restatement (exclusion rule: module docstring), phi to 1e-12; phi, point and gradient bit-equal to obstacle_grid_query at
    the returned point; -1, +inf, the first end and a zero gradient where every sample is outside"""
    capi = gpu
    rng = np.random.default_rng(11)
    edge = (np.array([1.0, 2, 3, 5, 7, 11, 13, 17]).reshape(2, 2, 2), np.array([1.0, -1.0, 2.0]), 0.5)
    with _capsule_ctx(capi) as ctx:
        for grid in (sphere_scene(), edge):
            ctx.set_obstacle_grid(*grid)
            seg, nint = _query_segments(grid, rng)
            phi, j, pt, gr = ctx.obstacle_grid_segment_query(seg, nint)
            excluded = n_out = n_mid = 0
            for k in range(len(seg)):
                r = segment_rule(grid, seg[k, :3], seg[k, 3:], np.zeros(3), int(nint[k]))
                if r["gap"] < GAP:
                    excluded += 1
                    continue
                assert j[k] == r["j"], (k, j[k], r["j"])
                if r["j"] < 0:
                    n_out += 1
                    assert phi[k] == np.inf and np.array_equal(pt[k], seg[k, :3]) and np.all(gr[k] == 0.0)
                    continue
                n_mid += 0 < r["j"] < nint[k]
                assert abs(phi[k] - r["phi"]) <= TOL * max(1.0, abs(r["phi"])), (k, phi[k], r["phi"])
                assert np.max(np.abs(pt[k] - r["c"])) <= TOL
            assert excluded <= 0.05 * len(seg), excluded
            assert n_out >= 30 and n_mid >= 30, (n_out, n_mid)
            ins = j >= 0
            val, g = ctx.obstacle_grid_query(pt[ins])
            assert np.array_equal(val, phi[ins]) and np.array_equal(g, gr[ins])
            one = ctx.obstacle_grid_segment_query(seg[:1], int(nint[0]))            # a count for all, a single segment
            assert one[0][0] == phi[0] and one[1][0] == j[0]
        # a tie is the first sample's: a segment in a plane of constant phi of the edge grid's x edge field
        flat = (np.full((2, 2, 2), -0.25), edge[1], edge[2])
        ctx.set_obstacle_grid(*flat)
        phi, j, pt, gr = ctx.obstacle_grid_segment_query(np.array([[1.0, -1.0, 2.0, 1.5, -0.5, 2.5]]), 7)
        assert j[0] == 0 and phi[0] == -0.25 and np.all(gr[0] == 0.0) and np.array_equal(pt[0], [1.0, -1.0, 2.0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", MODELS)
def test_values_and_clearance(gpu, monkeypatch, name, fo_):
    """COSTS_OLD (ddp_hip_cost_seq_aug) against the flag-off context's values plus the numpy terms, and ddp_hip_capsule_clearance
    against the yardstick, to 1e-12: all four kinds in one context, 19 + 4 pairs, batch 3, every instance and t its own
    geometry.  A block without an active pair keeps the flag-off value bit for bit; a pair whose samples are all outside the
    grid is invisible to the clearance"""
    capi = gpu
    T, B, mu = 4, 3, 30.0
    grid = sphere_scene()
    model, spec, o = cc.make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    caps = cc.pick_capsules(model)
    pairs = mixed_pairs(caps)
    assert len(pairs) == 23 and sorted({p[1] for p in pairs}) == [0, 1, 2, 3]
    g, w, share = grid_task(o, caps, pairs, xs, B, 52, grid)
    last = len(pairs) - 1
    w[0, 0, :] = 0.0
    w[0, 0, last] = 2.0                                                 # instance 0, t = 0: the one live pair is outside the grid
    active = check_grid_task(monkeypatch, o, caps, pairs, xs, g, w, grid, share)
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
    for b in range(B):
        add = cc.cp_terms(o, caps, pairs, xs[b], g[b], w[b])
        assert np.any(add != 0.0) and np.array_equal(add != 0.0, active[b])
        e = rel_err(got[True][b], got[False][b] + add)
        print("values", name, b, e)
        assert e <= TOL, (b, e)
        assert np.array_equal(got[True][b][~active[b]], got[False][b][~active[b]])
    ex = np.stack([cc.cp_clearance(o, caps, pairs, xs[b], g[b], w[b]) for b in range(B)])
    assert clear[0, 0] == np.inf and ex[0, 0] == np.inf and np.array_equal(np.isinf(clear), np.isinf(ex))
    fin = np.isfinite(ex)
    assert np.min(ex[fin]) < 0
    e = np.max(np.abs(clear[fin] - ex[fin]) / np.maximum(1.0, np.abs(ex[fin])))
    print("clearance", name, e)
    assert e <= TOL, e


LIN_CASES = [("chain6", 2, None), ("chain6", 0, None), ("chain6ff", 2, 0), ("tree38", 0, None), ("tree38", 2, None)]


def _fd_check(o, model, caps, pairs, x, g_t, w_t):
    """on the restatement alone: central differences at step 1e-6 of a live grid pair's d against the frozen-point gradient z, to
    1e-6 relative.  Returns how many pairs were compared"""
    h, n = 1e-6, 0
    q = x[:o.nq]
    E = cc.ends(o, caps, q)
    for i, pair in enumerate(pairs):
        if pair[1] != GRID or w_t[i] == 0.0:
            continue
        ev = cc.pair_eval(caps, E, pair, g_t[i])
        if ev["u"] is None:
            continue
        z, cols = cc.cp_z(o, model, caps, pair, q, ev)
        fd = np.zeros(o.nv)
        for c in cols:
            dx = np.zeros(o.n); dx[c] = h
            dp = cc.pair_eval(caps, cc.ends(o, caps, tc._integrate_x(o, x, dx)[:o.nq]), pair, g_t[i])["d"]
            dm = cc.pair_eval(caps, cc.ends(o, caps, tc._integrate_x(o, x, -dx)[:o.nq]), pair, g_t[i])["d"]
            fd[c] = (dp - dm) / (2 * h)
        assert np.max(np.abs(fd - z)) <= 1e-6 * max(1.0, np.max(np.abs(z))), (i, np.max(np.abs(fd - z)), np.max(np.abs(z)))
        n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, monkeypatch, name, fd_mode, fo_, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the restatement's frozen-point terms, batch 3, 19 + 4 pairs of all four
    kinds, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU, LUU, LUX,
    every velocity row and column and the q rows outside the active pairs' column sets bit for bit the flag-off values.  On the
    restatement alone: central differences of a grid pair's d agree with the frozen-point gradient (_fd_check)"""
    capi = gpu
    T, B = 3, 3
    grid = sphere_scene()
    model, spec, o = cc.make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    caps = cc.pick_capsules(model)
    pairs = mixed_pairs(caps)
    g, w, share = grid_task(o, caps, pairs, xs, B, 43, grid)
    w[1, 2, 0] = 0.0; w[0, T, 11] = 0.0
    active = check_grid_task(monkeypatch, o, caps, pairs, xs, g, w, grid, share)
    if stages is None and fd_mode == 2:
        X0 = xs[0].reshape(T + 1, o.nx)
        assert sum(_fd_check(o, model, caps, pairs, X0[t], g[0, t], w[0, t]) for t in range(T + 1)) >= 4
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
    for b in range(B):
        add = cc.cp_derivs(o, model, caps, pairs, xs[b], g[b], w[b])
        gonly = cc.cp_derivs(o, model, caps, pairs, xs[b], g[b], w[b] * np.array([p[1] == GRID for p in pairs]))
        assert np.max(np.abs(gonly["LX"])) > 0                          # the grid pairs contribute
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
            if model.ff and gonly["rows"][t].any():
                assert gonly["rows"][t][:6].all()                       # a world pair: the root's six columns carry it
    print("linearize", name, fd_mode, stages, "worst", worst, "active blocks", int(active.sum()), "of", active.size)


def blocking_task(o, caps, pairs, geom, xs, us, mults, fb, mu):
    """the sibling's: margins that leave xs clear by 1 cm at every t and a weight on the pair whose distance shrinks most under
    the full step.  A pair outside the grid on either trajectory keeps margin 0 and cannot be chosen"""
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
    both = np.isfinite(Do) & np.isfinite(Dn)
    g[..., 7] = np.where(np.isfinite(Do), Do - 0.01, 0.0)
    with np.errstate(invalid="ignore"):
        shrink = np.max(np.where(both, Do - Dn, -np.inf), axis=0)
    shrink[~np.all(both, axis=0)] = -np.inf
    i_ = int(np.argmax(shrink))
    sel = np.zeros((T + 1, len(pairs)))
    sel[:, i_] = 1.0
    unit = cc.cp_terms(o, caps, pairs, x1, g, sel).sum()
    return g, sel * (5.0 * abs(gain) / unit if unit > 0.0 else 0.0), gain, float(shrink[i_])


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path", [("tree38", None, 1), ("chain6ff", 0, 0)])
@pytest.mark.parametrize("n_alpha", [1, 4])
def test_forward_matches_emulation(gpu, monkeypatch, name, fo_, fwd_path, n_alpha):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the grid pairs' terms
    included (the siblings' emulation): five grid pairs, the old trajectory clear by 1 cm, the pair the full step brings closest
    weighted so that the full step is rejected; decisions are compared only where every candidate decides by more than 1e-9"""
    capi = gpu
    T, mu = 16, 1.0
    grid = sphere_scene()
    monkeypatch.setattr(cc, "pair_eval", grid_eval(grid))
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    caps = cc.pick_capsules(model)
    pairs = [(a, GRID, 0) for a in range(len(caps))]
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
            geom, _, share = grid_task(o, caps, pairs, xs, 1, seed + 100, grid, p_out=0.0)
            g, w, gain, shrink = blocking_task(o, caps, pairs, geom[0], xs[0], us[0], mults, fb, mu_o[0])
            if shrink > 0.01 and share <= 0.05:
                break
        assert shrink > 0.01, shrink
        set_task(ctx, grid, caps, pairs, g, w)
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
    assert rel_err(clear_old, cc.cp_clearance(o, caps, pairs, xs[0], g, w)) < 1e-9
    assert rel_err(clear_new, cc.cp_clearance(o, caps, pairs, xn_ref, g, w)) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [("tree38", 4, 2, None, 1), ("chain6ff", 4, 2, 0, 0)])
@pytest.mark.parametrize("mode", ["no_grid_pair", "zero_weights", "never"])
def test_neutrality(gpu, monkeypatch, name, T, fd_mode, fo_, fwd_path, mode):
    """linearise, both costs, sweep and forward, bit for bit: a capsule context with live pairs of the three older kinds computes
    the same whether or not a grid is resident ("no_grid_pair"); with grid pairs whose weights are all 0, and with non-zero
    weights on grid pairs that nothing comes near (margin -10), a context computes what the flag-off context computes"""
    capi = gpu
    mu, B = 10.0, 2
    grid = sphere_scene()
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    caps = cc.pick_capsules(model)
    if mode == "no_grid_pair":
        pairs = cc.pick_pairs(caps)
        g, w = cc.random_task(o, caps, pairs, xs, B, 33)
        assert cc.check_task(o, caps, pairs, xs, g, w, fractions=False).any()
    else:
        pairs = mixed_pairs(caps)
        g, w, _ = grid_task(o, caps, pairs, xs, B, 33, grid, p_out=0.0)
        monkeypatch.setattr(cc, "pair_eval", grid_eval(grid))
        if mode == "never":
            g[..., 7] = -10.0
            assert np.min([cc.cp_clearance(o, caps, pairs, xs[b], g[b], w[b]) for b in range(B)]) > 5.0
        else:
            w[:] = 0.0
    out = {}
    for on in (False, True):
        flags = capi.FLAG_TRACE | (capi.FLAG_CAPSULE_COST if on or mode == "no_grid_pair" else 0)
        with capi.Context(spec, flags=flags) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if mode == "no_grid_pair":
                if on:
                    ctx.set_obstacle_grid(*grid)
                cc.set_task(ctx, caps, pairs, g, w)
            elif on:
                set_task(ctx, grid, caps, pairs, g, w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
            if on and mode == "never":
                assert 5.0 < np.min(ctx.capsule_clearance(1)) < np.inf
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
def test_neutrality_solve(gpu, monkeypatch):
    """a 3-iteration ddp_hip_solve with non-zero weights on grid pairs that nothing comes near: log and result bit for bit the
    flag-off solve's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 4, 2, 3, 1e-9, 1e2, 1e-1, 10.0
    grid = sphere_scene()
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 101, held=True)
    caps = cc.pick_capsules(model)
    pairs = mixed_pairs(caps)
    g, w, _ = grid_task(o, caps, pairs, xs, B, 102, grid, p_out=0.0)
    g[..., 7] = -10.0
    w[:] = 50.0
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST if on else 0) as ctx:
            _setup(ctx, xs, us)
            if on:
                set_task(ctx, grid, caps, pairs, g, w)
            log = solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
            res[on] = (log, ctx.download("X"), ctx.download("U"))
    assert not np.array_equal(res[True][1], xs)
    assert np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(res[False][0][k]), np.asarray(res[True][0][k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", MODELS)
def test_equivalences(gpu, name, fo_):
    """(a) a degenerate capsule against the grid is an obstacle-flag grid slot with a collision sphere of the same radius, shift
    and margin: costs, LX, LXX, LFX, LFXX and clearances agree to 1e-12.  (b) on a field sampled from a plane n . p - h a grid
    pair is a CAPSULE_VS_HALFSPACE pair with the same n and h + n . s: the deeper end is a sample, and d and derivatives agree
    to 1e-12"""
    capi = gpu
    T, B, mu = 3, 2, 30.0
    model, spec, o = cc.make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 61)
    mults = tc._mults(o, xs[0], 62)
    rng = np.random.default_rng(63)
    caps = cc.pick_capsules(model)
    grid = sphere_scene()
    phi, origin, cell = grid
    lo, hi = extent(grid)

    def run(flags, prepare, clearance):
        with capi.Context(spec, flags=flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            prepare(ctx)
            ctx.linearize(capi.LIN_COST)
            r = {s: ctx.download(s) for s in ("LX", "LXX", "LFX", "LFXX")}
            ctx.cost_seq_aug(0, mu)
            r["COSTS_OLD"] = ctx.download("COSTS_OLD")
            r["clear"] = clearance(ctx)
            return r

    def agree(a, b, off):
        for s in ("LX", "LXX", "LFX", "LFXX", "COSTS_OLD"):
            assert not np.array_equal(a[s], off[s]), s                 # the term is there
            e = rel_err(a[s], b[s])
            print("equivalence", name, s, e)
            assert e <= TOL, (s, e)
        assert np.all(np.isfinite(a["clear"])) and np.min(a["clear"]) < 0
        assert np.max(np.abs(a["clear"] - b["clear"]) / np.maximum(1.0, np.abs(b["clear"]))) <= TOL
    off = run(0, lambda ctx: None, lambda ctx: None)
    # (a) the sphere of the sibling's capsules (end0 == end1), radius and all
    k = next(i for i, c in enumerate(caps) if c[1] == c[2])
    j, e0, _, r = caps[k]
    assert r > 0
    gc, go = np.zeros((B, T + 1, 1, 8)), np.zeros((B, T + 1, 1, 4))
    wgt = rng.uniform(0.5, 5.0, size=(B, T + 1, 1))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            p = o.frame_position(j, e0, X[t][:o.nq])
            x = lo + rng.uniform(0.1, 0.9, 3) * (hi - lo)
            s = p - x
            m = og.lookup(phi, origin, cell, p - s)[0] - r + rng.uniform(0.01, 0.1)      # penetrates by 1 .. 10 cm
            gc[b, t, 0, :3], gc[b, t, 0, 3:7], gc[b, t, 0, 7] = s, rng.normal(size=4), m
            go[b, t, 0, :3], go[b, t, 0, 3] = s, m

    def as_capsule(ctx):
        set_task(ctx, grid, [caps[k]], [(0, GRID, 0)], gc, wgt)

    def as_sphere(ctx):
        ctx.set_obstacle_grid(*grid)
        oc.set_task(ctx, [(j, e0, r)], (og.GRID,), go, wgt)
    agree(run(capi.FLAG_CAPSULE_COST, as_capsule, lambda ctx: ctx.capsule_clearance(0)),
          run(capi.FLAG_OBSTACLE_COST, as_sphere, lambda ctx: ctx.obstacle_clearance(0)), off)
    # (b) the plane: four capsules against it
    n, h = cc._unit(rng), 0.17
    plane = plane_scene(n, h)
    segs = [c for c in caps if c[1] != c[2]]
    pairs_g, pairs_h = [(a, GRID, 0) for a in range(len(segs))], [(a, HALF, 0) for a in range(len(segs))]
    gg, gh = np.zeros((B, T + 1, len(segs), 8)), np.zeros((B, T + 1, len(segs), 8))
    wgt = rng.uniform(0.5, 5.0, size=(B, T + 1, len(segs)))
    nmin = 99
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            E = cc.ends(o, segs, X[t][:o.nq])
            for a in range(len(segs)):
                nmin = min(nmin, intervals(segs[a][1], segs[a][2], cell))
                mid = 0.5 * (E[a][0] + E[a][1])
                s = mid - (lo + rng.uniform(0.45, 0.55, 3) * (hi - lo))          # the capsule stays inside the grid
                hs = h + cc._dot(n, s)
                d0 = min(cc._dot(n, E[a][0]), cc._dot(n, E[a][1])) - hs - segs[a][3]
                m = d0 + rng.uniform(0.01, 0.1)
                assert abs(cc._dot(n, E[a][0]) - cc._dot(n, E[a][1])) > 1e-6
                gg[b, t, a, :3], gg[b, t, a, 7] = s, m
                gh[b, t, a, :3], gh[b, t, a, 3], gh[b, t, a, 7] = n, hs, m
    assert nmin >= 2
    agree(run(capi.FLAG_CAPSULE_COST, lambda ctx: set_task(ctx, plane, segs, pairs_g, gg, wgt), lambda ctx: ctx.capsule_clearance(0)),
          run(capi.FLAG_CAPSULE_COST, lambda ctx: cc.set_task(ctx, segs, pairs_h, gh, wgt), lambda ctx: ctx.capsule_clearance(0)), off)


@pytest.mark.gpu
def test_refusals(gpu, monkeypatch):
    """kind 3 before a grid: E_ARG; the grid calls on a capsule-only context succeed; a non-finite geom entry, an ignored one
    included: E_ARG with nothing written; n_intervals out of range in the query: E_ARG; a grid of another cell size changes the
    sample count without a second set_pairs: query, cost and clearance agree with the restatement after the replacement"""
    capi = gpu
    T, B, mu = 3, 2, 30.0
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 71)
    caps = cc.pick_capsules(model)
    pairs = [(0, GRID, 0), (1, HALF, 0), (2, GRID, 0), (3, GRID, 0)]
    grid = sphere_scene()
    occ = og.scene()[0]
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:                   # neither flag
        assert code(capi, lambda: ctx.obstacle_grid_segment_query(np.zeros((1, 6)), 1)) == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        assert code(capi, lambda: ctx.set_capsule_pairs(capsules=caps, pairs=pairs)) == capi.E_ARG
        assert code(capi, lambda: ctx.obstacle_grid_segment_query(np.zeros((1, 6)), 1)) == capi.E_ARG
        assert code(capi, lambda: ctx.obstacle_grid()) == capi.E_ARG
        ctx.set_obstacle_occupancy(occ, og.scene()[1][1], og.scene()[1][2])         # the grid calls on a capsule-only context
        assert np.array_equal(ctx.obstacle_grid()[0], og.scene()[1][0])
        ctx.set_obstacle_grid(*grid)
        got = ctx.obstacle_grid()
        assert np.array_equal(got[0], grid[0]) and np.array_equal(got[1], grid[1]) and got[2] == grid[2]
        assert ctx.obstacle_grid_query(grid[1][None, :], grad=False)[0] == grid[0][0, 0, 0]
        ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
        assert code(capi, lambda: ctx.set_capsule_pairs(capsules=caps, pairs=pairs + [(0, 4, 0)])) == capi.E_ARG
        for bad in (-1, MAXN + 1):
            assert code(capi, lambda: ctx.obstacle_grid_segment_query(np.zeros((2, 6)), np.array([1, bad]))) == capi.E_ARG
        assert len(ctx.obstacle_grid_segment_query(np.zeros((0, 6)), 1)[0]) == 0
        g, w, share = grid_task(o, caps, pairs, xs, B, 72, grid, p_out=0.0)
        ctx.set_capsule_cost(geom=g, weight=w)
        for e in range(8):
            for bad in (np.nan, np.inf):
                gb = g.copy()
                gb[1, 2, 2, e] = bad
                assert code(capi, lambda: ctx.set_capsule_cost(geom=gb)) == capi.E_ARG, (e, bad)
        assert np.array_equal(ctx.capsule_cost()[0], g) and np.array_equal(ctx.capsule_cost()[1], w)
        # another cell size: other sample counts, the pairs as they are
        for cell in (0.05, 0.02, 0.11):
            grid2 = sphere_scene(cell=cell, origin=tuple(grid[1] + 0.5 * (np.array(grid[0].shape) - 1) * (grid[2] - cell)))
            counts = [intervals(c[1], c[2], cell) for c in caps]
            ctx.set_obstacle_grid(*grid2)
            monkeypatch.setattr(cc, "pair_eval", grid_eval(grid2))
            ctx.cost_seq_aug(0, mu)
            on = ctx.download("COSTS_OLD")
            ctx.set_capsule_cost(weight=np.zeros_like(w))
            ctx.cost_seq_aug(0, mu)
            off = ctx.download("COSTS_OLD")
            ctx.set_capsule_cost(weight=w)
            clear = ctx.capsule_clearance(0)
            n_ex = n_all = 0
            for b in range(B):
                X = xs[b].reshape(T + 1, o.nx)
                add = cc.cp_terms(o, caps, pairs, xs[b], g[b], w[b])
                assert rel_err(on[b], off[b] + add) <= TOL, (cell, b)
                ex = cc.cp_clearance(o, caps, pairs, xs[b], g[b], w[b])
                assert np.max(np.abs(clear[b] - ex) / np.maximum(1.0, np.abs(ex))) <= TOL
                for t in range(T + 1):
                    E = cc.ends(o, caps, X[t][:o.nq])
                    seg = np.array([np.concatenate([E[p[0]][0] - g[b, t, i, :3], E[p[0]][1] - g[b, t, i, :3]]) for i, p in enumerate(pairs)])
                    phi, j, pt, gr = ctx.obstacle_grid_segment_query(seg, [counts[p[0]] for p in pairs])
                    for i, p in enumerate(pairs):
                        r = segment_rule(grid2, seg[i, :3], seg[i, 3:], np.zeros(3), counts[p[0]])
                        n_all += 1
                        if r["gap"] < GAP:
                            n_ex += 1
                            continue
                        assert j[i] == r["j"] and (r["j"] < 0 or abs(phi[i] - r["phi"]) <= TOL), (cell, b, t, i)
            assert n_ex <= 0.05 * n_all, (n_ex, n_all)
        assert sorted({intervals(caps[0][1], caps[0][2], c) for c in (0.05, 0.02, 0.11)}) != [intervals(caps[0][1], caps[0][2], 0.05)]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 2])
def test_advance_shifts_rows(gpu, shift):
    """ddp_hip_advance: a grid pair's geometry and weights move like the others' (rows 0 .. T-1 by the hold rule, row T
    untouched), and the grid is what it was, bit for bit"""
    capi = gpu
    T, B = 3, 2
    grid = sphere_scene()
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    xs, us = _trajs(o, model, B, 181)
    caps = cc.pick_capsules(model)
    pairs = mixed_pairs(caps)
    g, w, _ = grid_task(o, caps, pairs, xs, B, 182, grid)
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as ctx:
        _setup(ctx, xs, us)
        set_task(ctx, grid, caps, pairs, g, w)
        before = ctx.obstacle_grid()
        ctx.advance(shift, None, capi.ADVANCE_NO_ROLL)
        g1, w1 = ctx.capsule_cost()
        after = ctx.obstacle_grid()
        seg = np.concatenate([grid[1] + grid[2] * np.array([3.25, 2.5, 4.75]), grid[1] + grid[2] * np.array([5.5, 6.25, 1.5])])[None, :]
        phi, j, pt, gr = ctx.obstacle_grid_segment_query(seg, 6)
    assert np.array_equal(g1, adv.np_advance(g, shift, terminal=True)) and np.array_equal(w1, adv.np_advance(w, shift, terminal=True))
    assert np.array_equal(g1[:, T], g[:, T]) and np.array_equal(g1[:, 0], g[:, shift]) and not np.array_equal(g1, g)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    r = segment_rule(grid, seg[0, :3], seg[0, 3:], np.zeros(3), 6)
    assert j[0] == r["j"] and abs(phi[0] - r["phi"]) <= TOL


def _shelf(o, joint, e0, e1, radius, q, cell=0.02, n=24):
    """an occupied 3 x 3 x 3 block beside the middle of the limb (e0 .. e1 of `joint`) at q, in a grid of n^3 nodes around it:
    the nearest placement, among offsets of 4 .. 8 cm across the limb, at which the capsule penetrates by 3 .. 8 mm at a middle
    sample while spheres of the same radius at the two ends stay clear.  On the yardstick alone"""
    a0, a1 = o.frame_position(joint, e0, q), o.frame_position(joint, e1, q)
    mid, axis = 0.5 * (a0 + a1), (a1 - a0) / np.linalg.norm(a1 - a0)
    across = np.cross(axis, [0.0, 0.0, 1.0] if abs(axis[2]) < 0.9 else [1.0, 0.0, 0.0])
    across /= np.linalg.norm(across)
    N = intervals(e0, e1, cell)
    occ = np.zeros((n, n, n), bool)
    occ[tuple(slice(n // 2 - 1, n // 2 + 2) for _ in range(3))] = True
    phi = og.signed_field(occ, cell)
    for delta in np.linspace(0.04, 0.08, 41):
        grid = (phi, mid + delta * across - cell * (n // 2), cell)     # the block's middle voxel at mid + delta across
        r = segment_rule(grid, a0, a1, np.zeros(3), N)
        ends_clear = min(og.lookup(*grid, a0)[0], og.lookup(*grid, a1)[0]) - radius
        if -0.008 <= r["phi"] - radius <= -0.003 and 0 < r["j"] < N and ends_clear > 0.02 and stable(r):
            return occ, grid, r["phi"] - radius
    raise AssertionError("no placement")


@pytest.mark.gpu
def test_forearm_clears_the_shelf(gpu):
    """tree38, T = 6: a 30 cm capsule on a leaf joint, and an occupied block beside its middle at the held posture, so that spheres
    at the two ends keep positive clearance while a middle sample penetrates by some millimetres.  The pair is weighted at the
    horizon's end.  After the solve the capsule's clearance there is greater than before and greater than -1 mm.  The same task
    with the two end spheres alone on the obstacle flag leaves the mid-limb penetration in place: the segment query on its
    result says so"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, iters, thr, mu, w_, n_ = 6, 12, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make("tree38", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 201, held=True)
    joint = oc.pick_points(model)[3][0]
    e0, e1, radius = (0.0, 0.0, 0.0), (0.0, 0.3, 0.0), 0.03
    qT = xs[0].reshape(T + 1, o.nx)[T][:o.nq]
    occ, grid, pen = _shelf(o, joint, e0, e1, radius, qT)
    N = intervals(e0, e1, grid[2])
    assert N == 15
    wt = np.zeros((T + 1, 1)); wt[T] = 1e6

    def limb(x):
        q = x.reshape(T + 1, o.nx)[T][:o.nq]
        return np.concatenate([o.frame_position(joint, e0, q), o.frame_position(joint, e1, q)])[None, :]
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as ctx:
        _setup(ctx, xs, us)
        ctx.set_obstacle_occupancy(occ, grid[1], grid[2])
        cc.set_task(ctx, [(joint, e0, e1, radius)], [(0, GRID, 0)], np.zeros((1, 8)), wt)
        before = ctx.capsule_clearance(0)[0]
        assert np.all(before[:T] == np.inf) and abs(before[T] - pen) <= 1e-9
        solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
        after = ctx.capsule_clearance(0)[0][T]
        x_cap = ctx.download("X")[0]
        seen = ctx.obstacle_grid_segment_query(limb(x_cap), N)[0][0] - radius
    print("shelf", "capsule before", before[T], "after", after)
    assert abs(seen - after) <= 1e-12
    assert after > before[T] and after > -1e-3, (before[T], after)
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        _setup(ctx, xs, us)
        ctx.set_obstacle_occupancy(occ, grid[1], grid[2])
        ctx.set_obstacle_points(points=[(joint, e0, radius), (joint, e1, radius)], kinds=[og.GRID])
        ctx.set_obstacle_cost(geom=np.zeros((1, 4)), weight=wt)
        ends_before = ctx.obstacle_clearance(0)[0][T]
        assert ends_before > 0.02                                       # the end spheres are clear: the obstacle flag sees nothing
        solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
        mid = ctx.obstacle_grid_segment_query(limb(ctx.download("X")[0]), N)[0][0] - radius
    print("shelf", "end spheres alone: mid-limb", mid)
    assert mid < 0.5 * pen, (mid, pen)                                  # (pen < 0: at least half the penetration is still there)
