"""Voxel-grid obstacles (DDP_HIP_OBSTACLE_GRID, include/ddp_hip/ddp_hip.h): an obstacle slot whose distance is read from a signed
distance field on a grid resident in the context, and the field built on the device from occupancy voxels,

    phi(v) = +cell (sqrt(D_occ(v)) - 0.5) for a free v,   -cell (sqrt(D_free(v)) - 0.5) for an occupied v
    s = (p_k - shift - origin) / cell,  i = min(floor(s), n - 2),  f = s - i,  phi(p), grad phi(p) trilinear over the 8 corners
    d_ko = phi(p_k) - r_k - margin,   u_ko = grad phi(p_k);   outside the grid d = +inf

The yardstick is numpy, written here: the brute-force nearest-voxel search for the field (signed_field) and the formula above for
the lookup (lookup).  Everything after d and u is the sibling's text, so the sibling's helpers (test_obstacle_cost.py: ob_terms,
ob_clearance, ob_grad_hess / ob_derivs, check_task, _emulate_forward) are used by import: they learn a pair's d and u from the
module's `pair`, which the tests here replace by one that knows the third kind (grid_pair).  Values, clearances and derivatives
are held to the figure the sibling holds the sphere and half-space kinds to, 1e-12 (it has no name there); the field to 4 ulp of
max(|phi|, cell): the squared distances are exact, so only one square root, one subtraction and one product round."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import test_advance as adv
import test_frame_cost as fc
import test_obstacle_cost as oc
import test_tracking_cost as tc
from problems import make
from synth import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPHERE, HALFSPACE, GRID = oc.SPHERE, oc.HALFSPACE, 2
TOL = 1e-12                  # what test_obstacle_cost.py holds values, clearances and derivatives to
DERIVS = oc.DERIVS
KINDS = (SPHERE, GRID, HALFSPACE, GRID)
_trajs, _setup = tc._trajs, tc._setup
_SIBLING_PAIR = oc.pair


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def sq_dist_to(mask, cap):
    """the least squared index distance from every voxel to a voxel where mask is True, by brute force; cap where there is none"""
    idx = np.argwhere(mask)
    out = np.full(mask.shape, float(cap))
    if len(idx) == 0:
        return out
    g = np.stack(np.meshgrid(*[np.arange(n) for n in mask.shape], indexing="ij"), -1).reshape(-1, 3)
    for lo in range(0, len(g), 4096):
        d = ((g[lo:lo + 4096, None, :] - idx[None, :, :]) ** 2).sum(-1).min(1)
        out.reshape(-1)[lo:lo + 4096] = d
    return out


def signed_field(occ, cell):
    occ = np.asarray(occ) != 0
    cap = sum(n * n for n in occ.shape)
    d_occ, d_free = sq_dist_to(occ, cap), sq_dist_to(~occ, cap)
    return np.where(occ, -cell * (np.sqrt(d_free) - 0.5), cell * (np.sqrt(d_occ) - 0.5))


def lookup(phi, origin, cell, p):
    """(phi(p), grad phi(p)) by the header's formula; (+inf, None) outside"""
    n = np.array(phi.shape)
    s = (np.asarray(p, dtype=float) - origin) / cell
    if not np.all((s >= 0) & (s <= n - 1)):
        return np.inf, None
    i = np.minimum(np.floor(s).astype(int), n - 2)
    f = s - i
    c = phi[i[0]:i[0] + 2, i[1]:i[1] + 2, i[2]:i[2] + 2]
    wx, wy, wz = (np.array([1 - f[a], f[a]]) for a in range(3))
    sg = np.array([-1.0, 1.0])
    val = np.einsum("abc,a,b,c", c, wx, wy, wz)
    g = np.array([np.einsum("abc,a,b,c", c, sg, wy, wz), np.einsum("abc,a,b,c", c, wx, sg, wz), np.einsum("abc,a,b,c", c, wx, wy, sg)]) / cell
    return float(val), g


def grid_pair(grid):
    """the sibling's pair(kind, g, p, r) with the third kind: g = (shift, margin), grid = (phi, origin, cell)"""
    phi, origin, cell = grid

    def pair(kind, g, p, r):
        if kind != GRID:
            return _SIBLING_PAIR(kind, g, p, r)
        val, grad = lookup(phi, origin, cell, np.asarray(p) - g[:3])
        if grad is None:
            return np.inf, None
        return val - r - g[3], (grad if np.any(grad != 0.0) else None)
    return pair


@functools.lru_cache(maxsize=None)
def scene(seed=0, shape=(7, 5, 9), p=0.15, cell=0.1, origin=(-0.1, 0.2, 0.0)):
    """(occ, (phi, origin, cell)): random occupancy and its field, computed once"""
    occ = np.random.default_rng(seed).uniform(size=shape) < p
    phi = signed_field(occ, cell)
    phi.setflags(write=False)
    return occ, (phi, np.array(origin, dtype=float), cell)


def grid_task(o, pts, kinds, xs, B, seed, grid):
    """geom (B, T+1, n_obs, 4) and weights (B, T+1, n_obs).  The sphere and half-space slots by the sibling's generator.  A grid
    slot, per (instance, t): the shift brings a chosen point to a random place inside the grid, f in [0.2, 0.8] on every axis, and
    the margin makes it penetrate by 0.01 .. 0.1 or stay clear by as much (the first grid slot: active at t = 0, clear at t = 1);
    the other points fall where they fall, many of them outside"""
    phi, origin, cell = grid
    rng = np.random.default_rng(seed)
    plain = tuple(SPHERE if k == GRID else k for k in kinds)
    geom, w = oc.random_task(o, pts, plain, xs, B, seed + 1)
    first = kinds.index(GRID)
    for b in range(B):
        X = xs[b].reshape(o.T + 1, o.nx)
        for t in range(o.T + 1):
            P = oc.positions(o, pts, X[t][:o.nq])
            for s_, kind in enumerate(kinds):
                if kind != GRID:
                    continue
                k = int(rng.integers(len(pts)))
                i = np.array([rng.integers(0, n - 1) for n in phi.shape])
                x = origin + cell * (i + rng.uniform(0.2, 0.8, 3))
                inside = rng.uniform() < 0.5
                if s_ == first and t < 2:
                    inside = t == 0
                sd = rng.uniform(0.01, 0.1) * (-1.0 if inside else 1.0)
                geom[b, t, s_, :3] = P[k] - x
                geom[b, t, s_, 3] = lookup(phi, origin, cell, P[k] - geom[b, t, s_, :3])[0] - pts[k][2] - sd
    return geom, w


def grid_pairs(o, pts, kinds, xs, geom, w, grid):
    """of one instance: the numbers of live grid pairs that are active, clear (inside, d > 0) and outside, and the least distance
    of an inside point's f to a cell boundary (the interpolant's gradient jumps there)"""
    phi, origin, cell = grid
    pair = grid_pair(grid)
    X = xs.reshape(o.T + 1, o.nx)
    n_act = n_clear = n_out = 0
    edge = np.inf
    for t in range(o.T + 1):
        for k, p in enumerate(oc.positions(o, pts, X[t][:o.nq])):
            for s_, kind in enumerate(kinds):
                if kind != GRID or w[t][s_] == 0.0:
                    continue
                d, _ = pair(kind, geom[t][s_], p, pts[k][2])
                if d == np.inf:
                    n_out += 1
                    continue
                s = (p - geom[t][s_][:3] - origin) / cell
                f = s - np.floor(s)
                edge = min(edge, float(np.min(np.minimum(f, 1.0 - f))))
                n_act += d < 0
                n_clear += d > 0
    return n_act, n_clear, n_out, edge


def check_grid_task(o, pts, kinds, xs, geom, w, grid, need=True):
    """the conditions on the inputs, on the yardstick alone (oc.pair is grid_pair(grid) here): the sibling's (no live pair within
    1e-6 of the surface) and, with `need`, in every instance at least one active and one clear grid pair and one point outside
    the grid; no inside point within 1e-9 of a cell boundary.  Returns the blocks' activity"""
    active = oc.check_task(o, pts, kinds, xs, geom, w, fractions=False)
    for b in range(xs.shape[0]):
        n_act, n_clear, n_out, edge = grid_pairs(o, pts, kinds, xs[b], geom[b], w[b], grid)
        assert edge > 1e-9, (b, edge)
        if need:
            assert n_act >= 1 and n_clear >= 1 and n_out >= 1, (b, n_act, n_clear, n_out)
    return active


def set_task(ctx, grid, pts, kinds, geom=None, weight=None):
    ctx.set_obstacle_grid(*grid)
    oc.set_task(ctx, pts, kinds, geom, weight)


def ulp_ok(got, ex, cell):
    return np.all(np.abs(got - ex) <= 4.0 * np.spacing(np.maximum(np.abs(ex), cell)))


# ---- CPU -------------------------------------------------------------------------------------------------------------------
W5 = oc.W5


def test_yardstick_field_against_scipy():
    """the brute force agrees exactly, on the seeded random 7 x 5 x 9 grid, with scipy's exact Euclidean transform, recorded in
    tests/golden/obstacle_grid/edt_scipy_7x5x9.npz (scipy.ndimage.distance_transform_edt of the occupancy and of its complement, scipy
    1.15.3; the occupancy is stored beside them, so a drift of the seeded scene shows as well).  No scipy is needed to run this"""
    occ, (phi, _, cell) = scene()
    assert 0 < occ.sum() < occ.size
    gold = np.load(os.path.join(ROOT, "tests", "golden", "obstacle_grid", "edt_scipy_7x5x9.npz"))
    assert np.array_equal(gold["occ"] != 0, occ)
    ref = np.where(occ, -cell * (gold["edt_of_occupied"] - 0.5), cell * (gold["edt_of_free"] - 0.5))
    assert np.array_equal(phi, ref)
    cap = sum(n * n for n in occ.shape)
    assert np.array_equal(sq_dist_to(occ, cap)[~occ], np.rint(gold["edt_of_free"][~occ] ** 2))    # the squared distances: integers
    assert np.array_equal(sq_dist_to(~occ, cap)[occ], np.rint(gold["edt_of_occupied"][occ] ** 2))


def test_yardstick_field_without_sources():
    """an all-free and an all-occupied grid stay finite: cap = nx^2 + ny^2 + nz^2 stands in"""
    assert signed_field(np.zeros((2, 3, 4), bool), 0.1).max() == 0.1 * (np.sqrt(29.0) - 0.5)
    assert signed_field(np.ones((2, 3, 4), bool), 0.1).min() == -0.1 * (np.sqrt(29.0) - 0.5)
    assert np.all(signed_field(np.zeros((2, 3, 4), bool), 0.1) == 0.1 * (np.sqrt(29.0) - 0.5))


def test_yardstick_gradient():
    """the lookup's gradient against a 5-point central difference of its value, to 5e-13 at 200 points with f in [0.2, 0.8];
    nodes exactly; outside +inf"""
    _, (phi, origin, cell) = scene()
    rng = np.random.default_rng(1)
    h = 1e-3 * cell
    worst = 0.0
    for _ in range(200):
        i = np.array([rng.integers(0, n - 1) for n in phi.shape])
        p = origin + cell * (i + rng.uniform(0.2, 0.8, 3))
        v, g = lookup(phi, origin, cell, p)
        fd = np.array([sum(cw * lookup(phi, origin, cell, p + s * h * e)[0] for s, cw in W5) / h for e in np.eye(3)])
        worst = max(worst, np.max(np.abs(fd - g)) / max(1.0, np.max(np.abs(g))))
    assert worst <= 5e-13, worst
    o0 = np.zeros(3)
    assert lookup(phi, o0, 0.25, 0.25 * np.array([6, 4, 8]))[0] == phi[6, 4, 8] and lookup(phi, o0, 0.25, 0.25 * np.array([2, 3, 5]))[0] == phi[2, 3, 5]
    assert lookup(phi, origin, cell, origin - 1e-9)[0] == np.inf


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.OBSTACLE_GRID == 2 and re.search(r"#define\s+DDP_HIP_OBSTACLE_GRID\s+2\b", header)
    assert capi.MAX_GRID_DIM == 256 and re.search(r"#define\s+DDP_HIP_MAX_GRID_DIM\s+256\b", header)
    assert capi.MAX_OBSTACLES == 8 and capi.FLAG_OBSTACLE_COST == 512
    L = capi.lib()
    for name in ("ddp_hip_obstacle_set_grid", "ddp_hip_obstacle_set_occupancy", "ddp_hip_obstacle_grid_download", "ddp_hip_obstacle_grid_query"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    for name in ("set_obstacle_grid", "set_obstacle_occupancy", "obstacle_grid", "obstacle_grid_query"):
        assert hasattr(capi.Context, name), name
    assert "shift" in capi.Context.set_obstacle_cost.__doc__ and "margin" in capi.Context.set_obstacle_cost.__doc__
    # shapes are checked before anything reaches the library: a context object without a device will do
    ctx = capi.Context.__new__(capi.Context)
    ctx._h = None
    o3 = np.zeros(3)
    for fn in (ctx.set_obstacle_grid, ctx.set_obstacle_occupancy):
        for args in ((np.zeros((3, 4)), o3, 0.1), (np.zeros(24), o3, 0.1), (np.zeros((2, 3, 4, 1)), o3, 0.1), (np.zeros((2, 3, 4)), np.zeros(2), 0.1),
                     (np.zeros((2, 3, 4)), np.zeros((3, 1)), 0.1), (np.zeros((2, 3, 4)), o3, np.full(3, 0.1)), (0.0, o3, 0.1)):
            with pytest.raises(ValueError):
                fn(*args)
    for pts in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 3, 1)), 0.0):
        with pytest.raises(ValueError):
            ctx.obstacle_grid_query(pts)


def test_obstacle_grid_block_host_logic():
    """host/test_obstacle_grid_block.cpp: the library's lookup, compiled for the host, against values worked out by hand on a
    2 x 2 x 2 and a 3 x 2 x 4 grid, the inside test at both ends of each axis, and cost_obstacle_geom_side with the new kind"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_obstacle_grid_block"])
    out = subprocess.run([os.path.join(host, "test_obstacle_grid_block")], capture_output=True, text=True)
    assert out.returncode == 0 and "obstacle grid block ok" in out.stdout, out.stdout + out.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _grid_ctx(capi, T=1, batch=1):
    model, spec, o = make("chain6", T, batch=batch, fd_mode=0)
    return capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS)


def _occupancy(case):
    rng = np.random.default_rng(7)
    if case == "random":
        return scene()[0]
    if case == "corner":
        occ = np.zeros((7, 5, 9), bool); occ[6, 0, 8] = True
    elif case == "all_free":
        occ = np.zeros((7, 5, 9), bool)
    elif case == "all_occupied":
        occ = np.ones((7, 5, 9), bool)
    elif case == "cube2":
        occ = np.zeros((2, 2, 2), bool); occ[1, 0, 1] = True
    elif case.startswith("slab"):
        occ = np.zeros((7, 5, 9), bool)
        occ[tuple(slice(2, 3) if a == int(case[-1]) else slice(None) for a in range(3))] = True
    else:
        occ = rng.uniform(size={"long_x": (256, 2, 3), "long_y": (2, 256, 3), "long_z": (3, 2, 256)}[case]) < 0.02
    return occ


FIELD_CASES = ["random", "corner", "all_free", "all_occupied", "cube2", "slab0", "slab1", "slab2", "long_x", "long_y", "long_z"]


@pytest.mark.gpu
def test_field_from_occupancy(gpu):
    """set_occupancy then obstacle_grid() against the brute force, to 4 ulp of max(|phi|, cell), one context through every case
    (each call replaces the grid of the one before, of another shape): 15 % random, one corner voxel, all free, all occupied,
    2 x 2 x 2 with one occupied, a one-voxel slab normal to each axis, and the longest line (256) on each of the three passes"""
    capi = gpu
    origin, cell = np.array([0.3, -0.2, 0.1]), 0.05
    with _grid_ctx(capi) as ctx:
        for case in FIELD_CASES:
            occ = _occupancy(case)
            if case.startswith("long"):
                assert 0 < occ.sum() < occ.size and max(occ.shape) == 256
            ex = signed_field(occ, cell)
            ctx.set_obstacle_occupancy(occ.astype(np.uint8) * 3, origin, cell)          # (any non-zero value is occupied)
            phi, o_, c_ = ctx.obstacle_grid()
            assert phi.shape == occ.shape and np.array_equal(o_, origin) and c_ == cell, case
            assert np.all(np.isfinite(phi)), case
            err = np.max(np.abs(phi - ex) / np.spacing(np.maximum(np.abs(ex), cell)))
            print("field", case, occ.shape, "occupied", int(occ.sum()), "worst ulp", err)
            assert ulp_ok(phi, ex, cell), (case, err)
            assert np.array_equal(phi < 0, occ), case


@pytest.mark.gpu
def test_query(gpu):
    """ddp_hip_obstacle_grid_query: 200 inside points, value and gradient, against the lookup; points outside on each side of
    each axis give +inf and a zero gradient; with origin 0 and cell 0.25 the nodes return the node values exactly; set_grid
    round-trips the field bit for bit"""
    capi = gpu
    _, (phi, origin, cell) = scene()
    rng = np.random.default_rng(3)
    n = np.array(phi.shape)
    pts = origin + cell * (np.stack([rng.integers(0, k - 1, size=200) for k in phi.shape], 1) + rng.uniform(0.0, 1.0, size=(200, 3)))
    with _grid_ctx(capi) as ctx:
        ctx.set_obstacle_grid(phi, origin, cell)
        got_phi, o_, c_ = ctx.obstacle_grid()
        assert np.array_equal(got_phi, phi) and np.array_equal(o_, origin) and c_ == cell
        val, grad = ctx.obstacle_grid_query(pts)
        ex = [lookup(phi, origin, cell, p) for p in pts]
        ev, eg = np.array([e[0] for e in ex]), np.array([e[1] for e in ex])
        print("query", rel_err(val, ev), rel_err(grad, eg))
        assert rel_err(val, ev) <= TOL and rel_err(grad, eg) <= TOL
        assert np.array_equal(ctx.obstacle_grid_query(pts, grad=False), val)
        mid = origin + cell * (n - 1) / 2.0
        out = []
        for a in range(3):
            for x in (origin[a] - 1e-9, origin[a] + cell * (n[a] - 1) + 1e-9, -50.0, 50.0):
                p = mid.copy(); p[a] = x
                out.append(p)
        val, grad = ctx.obstacle_grid_query(np.array(out))
        assert np.all(val == np.inf) and np.all(grad == 0.0)
        ctx.set_obstacle_grid(phi, np.zeros(3), 0.25)                              # (exact node positions: the end nodes are inside)
        nodes = np.stack(np.meshgrid(*[np.arange(k) for k in phi.shape], indexing="ij"), -1).reshape(-1, 3)
        val = ctx.obstacle_grid_query(0.25 * nodes, grad=False)
        assert np.array_equal(val.reshape(phi.shape), phi)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("chain6", None), ("chain6ff", 0), ("tree38", None)])
def test_values_and_clearance(gpu, monkeypatch, name, fo_):
    """COSTS_OLD / COSTS_NEW against the flag-off context's plus the numpy terms, and ddp_hip_obstacle_clearance along X and
    X_NEW, slots (SPHERE, GRID, HALFSPACE, GRID) with per-instance, per-t shifts and margins.  The yardstick finds in every
    instance an active and a clear grid pair and a point outside the grid, or the test fails"""
    capi = gpu
    T, B, mu = 3, 2, 30.0
    _, grid = scene()
    monkeypatch.setattr(oc, "pair", grid_pair(grid))
    model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    pts = oc.pick_points(model)
    geom, w = grid_task(o, pts, KINDS, xs, B, 52, grid)
    w[1, 2, 1] = 0.0
    active = check_grid_task(o, pts, KINDS, xs, geom, w, grid)
    active2 = check_grid_task(o, pts, KINDS, xs2, geom, w, grid, need=False)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (capi.FLAG_OBSTACLE_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                set_task(ctx, grid, pts, KINDS, geom, w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
            if on:
                clear = {0: ctx.obstacle_clearance(0), 1: ctx.obstacle_clearance(1)}
    for which, X, act in ((0, xs, active), (1, xs2, active2)):
        for b in range(B):
            add = oc.ob_terms(o, pts, KINDS, X[b], geom[b], w[b])
            ex = got[False][which][b] + add
            assert np.array_equal(add != 0.0, act[b]) and (which == 1 or np.any(add != 0.0))
            e = rel_err(got[True][which][b], ex)
            print("cost_seq_aug", name, which, b, e)
            assert e <= TOL, (which, b, e)
            assert np.array_equal(got[True][which][b][~act[b]], got[False][which][b][~act[b]])
            exc = oc.ob_clearance(o, pts, KINDS, X[b], geom[b], w[b])
            fin = np.isfinite(exc)
            assert np.array_equal(np.isinf(clear[which][b]), ~fin)
            ec = np.max(np.abs(clear[which][b][fin] - exc[fin]) / np.maximum(1.0, np.abs(exc[fin])))
            print("clearance", name, which, b, ec)
            assert ec <= TOL, (which, b, ec)
    # the grid slots alone: a block all of whose points are outside the grid has no clearance to report
    wg = w.copy(); wg[:, :, [0, 2]] = 0.0
    gfar = geom.copy(); gfar[0, 1, [1, 3], :3] += 10.0                           # one block sees the scene 10 m away
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | capi.FLAG_OBSTACLE_COST) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, grid, pts, KINDS, gfar, wg)
        got_c = ctx.obstacle_clearance(0)
    exc = np.stack([oc.ob_clearance(o, pts, KINDS, xs[b], gfar[b], wg[b]) for b in range(B)])
    assert np.array_equal(np.isinf(got_c), np.isinf(exc)) and got_c[0, 1] == np.inf
    fin = np.isfinite(exc)
    assert np.max(np.abs(got_c[fin] - exc[fin]) / np.maximum(1.0, np.abs(exc[fin]))) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", [("chain6", 2, None), ("chain6ff", 2, 0), ("tree38", 2, None)])
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, monkeypatch, name, fd_mode, fo_, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms (the sibling's point jacobians, the lookup's d
    and u), through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU, LUU, LUX,
    every velocity row and column and the q rows off the active points' paths bit for bit the flag-off values"""
    capi = gpu
    T, B = 3, 2
    _, grid = scene()
    monkeypatch.setattr(oc, "pair", grid_pair(grid))
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    pts = oc.pick_points(model)
    geom, w = grid_task(o, pts, KINDS, xs, B, 43, grid)
    w[1, 2, 3] = 0.0; w[0, T, 0] = 0.0
    active = check_grid_task(o, pts, KINDS, xs, geom, w, grid)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST if on else 0) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if on:
                set_task(ctx, grid, pts, KINDS, geom, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = oc.ob_derivs(o, model, pts, KINDS, xs[b], geom[b], w[b])
        only = oc.ob_derivs(o, model, pts, KINDS, xs[b], geom[b], np.where(np.array(KINDS) == GRID, w[b], 0.0))
        assert np.max(np.abs(only["LX"])) > 0 and np.max(np.abs(only["LXX"])) > 0           # the grid slots take part
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            e = rel_err(got[True][s][b], ex)
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
            if active[b, t]:
                assert not np.array_equal(blk, off) and not np.array_equal(gon, goff)
            else:
                assert np.array_equal(blk, off) and np.array_equal(gon, goff)
    print("linearize", name, stages, "worst", worst, "active blocks", int(active.sum()), "of", active.size)


def block_scene(cell):
    """7 x 5 x 9 nodes, a 3 x 3 x 3 block of occupied voxels in the middle; returns (occ, phi, the block's centre in index units)"""
    occ = np.zeros((7, 5, 9), bool)
    occ[2:5, 1:4, 3:6] = True
    return occ, signed_field(occ, cell), np.array([3.0, 2.0, 4.0])


def blocking_grid_task(o, pts, xs, us, mults, fb, mu, cell=0.04):
    """the sibling's blocking_task with a field: an occupied block centred where the point that moves most lands under the full
    step, and a margin that inflates it until the old trajectory clears it by 1 cm at every t.  Returns the grid, (geom, w) of one
    instance and the full step's cost difference without the obstacle"""
    T = o.T
    _, x1, u1 = o.forward_alpha(1.0, xs, us, mults, fb, mu)
    gain = (o.cost_seq_aug(x1, u1, mults, mu) - o.cost_seq_aug(xs, us, mults, mu)).sum()
    Xo, Xn = xs.reshape(T + 1, o.nx), x1.reshape(T + 1, o.nx)
    Po = np.array([oc.positions(o, pts, Xo[t][:o.nq]) for t in range(T + 1)])
    Pn = np.array([oc.positions(o, pts, Xn[t][:o.nq]) for t in range(T + 1)])
    move = np.linalg.norm(Pn - Po, axis=2)
    t_, k_ = np.unravel_index(np.argmax(move), move.shape)
    occ, phi, centre = block_scene(cell)
    origin = Pn[t_, k_] - cell * centre
    grid = (phi, origin, cell)
    vals = [lookup(phi, origin, cell, Po[t, k])[0] - pts[k][2] for t in range(T + 1) for k in range(len(pts))]
    margin = min(min(vals) - 0.01, 0.0)
    geom = np.tile(np.array([0.0, 0.0, 0.0, margin]), (T + 1, 1, 1))
    unit = grid_pair(grid)
    term = sum(0.5 * min(unit(GRID, geom[t, 0], Pn[t, k], pts[k][2])[0], 0.0) ** 2 for t in range(T + 1) for k in range(len(pts)))
    assert term > 0.0
    return occ, grid, geom, np.full((T + 1, 1), 5.0 * abs(gain) / term), gain


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path", [("tree38", None, 1), ("chain6ff", 0, 0)])
def test_forward_matches_emulation(gpu, monkeypatch, name, fo_, fwd_path):
    """ddp_hip_forward with n_alpha = 4 on a task whose full step the field blocks: the accepted step, X_NEW, U_NEW and dcost
    against the sibling's emulation with the grid terms added; the field comes from set_occupancy.  Asserted on the emulation
    alone first: the full step is accepted without the obstacle and rejected with it, and every candidate decides by more than
    1e-9 of the sum of the cost terms' magnitudes"""
    capi = gpu
    T, mu, n_alpha = 16, 1.0, 4
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, 1, 81, held=True)
    mults = tc._mults(o, xs[0], 85)
    pts = oc.pick_points(model)
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        occ, grid, geom, w, gain = blocking_grid_task(o, pts, xs[0], us[0], mults, fb, mu_o[0])
        monkeypatch.setattr(oc, "pair", grid_pair(grid))
        oc.check_task(o, pts, (GRID,), xs, geom[None], w[None], fractions=False)
        ctx.set_obstacle_occupancy(occ, grid[1], grid[2])
        assert ulp_ok(ctx.obstacle_grid()[0], grid[0], grid[2])
        oc.set_task(ctx, pts, (GRID,), geom, w)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
        clear_old, clear_new = ctx.obstacle_clearance(0)[0], ctx.obstacle_clearance(1)[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + oc.ob_terms(o, pts, (GRID,), X, geom, w)
    em = oc._emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, "gain", gain, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins)
    assert gain < 0.0
    assert np.all(oc.ob_terms(o, pts, (GRID,), xs[0], geom, w) == 0.0)
    assert step_ref < 1.0 and len(margins) > 1
    assert min(margins) > 1e-9, margins
    assert step[0] == step_ref, (step, step_ref)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)
    assert np.min(clear_old) > 0.0
    exc = oc.ob_clearance(o, pts, (GRID,), xn_ref, geom, w)
    assert np.array_equal(np.isinf(clear_new), np.isinf(exc))
    assert rel_err(clear_new[np.isfinite(exc)], exc[np.isfinite(exc)]) < 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [("tree38", 6, 2, None, 1), ("chain6ff", 6, 2, 0, 0)])
@pytest.mark.parametrize("mode", ["resident", "zero_weights", "untouched"])
def test_neutrality(gpu, monkeypatch, name, T, fd_mode, fo_, fwd_path, mode):
    """bit for bit what a context without the flag computes (linearise, both costs, sweep, forward): with a grid resident and no
    grid slot (far spheres and half-spaces of non-zero weight), with grid slots in the way of weight 0, and with grid slots of
    non-zero weight that neither the trajectory nor a candidate enters (one shifted 10 m away: every point outside; one in place
    with a margin of -10: every point inside it clear)"""
    capi = gpu
    mu, B = 10.0, 2
    _, grid = scene()
    monkeypatch.setattr(oc, "pair", grid_pair(grid))
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    pts = oc.pick_points(model)
    if mode == "resident":
        kinds, geom, w = oc._far_task(B, T)
    elif mode == "zero_weights":
        kinds = KINDS
        geom, w = grid_task(o, pts, kinds, xs, B, 33, grid)
        w[:] = 0.0
    else:
        kinds = (GRID, GRID)
        geom = np.zeros((B, T + 1, 2, 4))
        geom[..., 0, :3] = (10.0, -10.0, 10.0)
        geom[..., 1, :3] = oc.positions(o, pts, xs[0][:o.nq])[1] - (grid[1] + grid[2] * np.array([3.0, 2.0, 4.0]))
        geom[..., 1, 3] = -10.0
        w = np.full((B, T + 1, 2), 50.0)
        ex = np.stack([oc.ob_clearance(o, pts, kinds, xs[b], geom[b], w[b]) for b in range(B)])
        assert np.min(ex) > 5.0 and np.any(np.isfinite(ex))                       # some point is inside the grid, and clear
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (capi.FLAG_OBSTACLE_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on:
                set_task(ctx, grid, pts, kinds, geom, w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
            if on and mode == "untouched":
                c0, c1 = ctx.obstacle_clearance(0), ctx.obstacle_clearance(1)
                assert np.min(c0) > 5.0 and np.min(c1) > 5.0 and np.any(np.isfinite(c0))
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
def test_replacement(gpu, monkeypatch):
    """linearise, a refused set_grid (a NaN in phi) in between changes nothing, set_occupancy with other dims and another scene,
    linearise again: the second result matches the yardstick on the new grid and differs from the first; the slots' geometry
    and weights stay through the replacement"""
    capi = gpu
    T, B = 3, 2
    _, grid = scene()
    occ2, grid2 = scene(seed=5, shape=(13, 9, 17), p=0.4, cell=0.05)             # the same box, twice as fine, another scene
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 71)
    pts = oc.pick_points(model)
    kinds = (GRID, GRID)
    geom, w = grid_task(o, pts, kinds, xs, B, 72, grid)
    monkeypatch.setattr(oc, "pair", grid_pair(grid))
    check_grid_task(o, pts, kinds, xs, geom, w, grid)
    add1 = [oc.ob_derivs(o, model, pts, kinds, xs[b], geom[b], w[b]) for b in range(B)]
    monkeypatch.setattr(oc, "pair", grid_pair(grid2))
    check_grid_task(o, pts, kinds, xs, geom, w, grid2, need=False)
    add2 = [oc.ob_derivs(o, model, pts, kinds, xs[b], geom[b], w[b]) for b in range(B)]
    assert all(np.max(np.abs(a["LX"])) > 0 for a in add2)
    with capi.Context(spec) as ctx:
        _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
        ctx.linearize()
        off = {s: ctx.download(s) for s in DERIVS}
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
        set_task(ctx, grid, pts, kinds, geom, w)
        ctx.linearize()
        first = {s: ctx.download(s) for s in DERIVS}
        bad = grid[0].copy(); bad[3, 2, 1] = np.nan
        with pytest.raises(capi.DdpHipError) as exc:
            ctx.set_obstacle_grid(bad, grid[1], grid[2])
        assert exc.value.code == capi.E_ARG
        assert np.array_equal(ctx.obstacle_grid()[0], grid[0])
        ctx.linearize()
        for s in DERIVS:
            assert np.array_equal(ctx.download(s), first[s]), s
        ctx.set_obstacle_occupancy(occ2, grid2[1], grid2[2])
        phi2, o2, c2 = ctx.obstacle_grid()
        assert phi2.shape == (13, 9, 17) and ulp_ok(phi2, grid2[0], c2) and np.array_equal(o2, grid2[1]) and c2 == grid2[2]
        g1, w1 = ctx.obstacle_cost()
        assert np.array_equal(g1, geom) and np.array_equal(w1, w)
        ctx.linearize()
        second = {s: ctx.download(s) for s in DERIVS}
    for b in range(B):
        for s in ("LX", "LXX", "LFX", "LFXX"):
            assert rel_err(first[s][b], off[s][b] + add1[b][s]) <= TOL, (s, b)
            assert rel_err(second[s][b], off[s][b] + add2[b][s]) <= TOL, (s, b)
        assert not np.array_equal(first["LX"][b], second["LX"][b]) and not np.array_equal(first["LXX"][b], second["LXX"][b])


@pytest.mark.gpu
def test_refusals(gpu):
    capi = gpu
    T, B = 3, 2
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)
    L = capi.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pts = oc.pick_points(model)
    _, (phi, origin, cell) = scene()
    occ = scene()[0]

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_obstacle_grid(phi, origin, cell)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.set_obstacle_occupancy(occ, origin, cell)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.obstacle_grid()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.obstacle_grid_query(np.zeros((1, 3)))) == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        # before any grid: nothing to hand back, no slot of the kind
        assert code(lambda: ctx.obstacle_grid()) == capi.E_ARG
        assert code(lambda: ctx.obstacle_grid_query(np.zeros((1, 3)))) == capi.E_ARG
        assert code(lambda: ctx.set_obstacle_points(points=pts, kinds=[SPHERE, GRID, HALFSPACE])) == capi.E_ARG
        assert code(lambda: ctx.set_obstacle_points(points=pts, kinds=[GRID])) == capi.E_ARG

        def refused():
            dims = np.array(phi.shape, dtype=np.int32)
            dimp, op, pp = dims.ctypes.data_as(ip), origin.ctypes.data_as(dp), phi.ctypes.data_as(dp)
            ob = np.ascontiguousarray(occ, dtype=np.uint8)
            bp = ob.ctypes.data_as(C.POINTER(C.c_uint8))
            for args in ((None, op, cell, pp), (dimp, None, cell, pp), (dimp, op, cell, None)):
                assert L.ddp_hip_obstacle_set_grid(ctx._h, *args) == capi.E_ARG
            for args in ((None, op, cell, bp), (dimp, None, cell, bp), (dimp, op, cell, None)):
                assert L.ddp_hip_obstacle_set_occupancy(ctx._h, *args) == capi.E_ARG
            for a in range(3):
                for bad in (1, capi.MAX_GRID_DIM + 1):
                    shape = [2, 2, 2]; shape[a] = bad
                    assert code(lambda: ctx.set_obstacle_grid(np.zeros(shape), origin, cell)) == capi.E_ARG, shape
                    assert code(lambda: ctx.set_obstacle_occupancy(np.zeros(shape, bool), origin, cell)) == capi.E_ARG, shape
                    d = dims.copy(); d[a] = 0
                    assert L.ddp_hip_obstacle_set_grid(ctx._h, d.ctypes.data_as(ip), op, cell, pp) == capi.E_ARG
                    d[a] = -3
                    assert L.ddp_hip_obstacle_set_occupancy(ctx._h, d.ctypes.data_as(ip), op, cell, bp) == capi.E_ARG
                for bad in (np.nan, np.inf, -np.inf):
                    ob_ = origin.copy(); ob_[a] = bad
                    assert code(lambda: ctx.set_obstacle_grid(phi, ob_, cell)) == capi.E_ARG
                    assert code(lambda: ctx.set_obstacle_occupancy(occ, ob_, cell)) == capi.E_ARG
            for bad in (0.0, -0.1, np.nan, np.inf):
                assert code(lambda: ctx.set_obstacle_grid(phi, origin, bad)) == capi.E_ARG, bad
                assert code(lambda: ctx.set_obstacle_occupancy(occ, origin, bad)) == capi.E_ARG, bad
            for bad in (np.nan, np.inf, -np.inf):
                pb = phi.copy(); pb[6, 4, 8] = bad
                assert code(lambda: ctx.set_obstacle_grid(pb, origin, cell)) == capi.E_ARG, bad
        refused()
        assert code(lambda: ctx.obstacle_grid()) == capi.E_ARG                     # a refused call sets nothing
        ctx.set_obstacle_grid(phi, origin, cell)
        refused()
        got, o_, c_ = ctx.obstacle_grid()                                         # ... and leaves the old grid in force
        assert np.array_equal(got, phi) and np.array_equal(o_, origin) and c_ == cell
        dims, og, cl = np.zeros(3, dtype=np.int32), np.zeros(3), C.c_double(0.0)
        assert L.ddp_hip_obstacle_grid_download(ctx._h, dims.ctypes.data_as(ip), og.ctypes.data_as(dp), C.byref(cl), None) == 0   # shape only
        assert tuple(dims) == phi.shape and np.array_equal(og, origin) and cl.value == cell
        assert L.ddp_hip_obstacle_grid_download(ctx._h, None, og.ctypes.data_as(dp), C.byref(cl), None) == capi.E_ARG
        assert L.ddp_hip_obstacle_grid_download(ctx._h, dims.ctypes.data_as(ip), None, C.byref(cl), None) == capi.E_ARG
        assert L.ddp_hip_obstacle_grid_download(ctx._h, dims.ctypes.data_as(ip), og.ctypes.data_as(dp), None, None) == capi.E_ARG
        z = np.zeros(3)
        assert L.ddp_hip_obstacle_grid_query(ctx._h, 1, None, z.ctypes.data_as(dp), None) == capi.E_ARG
        assert L.ddp_hip_obstacle_grid_query(ctx._h, 1, z.ctypes.data_as(dp), None, None) == capi.E_ARG
        assert L.ddp_hip_obstacle_grid_query(ctx._h, -1, z.ctypes.data_as(dp), z.ctypes.data_as(dp), None) == capi.E_ARG
        assert L.ddp_hip_obstacle_grid_query(ctx._h, 0, None, None, None) == 0
        v, g = ctx.obstacle_grid_query(np.array([[np.nan, 0.0, 0.0]]))             # a NaN coordinate is NaN, not outside
        assert np.isnan(v[0]) and np.all(np.isnan(g))
        # the kind, now that a grid is resident; unknown kinds are what they were
        assert code(lambda: ctx.set_obstacle_points(points=pts, kinds=[SPHERE, 3, HALFSPACE])) == capi.E_ARG
        ctx.set_obstacle_points(points=pts, kinds=[SPHERE, GRID, HALFSPACE])
        no = 3
        gg = np.zeros((T + 1, no, 4))
        gg[:, 2, :3] = (0.0, 0.6, 0.8)
        gg[:, 1] = (7.0, -3.0, 0.5, -0.25)                                         # a shift of any length, a negative margin
        ctx.set_obstacle_cost(geom=gg, weight=np.ones(no))
        _setup(ctx, *_trajs(o, model, B, 5))
        for a in range(4):
            for bad in (np.nan, np.inf, -np.inf):
                gb = gg.copy(); gb[2, 1, a] = bad
                assert code(lambda: ctx.set_obstacle_cost(geom=gb)) == capi.E_ARG, (a, bad)
        assert np.array_equal(ctx.obstacle_cost()[0], np.broadcast_to(gg, (B, T + 1, no, 4)))
        assert np.all(ctx.obstacle_clearance(0) < np.inf)                          # (the half-space sees every point)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 2])
def test_advance_shifts_rows_and_keeps_the_grid(gpu, shift):
    """ddp_hip_advance: a grid slot's geometry and weights move like the others' (rows 0 .. T-1 by the hold rule, row T untouched),
    and the grid is what it was, bit for bit"""
    capi = gpu
    T, B = 3, 2
    occ, grid = scene()
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    xs, us = _trajs(o, model, B, 181)
    pts = oc.pick_points(model)
    geom, w = grid_task(o, pts, KINDS, xs, B, 182, grid)
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        _setup(ctx, xs, us)
        ctx.set_obstacle_occupancy(occ, grid[1], grid[2])
        before = ctx.obstacle_grid()
        oc.set_task(ctx, pts, KINDS, geom, w)
        ctx.advance(shift, None, capi.ADVANCE_NO_ROLL)
        g1, w1 = ctx.obstacle_cost()
        after = ctx.obstacle_grid()
        val = ctx.obstacle_grid_query(grid[1] + grid[2] * np.array([[3.25, 2.5, 4.75]]), grad=False)
    assert np.array_equal(g1, adv.np_advance(geom, shift, terminal=True)) and np.array_equal(w1, adv.np_advance(w, shift, terminal=True))
    assert np.array_equal(g1[:, T], geom[:, T]) and np.array_equal(g1[:, 0], geom[:, shift]) and not np.array_equal(g1, geom)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert rel_err(val, [lookup(grid[0], grid[1], grid[2], grid[1] + grid[2] * np.array([3.25, 2.5, 4.75]))[0]]) <= TOL


@pytest.mark.gpu
def test_reach_past_occupied_block(gpu, monkeypatch):
    """chain6, T = 40, no constraint: a tracking cost pulls the arm to a goal posture.  The flag-off solve's tip path is taken
    first and an occupied block is put on it, halfway (set_occupancy).  The yardstick confirms that this solution penetrates the
    field; with the grid slot's weight on, from the same start, the least clearance of the result is greater"""
    capi = gpu
    T, mu, iters, cell = 40, 1.0, 12, 0.02
    model, spec, o = oc._reach_problem(T)
    xs, us = _trajs(o, model, 1, 141, held=True)
    tip = (5, (0.0, 0.0, 0.0823), 0.03)
    rng = np.random.default_rng(142)
    goal = np.concatenate([xs[0][:o.nq] + 0.6 * rng.choice([-1.0, 1.0], size=o.nv), np.zeros(o.nv)])
    xref = np.tile(goal, (T + 1, 1))
    wx = np.tile(np.concatenate([np.full(o.nv, 200.0), np.full(o.nv, 1.0)]), (T + 1, 1))
    wx[T] *= 10.0

    def solve(ctx):
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            if not step[0] > 0.0:                                                   # no candidate lowers the cost: the iterate stays
                break
            ctx.swap_traj()
        return ctx.download("X")
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_tracking_cost(xref=xref, wx=wx)
        x_off = solve(ctx)
    Xo = x_off[0].reshape(T + 1, o.nx)
    path = np.array([o.frame_position(tip[0], tip[1], Xo[t][:o.nq]) for t in range(T + 1)])
    assert np.linalg.norm(path[T] - path[0]) > 0.1                                  # the tip travels
    occ, phi, centre = block_scene(cell)
    grid = (phi, path[T // 2] - cell * centre, cell)
    monkeypatch.setattr(oc, "pair", grid_pair(grid))
    geom, w = np.zeros((1, 4)), np.full(1, 1e5)
    pen_ref = -np.min(oc.ob_clearance(o, [tip], (GRID,), x_off[0], np.tile(geom, (T + 1, 1, 1)), np.ones((T + 1, 1))))
    assert pen_ref > 0.03, pen_ref                                                  # the unobstructed solve goes through the block
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS) as ctx:
        ctx.set_tracking_cost(xref=xref, wx=wx)
        ctx.set_obstacle_occupancy(occ, grid[1], grid[2])
        ctx.set_obstacle_points(points=[tip], kinds=[GRID])
        ctx.set_obstacle_cost(geom=geom, weight=w)
        _setup(ctx, x_off, us)
        clear_off = np.min(ctx.obstacle_clearance(0))
        assert abs(-clear_off - pen_ref) <= 1e-9
        _setup(ctx, xs, us)
        x_on = solve(ctx)
        clear_on = np.min(ctx.obstacle_clearance(0))
    print("reach", "clearance without", clear_off, "with", clear_on)
    assert clear_on > clear_off, (clear_on, clear_off)
    assert not np.array_equal(x_on, x_off)
