"""The run-time-shaped kernels on robots of other sizes and trees (tests/robots.py): everything a user's own robot runs is
instantiated for a size class (1 / 6 / 38 / 64 joints) and reads nv at run time, and the built-in robots reach one size per
class.  Every GPU test holds the device against the C oracle on the same TableModel, at the project's own tolerances, and
asserts the path ctx.info() reports, so that a case cannot silently stop reaching its kernel.  The add-on cost terms on these
robots are in test_cost_terms_other_robots.py (test_com_term stays here).

Horizons are 2 .. 4 and the batch is 3 (one instance per workgroup or lane group: the second and third catch a wrong instance
stride).  The oracle-only guards (the catalogue is what it claims; the line-search decisions do not hang on rounding) run
without a GPU.

Tiling of the generic sweep (DDP_HIP_BWD_CBX / DDP_HIP_BWD_CBU): bwd_assemble forms every entry of Q from its own column alone --
W = V_xx F(:, c) per column, the dense terms per (row, column), contract_slab one column at a time through a workgroup-wide
barrier -- in an order of operations that does not depend on which columns share a job.  The test asserts it: bit for bit the
default tiling's result."""
import functools

import numpy as np
import pytest

import robots
from problems import initial_trajectory, random_state
from synth import rel_err, synth_sweep_inputs, upload_sweep_inputs
from test_dynamics_parity import DERIV_SEQS, TENSOR_SEQS, _jitter_states, linearize_parity_on

B = 3
ALL = [n for n in robots.CATALOGUE if n not in ("tree57", "tree58")]
LIN = [n for n in ALL if n not in ("wide38x", "quad38")]          # one fallback tree of the 38s is enough for the linearisation
SWEPT = [n for n in ALL if n != "tree64"]
CONSTRAINED = [("fork5", "config"), ("tree21", "frame"), ("tree39", "config"), ("tree63", "config")]
K_SCALE = (1.0, 3.0, 30.0)                                         # feed-forward scales per instance: different steps per round
EPS, E1 = 2.220446049250313e-16, 1.4901161193847656e-08


def nv_of(name):
    return len(robots.CATALOGUE[name].parents)


def horizon(name):
    return 4 if nv_of(name) <= 21 else 3 if nv_of(name) <= 38 else 2


def expected_info(name, first_order_fd=1):
    """what ctx.info() reports for a catalogue robot: the run-time-tree linearisation, the latency forward kernel on wide38 alone,
    the Talos-shaped sweep at n = 76, m = 38 (config constraints of 38 rows included: up to 52 fit)"""
    return {"lin_path": 1, "first_order": 1 if first_order_fd else 2, "fwd_path": 1 if name == "wide38" else 0,
            "bwd_path": 1 if nv_of(name) == 38 else 0}


def assert_info(ctx, name, first_order_fd=1):
    info = ctx.info()
    for k, v in expected_info(name, first_order_fd).items():
        assert info[k] == v, (name, k, info)


@functools.lru_cache(maxsize=None)
def trajectories(name, T, fd_mode, first_order_fd, constraint, u_sigma=0.5):
    """(model, spec, oracle, [(xs, us)] * B): the oracle's rollouts of seeded controls from the neutral state"""
    model, spec, o = robots.problem(name, T, batch=B, fd_mode=fd_mode, first_order_fd=first_order_fd, constraint=constraint)
    return model, spec, o, [initial_trajectory(o, model, seed=10 + b, u_sigma=u_sigma)[1:][::-1] for b in range(B)]


def seeded_mults(o, xs, seed, jac_sigma=0.01):
    mults = o.alloc_affine(o.Etot)
    mults["origin"][:] = xs[:o.T * o.nx]
    if o.Etot:
        mults["jac"][:o.Etot * o.n] = jac_sigma * np.random.default_rng(seed).normal(size=o.Etot * o.n)
    return mults


def upload_affine(ctx, pre, a, b):
    for k in ("origin", "val", "jac"):
        s = f"{pre}_{k.upper()}"
        if ctx.seq_size(s):
            ctx.upload(s, a[k][:ctx.seq_size(s)], b, 1)


# ---- CPU: the catalogue -------------------------------------------------------------------------------------------------------
def test_catalogue_is_what_it_claims():
    from ddp_pinocchio_amd import capi
    sizes = {"pair2": 2, "fork5": 5, "star7": 7, "tree13": 13, "tree21": 21, "wide38": 38, "wide38x": 38, "deep38": 38, "quad38": 38,
             "tree39": 39, "tree40": 40, "TREE44": 44, "tree57": 57, "tree58": 58, "tree63": 63, "tree64": 64}
    assert {n: nv_of(n) for n in robots.CATALOGUE} == sizes
    compiled_in = [list(capi.BuiltinModel(capi.BUILTIN_CHAIN6).parent), list(capi.BuiltinModel(capi.BUILTIN_TREE38, 1).parent),
                   robots.ARM7, robots.BIPED12]
    shape = {}
    for name, r in robots.CATALOGUE.items():
        assert r.parents[0] == -1 and all(0 <= p < i for i, p in enumerate(r.parents) if i), name
        assert list(r.parents) not in compiled_in, name
        level, width, children = robots.tree_shape(r.parents)
        shape[name] = (len(width), int(width.max()), int(children.max()))
        assert width.max() <= 64, name                            # a tree level per wave (lin_plan.cpp)
        assert robots.open_slots(r.parents) <= 8, name            # what ddp_hip_create accepts (ctx.hip: build_slot_tables)
        m = robots.model(name)
        assert m.nv == len(r.parents) and list(m.parent) == list(r.parents)
        assert [int(j) for j in np.flatnonzero(m.jtype == capi.JOINT_PRISMATIC)] == list(r.prismatic)
    # the limits of the latency forward kernel (fwd_lat_supported): 8 joints per level, 16 levels, 3 children per joint
    assert shape["wide38"] == (7, 8, 3)                           # exactly at the width limit, inside the other two
    assert shape["wide38x"][1] == 9 and shape["wide38x"][0] <= 16 and shape["wide38x"][2] <= 3      # past one limit each, inside the others
    assert shape["deep38"][0] == 17 and shape["deep38"][1] <= 8 and shape["deep38"][2] <= 3
    assert shape["quad38"][2] == 4 and shape["quad38"][0] <= 16 and shape["quad38"][1] <= 8
    assert robots.open_slots(robots.by_level_numbering(robots.WIDE38)) > 8      # the same tree numbered level by level is refused
    # the Talos tree is numbered depth first -- a fork's next child follows the whole subtree of the one before -- and no fork of
    # wide38 is: the cooperative traversal meets every fork's children in another index pattern
    talos = list(capi.BuiltinModel(capi.BUILTIN_TREE38, 1).parent)
    for parents, depth_first in ((robots.WIDE38, False), (talos, True)):
        size = [1] * 38
        for i in range(37, 0, -1):
            size[parents[i]] += size[i]
        forks = [j for j in range(38) if parents.count(j) > 1]
        assert forks
        for j in forks:
            kids = [i for i, p in enumerate(parents) if p == j]
            assert all((b == a + size[a]) == depth_first for a, b in zip(kids, kids[1:])), (j, kids)
    assert len(robots.CATALOGUE["fork5"].prismatic) == 1 and len(robots.CATALOGUE["tree21"].prismatic) >= 2
    assert shape["fork5"][2] == 2 and robots.CATALOGUE["star7"].parents != robots.ARM7
    for name in ("tree13", "tree21", "tree39", "tree40", "tree63", "tree64"):
        assert shape[name][2] >= 2, name                          # branching
    # the sweep's LDS by the formulas of bwd.hip (gains_lds_bytes, assemble_lds_bytes at a 3-column job): which sizes pass the
    # default 64 KB of dynamic LDS, which pass a workgroup's 160 KB
    def gains(nv, box=False):
        ld = nv | 1
        return 8 * (ld * nv + ld * (2 * nv + 1) + ld * 2 * nv + ((ld * nv + 9 * nv) if box else 0))
    def assemble(nv, cn=3, emax=0):
        return 8 * (2 * nv + emax + 2 * nv * cn + 3 * nv * cn + (nv + 1) * 2 * nv)
    assert gains(39) <= 65536 < gains(40) and assemble(59) <= 65536 < assemble(60)
    assert gains(63) <= 163840 < gains(64) == 166920 and gains(57, True) <= 163840 < gains(58, True)


# ---- the forward's reference: the oracle's sequential halving, and how clearly each candidate decides --------------------------
@functools.lru_cache(maxsize=None)
def forward_case(name, batch=B):
    """Feedback from the oracle's own sweep on its own derivatives (fd_mode 0), the feed-forward scaled per instance by 1, 3, 30.
    Per instance: inputs, Oracle.forward's step and trajectory, and of every candidate the halving tries |sum(new - old)| over
    the summed magnitudes of the cost terms (the device adds them in another association)"""
    T = horizon(name)
    model, spec, o = robots.problem(name, T, batch=batch, fd_mode=0)
    out = []
    for b in range(batch):
        x0, us, xs = initial_trajectory(o, model, seed=20 + b, u_sigma=0.3)
        d = o.compute_derivatives(xs, us)
        mults = seeded_mults(o, xs, 0)
        bw = o.backward(d, xs, mults, reg=0.0, mu=1.0)
        assert bw["restarts"] == 0
        bw["fb"]["val"] *= K_SCALE[b % 3]
        step, xs_ref, us_ref, n_evals = o.forward(xs, us, mults, bw["fb"], bw["mu"])
        old = o.cost_seq_aug(xs, us, mults, bw["mu"])
        margins, dc = [], None
        for k in range(n_evals):
            dc, xn, un = o.forward_alpha(2.0 ** -k, xs, us, mults, bw["fb"], bw["mu"])
            new = o.cost_seq_aug(xn, un, mults, bw["mu"])
            margins.append(abs(dc) / (np.sum(np.abs(new)) + np.sum(np.abs(old))))
            assert (dc <= 0) == (k == n_evals - 1), (name, b, k, dc)       # the halving stops at the first candidate that does not cost more
        full = o.forward_alpha(1.0, xs, us, mults, bw["fb"], bw["mu"])
        out.append(dict(xs=xs, us=us, mults=mults, fb=bw["fb"], mu=bw["mu"], step=step, xs_ref=xs_ref, us_ref=us_ref, dc=dc,
                        n_evals=n_evals, margins=margins, full=full))
    return model, spec, o, out


@pytest.mark.parametrize("name", ALL)
def test_forward_decisions_do_not_hang_on_rounding(name):
    """on the oracle alone: every candidate tried decides by more than 1e-9 of the summed cost magnitudes, and at least one
    instance of the batch halves (the guard of test_cost_terms_together.py); the same for the batch of 9 on fork5"""
    for batch in (B, 9) if name == "fork5" else (B,):
        _, _, _, cases = forward_case(name, batch)
        assert all(min(c["margins"]) > 1e-9 for c in cases), [c["margins"] for c in cases]
        assert any(c["step"] < 1.0 for c in cases), [c["step"] for c in cases]
        assert all(c["step"] == 2.0 ** -(c["n_evals"] - 1) for c in cases)


@pytest.mark.parametrize("name,constraint", CONSTRAINED + [("tree64", "config")])
def test_constraints_are_live(name, constraint):
    """on the oracle alone: the constrained cases have the rows the issue names and constraint values that matter"""
    T = horizon(name)
    model, spec, o, trajs = trajectories(name, T, 0, 1, constraint)
    assert spec.Etot == (nv_of(name) * T if constraint == "config" else 3) and int(spec.ne.max()) == (nv_of(name) if constraint == "config" else 3)
    for xs, us in trajs:
        d = o.compute_derivatives(xs, us)
        assert np.max(np.abs(d["eq_val"][:o.Etot])) > 1e-3 and np.max(np.abs(d["eq_x"][:o.Etot * o.n])) > 1e-3


SOLVES = [("fork5", 2, 5, 1e2), ("tree39", 0, 4, 1e4)]


def solve_inputs(name, fd_mode):
    T = horizon(name)
    model, spec, o = robots.problem(name, T, batch=B, fd_mode=fd_mode, constraint="config")
    us0 = np.zeros(T * model.nv)
    xs0 = o.rollout(np.zeros(2 * model.nv), us0)
    return model, spec, o, xs0, us0, 0.01 * np.random.default_rng(3).normal(size=o.Etot * o.n)


@pytest.mark.parametrize("name,fd_mode,iters,mu", SOLVES)
def test_solve_cases_are_well_posed(name, fd_mode, iters, mu):
    """on the oracle alone: the loop amplifies the finite-difference noise of the derivatives from iteration to iteration, and any
    change of the point they are taken at, however small, draws that noise anew.  So the oracle's answer to a 1e-13 change of the
    initial controls is the noise floor of its own result (the same oracle built with FMA contraction moves by as much); the cases
    keep it a hundred times under the tolerance of the comparison.  Measured: fork5 in mode 2 at mu = 1e2 4e-7 after 5 iterations
    (at the chain's mu = 1e4 1e-4 after 3: two draws of the noise would be compared there), tree39 in mode 0 at mu = 1e4 1e-7"""
    model, spec, o, xs0, us0, seed = solve_inputs(name, fd_mode)
    kw = dict(max_iterations=iters, threshold=1e-8, mu=mu, reg=0.0, w=1e-1, n=10.0)
    ref = o.solve(xs0, us0, seed, **kw)
    assert ref[3]["iterations"] == iters                           # the loop runs every iteration asked for
    for k in range(3):
        us1 = us0 + 1e-13 * np.random.default_rng(k).normal(size=us0.size)
        moved = o.solve(o.rollout(np.zeros(2 * model.nv), us1), us1, seed, **kw)
        assert rel_err(moved[0], ref[0]) < 1e-6, (k, rel_err(moved[0], ref[0]))


# ---- GPU: dynamics ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_dynamics(gpu, name, monkeypatch):
    """eval_f at random states (1e-11) and a rollout from a NaN-filled X (1e-10): rollout_kernel<6> below its template size,
    <38> on other trees, <64>; the latency kernel on wide38, where the pipelined form equals the DDP_HIP_FWD_NO_PIPE form bit for bit"""
    capi = gpu
    T = horizon(name)
    model, spec, o = robots.problem(name, T, batch=B, fd_mode=0)
    nx, nv = o.nx, model.nv
    rng = np.random.default_rng(1000 + nv)
    x_rand = np.stack([random_state(model, rng) for _ in range(B)])
    u_rand = 3.0 * rng.normal(size=(B, T * nv))
    trajs = [initial_trajectory(o, model, seed=10 + b, u_sigma=0.5) for b in range(B)]

    def run():
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
            assert_info(ctx, name)
            X = np.full((B, (T + 1) * nx), np.nan)
            X[:, :nx] = x_rand
            ctx.upload("X", X); ctx.upload("U", u_rand)
            ctx.rollout()
            one = ctx.download("X")
            X[:, :nx] = np.stack([t[0] for t in trajs])
            ctx.upload("X", X); ctx.upload("U", np.stack([t[1] for t in trajs]))
            ctx.rollout()
            return one, ctx.download("X")
    one, got = run()
    for b in range(B):
        assert np.array_equal(one[b, :nx], x_rand[b])
        e1 = rel_err(one[b, nx:2 * nx], o.eval_f(x_rand[b], u_rand[b, :nv]))
        e2 = rel_err(got[b], trajs[b][2])
        print("dynamics", name, b, e1, e2)
        assert e1 < 1e-11 and e2 < 1e-10, (name, b, e1, e2)
    if name == "wide38":
        monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
        one_np, got_np = run()
        assert np.array_equal(one, one_np, equal_nan=True) and np.array_equal(got, got_np)


# ---- GPU: linearisation ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lin_cases(name, fd_mode, first_order_fd):
    model, spec, o, trajs = trajectories(name, horizon(name), fd_mode, first_order_fd, None)
    return model, spec, o, [(xs, us, o.compute_derivatives(xs, us)) for xs, us in trajs]


# fd_mode 2: the bound on forward-differenced jacobians, in ulps of f.  8 is the project's bar, 16 its documented ceiling
# (test_linearize_parity_other_tree_seeds: trees whose ABA intermediates are larger than f): the trees
# of 39 and more joints measured 8.4 .. 12.5 on the device.  deep38 measured 17.2 and TREE44 37: their bounds are 8 x the oracle's
# own sensitivity (f_sensitivity_ulps: 10.0 and 39.5 ulp measured, so 80 and 316), formed from the oracle alone in the test
ULPS = {"tree39": 16, "tree63": 16, "tree64": 16, "deep38": None, "TREE44": None}


def f_sensitivity_ulps(o, cases):
    """How far the oracle's own f moves, in ulps of max(1, |f|), when one input moves by one ulp: the largest |f(x +- ulp e_i, u) -
    f(x, u)| over the inputs, the points of the trajectories and both signs.  The ulp is that of max(|input|, 1): the rollouts
    start at q = v = 0, whose own ulp is a denormal, while sin / cos of a joint angle round at the ulp of 1.  Two correct
    evaluations of f that differ in the last bit of one intermediate differ by this much.  Measured: pair2 .. wide38 1.0 - 1.8,
    tree39 8.3, tree40 7.6, deep38 10.0, tree63 9.0, tree64 10.5, TREE44 39.5 (its distal links are light: |f_u| is large)"""
    n, m = o.n, o.m
    worst = 0.0
    for xs, us, d in cases:
        fscale = max(1.0, float(np.max(np.abs(d["f_val"]))))
        for t in range(o.T):
            x, u = xs[t * n:(t + 1) * n], us[t * m:(t + 1) * m]
            f0 = o.eval_f(x, u)
            for i in range(n + m):
                for sign in (1.0, -1.0):
                    xx, uu = x.copy(), u.copy()
                    v, k = (xx, i) if i < n else (uu, i - n)
                    v[k] += sign * np.spacing(max(abs(v[k]), 1.0))
                    worst = max(worst, float(np.max(np.abs(o.eval_f(xx, uu) - f0))) / (EPS * fscale))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("fd_mode,first_order_fd", [(2, 1), (0, 0)])
@pytest.mark.parametrize("name", LIN)
def test_linearize(gpu, name, fd_mode, first_order_fd):
    """fd_mode 2 on forward-differenced jacobians (lin_first_kernel, the mode-2 stencil on its caches: <6> below its size, <38>
    on other trees, <64>) at the finite-difference noise bound of ULPS ulp of f, end to end and with the oracle's first order
    resident (LIN_SECOND alone), FXX / FUU symmetric bit for bit; fd_mode 0 on analytic jacobians (the one-lane kernel of small
    models, the wave kernels <38> / <64>) at 1e-10 with exact zero tensors"""
    model, spec, o, cases = lin_cases(name, fd_mode, first_order_fd)
    ulps = ULPS.get(name, 8)
    if ulps is None:
        ulps = 8 * f_sensitivity_ulps(o, cases)
    seen = linearize_parity_on(gpu, model, spec, o, cases, ulps=ulps, info=expected_info(name, first_order_fd), symmetric=True)
    print("linearize", name, fd_mode, "bound", ulps, "largest first-order error in ulps of f:", seen)


@pytest.mark.gpu
@pytest.mark.parametrize("name,constraint,fd_mode,first_order_fd", [
    ("fork5", "config", 2, 1), ("tree21", "frame", 2, 1), ("tree39", "config", 2, 1),
    ("tree63", "config", 0, 1),      # the chain-rule kernels: eq_combine_kernel's two 63 x 126 matrices, 127 KB of dynamic LDS
    ("tree63", "config", 0, 0),      # ana_eq_kernel<64> with 63 rows
])
def test_linearize_constrained(gpu, name, constraint, fd_mode, first_order_fd):
    """the constraint stage on the same robots: EQ_VAL, EQ_X, EQ_U (and the constraint tensors in mode 2) at the bounds of
    test_linearize_parity"""
    model, spec, o, trajs = trajectories(name, horizon(name), fd_mode, first_order_fd, constraint)
    cases = [(xs, us, o.compute_derivatives(xs, us)) for xs, us in trajs]
    linearize_parity_on(gpu, model, spec, o, cases, ulps=ULPS.get(name, 8), info=expected_info(name, first_order_fd), symmetric=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fork5", "tree21", "tree63"])
def test_linearize_mode1(gpu, name):
    """analytic mode 1 (forward differences of analytic jacobians): second_m1_kernel<6> at nv = 5, the wave kernels <38> with a
    padded M and <64>; the tolerances of test_analytic_mode1_on_other_tree_sizes (tensors at the cond(M) noise floor)"""
    capi = gpu
    model, spec, o, cases = lin_cases(name, 1, 0)
    nv, T = model.nv, o.T
    with capi.Context(spec) as ctx:
        assert_info(ctx, name, 0)
        for b, (xs, us, d) in enumerate(cases):
            ctx.upload("X", xs, b, 1); ctx.upload("U", us, b, 1)
        ctx.linearize()
        got = {k: ctx.download(s) for k, s in {**DERIV_SEQS, **TENSOR_SEQS}.items() if ctx.seq_size(s)}
    for b, (xs, us, d) in enumerate(cases):
        jscale = max(1.0, float(np.max(np.abs(d["fx"]))), float(np.max(np.abs(d["fu"]))))
        cond = max(float(np.linalg.cond(o.crba(xs[t * 2 * nv:t * 2 * nv + nv]))) for t in range(T))
        for key in ("f_val", "fx", "fu", "fxx", "fux", "fuu"):
            ref = d[key][:got[key][b].size]
            err, scale = float(np.max(np.abs(got[key][b] - ref))), max(1.0, float(np.max(np.abs(ref))))
            assert np.all(np.isfinite(got[key][b])), key
            tol = 1e-12 * scale if key == "f_val" else (1e-10 * scale if key in ("fx", "fu") else 8 * EPS * cond * jscale / E1)
            print("mode1", name, b, key, err, tol)
            assert err <= tol, (key, b, err, tol)


# ---- GPU: cost sequence -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,constraint", CONSTRAINED + [("tree64", "config")])
def test_cost_seq_aug(gpu, name, constraint):
    """the augmented cost with random multipliers at 1e-11: cost_kernel<6> / <38> / <64> with emax = nv config rows at every
    step, or the 3-row frame constraint at T - 2"""
    capi = gpu
    T = horizon(name)
    model, spec, o, trajs = trajectories(name, T, 0, 1, constraint)
    rng = np.random.default_rng(4)
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        assert_info(ctx, name)
        refs = []
        for b, (xs, us) in enumerate(trajs):
            mults = o.alloc_affine(o.Etot)
            mults["origin"][:] = _jitter_states(o, model, xs[:T * o.nx], rng)
            mults["val"][:o.Etot] = rng.normal(size=o.Etot)
            mults["jac"][:o.Etot * o.n] = rng.normal(size=o.Etot * o.n)
            ctx.upload("X", xs, b, 1); ctx.upload("U", us, b, 1)
            upload_affine(ctx, "MULT", mults, b)
            refs.append(o.cost_seq_aug(xs, us, mults, mu=37.0))
        ctx.cost_seq_aug(0, 37.0)
        got = ctx.download("COSTS_OLD")
    for b in range(B):
        assert rel_err(got[b], refs[b]) < 1e-11, (b, rel_err(got[b], refs[b]))
        assert got[b][T] == 0.0


# ---- GPU: backward sweep ----------------------------------------------------------------------------------------------------------
def compare_sweep(ctx, b, o, ref):
    from test_bwd_parity import _compare_instance
    return _compare_instance(ctx, b, o, ref, o.T)


def device_derivs(ctx, o, b):
    d = o.alloc_derivs()
    for k, s in {**DERIV_SEQS, **(TENSOR_SEQS if ctx.info()["has_tensors"] else {})}.items():
        if ctx.seq_size(s):
            d[k][:ctx.seq_size(s)] = ctx.download(s, b, 1)[0]
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("tensors", [True, False])
@pytest.mark.parametrize("name,constraint", [(n, None) for n in SWEPT] + CONSTRAINED)
def test_sweep_on_device_derivatives(gpu, name, constraint, tensors):
    """linearise on the device, then the sweep against the oracle's on the same (the device's own) derivatives, as smoke() does:
    k, K, V_x, V_xx per step to 1e-10, reg / mu and the restart count exact.  The run-time-shaped pair launch_sweep<0, 0> at every
    size but (12, 6) and (76, 38): dynamic LDS past 64 KB for bwd_gains from nv = 40 and for bwd_assemble at 63; the Talos-shaped
    kernels on the 38-joint trees, on the symmetric tensors of the run-time-tree stencil"""
    capi = gpu
    T = horizon(name)
    model, spec, o, trajs = trajectories(name, T, 2, 1, constraint)
    mu0 = 100.0 if constraint else 1.0
    with capi.Context(spec, flags=capi.FLAG_TRACE | (0 if tensors else capi.FLAG_NO_TENSORS)) as ctx:
        assert_info(ctx, name)
        mults = []
        for b, (xs, us) in enumerate(trajs):
            ctx.upload("X", xs, b, 1); ctx.upload("U", us, b, 1)
            mults.append(seeded_mults(o, xs, 30 + b))
            upload_affine(ctx, "MULT", mults[b], b)
        ctx.linearize()
        ds = [device_derivs(ctx, o, b) for b in range(B)]
        rc, reg, mu, restarts = ctx.backward(0.0, mu0)
        for b, (xs, us) in enumerate(trajs):
            ref = o.backward(ds[b], xs, mults[b], reg=0.0, mu=mu0)
            assert restarts[b] == ref["restarts"] and reg[b] == ref["reg"] and mu[b] == ref["mu"], (b, restarts, reg, mu, ref["restarts"])
            worst = compare_sweep(ctx, b, o, ref)
            print("sweep", name, constraint, tensors, b, worst)
            assert worst < 1e-10, (name, b, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fork5", "tree13", "tree63"])
def test_sweep_restart_decisions(gpu, name):
    """synthetic inputs at (n, m) = (10, 5), (26, 13), (126, 63), instance 1 indefinite at a middle step: restart count, reg and
    mu equal to the oracle's, the neighbours untouched (test_backward_restart_decisions at these sizes)"""
    from test_bwd_parity import _oracle
    capi = gpu
    nv, T = nv_of(name), 4
    e = [0] * T
    o = _oracle(nv, T, e)
    _, spec, _ = robots.problem(name, T, batch=B)
    with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
        assert_info(ctx, name)
        refs = []
        for b in range(B):
            d, xs, us, mults = synth_sweep_inputs(T, nv, e, seed=50 + b, indefinite_at=2 if b == 1 else None)
            upload_sweep_inputs(ctx, d, xs, us, mults, b)
            refs.append(o.backward(d, xs, mults, reg=0.0, mu=0.25))
        rc, reg, mu, restarts = ctx.backward(reg=0.0, mu=0.25)
        assert rc == capi.EV_LLT_RESTART
        assert refs[1]["restarts"] >= 1 and refs[0]["restarts"] == 0 and refs[2]["restarts"] == 0
        for b in range(B):
            assert restarts[b] == refs[b]["restarts"]
            assert reg[b] == refs[b]["reg"] and mu[b] == refs[b]["mu"]     # bit exact decisions
            worst = compare_sweep(ctx, b, o, refs[b])
            assert worst < 1e-10, (b, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree13", "tree21"])
def test_sweep_tiling(gpu, name, monkeypatch):
    """column jobs of 8 x-columns and 16 u-columns (DDP_HIP_BWD_CBX / _CBU): the last x-job (2 columns) and the last u-job are
    narrower than the tile.  1e-10 against the oracle, and bit for bit the default tiling's result (module docstring)"""
    from test_bwd_parity import _oracle
    capi = gpu
    nv, T = nv_of(name), 3
    e = [0] * T
    o = _oracle(nv, T, e)
    _, spec, _ = robots.problem(name, T, batch=B)
    inputs = [synth_sweep_inputs(T, nv, e, seed=70 + b) for b in range(B)]
    refs = [o.backward(d, xs, mults, reg=0.0, mu=10.0) for d, xs, us, mults in inputs]
    out = {}
    for tiling in ("default", "wide"):
        if tiling == "wide":
            monkeypatch.setenv("DDP_HIP_BWD_CBX", "8")
            monkeypatch.setenv("DDP_HIP_BWD_CBU", "16")
        with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
            assert_info(ctx, name)
            for b, inp in enumerate(inputs):
                upload_sweep_inputs(ctx, *inp, b)
            rc, reg, mu, restarts = ctx.backward(reg=0.0, mu=10.0)
            assert rc == 0 and not restarts.any()
            for b in range(B):
                assert compare_sweep(ctx, b, o, refs[b]) < 1e-10, (tiling, b)
            out[tiling] = [ctx.download(s) for s in ("FB_VAL", "FB_JAC", "VX_TRACE", "VXX_TRACE")]
    for a, w in zip(out["default"], out["wide"]):
        assert np.array_equal(a, w)


# ---- GPU: forward sweep -----------------------------------------------------------------------------------------------------------
def run_forward(capi, name, n_alpha, batch=B, frozen=None):
    model, spec, o, cases = forward_case(name, batch)
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        assert_info(ctx, name)
        for b, c in enumerate(cases):
            ctx.upload("X", c["xs"], b, 1); ctx.upload("U", c["us"], b, 1)
            ctx.upload("X_NEW", c["xs"], b, 1); ctx.upload("U_NEW", c["us"], b, 1)
            upload_affine(ctx, "FB", c["fb"], b)
        if frozen is not None:
            ctx.upload("X_NEW", np.full_like(cases[frozen]["xs"], 7.0), frozen, 1)
            ctx.upload("U_NEW", np.full_like(cases[frozen]["us"], 7.0), frozen, 1)
            ctx.set_active([0 if b == frozen else 1 for b in range(batch)])
        rc, step, dcost = ctx.forward(np.array([c["mu"] for c in cases]), n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW"), ctx.download("U_NEW")
    for b, c in enumerate(cases):
        if b == frozen:
            assert np.all(xn[b] == 7.0) and np.all(un[b] == 7.0)             # a frozen instance is not searched
            continue
        step_ref, xs_ref, us_ref, dc_ref = (1.0, c["full"][1], c["full"][2], c["full"][0]) if n_alpha == 0 else (c["step"], c["xs_ref"], c["us_ref"], c["dc"])
        assert step[b] == step_ref, (name, n_alpha, b, step, step_ref)
        assert rel_err(xn[b], xs_ref) < 1e-9 and rel_err(un[b], us_ref) < 1e-9, (name, b)
        assert abs(dcost[b] - dc_ref) <= 1e-9 * max(1.0, abs(dc_ref)), (name, b, dcost[b], dc_ref)
        assert n_alpha == 0 or dcost[b] <= 0
    return step, dcost, xn, un


@pytest.mark.gpu
@pytest.mark.parametrize("n_alpha", [3, 8])
@pytest.mark.parametrize("name", ALL)
def test_forward(gpu, name, n_alpha, monkeypatch):
    """the accepted step exactly, X_NEW / U_NEW at 1e-9, dcost at 1e-9 max(1, |ref|) against Oracle.forward; the instances of the
    batch accept different steps in different rounds (n_alpha = 3: up to three rounds).  forward_kernel<6> / <38> / <64>, the
    latency kernel on wide38, its pipelined form bit for bit the DDP_HIP_FWD_NO_PIPE form there"""
    got = run_forward(gpu, name, n_alpha)
    if name == "wide38":
        monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
        for a, b in zip(got, run_forward(gpu, name, n_alpha)):
            assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree13", "tree63"])
def test_forward_without_line_search(gpu, name):
    """n_alpha = 0: the full step, accepted whatever it costs"""
    run_forward(gpu, name, 0)


@pytest.mark.gpu
def test_forward_many_instances_one_frozen(gpu):
    """fork5 at batch 9, n_alpha = 8: 72 lanes, one full workgroup holding several instances' candidates and one partly filled;
    instance 4 frozen by set_active"""
    run_forward(gpu, "fork5", 8, batch=9, frozen=4)


# ---- GPU: centre-of-mass term -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree21", "tree63"])
def test_com_term(gpu, name):
    """com_cost_kernel's lane split at 32 and 64 lanes per evaluation, batch 3 and T = 4 (15 evaluations: the last workgroup partly
    filled at 32 lanes): LX, LXX, LFX, LFXX, COSTS_OLD and the forward's decision against test_com_cost.py's numpy reference at
    that module's tolerances"""
    import test_com_cost as cc
    capi = gpu
    T, mu0 = 4, 1.0
    model, spec, o, trajs = trajectories(name, T, 0, 1, None, 0.3)
    xs, us = np.stack([t[0] for t in trajs]), np.stack([t[1] for t in trajs])
    tgt, w = cc.random_task(o, model, xs, B, 82, wscale=200.0, spread=0.02)
    w[1, 2, :] = 0.0
    with capi.Context(spec, flags=capi.FLAG_COM_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert_info(ctx, name)
        ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
        ctx.set_com_cost(target=tgt, weight=w)
        ctx.linearize()
        lin = {s: ctx.download(s) for s in ("LX", "LXX", "LFX", "LFXX")}
        ctx.cost_seq_aug(0, mu0)
        costs = ctx.download("COSTS_OLD")
        _, _, mu_o, _ = ctx.backward(0.0, mu0)
        ctx.upload("FB_VAL", ctx.download("FB_VAL") * np.array(K_SCALE)[:, None])
        fb = [{"origin": ctx.download("FB_ORIGIN")[b], "val": ctx.download("FB_VAL")[b], "jac": ctx.download("FB_JAC")[b]} for b in range(B)]
        rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
        xn, un = ctx.download("X_NEW"), ctx.download("U_NEW")
    halved = False
    for b in range(B):
        mults = o.alloc_affine(0)
        d = o.compute_derivatives(xs[b], us[b])                    # the plain cost's derivatives: bit for bit the device's (test_linearize)
        add = cc.com_derivs(o, model, xs[b], tgt[b], w[b])
        for s, k in (("LX", "lx"), ("LXX", "lxx"), ("LFX", "lfx"), ("LFXX", "lfxx")):
            ex = d[k][:lin[s][b].size] + add[s]
            assert np.max(np.abs(add[s])) > 0
            assert rel_err(lin[s][b], ex) <= 1e-12, (s, b, rel_err(lin[s][b], ex))
        ex = o.cost_seq_aug(xs[b], us[b], mults, mu0) + cc.com_terms(o, model, xs[b], tgt[b], w[b])
        assert costs[b][T] != 0.0 and rel_err(costs[b], ex) <= 1e-12, (b, rel_err(costs[b], ex))

        def cost(X, U):
            return o.cost_seq_aug(X, U, mults, mu_o[b]) + cc.com_terms(o, model, X, tgt[b], w[b])
        em = cc._emulate_forward(o, xs[b], us[b], mults, fb[b], mu_o[b], 8, cost)
        assert em is not None
        step_ref, xn_ref, un_ref, new, margins = em
        print("com forward", name, b, step[b], step_ref, margins)
        assert min(margins) > 1e-9, margins               # a condition on the inputs: the decisions do not hang on rounding
        assert step[b] == step_ref, (b, step, step_ref)
        assert rel_err(xn[b], xn_ref) < 1e-9 and rel_err(un[b], un_ref) < 1e-9
        assert abs(dcost[b] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[b], new)
        halved |= step_ref < 1.0
    assert halved


# ---- GPU: whole solve -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,iters,mu", SOLVES)
def test_whole_solve(gpu, name, fd_mode, iters, mu):
    """ddp_hip_solve against the oracle's solve, config constraint at every step, with the tolerances of
    test_whole_solve_against_oracle's chain6 case (finite-difference jacobians on both sides) and its parameters but mu on fork5
    (test_solve_cases_are_well_posed)"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, w, n, tol = horizon(name), 1e-1, 10.0, 1e-4
    model, spec, o, xs0, us0, seed = solve_inputs(name, fd_mode)
    xs_ref, us_ref, fb_ref, log_ref = o.solve(xs0, us0, seed, max_iterations=iters, threshold=1e-8, mu=mu, reg=0.0, w=w, n=n)
    with capi.Context(spec) as ctx:
        assert_info(ctx, name)
        for b in range(B):
            ctx.upload("X", xs0, b, 1); ctx.upload("U", us0, b, 1)
            ctx.upload("X_NEW", xs0, b, 1); ctx.upload("U_NEW", us0, b, 1)
            ctx.upload("MULT_ORIGIN", xs0[:T * o.nx], b, 1)
            ctx.upload("MULT_VAL", np.zeros(o.Etot), b, 1)
            ctx.upload("MULT_JAC", seed, b, 1)
        log = solver.solve(ctx, iters, 1e-8, mu, 0.0, w, n)
        xs, us = ctx.download("X"), ctx.download("U")
    for b in range(1, B):
        assert np.array_equal(xs[0], xs[b]) and np.array_equal(us[0], us[b])     # instances are independent and deterministic
    print("solve", name, rel_err(xs[0], xs_ref), rel_err(us[0], us_ref), log["opt_constr"][0], log_ref["opt_constr"], log["iterations"], log_ref["iterations"])
    assert log["mu"][0] == log_ref["mu"], (log["mu"], log_ref["mu"])
    assert rel_err(xs[0], xs_ref) < tol, rel_err(xs[0], xs_ref)
    assert rel_err(us[0], us_ref) < 10 * tol, rel_err(us[0], us_ref)
    assert abs(log["opt_constr"][0] - log_ref["opt_constr"]) <= 100 * tol * max(1.0, log_ref["opt_constr"])


# ---- GPU: the limits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_sweep_at_64_joints(gpu):
    """nv = 64: bwd_gains would need 166 920 B of LDS, a workgroup has 160 KB.  backward and solve answer E_UNSUPPORTED from the
    host-side check, nothing is launched and nothing resident changes; the context stays usable: a following rollout matches"""
    capi = gpu
    T = 2
    model, spec, o, trajs = trajectories("tree64", T, 0, 1, None)
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        assert_info(ctx, "tree64")
        for b, (xs, us) in enumerate(trajs):
            ctx.upload("X", xs, b, 1); ctx.upload("U", us, b, 1)
        for s in ("FB_VAL", "FB_JAC", "FX"):
            ctx.fill(s, 7.0)
        with pytest.raises(capi.DdpHipError) as ei:
            ctx.backward(0.0, 1.0)
        assert ei.value.code == capi.E_UNSUPPORTED
        with pytest.raises(capi.DdpHipError) as ei:
            ctx.solve(3, 1e-8, 1.0, 0.0, 0.1, 10.0)
        assert ei.value.code == capi.E_UNSUPPORTED
        for s in ("FB_VAL", "FB_JAC", "FX"):                       # neither the sweep nor the solve's first linearisation ran
            assert np.all(ctx.download(s) == 7.0), s
        X = np.full((B, (T + 1) * o.nx), np.nan)
        X[:, :o.nx] = 0.0
        ctx.upload("X", X)
        ctx.rollout()
        got = ctx.download("X")
        for b, (xs, us) in enumerate(trajs):
            assert rel_err(got[b], xs) < 1e-10


@pytest.mark.gpu
def test_box_sweep_at_57_joints(gpu):
    """control bounds: the box QP's second copy of Q_uu fits a workgroup's LDS up to nv = 57 (160 512 B).  Per step, from the device's
    own V(t+1), against test_control_bounds.py's yardstick at its tolerance (test_sweep_parity_at_size: clamped set equal, k, K,
    V_x, V_xx to 1e-10)"""
    import test_control_bounds as cb
    capi = gpu
    nv, T = 57, 3
    n, m = 2 * nv, nv
    ne = np.zeros(T, dtype=np.int64)
    Epre = np.zeros(T + 1, dtype=np.int64)
    _, spec, _ = robots.problem("tree57", T, batch=1)
    with capi.Context(spec, flags=capi.FLAG_TRACE | capi.FLAG_CONTROL_BOUNDS) as ctx:
        assert_info(ctx, "tree57")
        d, xs, us, mults = synth_sweep_inputs(T, nv, ne, seed=1)
        upload_sweep_inputs(ctx, d, xs, us, mults, 0)
        lo, hi = cb._sweep_bounds(us, T, m, 0.05, 1)
        ctx.set_control_bounds(lo=lo, hi=hi)
        rc, reg, mu, restarts = ctx.backward(0.0, 10.0)
        assert rc == 0 and restarts[0] == 0 and reg[0] == 0.0 and mu[0] == 10.0
        k_dev, K_dev = ctx.download("FB_VAL")[0].reshape(T, m), ctx.download("FB_JAC")[0].reshape(T, n, m).transpose(0, 2, 1)
        Vx_dev, Vxx_dev = ctx.download("VX_TRACE")[0].reshape(T, n), ctx.download("VXX_TRACE")[0].reshape(T, n, n).transpose(0, 2, 1)
        stat = ctx.download("BOX_STAT")[0].reshape(T, 2)
    U = us.reshape(T, m)
    nclamped = 0
    for t in range(T - 1, -1, -1):
        Vx = d["lfx"][:n] if t == T - 1 else Vx_dev[t + 1]
        Vxx = cb.mat(d["lfxx"], 0, n, n) if t == T - 1 else Vxx_dev[t + 1]
        bl, bh = lo[t] - U[t], hi[t] - U[t]
        r = cb.yard_step(t, n, m, ne, Epre, d, mults, Vx, Vxx, 0.0, 10.0, bl, bh, True)
        assert r is not None, t
        c_dev = np.all(K_dev[t] == 0.0, axis=1)
        assert stat[t][0] == c_dev.sum() and stat[t][1] < cb.MAX_ITER, (t, stat[t])
        assert np.all(k_dev[t] >= bl) and np.all(k_dev[t] <= bh), t
        assert np.array_equal(c_dev, r["c"]) or r["margin"] < cb.INDECISIVE, (t, r["margin"])
        if np.array_equal(c_dev, r["c"]):
            nclamped += int(c_dev.sum())
            worst = max(rel_err(k_dev[t], r["k"]), rel_err(K_dev[t], r["K"]), rel_err(Vx_dev[t], r["Vx"]), rel_err(Vxx_dev[t], r["Vxx"]))
            assert worst <= 1e-10, (t, worst)
    assert nclamped > T


@pytest.mark.gpu
def test_no_box_sweep_at_58_joints(gpu):
    """... and from nv = 58 (168 904 B) the sweep with control bounds answers E_UNSUPPORTED the same way"""
    capi = gpu
    T = 2
    _, spec, _ = robots.problem("tree58", T, batch=1)
    with capi.Context(spec, flags=capi.FLAG_CONTROL_BOUNDS | capi.FLAG_NO_TENSORS) as ctx:
        assert_info(ctx, "tree58")
        ctx.set_control_bounds(lo=-1.0, hi=1.0)
        ctx.fill("FB_VAL", 7.0)
        with pytest.raises(capi.DdpHipError) as ei:
            ctx.backward(0.0, 1.0)
        assert ei.value.code == capi.E_UNSUPPORTED
        assert np.all(ctx.download("FB_VAL") == 7.0)
    # without bounds the same robot sweeps: the limit is the box QP's
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        assert_info(ctx, "tree58")
        d, xs, us, mults = synth_sweep_inputs(T, 58, [0] * T, seed=2, tensors=False)
        upload_sweep_inputs(ctx, d, xs, us, mults, 0, tensors=False)
        rc, reg, mu, restarts = ctx.backward(0.0, 10.0)
        assert rc == 0 and restarts[0] == 0
