"""Joint armature (reflected rotor inertia; ddp_hip_set_armature / ddp_hip_get_armature / ddp_hip_model_set_armature, ddp_hip.h):

    qdd = (M(q) + diag(a))^-1 (tau - h(q, v)),   h = RNEA(q, v, 0);   in the ABA: D_i = S_i^T IA_i S_i + a_i and nothing else.

The yardstick is the unchanged oracle's pieces: solve(crba(q) + diag(a), tau - rnea(q, v, 0)) and rnea_derivatives at that
acceleration.  Tolerances that compare against it are measured at a = 0 in the test itself (e0: the same formula against the
device's zero-armature value, which the existing tests pin to the oracle) and allowed 10 max(e0, 1e-13): the two sides share no
operation order, and diag(a) only improves the conditioning.  The armature values are large (0, 0.5 .. 2 and once 10 times
M_ii(q0)), and every comparison also asserts that the quantity moved by more than 1e-3 relative from its zero-armature value, so
an implementation that ignores the values cannot pass.  Shapes: T = 2 .. 6, batch 1 .. 2.
[measured on an MI355X: DESIGN.md, section "Armature"]"""
import os
import re

import numpy as np
import pytest

import robots
import test_tracking_cost as tc
from problems import held_trajectory, make, random_state
from synth import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, E1, E2 = 2.220446049250313e-16, 1.4901161193847656e-08, 1.220703125e-04
H = 1e-3
W5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
LIN = ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU")
SWITCHES = ("DDP_HIP_NO_STATIC", "DDP_HIP_NO_QCACHE", "DDP_HIP_CFG_FULL_ABA", "DDP_HIP_QCACHE_DENSE", "DDP_HIP_VCACHE_DENSE",
            "DDP_HIP_LIN_SERIAL", "DDP_HIP_LIN_FORKS", "DDP_HIP_K3_NO_PACK", "DDP_HIP_FXX_FULL", "DDP_HIP_K3_NO_SYM", "DDP_HIP_QWS_BT",
            "DDP_HIP_FWD_NO_PIPE", "DDP_HIP_ANA_OWN_ABA", "DDP_HIP_ANA_SPLIT", "DDP_HIP_ANA_EQ_KERNEL")
MOVED = 1e-3


# ---- problems and the yardstick --------------------------------------------------------------------------------------------
def problem(name, T, batch=1, fd_mode=2, first_order_fd=1):
    """(model, spec, oracle): a built-in problem of problems.make, "free6" (chain6 without its constraint) or a catalogue robot"""
    if name in robots.CATALOGUE:
        return robots.problem(name, T, batch=batch, fd_mode=fd_mode, first_order_fd=first_order_fd)
    if name == "free6":
        from ddp_pinocchio_amd import capi
        from oracle.binding import Oracle
        model = capi.BuiltinModel(capi.BUILTIN_CHAIN6)
        kw = dict(dt=0.01, c=1.0, fd_mode=fd_mode, first_order_fd=first_order_fd, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
        return model, capi.ProblemSpec(model, T, batch=batch, **kw), Oracle(model, T, **kw)
    return make(name, T, batch=batch, fd_mode=fd_mode, first_order_fd=first_order_fd)


def armature_for(o, model, q0=None):
    """[nv]: joint k (counted without a free-flyer root's six rows) gets (0, 0.5, 1, 2)[k % 4] M_ii(q0), the last joint 10 M_ii(q0)"""
    q0 = o.neutral() if q0 is None else q0
    d = np.diag(o.crba(q0))
    first = 6 if model.ff else 0
    a = np.zeros(o.nv)
    for k, i in enumerate(range(first, o.nv)):
        a[i] = (0.0, 0.5, 1.0, 2.0)[k % 4] * d[i]
    a[o.nv - 1] = 10.0 * d[o.nv - 1]
    assert np.all(a[:first] == 0.0) and np.sum(a == 0.0) > first and np.all(a >= 0.0)
    return a


def ref_aba(o, a, q, v, tau):
    return np.linalg.solve(o.crba(q) + np.diag(a), tau - o.rnea(q, v, np.zeros(o.nv)))


def ref_eval_f(o, a, x, u):
    """eval_to on a vector-space model with the reference forward dynamics"""
    nv, dt = o.nv, o.p.dt
    return np.concatenate([x[:nv] + dt * x[nv:], x[nv:] + dt * ref_aba(o, a, x[:nv], x[nv:], u)])


def ref_first_order(o, a, x, u):
    """the velocity rows of (f_x, f_u): dt [-(M+A)^-1 dtau/dq | -(M+A)^-1 dtau/dv] + [0 | I], dt (M+A)^-1, dtau at the armature
    dynamics' acceleration"""
    nv, dt = o.nv, o.p.dt
    q, v = x[:nv], x[nv:]
    dq, dv, M = o.rnea_derivatives(q, v, ref_aba(o, a, q, v, u))
    Minv = np.linalg.inv(M + np.diag(a))
    return np.hstack([-dt * Minv @ dq, np.eye(nv) - dt * Minv @ dv]), dt * Minv


def moved(a, b):
    """how far a is from its zero-armature value b: the largest entry-wise relative change over the entries of b that are not
    negligible beside its largest (the models' inertias span five decades, a change of the root's entries would drown in a
    norm-wise measure)"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    live = np.abs(b) > 1e-6 * np.max(np.abs(b))
    return float(np.max(np.abs(a[live] - b[live]) / np.abs(b[live])))


def _mat(flat, t, r, c):
    return flat[t * r * c:(t + 1) * r * c].reshape(c, r).T


def _trajs(o, model, B, seed, u_sigma=0.3):
    trs = [held_trajectory(o, model, seed=seed + b, u_sigma=u_sigma) for b in range(B)]
    return np.stack([tr[2] for tr in trs]), np.stack([tr[1] for tr in trs])


def _clear(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _linearize(capi, monkeypatch, spec, X, U, a, env=(), flags=0, seqs=LIN):
    """the outputs of one linearisation in a context created under the switches `env`, armature a (None: never set)"""
    _clear(monkeypatch)
    for k in env:
        monkeypatch.setenv(k, "1")
    try:
        with capi.Context(spec, flags=flags) as ctx:
            for k in env:
                monkeypatch.delenv(k)
            if a is not None:
                ctx.set_armature(a)
            ctx.upload("X", X); ctx.upload("U", U)
            ctx.linearize()
            out = {s: ctx.download(s) for s in seqs if ctx.seq_size(s)}
            out["lin_path"] = ctx.info()["lin_path"]
    finally:
        _clear(monkeypatch)
    return out


# ---- 12: CPU ---------------------------------------------------------------------------------------------------------------
def test_interface():
    """the three symbols are declared, exported and in capi.EXPORTS, the ABI stays 3, the wrappers exist, and a wrong length is
    refused before any device call (ProblemSpec, and the set calls of objects that have no handle)"""
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    L = capi.lib()
    for name in ("ddp_hip_set_armature", "ddp_hip_get_armature", "ddp_hip_model_set_armature"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    for cls, names in ((capi.Context, ("set_armature", "get_armature")), (capi.ModelHandle, ("set_armature",))):
        for name in names:
            assert hasattr(cls, name), name
    model = capi.BuiltinModel(capi.BUILTIN_CHAIN6)
    assert capi.ProblemSpec(model, 3).armature is None
    assert np.array_equal(capi.ProblemSpec(model, 3, armature=np.arange(6.0)).armature, np.arange(6.0))
    for bad in (np.zeros(5), np.zeros(7), np.zeros((2, 6)), 1.0):
        with pytest.raises(ValueError):
            capi.ProblemSpec(model, 3, armature=bad)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = capi.ProblemSpec(model, 3), 1, None
    h = capi.ModelHandle.__new__(capi.ModelHandle)
    h.model, h.nv, h.nq, h._h = model, 6, 6, None
    for obj in (ctx, h):
        with pytest.raises(ValueError):
            obj.set_armature(np.zeros(5))


def test_yardstick_zero_armature():
    """the reference formula at a = 0 is the oracle's own aba (1e-12), on every model of this file: a check of the oracle alone"""
    for name in ("chain6", "tree38", "tree21", "chain6ff"):
        model, _, o = problem(name, 2)
        rng = np.random.default_rng(3)
        for _ in range(3):
            x = random_state(model, rng, 0.7)
            q, v, tau = x[:o.nq], x[o.nq:], 2.0 * rng.normal(size=o.nv)
            assert rel_err(ref_aba(o, np.zeros(o.nv), q, v, tau), o.aba(q, v, tau)) < 1e-12, name


# ---- 1: forward dynamics against the oracle's pieces ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "tree38", "tree21", "chain6ff"])
def test_aba_against_oracle_pieces(gpu, name):
    """ModelHandle.aba after set_armature against solve(crba + diag(a), tau - rnea(q, v, 0)) at random (q, v, tau); e0: the same
    formula at a = 0 against the zero-armature handle; bound 10 max(e0, 1e-13).  (The oracle's crba and rnea cover the
    free-flyer model: test_yardstick_zero_armature.)"""
    capi = gpu
    model, _, o = problem(name, 2)
    a = armature_for(o, model)
    rng = np.random.default_rng(11)
    e0 = ea = 0.0
    mv = np.inf
    with capi.ModelHandle(model) as h0, capi.ModelHandle(model) as h:
        h.set_armature(a)
        for _ in range(4):
            x = random_state(model, rng, 0.7)
            q, v, tau = x[:o.nq], x[o.nq:], 2.0 * rng.normal(size=o.nv)
            base = h0.aba(q, v, tau)
            got = h.aba(q, v, tau)
            e0 = max(e0, rel_err(base, ref_aba(o, np.zeros(o.nv), q, v, tau)))
            ea = max(ea, rel_err(got, ref_aba(o, a, q, v, tau)))
            mv = min(mv, moved(got, base))
    bound = 10.0 * max(e0, 1e-13)
    print(f"aba {name}: e0 {e0:.3e} error with armature {ea:.3e} bound {bound:.3e} moved {mv:.3e}")
    assert ea <= bound, (ea, bound)
    assert mv > MOVED


# ---- 2: an exact physical equivalent ----------------------------------------------------------------------------------------
def _with_root_inertia(capi, model, a0):
    """the model with a0 n n^T, n the root joint's axis, added to the root link's rotational inertia"""
    Ic = np.array(model.Ic, dtype=np.float64)
    n = np.asarray(model.axis[0], dtype=np.float64)
    Ic[0] = Ic[0] + a0 * np.outer(n, n)
    return capi.TableModel(model.parent, model.jtype, model.axis, model.Rp, model.pp, model.mass_j, model.com, Ic, gravity=tuple(model.gravity))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["free6", "tree21"])
def test_root_armature_is_link_inertia(gpu, name):
    """armature a on a root revolute joint of a fixed-base model is the mechanics of a n n^T added to that link's rotational
    inertia (its angular velocity is along n: no bias term changes): aba, a rollout and the analytic FX / FU of the two contexts
    agree to 1e-10 relative, and differ from the plain model's by more than 1e-3"""
    capi = gpu
    T, B = 4, 2
    model, spec, o = problem(name, T, batch=B, fd_mode=0, first_order_fd=0)
    assert model.parent[0] == -1 and model.jtype[0] == capi.JOINT_REVOLUTE
    a = np.zeros(o.nv)
    a[0] = 2.0 * o.crba(o.neutral())[0, 0]
    heavy = _with_root_inertia(capi, model, a[0])
    spec_h = capi.ProblemSpec(heavy, T, dt=spec.dt, c=spec.c, batch=B, fd_mode=0, first_order_fd=0)
    rng = np.random.default_rng(21)
    with capi.ModelHandle(model) as h0, capi.ModelHandle(model) as ha, capi.ModelHandle(heavy) as hh:
        ha.set_armature(a)
        for _ in range(3):
            x = random_state(model, rng, 0.7)
            q, v, tau = x[:o.nq], x[o.nq:], 2.0 * rng.normal(size=o.nv)
            assert rel_err(ha.aba(q, v, tau), hh.aba(q, v, tau)) < 1e-10
            assert moved(ha.aba(q, v, tau), h0.aba(q, v, tau)) > MOVED
    X, U = _trajs(o, model, B, 22)
    Xn = np.full_like(X, np.nan); Xn[:, :o.nx] = X[:, :o.nx]
    out = {}
    for tag, sp, arm in (("plain", spec, None), ("armature", spec, a), ("inertia", spec_h, None)):
        with capi.Context(sp, flags=capi.FLAG_NO_TENSORS) as ctx:
            if arm is not None:
                ctx.set_armature(arm)
            ctx.upload("X", Xn); ctx.upload("U", U)
            ctx.rollout()
            roll = ctx.download("X")
            ctx.upload("X", X)
            ctx.linearize()
            assert ctx.info()["first_order"] == 2
            out[tag] = {"X": roll, "FX": ctx.download("FX"), "FU": ctx.download("FU"), "F_VAL": ctx.download("F_VAL")}
    for s in ("X", "FX", "FU", "F_VAL"):
        e = rel_err(out["armature"][s], out["inertia"][s])
        mv = moved(out["armature"][s], out["plain"][s])
        print(f"equivalent {name} {s}: {e:.3e}, moved {mv:.3e}")
        assert np.all(np.isfinite(out["inertia"][s])) and e < 1e-10, (s, e)
        if s in ("FX", "FU"):
            assert mv > MOVED, (s, mv)
    # (the rolled-out states: the velocities of a 4-step rollout move by dt * the change of the accelerations)
    nv = o.nv
    va, vp = (out[k]["X"].reshape(B, T + 1, o.nx)[:, 1:, nv:] for k in ("armature", "plain"))
    assert moved(va, vp) > MOVED


# ---- 3: analytic first order ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode", [("chain6", 0), ("tree38", 0), ("tree38", 1), ("tree21", 0)])
def test_analytic_first_order(gpu, monkeypatch, name, fd_mode):
    """first_order_fd = 0: the velocity rows of FX / FU against the oracle's rnea_derivatives at the armature dynamics'
    acceleration; e0 the same comparison at a = 0, bound 10 max(e0, 1e-13) relative.  chain6: the one-lane variant, tree38 and
    tree21: the wave-per-evaluation kernels (tree38 in mode 1 the fused pass with M^-1 in LDS)"""
    capi = gpu
    T = 3
    model, spec, o = problem(name, T, fd_mode=fd_mode, first_order_fd=0)
    a = armature_for(o, model)
    X, U = _trajs(o, model, 1, 31)
    flags = capi.FLAG_NO_TENSORS if fd_mode == 0 else 0
    nv, n, m = o.nv, o.n, o.m
    errs = {}
    got = {}
    for tag, arm in (("zero", np.zeros(nv)), ("armature", a)):
        got[tag] = _linearize(capi, monkeypatch, spec, X, U, None if tag == "zero" else arm, flags=flags, seqs=("F_VAL", "FX", "FU"))
        ex = ef = ev = 0.0
        for t in range(T):
            x, u = X[0].reshape(T + 1, o.nx)[t], U[0].reshape(T, m)[t]
            rx, ru = ref_first_order(o, arm, x, u)
            fx, fu = _mat(got[tag]["FX"][0], t, n, n), _mat(got[tag]["FU"][0], t, n, m)
            ex = max(ex, rel_err(fx[nv:], rx)); ef = max(ef, rel_err(fu[nv:], ru))
            ev = max(ev, rel_err(got[tag]["F_VAL"][0][t * o.nx:(t + 1) * o.nx], ref_eval_f(o, arm, x, u)))
            assert np.array_equal(fx[:nv], np.hstack([np.eye(nv), o.p.dt * np.eye(nv)])) and not np.any(fu[:nv])
        errs[tag] = (ex, ef, ev)
    for k, s in enumerate(("FX", "FU", "F_VAL")):
        bound = 10.0 * max(errs["zero"][k], 1e-13)
        mv = moved(got["armature"][s], got["zero"][s])
        print(f"analytic {name} mode {fd_mode} {s}: e0 {errs['zero'][k]:.3e} with armature {errs['armature'][k]:.3e} bound {bound:.3e} moved {mv:.3e}")
        assert errs["armature"][k] <= bound, (s, errs["armature"][k], bound)
        if s != "F_VAL":
            assert mv > MOVED, (s, mv)


@pytest.mark.gpu
def test_analytic_first_order_free_flyer(gpu, monkeypatch):
    """chain6 on a free-flyer root: FX / FU (first_order_fd = 0) and ModelHandle.aba_derivatives against 5-point central
    differences (H = 1e-3) of the device's own aba with armature along integrate, at the 1e-8 max(1, |.|) test_ff_analytic.py
    uses for that comparison; d qdd / d tau against inv(crba + diag(a)) at that file's 1e-12 cond bound"""
    capi = gpu
    T = 3
    model, spec, o = problem("chain6ff", T, fd_mode=0, first_order_fd=0)
    a = armature_for(o, model)
    X, U = _trajs(o, model, 1, 35)
    nv, nq, n, m, dt = o.nv, o.nq, o.n, o.m, o.p.dt
    got = _linearize(capi, monkeypatch, spec, X, U, a, flags=capi.FLAG_NO_TENSORS, seqs=("FX", "FU"))
    zero = _linearize(capi, monkeypatch, spec, X, U, None, flags=capi.FLAG_NO_TENSORS, seqs=("FX", "FU"))
    with capi.ModelHandle(model) as h:
        h.set_armature(a)
        for t in (0, T - 1):
            x, u = X[0].reshape(T + 1, o.nx)[t], U[0].reshape(T, m)[t]
            q, v = x[:nq], x[nq:]
            dq, dv = np.zeros((nv, nv)), np.zeros((nv, nv))
            for j in range(nv):
                e = np.zeros(nv); e[j] = 1.0
                dq[:, j] = sum(c * h.aba(o.integrate(q, s * H * e), v, u) for s, c in W5) / H
                dv[:, j] = sum(c * h.aba(q, v + s * 100 * H * e, u) for s, c in W5) / (100 * H)
            MA = o.crba(q) + np.diag(a)
            Minv = np.linalg.inv(MA)
            gq, gv, gt = h.aba_derivatives(q, v, u)
            fx, fu = _mat(got["FX"][0], t, n, n), _mat(got["FU"][0], t, n, m)
            for what, g, r in (("dq", gq, dq), ("dv", gv, dv), ("fx q", fx[nv:, :nv], dt * dq), ("fx v", fx[nv:, nv:], np.eye(nv) + dt * dv)):
                err = float(np.max(np.abs(g - r)))
                print(f"free flyer t {t} {what}: {err:.3e} scale {max(1.0, float(np.max(np.abs(r)))):.3e}")
                assert err <= 1e-8 * max(1.0, float(np.max(np.abs(r)))), (what, err)
            for what, g, r in (("dtau", gt, Minv), ("fu", fu[nv:], dt * Minv)):
                assert float(np.max(np.abs(g - r))) <= 1e-12 * np.linalg.cond(MA) * max(1.0, float(np.max(np.abs(r)))), what
    for s in ("FX", "FU"):
        assert moved(got[s], zero[s]) > MOVED, s


# ---- 4: FD first order against analytic -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "tree38", "tree21", "chain6ff"])
def test_fd_first_order_against_analytic(gpu, monkeypatch, name):
    """first_order_fd = 1 against first_order_fd = 0, armature set.  test_analytic_derivs.py holds each side to the oracle (1e-10
    the analytic one) and has no direct comparison of the two; the bound here is the forward difference's own error about the
    exact jacobian, written down: truncation eps / 2 * max|f_xx| (eps = E1; f_xx from this context's mode-2 tensors) plus the
    rounding 8 EPS fscale / E1 that test_dynamics_parity.py allows an FD jacobian, both times 2"""
    capi = gpu
    T = 2
    model, spec_fd, o = problem(name, T, fd_mode=2, first_order_fd=1)
    _, spec_an, _ = problem(name, T, fd_mode=0, first_order_fd=0)
    a = armature_for(o, model)
    X, U = _trajs(o, model, 1, 41)
    fd = _linearize(capi, monkeypatch, spec_fd, X, U, a)
    an = _linearize(capi, monkeypatch, spec_an, X, U, a, flags=capi.FLAG_NO_TENSORS, seqs=("F_VAL", "FX", "FU"))
    fscale = max(1.0, float(np.max(np.abs(an["F_VAL"]))))
    curv = max(float(np.max(np.abs(fd[s]))) for s in ("FXX", "FUX", "FUU"))
    tol = 2.0 * (0.5 * E1 * curv + 8 * EPS * fscale / E1)
    for s in ("FX", "FU"):
        err = float(np.max(np.abs(fd[s] - an[s])))
        print(f"fd against analytic {name} {s}: {err:.3e} tolerance {tol:.3e} (curvature {curv:.3e})")
        assert np.all(np.isfinite(fd[s])) and err <= tol, (s, err, tol)
    assert rel_err(fd["F_VAL"], an["F_VAL"]) < 1e-12


# ---- 5: every stencil path agrees with the monolithic one -------------------------------------------------------------------
BITWISE = (("DDP_HIP_QCACHE_DENSE",), ("DDP_HIP_VCACHE_DENSE",), ("DDP_HIP_LIN_SERIAL",))
NOISE = (("DDP_HIP_NO_STATIC",), ("DDP_HIP_NO_QCACHE",), ("DDP_HIP_NO_STATIC", "DDP_HIP_NO_QCACHE"))


def _qq_split(fxx, T, n, nv):
    """(the (q, q) block, the tensor with that block zeroed) of f_xx [t][k][j][i]"""
    f = fxx.reshape(-1, T, n, n, n).copy()
    qq = f[:, :, :nv, :nv, :].copy()
    f[:, :, :nv, :nv, :] = 0.0
    return qq, f


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode", [("chain6", 2), ("tree38", 2), ("chain6", 1), ("tree38", 1), ("tree21", 2)])
def test_stencil_paths_agree(gpu, monkeypatch, name, fd_mode):
    """With armature set, F_VAL, FX, FU, FXX, FUX, FUU of the default context against contexts created under each development
    switch, by the criterion of that pair's own A/B test:
      QCACHE_DENSE, VCACHE_DENSE, LIN_SERIAL   bit for bit (test_sparse_caches.py, test_sparse_vcache.py, test_lin_overlap.py)
      CFG_FULL_ABA                             bit for bit but the (q, q) block of f_xx, that within the finite-difference noise
                                               bound 64 EPS fscale / E2^2 + 4 (8 EPS fscale / E1) / E2 (test_cfg_splice.py)
      NO_STATIC                                mode 2: F_VAL bit for bit, first order 32 EPS fscale / E1, second order 64 EPS fscale /
                                               E2^2 + 4 tol1 / E2, each times max(1, |reference|) (test_dynamics_parity.py); mode 1
                                               (analytic jacobians, the accelerations of the perturbed points from the static kernels
                                               or not): FX 1e-12 relative, FU and FUU bit for bit, FXX / FUX 8 EPS cond jscale / E1
                                               (test_analytic_derivs.py: test_mode1_static_accelerations_against_own_forward_dynamics)
      NO_QCACHE, NO_STATIC + NO_QCACHE         no A/B test of their own: NO_STATIC's criterion (F_VAL to 32 EPS fscale).  The last is
                                               the monolithic leg, aba_tree per point, which test_aba_against_oracle_pieces pins
    tree21 runs on the run-time tree whatever the switches say: there NO_QCACHE is the caches against the monolithic ABA."""
    capi = gpu
    T, B = 2, 2
    fo = 0 if fd_mode == 1 else 1
    model, spec, o = problem(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    a = armature_for(o, model)
    X, U = _trajs(o, model, B, 51)
    nv, n = o.nv, o.n
    new = _linearize(capi, monkeypatch, spec, X, U, a)
    zero = _linearize(capi, monkeypatch, spec, X, U, None)
    for s in LIN[1:]:
        assert np.all(np.isfinite(new[s])), s
        if s != "FUU":                                                  # (f is affine in u: f_uu is rounding noise, in mode 1 exact zeros)
            assert moved(new[s], zero[s]) > MOVED, s
    fscale = max(1.0, float(np.max(np.abs(new["F_VAL"]))))
    for env in BITWISE:
        old = _linearize(capi, monkeypatch, spec, X, U, a, env=env)
        for s in LIN:
            assert np.array_equal(new[s], old[s]), (env, s, int(np.sum(new[s] != old[s])))
    old = _linearize(capi, monkeypatch, spec, X, U, a, env=("DDP_HIP_CFG_FULL_ABA",))
    for s in LIN:
        if s != "FXX":
            assert np.array_equal(new[s], old[s]), ("CFG_FULL_ABA", s)
    (qa, ra), (qb, rb) = _qq_split(new["FXX"], T, n, nv), _qq_split(old["FXX"], T, n, nv)
    assert np.array_equal(ra, rb)
    tol_qq = 64 * EPS * fscale / (E2 * E2) + 4 * (8 * EPS * fscale / E1) / E2
    print(f"paths {name} mode {fd_mode} CFG_FULL_ABA: (q, q) difference {float(np.max(np.abs(qa - qb))):.3e} bound {tol_qq:.3e}")
    assert float(np.max(np.abs(qa - qb))) <= tol_qq
    if fd_mode == 1:
        Xr = X[0].reshape(T + 1, o.nx)
        cond = max(float(np.linalg.cond(o.crba(Xr[t][:nv]) + np.diag(a))) for t in range(T))
    for env in NOISE:
        old = _linearize(capi, monkeypatch, spec, X, U, a, env=env)
        worst = {}
        for s in LIN:
            d, r = float(np.max(np.abs(new[s] - old[s]))), max(1.0, float(np.max(np.abs(old[s]))))
            worst[s] = d
            if fd_mode == 2:
                tol1 = 32 * EPS * fscale / E1
                tol2 = 64 * EPS * fscale / (E2 * E2) + 4 * tol1 / E2
                if s == "F_VAL":
                    assert np.array_equal(new[s], old[s]) if env == ("DDP_HIP_NO_STATIC",) else d <= 32 * EPS * fscale, (env, s, d)
                else:
                    assert d <= (tol1 if s in ("FX", "FU") else tol2) * r, (env, s, d)
            else:
                jscale = max(1.0, float(np.max(np.abs(old["FX"]))), float(np.max(np.abs(old["FU"]))))
                if s == "F_VAL":
                    assert d <= 32 * EPS * fscale, (env, s, d)
                elif s == "FX":
                    assert rel_err(new[s], old[s]) < 1e-12, (env, s)
                elif s in ("FU", "FUU"):
                    assert np.array_equal(new[s], old[s]), (env, s)
                else:
                    assert d <= 8 * EPS * cond * jscale / E1, (env, s, d, 8 * EPS * cond * jscale / E1)
        print(f"paths {name} mode {fd_mode} {'+'.join(e[8:] for e in env)}: lin_path {old['lin_path']} (default {new['lin_path']}) largest differences",
              {s: f"{v:.2e}" for s, v in worst.items()})


# ---- 6: a coarse check of the tensors' values -------------------------------------------------------------------------------
def np_stencil(o, a, x, u):
    """the mode-2 stencil (second_order_deriv_2: eps = DBL_EPSILON^(1/4), forward-differenced jacobians with eps = sqrt(DBL_EPSILON))
    over the reference dynamics, on a vector-space model: (fxx [k][j][i], fux [k = x][j = u][i], fuu [k][j][i])"""
    n, m = o.n, o.m
    z = np.concatenate([x, u])
    f = lambda zz: ref_eval_f(o, a, zz[:n], zz[n:])
    f0 = f(z)
    N = n + m
    J = np.zeros((N, n))
    for i in range(N):
        d = np.zeros(N); d[i] = E1
        J[i] = (f(z + d) - f0) / E1
    e2 = E2 * E2
    Tn = np.zeros((N, N, n))
    for i in range(N):
        d = np.zeros(N); d[i] = E2
        Tn[i, i] = 2.0 * (f(z + d) - f0 - E2 * J[i]) / e2
    for i in range(N):
        for j in range(i + 1, N):
            d = np.zeros(N); d[i] = E2; d[j] = E2
            val = 0.5 * (2.0 * (f(z + d) - f0 - E2 * J[i] - E2 * J[j]) / e2 - Tn[i, i] - Tn[j, j])
            Tn[i, j] = val; Tn[j, i] = val
    return Tn[:n, :n], Tn[:n, n:], Tn[n:, n:]


@pytest.mark.gpu
def test_tensor_values_coarse(gpu, monkeypatch):
    """chain6, T = 2: the numpy restatement of the mode-2 stencil over the reference formula against the device's tensors.  The
    tolerance is measured: e2 is the same numpy stencil at a = 0 against the zero-armature device (which equals the oracle
    there), the largest absolute difference over the three tensors; with armature 10 e2 is allowed"""
    capi = gpu
    T = 2
    model, spec, o = problem("free6", T, fd_mode=2, first_order_fd=1)
    a = armature_for(o, model)
    X, U = _trajs(o, model, 1, 61, u_sigma=0.05)
    n, m = o.n, o.m
    err = {}
    got = {}
    for tag, arm in (("zero", np.zeros(o.nv)), ("armature", a)):
        got[tag] = _linearize(capi, monkeypatch, spec, X, U, None if tag == "zero" else arm)
        worst = {"FXX": 0.0, "FUX": 0.0, "FUU": 0.0}
        for t in range(T):
            x, u = X[0].reshape(T + 1, o.nx)[t], U[0].reshape(T, m)[t]
            rxx, rxu, ruu = np_stencil(o, arm, x, u)
            dev = {"FXX": got[tag]["FXX"][0].reshape(T, n, n, n)[t], "FUX": got[tag]["FUX"][0].reshape(T, n, m, n)[t],
                   "FUU": got[tag]["FUU"][0].reshape(T, m, m, n)[t]}
            for s, r in (("FXX", rxx), ("FUX", rxu), ("FUU", ruu)):
                worst[s] = max(worst[s], float(np.max(np.abs(dev[s] - r))))
        err[tag] = worst
    e2, ea = max(err["zero"].values()), max(err["armature"].values())
    print(f"coarse: e2 {e2:.3e} with armature {ea:.3e} bound {10 * e2:.3e}; per tensor", err, "largest entries",
          {s: float(np.max(np.abs(got["armature"][s]))) for s in ("FXX", "FUX", "FUU")})
    assert e2 > 0.0 and ea <= 10.0 * e2, err
    for s in ("FXX", "FUX"):                                            # (f is affine in u: f_uu is rounding noise)
        assert moved(got["armature"][s], got["zero"][s]) > MOVED, s


# ---- 7: rollout and forward -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "tree38", "tree21", "chain6ff"])
def test_rollout_is_step_by_step_aba(gpu, name):
    """ddp_hip_rollout's X against a numpy integration that calls ModelHandle.aba (armature set) step by step, 1e-12 relative"""
    capi = gpu
    T, B = 5, 2
    model, spec, o = problem(name, T, batch=B, fd_mode=0)
    a = armature_for(o, model)
    X0, U = _trajs(o, model, B, 71)
    nq, nv, dt = o.nq, o.nv, o.p.dt
    Xn = np.full_like(X0, np.nan); Xn[:, :o.nx] = X0[:, :o.nx]
    out = {}
    for tag in ("zero", "armature"):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
            if tag == "armature":
                ctx.set_armature(a)
            ctx.upload("X", Xn); ctx.upload("U", U)
            ctx.rollout()
            out[tag] = ctx.download("X")
    ref = np.zeros_like(X0)
    with capi.ModelHandle(model) as h:
        h.set_armature(a)
        for b in range(B):
            x = X0[b, :o.nx].copy()
            ref[b, :o.nx] = x
            for t in range(T):
                acc = h.aba(x[:nq], x[nq:], U[b].reshape(T, nv)[t])
                q = o.integrate(x[:nq], dt * x[nq:]) if model.ff else x[:nq] + dt * x[nq:]
                x = np.concatenate([q, x[nq:] + acc * dt])
                ref[b, (t + 1) * o.nx:(t + 2) * o.nx] = x
    e = rel_err(out["armature"], ref)
    va, vz = (out[k].reshape(B, T + 1, o.nx)[:, 1:, nq:] for k in ("armature", "zero"))
    print(f"rollout {name}: {e:.3e}, velocities moved {moved(va, vz):.3e}")
    assert np.all(np.isfinite(out["armature"])) and e < 1e-12
    assert moved(va, vz) > MOVED


@pytest.mark.gpu
@pytest.mark.parametrize("n_alpha", [0, 4])
@pytest.mark.parametrize("name", ["free6", "chain6ff", "tree38"])
def test_forward_pipelined_against_plain(gpu, monkeypatch, name, n_alpha):
    """ddp_hip_forward (n_alpha = 4) and the open-loop rollout (n_alpha = 0) with armature set: a default context against one
    created under DDP_HIP_FWD_NO_PIPE, bit for bit.  chain6 and chain6 on a free flyer roll out one lane per candidate in both
    (the model table in LDS, armature with it); tree38 is where the pipelined latency kernel and its four-candidate form exist"""
    capi = gpu
    T, B = 3, 2
    model, spec, o = problem(name, T, batch=B, fd_mode=0)
    a = armature_for(o, model)
    X, U = _trajs(o, model, B, 81)
    rng = np.random.default_rng(82)
    fb_val, fb_jac = 0.1 * rng.normal(size=(B, T * o.m)), 0.1 * rng.normal(size=(B, T * o.m * o.n))
    out = {}
    for tag, env, arm in (("pipe", (), a), ("plain", ("DDP_HIP_FWD_NO_PIPE",), a), ("zero", (), None)):
        _clear(monkeypatch)
        for k in env:
            monkeypatch.setenv(k, "1")
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
            _clear(monkeypatch)
            if arm is not None:
                ctx.set_armature(arm)
            if name == "tree38":
                assert ctx.info()["fwd_path"] == 1
            if n_alpha == 0:
                Xn = np.full_like(X, np.nan); Xn[:, :o.nx] = X[:, :o.nx]
                ctx.upload("X", Xn); ctx.upload("U", U)
                ctx.rollout()
                out[tag] = {"X": ctx.download("X")}
            else:
                ctx.upload("X", X); ctx.upload("U", U); ctx.upload("X_NEW", X); ctx.upload("U_NEW", U)
                ctx.upload("FB_ORIGIN", X[:, :T * o.nx]); ctx.upload("FB_VAL", fb_val); ctx.upload("FB_JAC", fb_jac)
                rc, step, dcost = ctx.forward(1.0, n_alpha=n_alpha)
                out[tag] = {"X_NEW": ctx.download("X_NEW"), "U_NEW": ctx.download("U_NEW"), "step": step, "dcost": dcost, "rc": np.array(rc)}
    for s in out["pipe"]:
        assert np.all(np.isfinite(out["plain"][s])), s
        assert np.array_equal(out["pipe"][s], out["plain"][s]), s
    s = "X" if n_alpha == 0 else "X_NEW"
    assert not np.array_equal(out["pipe"][s], out["zero"][s])


# ---- 8: joint accelerations -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["free6", "tree38", "chain6ff"])
def test_joint_accel_cost_follows(gpu, name):
    """DDP_HIP_FLAG_JOINT_ACCEL_COST with armature set: ddp_hip_joint_accel returns ModelHandle.aba with armature along the
    trajectory (1e-12, test_joint_accel_cost.py's TOL_ABA), and the term's LX / LU match 5-point central differences (H = 1e-3
    and H / 2, extrapolated) of its own cost values (cost_seq_aug with the flag minus without, states stepped along integrate) at the 1e-8 max(1, |.|)
    that file holds its differenced yardstick to.  [tree38 with the stencil at H alone: LX off by 3.9e-5 at either target spread, scales
    1.5e3 and 76 -- the stencil's own H^4 term, not the residual's; the u directions at H: LU off by 7.1e-8 at a scale of 5.1, the
    rounding of costs of 5e4 over H]"""
    capi = gpu
    T, B = 3, 1
    model, spec, o = problem(name, T, batch=B, fd_mode=0, first_order_fd=0)
    a = armature_for(o, model)
    X, U = _trajs(o, model, B, 91)
    nq, nv, n, m = o.nq, o.nv, o.n, o.m
    rng = np.random.default_rng(92)
    flag = capi.FLAG_JOINT_ACCEL_COST | capi.FLAG_NO_TENSORS
    with capi.ModelHandle(model) as h, capi.ModelHandle(model) as h0, capi.Context(spec, flags=flag) as ctx, \
            capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as off:
        h.set_armature(a)
        for c in (ctx, off):
            c.set_armature(a)
            c.upload("X", X); c.upload("U", U); c.upload("X_NEW", X); c.upload("U_NEW", U)
        Xr, Ur = X[0].reshape(T + 1, o.nx), U[0].reshape(T, m)
        acc = np.stack([h.aba(Xr[t][:nq], Xr[t][nq:], Ur[t]) for t in range(T)])
        acc0 = np.stack([h0.aba(Xr[t][:nq], Xr[t][nq:], Ur[t]) for t in range(T)])
        got = ctx.joint_accel(0)[0]
        print(f"joint_accel {name}: {rel_err(got, acc):.3e}, moved {moved(got, acc0):.3e}")
        assert rel_err(got, acc) < 1e-12 and moved(got, acc0) > MOVED
        # (targets close to the accelerations: the differenced cost's rounding, 4 EPS |cost| / H, goes with the residual squared, the
        # gradient with the residual)
        aref = acc + 0.05 * np.maximum(1.0, np.abs(acc)) * rng.normal(size=acc.shape)
        w = rng.uniform(0.1, 2.0, size=acc.shape)
        ctx.set_joint_accel_cost(target=aref[None], weight=w[None])
        ctx.linearize(); off.linearize()
        lx = (ctx.download("LX")[0] - off.download("LX")[0]).reshape(T, n)
        lu = (ctx.download("LU")[0] - off.download("LU")[0]).reshape(T, m)

        def term(t, x, u):
            Xp, Up = X.copy(), U.copy()
            Xp[0, t * o.nx:(t + 1) * o.nx] = x; Up[0, t * m:(t + 1) * m] = u
            vals = []
            for c in (ctx, off):
                c.upload("X_NEW", Xp); c.upload("U_NEW", Up)
                c.cost_seq_aug(1, 1.0)
                vals.append(c.download("COSTS_NEW")[0][t])
            return vals[0] - vals[1]
        t = 1

        def d5(fun, h0=H):
            """the 5-point stencil at h0 and h0 / 2, extrapolated: the h^4 term cancels (on the Talos-like tree it is 4e-5 at H alone,
            whatever the residual: the fifth derivative of the squared accelerations)"""
            g1, g2 = (sum(cw * fun(s * h) for s, cw in W5) / h for h in (h0, h0 / 2))
            return (16.0 * g2 - g1) / 15.0
        gx, gu = np.zeros(n), np.zeros(m)
        for j in range(n):
            e = np.zeros(n); e[j] = 1.0
            step = lambda s: np.concatenate([o.integrate(Xr[t][:nq], s * e[:nv]) if model.ff else Xr[t][:nq] + s * e[:nv], Xr[t][nq:] + s * e[nv:]])
            gx[j] = d5(lambda s: term(t, step(s), Ur[t]))
        for j in range(m):
            e = np.zeros(m); e[j] = 1.0
            # (a is affine in u, the term a quadratic: the stencil is exact at any step, and at 100 H -- test_ff_analytic.py's step
            # for its exact directions -- the rounding of the differenced costs, which carry c/2 |u|^2 = 5e4 on the Talos-like tree, is
            # a hundredth: 7e-8 at H against an LU of 5)
            gu[j] = d5(lambda s: term(t, Xr[t], Ur[t] + s * e), 100 * H)
        for what, g, r in (("LX", lx[t], gx), ("LU", lu[t], gu)):
            err, scale = float(np.max(np.abs(g - r))), max(1.0, float(np.max(np.abs(r))))
            print(f"joint accel cost {name} {what}: {err:.3e} scale {scale:.3e}")
            assert np.max(np.abs(r)) > 0 and err <= 1e-8 * scale, (what, err, scale)


# ---- 9: whole solve ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_solve(gpu):
    """chain6 without constraints tracking a posture 0.05 rad away over T = 6 (weights 1e3 running, 1e5 at the end on q, 1 on v;
    c = 1e-3): ddp_hip_solve converges with and without armature (optimality below 1e-6); the two U differ by more than 1e-3
    relative; the zero-armature U replayed open loop under the armature dynamics costs strictly more tracking error than the
    armature-aware solution"""
    from ddp_pinocchio_amd import solver
    from oracle.binding import Oracle
    capi = gpu
    T = 6
    model = capi.BuiltinModel(capi.BUILTIN_CHAIN6)
    kw = dict(dt=0.01, c=1e-3, fd_mode=0, first_order_fd=0, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    spec, o = capi.ProblemSpec(model, T, batch=1, **kw), Oracle(model, T, **kw)
    X, U = _trajs(o, model, 1, 101, u_sigma=0.0)
    a = armature_for(o, model, X[0][:o.nq])
    rng = np.random.default_rng(102)
    posture = np.concatenate([X[0][:o.nq] + 0.05 * rng.normal(size=o.nv), np.zeros(o.nv)])
    ref = {"xref": np.tile(posture, (1, T + 1, 1)), "wx": np.tile(np.concatenate([np.full(o.nv, 1e3), np.ones(o.nv)]), (1, T + 1, 1)),
           "uref": np.zeros((1, T, o.m)), "wu": np.zeros((1, T, o.m))}
    ref["wx"][0, T, :o.nv] = 1e5
    res = {}
    for tag, arm in (("zero", None), ("armature", a)):
        with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
            if arm is not None:
                ctx.set_armature(arm)
            tc._setup(ctx, X, U)
            tc.upload_ref(ctx, ref)
            log = solver.solve(ctx, 100, 1e-6, 1.0, 0.0, 1e-1, 10.0)
            res[tag] = (bool(log["done"][0]), int(log["iterations"][0]), float(log["opt_obj"][0]), ctx.download("X")[0], ctx.download("U")[0])
    print("whole solve (done, iterations, opt_obj): zero", res["zero"][:3], "armature", res["armature"][:3])
    assert res["zero"][0] and res["armature"][0]
    du = moved(res["armature"][4], res["zero"][4])
    assert du > MOVED, du
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        ctx.set_armature(a)
        Xn = np.full_like(X, np.nan); Xn[:, :o.nx] = X[:, :o.nx]
        ctx.upload("X", Xn); ctx.upload("U", res["zero"][4][None])
        ctx.rollout()
        replay = ctx.download("X")[0]
    track = {k: float(tc.track_terms(o, kw["c"], x, u, ref).sum()) for k, (x, u) in
             (("replay", (replay, res["zero"][4])), ("aware", (res["armature"][3], res["armature"][4])), ("zero", (res["zero"][3], res["zero"][4])))}
    total = {k: float(tc.full_cost(o, kw["c"], x, u, ref).sum()) for k, (x, u) in
             (("replay", (replay, res["zero"][4])), ("aware", (res["armature"][3], res["armature"][4])))}
    print("tracking cost", track, "total", total, "U differ", du)
    assert track["replay"] > track["aware"] and total["replay"] > total["aware"]


# ---- 10: zero is nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "tree38"])
def test_zero_is_nothing(gpu, name):
    """linearise, backward, forward and ddp_hip_solve at T = 2 on three contexts -- a fresh one, one after set_armature(zeros),
    one after set_armature(non-zero) then set_armature(zeros) -- give the same bits in every sequence"""
    capi = gpu
    T, B, mu = 2, 2, 10.0
    model, spec, o = problem(name, T, batch=B, fd_mode=2)
    a = armature_for(o, model)
    X, U = _trajs(o, model, B, 111)
    mults = tc._mults(o, X[0], 112)
    seqs = ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU", "LX", "LU", "LXX", "LUX", "LUU", "EQ_VAL", "EQ_X", "EQ_U", "EQ_XX", "EQ_UX", "EQ_UU")
    runs = []
    for how in ("fresh", "zeros", "set then zeros"):
        with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
            if how != "fresh":
                if how == "set then zeros":
                    ctx.set_armature(a)
                    tc._setup(ctx, X, U, mults, o.Etot)
                    ctx.linearize()                          # (the non-zero values were in force for a whole linearisation)
                ctx.set_armature(np.zeros(o.nv))
                assert not np.any(ctx.get_armature())
            tc._setup(ctx, X, U, mults, o.Etot)
            ctx.linearize()
            out = {s: ctx.download(s) for s in seqs if ctx.seq_size(s)}
            rc, reg, mu_o, restarts = ctx.backward(0.0, mu)
            out.update(rc_b=np.array(rc), reg=reg, mu=mu_o, restarts=restarts)
            for s in ("FB_VAL", "FB_JAC", "VX_TRACE", "VXX_TRACE"):
                out[s] = ctx.download(s)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=4)
            out.update(rc_f=np.array(rc), step=step, dcost=dcost, X_NEW=ctx.download("X_NEW"), U_NEW=ctx.download("U_NEW"))
            tc._setup(ctx, X, U, mults, o.Etot)
            _, log = ctx.solve(3, 1e-9, mu, 0.0, 1e-1, 10.0, n_alpha=4)
            out.update(X=ctx.download("X"), U=ctx.download("U"), **{"log_" + k: np.asarray(v) for k, v in log.items()})
            runs.append(out)
    for k in runs[0]:
        if k in ("F_VAL", "FX", "FXX", "FB_JAC", "X_NEW", "X", "U"):
            assert np.all(np.isfinite(runs[0][k])), k
        for other in runs[1:]:
            assert np.array_equal(runs[0][k], other[k], equal_nan=True), k


# ---- 11: refusals and persistence -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_and_persistence(gpu, monkeypatch):
    capi = gpu
    T = 2
    model, spec, o = problem("chain6", T, fd_mode=2)
    a = armature_for(o, model)
    X, U = _trajs(o, model, 1, 121)
    with capi.Context(spec) as ctx, capi.ModelHandle(model) as h:
        assert not np.any(ctx.get_armature())
        ctx.set_armature(a)
        assert np.array_equal(ctx.get_armature(), a)
        for bad in (None, np.where(np.arange(6) == 2, np.nan, a), np.where(np.arange(6) == 4, np.inf, a), np.where(np.arange(6) == 1, -1e-9, a)):
            for obj, where in ((ctx, "set_armature"), (h, "model_set_armature")):
                with pytest.raises(capi.DdpHipError) as ei:
                    obj.set_armature(bad)
                assert ei.value.code == capi.E_ARG, (where, bad)
            assert np.array_equal(ctx.get_armature(), a)              # a refused call leaves the old values in force
        # a second set between two linearisations takes effect on the second
        ctx.upload("X", X); ctx.upload("U", U)
        ctx.linearize()
        first = {s: ctx.download(s) for s in LIN}
        ctx.set_armature(2.0 * a)
        assert np.array_equal(ctx.get_armature(), 2.0 * a)
        ctx.linearize()
        second = {s: ctx.download(s) for s in LIN}
    twice = _linearize(capi, monkeypatch, spec, X, U, 2.0 * a)
    once = _linearize(capi, monkeypatch, spec, X, U, a)
    for s in LIN:
        assert np.array_equal(first[s], once[s]) and np.array_equal(second[s], twice[s]), s
    assert not np.array_equal(first["FX"], second["FX"])
    # ProblemSpec(armature=...) is applied right after create
    spec_a = capi.ProblemSpec(model, T, dt=spec.dt, c=spec.c, batch=1, eq_kind=spec.eq_kind, eq_advance=spec.eq_advance, ne=spec.ne,
                              eq_target=spec.eq_target, fd_mode=2, armature=a)
    with capi.Context(spec_a) as ctx:
        assert np.array_equal(ctx.get_armature(), a)
    # a free-flyer root's six rows carry none
    ffm, ffspec, ffo = problem("chain6ff", T, fd_mode=0)
    fa = armature_for(ffo, ffm)
    with capi.Context(ffspec, flags=capi.FLAG_NO_TENSORS) as ctx, capi.ModelHandle(ffm) as h:
        ctx.set_armature(fa); h.set_armature(fa)
        assert np.array_equal(ctx.get_armature(), fa)
        for row in (0, 5):
            bad = fa.copy(); bad[row] = 0.1
            for obj in (ctx, h):
                with pytest.raises(capi.DdpHipError) as ei:
                    obj.set_armature(bad)
                assert ei.value.code == capi.E_ARG
            assert np.array_equal(ctx.get_armature(), fa)
    # the pendulum's closed form is the reference's own
    pm, pspec, _ = problem("pendulum", 4, fd_mode=0)
    with capi.Context(pspec, flags=capi.FLAG_NO_TENSORS) as ctx, capi.ModelHandle(pm) as h:
        for call in (lambda: ctx.set_armature(np.zeros(1)), ctx.get_armature, lambda: h.set_armature(np.zeros(1))):
            with pytest.raises(capi.DdpHipError) as ei:
                call()
            assert ei.value.code == capi.E_UNSUPPORTED
    with pytest.raises(capi.DdpHipError) as ei:
        capi.Context(capi.ProblemSpec(pm, 4, fd_mode=0, armature=np.zeros(1)), flags=capi.FLAG_NO_TENSORS)
    assert ei.value.code == capi.E_UNSUPPORTED
