"""Analytic first order for free-flyer (SE(3) root) models: dynamics_t::first_order_deriv (problem.hpp:463-503) with
d_integrate_dq / dv on the root block and d_dynamics_aba in the tangent, for fd_mode 0 and 2, with and without the frame
constraint.

The yardstick.  The oracle's own first order falls back to forward differences for a free flyer, so the expected jacobians
are assembled here from oracle primitives: a 5-point central difference of Oracle.aba along q (+) (+-h e_j), +-2h (truncation
O(h^4) ~ 1e-12 at h = 1e-3), the same stencil along v (exact there: qdd is quadratic in v), inv(Oracle.crba) for d qdd/d tau, Oracle.d_integrate_dq / dv for the
configuration rows, Oracle.frame_jacobian (WORLD rows) chained through the look-ahead steps for the constraint."""
import numpy as np
import pytest

from problems import held_trajectory, initial_trajectory, make, random_state
from synth import rel_err

H = 1e-3
EPS = np.finfo(float).eps


def _aba_partials(o, q, v, tau, h=H):
    """(d qdd/dq, d qdd/dv) by 5-point central differences; q directions along integrate(q, s e_j).  qdd is quadratic in v,
    where the stencil is exact: the v steps are 100 h, which cuts the rounding term"""
    nv = o.nv
    dq, dv = np.zeros((nv, nv)), np.zeros((nv, nv))
    w = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for j in range(nv):
        e = np.zeros(nv); e[j] = 1.0
        dq[:, j] = sum(c * o.aba(o.integrate(q, s * h * e), v, tau) for s, c in w) / h
        dv[:, j] = sum(c * o.aba(q, v + s * 100 * h * e, tau) for s, c in w) / (100 * h)
    return dq, dv


def expected_first_order(o, x, u):
    """(f_x, f_u) as matrices, problem.hpp:463-503 on the group"""
    nq, nv, dt = o.nq, o.nv, o.p.dt
    q, v = x[:nq], x[nq:]
    daq, dav = _aba_partials(o, q, v, u)
    Minv = np.linalg.inv(o.crba(q))
    fx = np.zeros((2 * nv, 2 * nv)); fu = np.zeros((2 * nv, nv))
    fx[:nv, :nv] = o.d_integrate_dq(q, dt * v)
    fx[:nv, nv:] = dt * o.d_integrate_dv(q, dt * v)
    fx[nv:, :nv] = dt * daq
    fx[nv:, nv:] = np.eye(nv) + dt * dav
    fu[nv:, :] = dt * Minv
    return fx, fu


def expected_eq(o, x, u, joint, off, K):
    """(eq_x, eq_u) of the frame constraint through K look-ahead steps: C f_x(x_{K-1}) ... f_x(x_0), inner eq_n_u dropped"""
    nq, nv = o.nq, o.nv
    xs = [x]
    for _ in range(K):
        xs.append(o.eval_f(xs[-1], u))
    C = np.zeros((3, 2 * nv))
    C[:, :nv] = o.frame_jacobian(joint, off, xs[K][:nq])
    for k in range(K - 1, 0, -1):
        C = C @ expected_first_order(o, xs[k], u)[0]
    fx0, fu0 = expected_first_order(o, x, u)
    return C @ fx0, C @ fu0


def _mat(flat, t, r, c):
    return flat[t * r * c:(t + 1) * r * c].reshape(c, r).T


def _scale(a):
    return max(1.0, float(np.max(np.abs(a))))


# ---- the yardstick itself (CPU) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6ff", "tree38ff"])
def test_yardstick_converged(name):
    model, _, o = make(name, 2, first_order_fd=0)
    rng = np.random.default_rng(11)
    for _ in range(2):
        x = random_state(model, rng, 0.3)
        q, v, tau = x[:o.nq], x[o.nq:], rng.normal(size=o.nv)
        dq1, dv1 = _aba_partials(o, q, v, tau, H)
        dq2, dv2 = _aba_partials(o, q, v, tau, H / 2)
        assert np.max(np.abs(dq1 - dq2)) <= 1e-9 * _scale(dq1)
        assert np.max(np.abs(dv1 - dv2)) <= 1e-9 * _scale(dv1)
        Minv = np.linalg.inv(o.crba(q))
        assert np.max(np.abs(Minv @ o.crba(q) - np.eye(o.nv))) <= 1e-12 * np.linalg.cond(o.crba(q))


@pytest.mark.parametrize("name", ["chain6ff", "tree38ff"])
def test_yardstick_matches_oracle_fd(name):
    model, _, o = make(name, 2, first_order_fd=0)
    rng = np.random.default_rng(12)
    x = random_state(model, rng, 0.5)
    u = rng.normal(size=o.nv)
    fx, fu = expected_first_order(o, x, u)
    fx_fd, fu_fd, _ = o.first_order_f(x, u)         # the oracle's free-flyer fallback: forward differences
    n = o.n
    fx_fd = np.asarray(fx_fd).reshape(n, n).T if np.ndim(fx_fd) == 1 else fx_fd
    fu_fd = np.asarray(fu_fd).reshape(o.m, n).T if np.ndim(fu_fd) == 1 else fu_fd
    assert np.max(np.abs(fx - fx_fd)) <= 1e-6 * _scale(fx)
    assert np.max(np.abs(fu - fu_fd)) <= 1e-6 * _scale(fu)


# ---- device ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6ff", "tree38ff"])
def test_model_handle_aba_derivatives(gpu, name):
    capi = gpu
    model, _, o = make(name, 2, first_order_fd=0)
    rng = np.random.default_rng(21)
    with capi.ModelHandle(model) as h:
        for _ in range(3):
            x = random_state(model, rng, 0.7)
            q, v, tau = x[:o.nq], x[o.nq:], 2.0 * rng.normal(size=o.nv)
            dq, dv, dtau = h.aba_derivatives(q, v, tau)
            eq, ev = _aba_partials(o, q, v, tau)
            M = o.crba(q)
            assert np.max(np.abs(dq - eq)) <= 1e-8 * _scale(eq), np.max(np.abs(dq - eq))
            assert np.max(np.abs(dv - ev)) <= 1e-8 * _scale(ev), np.max(np.abs(dv - ev))
            Minv = np.linalg.inv(M)
            assert np.max(np.abs(dtau - Minv)) <= 1e-12 * np.linalg.cond(M) * _scale(Minv)


def _traj(o, model, B, seed):
    xs, us = [], []
    for b in range(B):
        _, u_, x_ = held_trajectory(o, model, seed=seed + b, q0_sigma=0.4)
        xs.append(x_); us.append(u_)
    return np.stack(xs), np.stack(us)


def _sample_ts(T):
    ts = sorted(set([0, T - 2, T - 1] + list(np.linspace(0, T - 1, 16).astype(int))))
    return ts


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B", [("chain6ff", 10, 1), ("chain6ff_frame", 10, 1), ("tree38ff", 200, 2), ("tree38ff_frame", 200, 2)])
def test_linearize_mode0(gpu, name, T, B):
    capi = gpu
    model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=0)
    _, spec_fd, _ = make(name, T, batch=B, fd_mode=0, first_order_fd=1)
    xs, us = _traj(o, model, B, 40)
    n, m = o.n, o.m
    out = {}
    for key, sp in (("ana", spec), ("fd", spec_fd)):
        with capi.Context(sp) as ctx:
            if key == "ana":
                assert ctx.info()["first_order"] == 2
            ctx.upload("X", xs); ctx.upload("U", us)
            ctx.linearize()
            out[key] = {s: ctx.download(s) for s in ("F_VAL", "FX", "FU", "EQ_VAL", "EQ_X", "EQ_U") if ctx.seq_size(s)}
    for s in ("F_VAL", "EQ_VAL"):
        if s in out["ana"]:
            assert np.array_equal(out["ana"][s], out["fd"][s]), s
    Etot = o.Etot
    for b in range(B):
        x_t = xs[b].reshape(T + 1, o.nx)
        u_t = us[b].reshape(T, m)
        for t in _sample_ts(T):
            fx, fu = expected_first_order(o, x_t[t], u_t[t])
            gx, gu = _mat(out["ana"]["FX"][b], t, n, n), _mat(out["ana"]["FU"][b], t, n, m)
            assert np.max(np.abs(gx - fx)) <= 1e-8 * _scale(fx), (t, np.max(np.abs(gx - fx)))
            assert np.max(np.abs(gu - fu)) <= 1e-8 * _scale(fu), (t, np.max(np.abs(gu - fu)))
        if Etot:
            t = T - 2
            ex, eu = expected_eq(o, x_t[t], u_t[t], spec.frame_joint, spec.frame_off, spec.eq_advance)
            got_x = out["ana"]["EQ_X"][b][:3 * n].reshape(n, 3).T
            got_u = out["ana"]["EQ_U"][b][:3 * m].reshape(m, 3).T
            assert np.max(np.abs(got_x - ex)) <= 1e-8 * _scale(ex), np.max(np.abs(got_x - ex))
            assert np.max(np.abs(got_u - eu)) <= 1e-8 * _scale(eu), np.max(np.abs(got_u - eu))


def _integrate_x(o, x, d):
    nq, nv = o.nq, o.nv
    return np.concatenate([o.integrate(x[:nq], d[:nv]), x[nq:] + d[nv:]])


def _difference_out(o, x0, x1):
    nq = o.nq
    return np.concatenate([o.difference(x0[:nq], x1[:nq]), x1[nq:] - x0[nq:]])


def _mode2_restated(o, f, x, u, J):
    """finite_diff_hessian_compute::second_order_deriv_2 (problem.hpp:152-298), J = [f_x | f_u] given; f(x, u) -> tangent rows
    via difference_out against f(x, u) (f_difference) or plain subtraction (vector-valued f)"""
    n, m = o.n, o.m
    W = n + m
    eps = np.sqrt(np.sqrt(EPS)); eps2 = eps * eps
    f0 = f(x, u)

    def at(dirs):
        d = np.zeros(n); uu = u.copy()
        for i in dirs:
            if i < n: d[i] += eps
            else: uu[i - n] += eps
        return f(_integrate_x(o, x, d), uu)
    diff = (lambda a, b: _difference_out(o, a, b)) if f0.size == o.nx else (lambda a, b: b - a)
    diag = [2 * (diff(f0, at([i])) - eps * J[:, i]) / eps2 for i in range(W)]
    R = f0.size if f0.size != o.nx else n
    full = np.zeros((R, W, W))
    for i in range(W):
        full[:, i, i] = diag[i]
        for j in range(i + 1, W):
            df = 2 * (diff(f0, at([i, j])) - eps * J[:, i] - eps * J[:, j])
            full[:, i, j] = full[:, j, i] = 0.5 * (df / eps2 - diag[i] - diag[j])
    return full


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6ff", "chain6ff_frame"])
def test_mode2_on_analytic_jacobians(gpu, name):
    capi = gpu
    T = 3
    model, spec, o = make(name, T, fd_mode=2, first_order_fd=0)
    _, spec_fd, _ = make(name, T, fd_mode=2, first_order_fd=1)
    _, us, xs = held_trajectory(o, model, seed=5, q0_sigma=0.4)
    us = us + 0.3 * np.random.default_rng(6).normal(size=us.size)
    xs = o.rollout(xs[:o.nx], us)
    n, m = o.n, o.m
    got = {}
    for key, sp in (("ana", spec), ("fd", spec_fd)):
        with capi.Context(sp) as ctx:
            ctx.upload("X", xs); ctx.upload("U", us)
            ctx.linearize()
            got[key] = {s: ctx.download(s)[0] for s in ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU", "EQ_VAL", "EQ_X", "EQ_U",
                                                         "EQ_XX", "EQ_UX", "EQ_UU") if ctx.seq_size(s)}
    g = got["ana"]
    assert not np.array_equal(g["FXX"], got["fd"]["FXX"])
    x_t = xs.reshape(T + 1, o.nx); u_t = us.reshape(T, m)
    for t in range(T):
        J = np.concatenate([_mat(g["FX"], t, n, n), _mat(g["FU"], t, n, m)], axis=1)
        full = _mode2_restated(o, o.eval_f, x_t[t], u_t[t], J)
        fscale = _scale(g["F_VAL"])
        tol = 64 * EPS * fscale / np.sqrt(EPS) + 1e-9 * _scale(J) / EPS ** 0.25
        fxx = g["FXX"][t * n * n * n:(t + 1) * n * n * n].reshape(n, n, n).transpose(2, 1, 0)
        fux = g["FUX"][t * n * n * m:(t + 1) * n * n * m].reshape(n, m, n).transpose(2, 1, 0)
        fuu = g["FUU"][t * n * m * m:(t + 1) * n * m * m].reshape(m, m, n).transpose(2, 1, 0)
        assert np.max(np.abs(fxx - full[:, :n, :n])) <= tol * max(1.0, _scale(full)), np.max(np.abs(fxx - full[:, :n, :n]))
        assert np.max(np.abs(fux - full[:, n:, :n])) <= tol * max(1.0, _scale(full)), np.max(np.abs(fux - full[:, n:, :n]))
        assert np.max(np.abs(fuu - full[:, n:, n:])) <= tol * max(1.0, _scale(full))
    if "EQ_X" in g:
        t = T - 2
        e = 3
        J = np.concatenate([g["EQ_X"][:e * n].reshape(n, e).T, g["EQ_U"][:e * m].reshape(m, e).T], axis=1)
        joint, off, K = spec.frame_joint, spec.frame_off, spec.eq_advance

        def eqf(x, u):
            xa = x
            for _ in range(K):
                xa = o.eval_f(xa, u)
            return o.frame_position(joint, off, xa[:o.nq]) - np.array([0.3, 0.2, 0.4])
        full = _mode2_restated(o, eqf, x_t[t], u_t[t], J)
        tol = 64 * EPS * max(1.0, np.max(np.abs(g["EQ_VAL"]))) / np.sqrt(EPS) + 1e-9 * _scale(J) / EPS ** 0.25
        exx = g["EQ_XX"][:e * n * n].reshape(n, n, e).transpose(2, 1, 0)
        eux = g["EQ_UX"][:e * n * m].reshape(n, m, e).transpose(2, 1, 0)
        assert np.max(np.abs(exx - full[:, :n, :n])) <= tol * max(1.0, _scale(full)), np.max(np.abs(exx - full[:, :n, :n]))
        assert np.max(np.abs(eux - full[:, n:, :n])) <= tol * max(1.0, _scale(full))


@pytest.mark.gpu
def test_sweep_parity_at_size(gpu):
    """tree38ff_frame, T = 200, tensor-free, the benchmark's constrained leg: the device's analytic derivatives through
    Oracle.backward / forward vs the device sweep"""
    capi = gpu
    T, mu = 200, 1e3
    model, spec, o = make("tree38ff_frame", T, fd_mode=0, first_order_fd=0)
    x0, us, xs = initial_trajectory(o, model, seed=7, u_sigma=0.1)
    mults = o.alloc_affine(o.Etot)
    mults["origin"][:] = xs[:T * o.nx]
    mults["jac"][:o.Etot * o.n] = 0.01 * np.random.default_rng(8).normal(size=o.Etot * o.n)
    names = {"lfx": "LFX", "lfxx": "LFXX", "lx": "LX", "lu": "LU", "lxx": "LXX", "lux": "LUX", "luu": "LUU", "f_val": "F_VAL",
             "fx": "FX", "fu": "FU", "eq_val": "EQ_VAL", "eq_x": "EQ_X", "eq_u": "EQ_U"}
    with capi.Context(spec, flags=capi.FLAG_TRACE | capi.FLAG_NO_TENSORS) as ctx:
        ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
        for k, sname in (("origin", "MULT_ORIGIN"), ("val", "MULT_VAL"), ("jac", "MULT_JAC")):
            ctx.upload(sname, mults[k][:ctx.seq_size(sname)])
        ctx.linearize()
        d = o.alloc_derivs()
        for k, sname in names.items():
            if ctx.seq_size(sname):
                d[k][:ctx.seq_size(sname)] = ctx.download(sname)[0]
        ref = o.backward(d, xs, mults, 0.0, mu)
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        assert int(restarts[0]) == ref["restarts"] and mu_out[0] == ref["mu"] and reg[0] == ref["reg"]
        K = ctx.download("FB_JAC")[0]
        k_ = ctx.download("FB_VAL")[0]
        Vx = ctx.download("VX_TRACE")[0]
        assert rel_err(K, ref["fb"]["jac"][:K.size]) < 1e-9 and rel_err(Vx, ref["Vx"]) < 1e-9
        # k: 2.5e-9 relative.  Its error is 0 at t = T-1 and grows smoothly to ~1e-7 at t = 0 (|k| ~ 12): one ulp of the
        # derivative inputs carried back through 200 Riccati steps of a free fall, the same on either derivative path
        assert rel_err(k_, ref["fb"]["val"][:k_.size]) < 1e-8
        step_ref, _, _, _ = o.forward(xs, us, mults, ref["fb"], ref["mu"])
        rc, step, _ = ctx.forward(mu_out, n_alpha=8)
        assert step[0] == step_ref, (step, step_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode", [("chain6ff_frame", 0), ("chain6ff", 2)])
def test_whole_solve(gpu, name, fd_mode):
    """ddp_hip_solve against the stepwise loop on the analytic jacobians, and run to run.  (No descent is asserted: the
    reference's frame jacobian is the top rows of the WORLD-frame spatial jacobian, not dp/dq -- tests/test_lie.py,
    test_free_flyer_whole_solve -- so the line search may run to its floor; the two loops must still agree bit for bit.  In mode 2
    that frame jacobian leaves Q_uu indefinite and the sweep gives up on restarts (tests/test_constrained_full.py), so mode 2
    solves the unconstrained arm.)"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, iters, thr, mu, w, n = 8, 4, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, fd_mode=fd_mode, first_order_fd=0)
    us0 = 0.02 * np.random.default_rng(50).normal(size=T * model.nv)
    xs0 = o.rollout(initial_trajectory(o, model, seed=9)[0], us0)
    flags = 0 if fd_mode else capi.FLAG_NO_TENSORS

    def run(stepwise):
        with capi.Context(spec, flags=flags) as ctx:
            assert ctx.info()["first_order"] == 2
            ctx.upload("X", xs0); ctx.upload("U", us0); ctx.upload("X_NEW", xs0); ctx.upload("U_NEW", us0)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs0[:T * o.nx]); ctx.upload("MULT_VAL", np.zeros(o.Etot)); ctx.upload("MULT_JAC", np.zeros(o.Etot * o.n))
            log = (solver.solve_stepwise if stepwise else solver.solve)(ctx, iters, thr, mu, 0.0, w, n)
            return log, ctx.download("X"), ctx.download("U")
    la, xa, ua = run(False)
    lb, xb, ub = run(True)
    lc, xc, uc = run(False)
    assert np.all(np.isfinite(xa)) and np.all(np.isfinite(ua))
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    assert np.array_equal(xa, xc) and np.array_equal(ua, uc)
    for k in ("iterations", "mu", "reg", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(la[k]), np.asarray(lb[k])), k
        assert np.array_equal(np.asarray(la[k]), np.asarray(lc[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("first_order_fd", [0, 1])
def test_refusals_unchanged(gpu, first_order_fd):
    capi = gpu
    _, spec, _ = make("chain6ff", 4, fd_mode=1, first_order_fd=first_order_fd)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(spec)
    assert exc.value.code == capi.E_UNSUPPORTED
    model = capi.BuiltinModel(capi.BUILTIN_CHAIN6_FF)
    spec = capi.ProblemSpec(model, 4, batch=1, fd_mode=2, first_order_fd=first_order_fd, eq_kind=capi.EQ_CONFIG, eq_advance=2,
                            ne=np.full(4, 6, dtype=np.int64), eq_target=np.zeros(24))
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(spec)
    assert exc.value.code == capi.E_UNSUPPORTED
