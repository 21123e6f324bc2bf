"""Per-instance quadratic tracking costs (DDP_HIP_FLAG_TRACKING_COST, include/ddp_hip/ddp_hip.h):

    l(t, x, u) = c/2 |u|^2 + 1/2 sum_i wx[t][i] d_i^2 + 1/2 sum_j wu[t][j] (u_j - uref[t][j])^2,   lf(x_T) = 1/2 sum_i wx[T][i] d_i^2

with d = x (-) xref.  The oracle has no such cost, so the yardstick is the numpy restatement below, built on oracle primitives
(integrate, difference, d_difference_dq_finish for the free-flyer root's Jlog6, eval_f, forward_alpha, backward).  The
constraint terms of cost_seq_aug come from Oracle.cost_seq_aug (its l is c/2 |u|^2 and its lf 0: the tracking terms add)."""
import numpy as np
import pytest

from problems import held_trajectory, initial_trajectory, make, neutral_state
from synth import rel_err, stepwise_backward_check

H = 1e-3
DERIVS = ("LX", "LXX", "LU", "LUU", "LUX", "LFX", "LFXX")


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def _diff(o, xr, x):
    """d = x (-) xr in the tangent (lie::difference_x)"""
    nq = o.nq
    if nq == o.nv:
        return x - xr
    return np.concatenate([o.difference(xr[:nq], x[:nq]), x[nq:] - xr[nq:]])


def _jac(o, xr, x):
    """J = dd/d(delta x) along x (+) delta: the identity but on a free-flyer root block (Jlog6 = dDifference ARG1)"""
    J = np.eye(o.n)
    if o.nq != o.nv:
        J[:6, :6] = o.d_difference_dq_finish(xr[:o.nq], x[:o.nq])[:6, :6]
    return J


def _integrate_x(o, x, dx):
    nq = o.nq
    return np.concatenate([o.integrate(x[:nq], dx[:o.nv]), x[nq:] + dx[o.nv:]])


def track_terms(o, c, xs, us, ref, b=0):
    """the tracking terms of instance b per t (T+1 values; the last is lf); c/2 |u|^2 not included"""
    T, nx, m = o.T, o.nx, o.m
    X, U = xs.reshape(T + 1, nx), us.reshape(T, m)
    out = np.zeros(T + 1)
    for t in range(T + 1):
        d = _diff(o, ref["xref"][b][t], X[t])
        out[t] = 0.5 * np.sum(ref["wx"][b][t] * d * d)
        if t < T:
            du = U[t] - ref["uref"][b][t]
            out[t] += 0.5 * np.sum(ref["wu"][b][t] * du * du)
    return out


def full_cost(o, c, xs, us, ref, b=0):
    """l_t (t < T) and lf of the unconstrained problem"""
    T, m = o.T, o.m
    out = track_terms(o, c, xs, us, ref, b)
    out[:T] += 0.5 * c * np.sum(us.reshape(T, m) ** 2, axis=1)
    return out


def expected_derivs(o, c, xs, us, ref, b=0):
    """LX .. LFXX of instance b in the library's flat (column-major) layout"""
    T, n, m, nx = o.T, o.n, o.m, o.nx
    X, U = xs.reshape(T + 1, nx), us.reshape(T, m)
    out = {k: [] for k in DERIVS}
    for t in range(T + 1):
        xr, w = ref["xref"][b][t], ref["wx"][b][t]
        d, J = _diff(o, xr, X[t]), _jac(o, xr, X[t])
        gx, gxx = J.T @ (w * d), J.T @ np.diag(w) @ J
        if t == T:
            out["LFX"].append(gx); out["LFXX"].append(gxx.ravel(order="F"))
            continue
        wu, ur = ref["wu"][b][t], ref["uref"][b][t]
        out["LX"].append(gx); out["LXX"].append(gxx.ravel(order="F"))
        out["LU"].append(c * U[t] + wu * (U[t] - ur))
        out["LUU"].append((c * np.eye(m) + np.diag(wu)).ravel(order="F"))
        out["LUX"].append(np.zeros(m * n))
    return {k: np.concatenate(v) for k, v in out.items()}


def random_ref(o, model, xs, us, B, seed, wscale=1.0, spread=0.3):
    """per-instance references near the trajectories (xs, us: (B, ...)) and positive weights"""
    rng = np.random.default_rng(seed)
    T, n, m, nx = o.T, o.n, o.m, o.nx
    ref = {"xref": np.zeros((B, T + 1, nx)), "wx": wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, n)),
           "uref": np.zeros((B, T, m)), "wu": wscale * rng.uniform(0.0, 1.0, size=(B, T, m))}
    for b in range(B):
        X = xs[b].reshape(T + 1, nx)
        for t in range(T + 1):
            ref["xref"][b][t] = _integrate_x(o, X[t], spread * rng.normal(size=n))
        ref["uref"][b] = us[b].reshape(T, m) + spread * rng.normal(size=(T, m))
    return ref


def upload_ref(ctx, ref, first=0):
    B = ref["xref"].shape[0]
    ctx.set_tracking_cost(xref=ref["xref"], wx=ref["wx"], uref=ref["uref"], wu=ref["wu"], first=first, count=B)


def _trajs(o, model, B, seed, held=False):
    xs, us = [], []
    for b in range(B):
        if held:
            _, u_, x_ = held_trajectory(o, model, seed=seed + b, q0_sigma=0.3)
        else:
            _, u_, x_ = initial_trajectory(o, model, seed=seed + b, u_sigma=0.2)
        xs.append(x_); us.append(u_)
    return np.stack(xs), np.stack(us)


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff"])
def test_yardstick_gradient(name):
    """lx from the definition against a 5-point central difference of the numpy cost along x (+) (+-h e_j), +-2h; on
    vector-space models lxx against the central difference of lx (exact: lx is affine in x)"""
    T = 2
    model, _, o = make(name, T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 3)
    ref = random_ref(o, model, xs, us, 1, 4)
    c = 1.0
    X = xs[0].reshape(T + 1, o.nx)
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for t in (0, T):
        ex = expected_derivs(o, c, xs[0], us[0], ref)
        gx = ex["LFX"] if t == T else ex["LX"][t * o.n:(t + 1) * o.n]
        gxx = ex["LFXX"] if t == T else ex["LXX"][t * o.n * o.n:(t + 1) * o.n * o.n]
        gxx = gxx.reshape(o.n, o.n).T

        def cost_at(dx):
            xs2 = X.copy()
            xs2[t] = _integrate_x(o, X[t], dx)
            return track_terms(o, c, xs2.ravel(), us[0], ref)[t]
        fd = np.zeros(o.n)
        for j in range(o.n):
            e = np.zeros(o.n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fd - gx)) <= 1e-8 * max(1.0, np.max(np.abs(gx))), np.max(np.abs(fd - gx))
        if o.nq == o.nv:
            def grad_at(dx):
                xr, w = ref["xref"][0][t], ref["wx"][0][t]
                return _jac(o, xr, X[t] + dx).T @ (w * _diff(o, xr, X[t] + dx))
            fdh = np.stack([(grad_at(H * np.eye(o.n)[j]) - grad_at(-H * np.eye(o.n)[j])) / (2 * H) for j in range(o.n)], axis=1)
            assert np.max(np.abs(fdh - gxx)) <= 1e-8 * max(1.0, np.max(np.abs(gxx)))
            assert np.array_equal(gxx, gxx.T)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _setup(ctx, xs, us, mults=None, Etot=0):
    ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
    if Etot:
        B = xs.shape[0]
        for k, s in (("origin", "MULT_ORIGIN"), ("val", "MULT_VAL"), ("jac", "MULT_JAC")):
            ctx.upload(s, np.tile(mults[k][:ctx.seq_size(s)], (B, 1)))


def _mults(o, xs0, seed):
    mults = o.alloc_affine(o.Etot)
    mults["origin"][:] = xs0[:o.T * o.nx]
    if o.Etot:
        mults["jac"][:o.Etot * o.n] = 0.01 * np.random.default_rng(seed).normal(size=o.Etot * o.n)
    return mults


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo,flags,fwd_path", [
    ("tree38", 24, 2, None, 0, 1),                # static mode-2 stencil, K3h sweep, latency forward
    ("chain6", 10, 2, None, 0, 0),                # config constraint, lane-per-rollout forward
    ("tree38ff_frame", 24, 0, 0, 1, 1),           # analytic mode 0, tensor-free, frame constraint
])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo, flags, fwd_path):
    """flag on, every weight 0 (references far from the trajectory): bit for bit what the flag-off context computes"""
    capi = gpu
    mu = 10.0
    model, spec, o = make(name, T, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, 1, 31, held=True)
    mults = _mults(o, xs[0], 32)
    ref = random_ref(o, model, xs, us, 1, 33, spread=1.0)
    ref["wx"][:] = 0.0; ref["wu"][:] = 0.0
    out = {}
    for on in (False, True):
        fl = capi.FLAG_TRACE | flags | (capi.FLAG_TRACKING_COST if on else 0)
        with capi.Context(spec, flags=fl) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on:
                upload_ref(ctx, ref)
            ctx.linearize()
            r = {s: ctx.download(s) for s in DERIVS}
            if name == "tree38":
                r["stream"] = ctx.bwd_stream_bytes()
            ctx.cost_seq_aug(0, mu)
            r["COSTS_OLD"] = ctx.download("COSTS_OLD")
            ctx.cost_seq_aug(1, mu)
            r["COSTS_NEW"] = ctx.download("COSTS_NEW")
            rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
            r["bwd"] = (rc, reg, mu_out, restarts)
            for s in ("FB_ORIGIN", "FB_VAL", "FB_JAC", "VX_TRACE"):
                r[s] = ctx.download(s)
            rc, step, dcost = ctx.forward(mu_out, n_alpha=8)
            r["fwd"] = (rc, step, dcost)
            r["X_NEW"], r["U_NEW"] = ctx.download("X_NEW"), ctx.download("U_NEW")
            out[on] = r
    a, b = out[False], out[True]
    for k in a:
        if isinstance(a[k], tuple):
            for u, v in zip(a[k], b[k]):
                assert np.array_equal(u, v), k
        else:
            assert np.array_equal(a[k], b[k]), k
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo", [("chain6", 2, None), ("tree38", 2, None), ("chain6ff", 2, 0), ("tree38ff", 0, 0)])
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo, stages):
    """LX .. LFXX against the definition, batch 3 with different references and weights per instance, through
    ddp_hip_linearize and through ddp_hip_linearize_stages(LIN_COST)"""
    capi = gpu
    T, B, c = 6, 3, 1.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 41)
    ref = random_ref(o, model, xs, us, B, 42)
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST) as ctx:
        _setup(ctx, xs, us, _mults(o, xs[0], 43), o.Etot)
        upload_ref(ctx, ref)
        ctx.linearize(None if stages is None else capi.LIN_COST)
        got = {s: ctx.download(s) for s in DERIVS}
    for b in range(B):
        ex = expected_derivs(o, c, xs[b], us[b], ref, b)
        for s in DERIVS:
            if s == "LUX":
                assert np.all(got[s][b] == 0.0)
                continue
            assert rel_err(got[s][b], ex[s]) <= 1e-12, (s, b, rel_err(got[s][b], ex[s]))
        n = o.n
        for t in range(T):
            blk = got["LXX"][b][t * n * n:(t + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None), ("tree38_frame", 0, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the oracle's augmented cost plus the tracking terms, c_T = lf included"""
    capi = gpu
    T, B, mu = 12, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    ref = random_ref(o, model, xs, us, B, 52)
    mults = _mults(o, xs[0], 53)
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        upload_ref(ctx, ref)
        ctx.cost_seq_aug(0, mu)
        ctx.cost_seq_aug(1, mu)
        got = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + track_terms(o, 1.0, X[b], U[b], ref, b)
            assert got[which][b][T] != 0.0
            assert rel_err(got[which][b], ex) <= 1e-12, (which, b, rel_err(got[which][b], ex))


def _k3h_bytes(n, m):
    cxx, cux, cuu = n * (n + 1) // 2, n * m, m * (m + 1) // 2
    return 8 * ((cxx + cux + cuu) * (n - m) + 2 * cxx - n + cux)


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with V_x != 0 from the tracking cost, on the device's own derivatives (tensors included) against
    Oracle.backward.  Every step redone alone by the oracle from the device's own V(t+1) must land on the device's k_t, K_t,
    V_x(t), V_xx(t) to 1e-10 (synth.stepwise_backward_check); end to end the light distal links' open-loop instability carries
    one ulp to ~1e-6 over the horizon between any two correct implementations, so the whole recursion is held to 1e-5 and its
    first ten steps to 1e-10.  At the Talos size the sweep runs on K3h.  (tree38 at T = 60: at T = 200 no full-DDP sweep with
    V != 0 stays positive definite in double, on the oracle as on the device, tensor-free included -- DESIGN.md 4d)"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    ref = random_ref(o, model, xs, us, 1, 72, wscale=0.1, spread=0.05)
    mults = _mults(o, xs[0], 73)
    n, m = o.n, o.m
    names = {"lfx": "LFX", "lfxx": "LFXX", "lx": "LX", "lu": "LU", "lxx": "LXX", "lux": "LUX", "luu": "LUU", "f_val": "F_VAL",
             "fx": "FX", "fu": "FU", "fxx": "FXX", "fux": "FUX", "fuu": "FUU", "eq_val": "EQ_VAL", "eq_x": "EQ_X", "eq_u": "EQ_U",
             "eq_xx": "EQ_XX", "eq_ux": "EQ_UX", "eq_uu": "EQ_UU"}
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        upload_ref(ctx, ref)
        ctx.linearize()
        if name == "tree38":
            assert ctx.bwd_stream_bytes() == _k3h_bytes(n, m)
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        d = o.alloc_derivs()
        for k, s in names.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
        assert np.max(np.abs(d["lfx"][:n])) > 0
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
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
    assert worst < 1e-10, worst
    for seq, r in (("FB_VAL", ref_b["fb"]["val"]), ("FB_JAC", ref_b["fb"]["jac"]), ("VX_TRACE", ref_b["Vx"]), ("VXX_TRACE", ref_b["Vxx"])):
        g, r = got[seq], r[:got[seq].size]
        assert rel_err(g, r) < 1e-5, (seq, rel_err(g, r))
        tail = slice(-10 * (g.size // T), None)                    # the first ten steps of the sweep
        assert rel_err(g[tail], r[tail]) < 1e-10, (seq, rel_err(g[tail], r[tail]))


def _emulate_forward(o, c, xs, us, fb, mu, n_alpha, ref):
    """sequential halving with the numpy cost: the first step 2^-k with sum_t (new - old) <= 0 (n_alpha = 0: the full step)"""
    mults = o.alloc_affine(0)
    old = full_cost(o, c, xs, us, ref).sum()
    for k in range(34):
        step = 2.0 ** -k
        _, xn, un = o.forward_alpha(step, xs, us, mults, fb, mu)
        if n_alpha == 0 or full_cost(o, c, xn, un, ref).sum() - old <= 0:
            return step, xn, un
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,fwd_path", [("tree38", 0, None, 1), ("chain6ff", 0, 0, 0), ("tree38ff", 0, 0, 1)])
@pytest.mark.parametrize("n_alpha", [0, 1, 8])
@pytest.mark.parametrize("k_scale", [1.0, 3.0])
def test_forward_matches_emulation(gpu, name, fd_mode, fo, fwd_path, n_alpha, k_scale):
    """accepted step, X_NEW and U_NEW against Oracle.forward_alpha rollouts costed with numpy; k_scale 3 overshoots the
    minimum along the step so that the full step is rejected and the halving runs"""
    capi = gpu
    T, c, mu = 16, 1.0, 1.0
    model, spec, o = make(name, T, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, 1, 81, held=True)
    ref = random_ref(o, model, xs, us, 1, 82, spread=0.2)
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us)
        upload_ref(ctx, ref)
        ctx.linearize()
        ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        rc, step, dcost = ctx.forward(mu, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
    em = _emulate_forward(o, c, xs[0], us[0], fb, mu, n_alpha, ref)
    assert em is not None
    step_ref, xn_ref, un_ref = em
    assert step[0] == step_ref, (step, step_ref)
    if k_scale != 1.0 and n_alpha:
        assert step[0] < 1.0
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    new = full_cost(o, c, xn_ref, un_ref, ref).sum() - full_cost(o, c, xs[0], us[0], ref).sum()
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo, flags):
    """batch 4, four different tasks, through ddp_hip_solve: each instance as a batch-1 context given that instance's data"""
    capi = gpu
    T, B = 20, 4
    iters, thr, mu, w, n = 6, 1e-9, 10.0, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    _, spec1, _ = make(name, T, batch=1, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 91, held=True)
    ref = random_ref(o, model, xs, us, B, 92, spread=0.3)

    def run(sp, sl):
        with capi.Context(sp, flags=capi.FLAG_TRACKING_COST | flags) as ctx:
            _setup(ctx, xs[sl], us[sl])
            ctx.set_tracking_cost(xref=ref["xref"][sl], wx=ref["wx"][sl], uref=ref["uref"][sl], wu=ref["wu"][sl])
            _, log = ctx.solve(iters, thr, mu, 0.0, w, n, n_alpha=8)
            return log, ctx.download("X"), ctx.download("U"), ctx.info()
    lb, Xb, Ub, ib = run(spec, slice(0, B))
    assert len({tuple(Xb[b][-o.nx:]) for b in range(B)}) == B
    for b in range(B):
        l1, X1, U1, i1 = run(spec1, slice(b, b + 1))
        for k in ("iterations", "result", "last_step", "mu", "reg"):
            assert l1[k][0] == lb[k][b], (k, b)
        assert rel_err(X1[0], Xb[b]) <= 1e-12 and rel_err(U1[0], Ub[b]) <= 1e-12
        same = {k: v for k, v in i1.items() if k != "hbm_bytes"} == {k: v for k, v in ib.items() if k != "hbm_bytes"}
        if same:
            assert np.array_equal(X1[0], Xb[b]) and np.array_equal(U1[0], Ub[b])
            for k in ("opt_obj", "opt_constr", "w", "n"):
                assert l1[k][0] == lb[k][b], (k, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w, n = 10, 2, 5, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    xs, us = _trajs(o, model, B, 101, held=True)
    ref = random_ref(o, model, xs, us, B, 102)
    mults = _mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            upload_ref(ctx, ref)
            log = (solver.solve_stepwise if stepwise else solver.solve)(ctx, iters, thr, mu, 0.0, w, n)
            return log, ctx.download("X"), ctx.download("U")
    la, xa, ua = run(False)
    lb, xb, ub = run(True)
    assert np.all(np.isfinite(xa))
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(la[k]), np.asarray(lb[k])), k


@pytest.mark.gpu
def test_pendulum_terminal_weight(gpu):
    """the pendulum task of test/pendulum_ddp.cpp (q = 3.14 at the end) as a terminal cost instead of a constraint: the
    final error shrinks as the weight grows"""
    capi = gpu
    T, target = 100, 3.14
    model = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    spec = capi.ProblemSpec(model, T, dt=0.01, c=1.0, batch=1, fd_mode=2)
    from oracle.binding import Oracle
    o = Oracle(model, T, dt=0.01, c=1.0, fd_mode=2)
    us = np.zeros(T)
    xs = o.rollout(np.zeros(2), us)
    errs = []
    for wq in (1e1, 1e3, 1e5):
        with capi.Context(spec, flags=capi.FLAG_TRACKING_COST) as ctx:
            _setup(ctx, xs[None], us[None])
            xref = np.zeros((T + 1, 2)); xref[T, 0] = target
            wx = np.zeros((T + 1, 2)); wx[T, 0] = wq
            ctx.set_tracking_cost(xref=xref, wx=wx)
            _, log = ctx.solve(300, 1e-9, 1e2, 0.0, 1e-1, 10.0, n_alpha=8)
            X = ctx.download("X")[0].reshape(T + 1, 2)
        assert np.all(np.isfinite(X))
        errs.append(abs(X[T, 0] - target))
    assert errs[0] > errs[1] > errs[2], errs
    assert errs[2] < 0.025, errs          # (1.6e-2 measured: a one-second swing-up, the torque cost balances 1e5 |q_T - 3.14|)


@pytest.mark.gpu
def test_posture_tracking_descends(gpu):
    """tree38, no constraint, tracking a posture: sum_t COSTS_OLD never increases over the iterations, and the tracking error
    at the end is below the initial one"""
    capi = gpu
    T, mu, iters = 40, 1.0, 8
    model, spec, o = make("tree38", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 111)
    rng = np.random.default_rng(112)
    posture = np.concatenate([0.3 * rng.normal(size=o.nv), np.zeros(o.nv)])
    xref = np.tile(posture, (T + 1, 1))
    wx = np.concatenate([np.full(o.nv, 10.0), np.full(o.nv, 0.1)])
    wx = np.tile(wx, (T + 1, 1))

    def err(X):
        return np.linalg.norm(X.reshape(T + 1, o.nx)[:, :o.nv] - posture[:o.nv])
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_tracking_cost(xref=xref, wx=wx)
        costs = []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            ctx.swap_traj()
        final = ctx.download("X")[0]
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
    assert err(final) < err(xs[0])


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    capi = gpu
    T = 4
    model, spec, o = make("chain6ff", T, fd_mode=0, first_order_fd=0)
    n, m, nx = o.n, o.m, o.nx
    with capi.Context(spec) as ctx:
        for s, size in (("COST_XREF", (T + 1) * nx), ("COST_WX", (T + 1) * n), ("COST_UREF", T * m), ("COST_WU", T * m)):
            assert ctx.seq_size(s) == size
            with pytest.raises(capi.DdpHipError) as exc:
                ctx.upload(s, np.zeros(size))
            assert exc.value.code == capi.E_UNSUPPORTED
            with pytest.raises(capi.DdpHipError) as exc:
                ctx.download(s)
            assert exc.value.code == capi.E_UNSUPPORTED
            assert not ctx.device_ptr(s)
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST) as ctx:
        assert np.array_equal(ctx.download("COST_XREF")[0], np.tile(neutral_state(model), T + 1))
        for s in ("COST_WX", "COST_UREF", "COST_WU"):
            assert np.array_equal(ctx.download(s)[0], np.zeros(ctx.seq_size(s)))
        for s in ("COST_WX", "COST_WU"):
            for bad in (-1e-3, np.nan, np.inf):
                a = np.ones(ctx.seq_size(s)); a[1] = bad
                with pytest.raises(capi.DdpHipError) as exc:
                    ctx.upload(s, a)
                assert exc.value.code == capi.E_ARG, (s, bad)
                with pytest.raises(capi.DdpHipError) as exc:
                    ctx.fill(s, bad)
                assert exc.value.code == capi.E_ARG, (s, bad)
            assert np.array_equal(ctx.download(s)[0], np.zeros(ctx.seq_size(s)))
        xr = np.tile(neutral_state(model), (T + 1, 1))
        xr[2, 3:7] *= 1 + 1e-9
        with pytest.raises(capi.DdpHipError) as exc:
            ctx.set_tracking_cost(xref=xr)
        assert exc.value.code == capi.E_ARG
        xr[2, 3:7] = [0.5, 0.5, 0.5, 0.5]
        ctx.set_tracking_cost(xref=xr)
        assert np.array_equal(ctx.download("COST_XREF")[0], xr.ravel())
    _, spec_v, _ = make("chain6", T, fd_mode=0)
    with capi.Context(spec_v, flags=capi.FLAG_TRACKING_COST) as ctx:
        assert np.array_equal(ctx.download("COST_XREF")[0], np.zeros((T + 1) * 12))
        ctx.set_tracking_cost(xref=np.full((T + 1, 12), 7.0))        # no quaternion on a vector-space model
