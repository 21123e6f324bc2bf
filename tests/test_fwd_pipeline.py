"""The pipelined form of the forward latency kernel (fwd.hip: forward_kernel_lat2<…, PIPE>; DESIGN.md section 4, "Forward")
against the four-candidate form that DDP_HIP_FWD_NO_PIPE forces: the helper wave forms step t + 1's placements, inertia sums,
U, 1/D, Ia and X^T Ia X while step t runs, every entry by the same operations in the same order, so the two forms agree bit
for bit.  Two contexts per case, the second created under the switch; inputs are uploaded, never computed by either form."""
import numpy as np
import pytest

from problems import make, random_state

pytestmark = pytest.mark.gpu

OUTS = ("X_NEW", "U_NEW")


def _compute_units(capi):
    """what ddp_hip_create reads: hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount = 63 in hip_runtime_api.h), through
    the library's own handle (dlsym reaches its dependencies)"""
    import ctypes as C
    n = C.c_int(0)
    assert capi.lib().hipDeviceGetAttribute(C.byref(n), 63, 0) == 0
    return n.value


def _inputs(name, T, B, seed, k_sigma=0.1):
    """B instances: a random start state, random controls, the oracle's rollout of them, random gains"""
    model, spec, o = make(name, T, batch=B, fd_mode=0)
    rng = np.random.default_rng(seed)
    nv = model.nv
    xs, us = [], []
    for _ in range(B):
        u = 0.3 * rng.normal(size=T * nv)
        xs.append(o.rollout(random_state(model, rng, 0.3), u)); us.append(u)
    inp = {"X": np.stack(xs), "U": np.stack(us), "FB_VAL": k_sigma * rng.normal(size=(B, T * nv)),
           "FB_JAC": k_sigma * rng.normal(size=(B, T * nv * 2 * nv))}
    inp["FB_ORIGIN"] = inp["X"][:, :T * o.nx].copy()
    if o.Etot:
        inp["MULT_ORIGIN"] = inp["X"][:, :T * o.nx].copy()
        inp["MULT_VAL"] = 0.1 * rng.normal(size=(B, o.Etot))
        inp["MULT_JAC"] = 0.01 * rng.normal(size=(B, o.Etot * o.n))
    return model, spec, o, inp


def _forward(capi, spec, inp, n_alpha, mu=1.0, flags=0, setup=None, first=0, count=None):
    """one ddp_hip_forward of instances first .. first + count - 1 of `inp` in a context of their own"""
    count = spec.batch if count is None else count
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | flags) as ctx:
        assert ctx.info()["fwd_path"] == 1
        for s, arr in inp.items():
            ctx.upload(s, arr[first:first + count])
        ctx.upload("X_NEW", inp["X"][first:first + count]); ctx.upload("U_NEW", inp["U"][first:first + count])
        if setup:
            setup(ctx)
        rc, step, dcost = ctx.forward(mu, n_alpha=n_alpha)
        out = {s: ctx.download(s) for s in OUTS}
    out["step"], out["dcost"], out["rc"] = step, dcost, rc
    return out


def _pair(capi, monkeypatch, spec, inp, n_alpha, **kw):
    got = _forward(capi, spec, inp, n_alpha, **kw)
    monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
    ref = _forward(capi, spec, inp, n_alpha, **kw)
    monkeypatch.delenv("DDP_HIP_FWD_NO_PIPE")
    return got, ref


def _same(got, ref):
    assert got["rc"] == ref["rc"]
    for s in OUTS + ("step", "dcost"):
        assert np.all(np.isfinite(ref[s])), s
        assert np.array_equal(got[s], ref[s]), (s, float(np.max(np.abs(got[s] - ref[s]))))


@pytest.mark.parametrize("n_alpha", [1, 3, 8])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_pipe_bit_for_bit(gpu, monkeypatch, T, n_alpha):
    """T = 1: no hand-off between the waves, 2: one, 5: both record buffers twice.  n_alpha = 1: a candidate alone in its
    workgroup, 3: a partly filled last workgroup, 8: the full set"""
    model, spec, o, inp = _inputs("tree38", T, 3, seed=100 + T)
    got, ref = _pair(gpu, monkeypatch, spec, inp, n_alpha)
    _same(got, ref)
    assert np.any(got["U_NEW"] != inp["U"])                      # a candidate was rolled out and copied


def test_pipe_free_flyer(gpu, monkeypatch):
    model, spec, o, inp = _inputs("tree38ff", 5, 3, seed=7)
    got, ref = _pair(gpu, monkeypatch, spec, inp, 8)
    _same(got, ref)


@pytest.mark.parametrize("name", ["tree38", "tree38ff"])
def test_pipe_rollout(gpu, monkeypatch, name):
    """ctx.rollout(): the open-loop instantiation"""
    capi = gpu
    model, spec, o, inp = _inputs(name, 5, 3, seed=8)
    out = []
    for no_pipe in (False, True):
        if no_pipe:
            monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
            bad = np.full_like(inp["X"], np.nan); bad[:, :o.nx] = inp["X"][:, :o.nx]
            ctx.upload("X", bad); ctx.upload("U", inp["U"])
            ctx.rollout()
            out.append(ctx.download("X"))
    monkeypatch.delenv("DDP_HIP_FWD_NO_PIPE")
    assert np.all(np.isfinite(out[1])) and np.array_equal(out[0], out[1])
    assert np.max(np.abs(out[0] - inp["X"])) < 1e-9              # (and it is the oracle's rollout)


def test_pipe_tracking_cost_and_bounds(gpu, monkeypatch):
    """the COST bit 0 / BOX instantiation: inline tracking terms, controls clamped where the bounds bind"""
    capi = gpu
    T, B = 5, 3
    model, spec, o, inp = _inputs("tree38", T, B, seed=9)
    rng = np.random.default_rng(90)
    xref = inp["X"].reshape(B, T + 1, o.nx) + 0.1 * rng.normal(size=(B, T + 1, o.nx))
    wx, wu = rng.uniform(0.5, 2.0, size=(B, T + 1, o.n)), rng.uniform(0.5, 2.0, size=(B, T, model.nv))
    uref = 0.1 * rng.normal(size=(B, T, model.nv))

    def setup(ctx):
        ctx.set_tracking_cost(xref=xref, wx=wx, uref=uref, wu=wu)
        ctx.set_control_bounds(lo=-0.25, hi=0.25)

    got, ref = _pair(capi, monkeypatch, spec, inp, 8, flags=capi.FLAG_TRACKING_COST | capi.FLAG_CONTROL_BOUNDS, setup=setup)
    _same(got, ref)
    assert np.any(np.abs(got["U_NEW"]) == 0.25)                  # a bound binds in the accepted rollout


def test_pipe_constrained(gpu, monkeypatch):
    """tree38_frame: the rollout on this kernel, the candidates' cost terms on cand_cost_kernel"""
    model, spec, o, inp = _inputs("tree38_frame", 5, 3, seed=10)
    assert o.Etot > 0
    got, ref = _pair(gpu, monkeypatch, spec, inp, 8, mu=100.0)
    _same(got, ref)


def test_pipe_later_rounds(gpu, monkeypatch):
    """u = 0 is optimal for l = c/2 |u|^2, so a feed-forward of ones is rejected at every step size: all five rounds of eight
    run (p.round > 0), the call reports the floor and leaves the last rollout tried in X_NEW"""
    capi = gpu
    T, B = 5, 3
    model, spec, o, inp = _inputs("tree38", T, B, seed=11)
    inp["U"][:] = 0.0
    inp["X"] = np.stack([o.rollout(inp["X"][b, :o.nx], inp["U"][b]) for b in range(B)])
    inp["FB_ORIGIN"] = inp["X"][:, :T * o.nx].copy()
    inp["FB_VAL"][:] = 1.0
    got, ref = _pair(capi, monkeypatch, spec, inp, 8)
    assert ref["rc"] == capi.EV_LINESEARCH_FLOOR and np.all(ref["step"] == 2.0 ** -34)
    _same(got, ref)
    assert np.any(got["U_NEW"] != 0.0)


def test_form_selection(gpu):
    """The pipelined grid, one workgroup per (instance, two candidates), is used while it fits the compute units.  At n_alpha = 8
    the largest such batch is CUs / 4 (64 on an MI355X); a context one instance larger takes the four-candidate form and agrees
    bit for bit with a three-instance (pipelined) run of its first instances, and so does one of exactly that batch"""
    capi = gpu
    cus = _compute_units(capi)
    bmax = cus // 4
    assert 3 <= bmax <= 256, cus
    T = 2
    model, spec, o, inp = _inputs("tree38", T, bmax + 1, seed=12)
    big = _forward(capi, spec, inp, 8)                           # bmax + 1 instances: four candidates per workgroup
    _, spec_fit, _ = make("tree38", T, batch=bmax, fd_mode=0)
    fit = _forward(capi, spec_fit, inp, 8, count=bmax)           # bmax instances: the pipelined grid fills the device
    _, spec3, _ = make("tree38", T, batch=3, fd_mode=0)
    small = _forward(capi, spec3, inp, 8, count=3)
    for s in OUTS + ("step", "dcost"):
        assert np.all(np.isfinite(big[s])), s
        assert np.array_equal(big[s][:3], small[s]), s
        assert np.array_equal(big[s][:bmax], fit[s]), s
