"""The static first order's u waves and the u diagonal on LDS-staged operands (lin_static.hip: lin_static_first_tau_kernel,
lin_static_first_tau_fused_kernel) against the scalar-path kernels kept behind DDP_HIP_FIRST_SCALAR.

Only where an evaluation's operands come from changes, not its operation sequence, so every output is equal bit for bit: each
test builds two contexts in one process -- the default one and one created under the switch -- on the same model and inputs and
requires np.array_equal.  Every compiled-in topology at BT = 6 and BT = 9 (neither a multiple of 8): in every tensor layout and
under the schedule switches tests/test_lin_overlap.py cycles through, stage by stage against the fused call (the u diagonal comes
out of the first order's u waves only when one call runs both orders), in a tensor-free context (which has no f_uu to touch) and
in analytic mode 1 (the waves leave accelerations instead of jacobian columns)."""
import numpy as np
import pytest

import robots
from problems import make

SWITCH = "DDP_HIP_FIRST_SCALAR"
OTHERS = ("DDP_HIP_LIN_SERIAL", "DDP_HIP_LIN_FORKS", "DDP_HIP_K3_NO_PACK", "DDP_HIP_FXX_FULL", "DDP_HIP_K3_NO_SYM",
          "DDP_HIP_CFG_FULL_ABA", "DDP_HIP_NO_STATIC", "DDP_HIP_QWS_BT")
FIVE = ("FX", "FU", "FXX", "FUX", "FUU")
TOPOLOGIES = ("chain6", "arm7", "biped12", "tree38")
SHAPES = ((2, 3), (3, 3))      # (batch, T)
# the tensor layouts and the schedules of tests/test_lin_overlap.py
ENVS = ((), (("DDP_HIP_K3_NO_PACK", "1"),), (("DDP_HIP_FXX_FULL", "1"),), (("DDP_HIP_K3_NO_SYM", "1"),), (("DDP_HIP_QWS_BT", "16"),),
        (("DDP_HIP_LIN_SERIAL", "1"),))


def _spec(capi, name, T, B, fd_mode=2, first_order_fd=1):
    if name in ("arm7", "biped12"):
        parents = {"arm7": robots.ARM7, "biped12": robots.BIPED12}[name]
        model = robots.seeded_tree(parents, seed=len(parents))
        return model, capi.ProblemSpec(model, T, batch=B, dt=0.01, c=1.0, fd_mode=fd_mode, first_order_fd=first_order_fd,
                                       eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    model, spec, _ = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=first_order_fd)
    return model, spec


def _inputs(model, T, B, seed):
    rng = np.random.default_rng(seed)
    n = 2 * model.nv
    return 0.1 * rng.normal(size=(B, (T + 1) * n)), 0.1 * rng.normal(size=(B, T * model.nv))


def _pair(capi, monkeypatch, spec, env=(), flags=0):
    """(staged context, scalar-path context): the switches are read once, by ddp_hip_create"""
    for name in OTHERS + (SWITCH,):
        monkeypatch.delenv(name, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    new = capi.Context(spec, flags=flags)
    monkeypatch.setenv(SWITCH, "1")
    old = capi.Context(spec, flags=flags)
    monkeypatch.delenv(SWITCH)
    for k, _ in env:
        monkeypatch.delenv(k)
    return new, old


def _equal(new, old, seqs, what):
    for s in seqs:
        a, r = new.download(s), old.download(s)
        assert a.shape == r.shape and a.size > 0, (what, s)
        assert not np.any(np.isnan(a)) and not np.any(np.isnan(r)), (what, s)
        assert np.array_equal(a, r), (what, s, int(np.sum(a != r)), a.size)


def _run(new, old, X, U, stages=((None,), (None,))):
    for ctx, st in zip((new, old), stages):
        ctx.upload("X", X)
        ctx.upload("U", U)
        for s in st:
            ctx.linearize(s)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_mode2_every_layout_and_schedule(gpu, monkeypatch, name, B, T):
    model, spec = _spec(gpu, name, T, B)
    X, U = _inputs(model, T, B, seed=11)
    for env in ENVS:
        new, old = _pair(gpu, monkeypatch, spec, env)
        with new, old:
            assert new.info()["lin_path"] >= 2 and old.info()["lin_path"] == new.info()["lin_path"]    # a static topology
            _run(new, old, X, U)
            _equal(new, old, FIVE, env)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_stage_by_stage_against_the_fused_call(gpu, monkeypatch, name, B, T):
    """first order alone, then second order alone (the separate f_u and u-diagonal launches) against one call that runs both
    (the fused u wave), each on the staged and on the scalar path"""
    capi = gpu
    model, spec = _spec(capi, name, T, B)
    X, U = _inputs(model, T, B, seed=12)
    staged = (capi.LIN_COST | capi.LIN_FIRST, capi.LIN_SECOND)
    for st_new, st_old in ((staged, (None,)), (staged, staged), ((None,), staged)):
        new, old = _pair(capi, monkeypatch, spec)
        with new, old:
            _run(new, old, X, U, (st_new, st_old))
            _equal(new, old, FIVE, (st_new, st_old))
    # ... and the two forms of the staged path against each other
    for k in OTHERS + (SWITCH,):
        monkeypatch.delenv(k, raising=False)
    with capi.Context(spec) as a, capi.Context(spec) as b:
        _run(a, b, X, U, (staged, (None,)))
        _equal(a, b, FIVE, "staged path: stage by stage / fused")


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_tensor_free_context(gpu, monkeypatch, name, B, T):
    capi = gpu
    model, spec = _spec(capi, name, T, B, fd_mode=0)
    X, U = _inputs(model, T, B, seed=13)
    new, old = _pair(capi, monkeypatch, spec, flags=capi.FLAG_NO_TENSORS)
    with new, old:
        assert new.info()["lin_path"] >= 2
        _run(new, old, X, U)
        _equal(new, old, ("FX", "FU"), "tensor-free")
        assert not new.device_ptr("FUU") and not old.device_ptr("FUU")     # no f_uu in memory: nothing for a u wave to touch


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("name", TOPOLOGIES)
def test_mode1_accelerations(gpu, monkeypatch, name, B, T):
    """analytic first order, forward differences of the jacobians: on the larger trees the perturbed points' accelerations come
    from the first-order waves (LinParams::accel_out)"""
    from test_dynamics_parity import DERIV_SEQS, TENSOR_SEQS
    capi = gpu
    model, spec = _spec(capi, name, T, B, fd_mode=1, first_order_fd=0)
    X, U = _inputs(model, T, B, seed=14)
    new, old = _pair(capi, monkeypatch, spec)
    with new, old:
        _run(new, old, X, U)
        seqs = [s for s in list(DERIV_SEQS.values()) + list(TENSOR_SEQS.values()) if new.seq_size(s)]
        assert "FXX" in seqs and "FU" in seqs
        _equal(new, old, seqs, "mode 1")
