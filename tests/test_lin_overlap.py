"""The concurrent schedule of a static-topology linearisation (LinPlan::forks) against the single-stream
order kept behind DDP_HIP_LIN_SERIAL.

No kernel changes with the schedule, so every output is equal bit for bit; what can go wrong is an edge of the launch graph: a
kernel started ahead of what it reads, two users of the configuration-level workspace overlapping, a side stream left running
when the entry point returns.  Every GPU test builds two contexts in one process -- the default one and one created under the
switch -- on the same model and inputs and requires np.array_equal.  The CPU test reads the schedule off the plan."""
import os
import subprocess

import numpy as np
import pytest

from problems import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddp_pinocchio_amd", "csrc")
SIX = ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU")
SWITCHES = ("DDP_HIP_LIN_SERIAL", "DDP_HIP_LIN_FORKS", "DDP_HIP_K3_NO_PACK", "DDP_HIP_FXX_FULL", "DDP_HIP_K3_NO_SYM",
            "DDP_HIP_CFG_FULL_ABA", "DDP_HIP_NO_STATIC", "DDP_HIP_QWS_BT")


def _inputs(model, T, B, seed):
    """x, u ~ N(0, 0.1^2): every (instance, t) a point of its own (a linearisation does not need a rollout)"""
    rng = np.random.default_rng(seed)
    n = 2 * model.nv
    return 0.1 * rng.normal(size=(B, (T + 1) * n)), 0.1 * rng.normal(size=(B, T * model.nv))


def _pair(capi, monkeypatch, spec, env=()):
    """(concurrent context, serial context): the switches are read once, by ddp_hip_create"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    conc = capi.Context(spec)
    monkeypatch.setenv("DDP_HIP_LIN_SERIAL", "1")
    ser = capi.Context(spec)
    monkeypatch.delenv("DDP_HIP_LIN_SERIAL")
    return conc, ser


def _equal(conc, ser, seqs):
    for s in seqs:
        a, r = conc.download(s), ser.download(s)
        assert a.shape == r.shape and a.size > 0, s
        assert np.all(np.isfinite(r)), s
        assert np.array_equal(a, r), (s, int(np.sum(a != r)), a.size)


def _six_arrays(capi, monkeypatch, name, B, T, env=(), seed=5):
    model, spec, _ = make(name, T, batch=B, fd_mode=2, first_order_fd=1)
    X, U = _inputs(model, T, B, seed)
    conc, ser = _pair(capi, monkeypatch, spec, env)
    with conc, ser:
        assert conc.info()["lin_path"] >= 2 and ser.info()["lin_path"] == conc.info()["lin_path"]    # a static topology
        for ctx in (conc, ser):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.linearize()
        _equal(conc, ser, SIX)


@pytest.mark.gpu
def test_talos_tree_across_workspace_slices(gpu, monkeypatch):
    """BT = 200 with a 16-entry workspace: the first order's q columns run two slices (176 and 24), the configuration level four
    (66 spine sets each, the last one short), both on the one workspace, whose hand-over between slices and between its two users
    the fork must respect."""
    _six_arrays(gpu, monkeypatch, "tree38", 4, 50, env=(("DDP_HIP_QWS_BT", "16"),))


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["DDP_HIP_K3_NO_PACK", "DDP_HIP_FXX_FULL", "DDP_HIP_K3_NO_SYM"])
def test_other_tensor_layouts(gpu, monkeypatch, switch):
    """the contract layout, and the layout with mirror images and zero rows: the branches write disjoint columns there as well"""
    _six_arrays(gpu, monkeypatch, "tree38", 2, 12, env=((switch, "1"), ("DDP_HIP_QWS_BT", "16")))


@pytest.mark.gpu
def test_compiled_in_small_topology(gpu, monkeypatch):
    """TopoChain6: 15 pairs, one wave of them per (instance, t); the joins hold on a degenerate branch structure"""
    model, spec, _ = make("chain6", 20, batch=3, fd_mode=2, first_order_fd=1)
    X, U = _inputs(model, 20, 3, seed=6)
    conc, ser = _pair(gpu, monkeypatch, spec)
    with conc, ser:
        assert conc.info()["lin_path"] >= 2 and ser.info()["lin_path"] == conc.info()["lin_path"]
        for ctx in (conc, ser):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.linearize()
        _equal(conc, ser, SIX + ("EQ_X", "EQ_XX"))


@pytest.mark.gpu
def test_five_linearisations_without_host_synchronisation(gpu, monkeypatch):
    """Async mode, the trajectory buffers swapped between calls so that consecutive calls read different inputs: a side stream
    still running at return would have its caches overwritten by the next call."""
    capi = gpu
    B, T = 4, 50
    model, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    X, U = _inputs(model, T, B, seed=7)
    X2, U2 = _inputs(model, T, B, seed=8)
    conc, ser = _pair(capi, monkeypatch, spec, env=(("DDP_HIP_QWS_BT", "16"),))
    with conc, ser:
        for ctx in (conc, ser):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.upload("X_NEW", X2)
            ctx.upload("U_NEW", U2)
            ctx.set_async(True)
        for ctx in (conc, ser):
            for k in range(5):
                ctx.linearize()
                if k < 4:
                    ctx.swap_traj()
        _equal(conc, ser, SIX)              # (a download waits for the context's stream, and for nothing else)
        for ctx in (conc, ser):
            ctx.set_async(False)
        assert np.array_equal(conc.download("X"), X) and np.array_equal(ser.download("X"), X)   # four swaps: back where it began


@pytest.mark.gpu
def test_sweeps_between_two_linearisations(gpu, monkeypatch):
    """linearise, backward, forward, swap, linearise: the sweeps run on the context's stream alone and must see finished tensors"""
    capi = gpu
    B, T = 2, 12
    model, spec, o = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    rng = np.random.default_rng(9)
    U = 0.1 * rng.normal(size=(B, T * model.nv))
    x0 = np.zeros(2 * model.nv)
    X = np.stack([o.rollout(x0, U[b]) for b in range(B)])
    conc, ser = _pair(capi, monkeypatch, spec)
    got = []
    with conc, ser:
        for ctx in (conc, ser):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.upload("X_NEW", X)
            ctx.upload("U_NEW", U)
            ctx.linearize()
            rc, reg, mu, restarts = ctx.backward(0.0, 1.0)
            assert rc == 0
            rc, step, dcost = ctx.forward(mu, n_alpha=8)
            ctx.swap_traj()
            ctx.linearize()
            got.append((reg, mu, step, restarts, dcost))
        for a, r in zip(got[0], got[1]):
            assert np.array_equal(a, r), (a, r)
        _equal(conc, ser, ("FB_VAL", "FB_JAC", "X", "U", "COSTS_OLD") + SIX)


@pytest.mark.gpu
def test_stage_by_stage(gpu, monkeypatch):
    """first order alone, then second order alone: the second call builds the caches again inside its own bracket, and its spine
    pre-pass, forked right behind them, finds the workspace as the first call's q columns left it"""
    capi = gpu
    B, T = 2, 12
    model, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    X, U = _inputs(model, T, B, seed=10)
    conc, ser = _pair(capi, monkeypatch, spec, env=(("DDP_HIP_QWS_BT", "16"),))
    with conc, ser:
        for ctx in (conc, ser):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.linearize(capi.LIN_COST | capi.LIN_FIRST)
            ctx.linearize(capi.LIN_SECOND)
        _equal(conc, ser, SIX)


def _schedule(env):
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_table"])
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    out = subprocess.run([os.path.join(ROOT, "build", "lin_plan_table"), "schedule"], capture_output=True, text=True, check=True, env=e).stdout.split()
    return dict(zip(out[0::2], (int(v) for v in out[1::2])))


def test_plan_reports_the_schedule():
    """the flagship plan through read_switches and lin_plan_decide (a host program: no device): the forks are there by default,
    gone under the switch, one at a time under the A/B knob, and never beside the full-ABA level's own two-stream pipeline"""
    default = _schedule({})
    assert default["topo"] == 1 and default["forks"] == 3
    assert _schedule({"DDP_HIP_LIN_SERIAL": "1"})["forks"] == 0
    assert _schedule({"DDP_HIP_LIN_FORKS": "1"})["forks"] == 1
    assert _schedule({"DDP_HIP_LIN_FORKS": "1", "DDP_HIP_LIN_SERIAL": "1"})["forks"] == 0
    assert _schedule({"DDP_HIP_CFG_FULL_ABA": "1"})["forks"] == 0
    assert _schedule({"DDP_HIP_NO_STATIC": "1"}) == {"forks": 0, "topo": 0}
