"""The linearisation plan (csrc/lin_plan.cpp: lin_plan_decide) over the whole cross product of its inputs, on the CPU: a small host
program compiled from that one file prints one line per combination -- model kind x nv in {1, 6, 7, 38, 39, 64} x free flyer x
first_order_fd x fd_mode x tensors x Etot in {0, > 0} x eq_kind x eq_advance in {1, 2, 3} x topology matched or not x each
development switch on its own -- and the invariants below follow from what the kernels of each leg read, not from the plan's
own code.  They are held on the combinations a context can be created with: `created` (ddp_hip_create's argument checks) and
not `refuse` (lin_setup's refusal).  Together they make the refusals that used to sit behind the launches unreachable."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddp_pinocchio_amd", "csrc")

# the enums of csrc/internal.h, in their order
BASE, ANALYTIC_SMALL, ANALYTIC_WAVE, ANALYTIC_FF, FD_STATIC, FD_GENERIC = range(6)
S_NONE, S_ZEROS, S_MODE2_STATIC, S_MODE2_CACHES, S_MODE2_PLAIN, S_MODE1_SMALL, S_MODE1_WAVE = range(7)
EQ_NONE, EQ_PER_LANE, EQ_ANALYTIC, EQ_CHAIN = range(4)
J_NONE, J_FD, J_FF = range(3)
E_NONE, E_ZEROS, E_MODE2, E_MODE1_SMALL, E_MODE1_WAVE = range(5)
KIND_NONE, KIND_CONFIG, KIND_FRAME = range(3)


class Table:
    def __init__(self, names, switches, rows):
        self.switches = switches
        self.n = rows.shape[0]
        for k, name in enumerate(names):
            setattr(self, name, rows[:, k])

    def on(self, switch):
        return self.sw == self.switches.index(switch)


@pytest.fixture(scope="module")
def table():
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_table"])
    out = subprocess.run([os.path.join(ROOT, "build", "lin_plan_table")], capture_output=True, text=True, check=True).stdout
    head, sw, body = out.split("\n", 2)
    names = head.split()
    rows = np.fromstring(body, dtype=np.int64, sep=" ").reshape(-1, len(names))
    t = Table(names, sw.split()[1:], rows)
    assert t.n == 2 * 6 * 2 * 2 * 3 * 2 * 2 * 3 * 3 * 2 * 13        # the full cross product
    t.live = (t.created == 1) & (t.refuse == 0)
    return t


def implies(t, a, b, what):
    bad = np.flatnonzero(t.live & a & ~b)
    assert bad.size == 0, f"{what}: {bad.size} combinations, first at table row {bad[0]}"


def test_every_leg_has_the_workspaces_it_reads(table):
    t = table
    static_ws = (t.topo > 0) & (t.ws_lin == 1) & (t.ws_qws == 1)
    stencil_caches = (t.ws_lin == 1) & (t.ncfg == t.nv + 1) & (t.nvcfg == 2 * t.nv + 1)
    split = t.on("ana_split")
    # the static-topology kernels read the caches and the configuration-level workspace; the stencil, every cache entry
    implies(t, t.first == FD_STATIC, static_ws & (t.ncfg >= 1) & (t.nvcfg >= 1), "FdStatic")
    implies(t, t.second == S_MODE2_STATIC, static_ws & stencil_caches, "Mode2Static")
    implies(t, (t.second == S_MODE2_STATIC) & t.on("cfg_full_aba"), t.ws_qws2 == 1, "Mode2Static, full ABA")
    implies(t, t.second == S_MODE2_CACHES, stencil_caches & (t.topo == 0), "Mode2Caches")
    # lin_analytic.hip: every launch is sliced by ana_nbt; the three-kernel form reads T and M, the fused stage 1 reads M^-1 at the
    # trajectory points, ana_eq_kernel's stage 1 reads F and M per slice, the static accelerations land in A
    wave_leg = (t.first == ANALYTIC_WAVE) | (t.second == S_MODE1_WAVE) | (t.eq == EQ_ANALYTIC) | (t.eq_second == E_MODE1_WAVE)
    implies(t, wave_leg | (t.first == ANALYTIC_FF) | (t.eq_jac == J_FF), t.ana_sliced == 1, "analytic legs")
    implies(t, wave_leg, (t.first == ANALYTIC_WAVE) & (t.nj >= 38) & (t.ff == 0), "wave legs come with the wave first order")
    implies(t, wave_leg & split, (t.ws_ana_T == 1) & (t.ws_ana_M == 1), "three-kernel analytic form")
    implies(t, (t.second == S_MODE1_WAVE) & ~split, t.ws_ana_M0 == 1, "fused mode 1")
    implies(t, (t.eq_second == E_MODE1_WAVE) & (t.eq_inline == 0), (t.ws_ana_F == 1) & (t.ws_ana_M == 1), "mode-1 constraint tensors")
    implies(t, t.eq_inline == 1, (t.eq_second == E_MODE1_WAVE) & (t.eq_kind == KIND_CONFIG) & ~split, "inline constraint tensors")
    implies(t, t.accel_static == 1, (t.ws_ana_A == 1) & static_ws & (t.second == S_MODE1_WAVE), "static accelerations")
    implies(t, t.accel_with_u == 1, (t.accel_static == 1) & (t.etot == 1), "static accelerations along u")
    # the constraint chain: the three kernels read eq_ws, whose partition fits the allocation
    implies(t, t.eq == EQ_CHAIN, t.ws_eq == 1, "Chain")
    implies(t, t.ws_eq == 1, (0 < t.eq_fxk_off) & (t.eq_fxk_off <= t.eq_c_off) & (t.eq_c_off < t.eq_words), "eq_ws partition")
    implies(t, (t.eq_jac != J_NONE), (t.eq == EQ_CHAIN) & (t.K > 1) & (t.eq_c_off > t.eq_fxk_off), "look-ahead jacobians")
    implies(t, (t.eq == EQ_CHAIN) & (t.K > 1), t.eq_jac == np.where(t.fo_fd == 1, J_FD, J_FF), "look-ahead jacobians' source")
    implies(t, t.etot == 1, t.eq != EQ_NONE, "constraint rows without a leg")
    implies(t, t.etot == 0, (t.eq == EQ_NONE) & (t.eq_second == E_NONE), "a constraint leg without rows")


def test_legs_that_cannot_run_are_never_selected(table):
    """the refusals the launch code used to carry (DDP_HIP_E_UNSUPPORTED at linearise time)"""
    t = table
    m1 = (t.second == S_MODE1_SMALL) | (t.second == S_MODE1_WAVE)
    analytic = (t.first == ANALYTIC_SMALL) | (t.first == ANALYTIC_WAVE) | (t.first == ANALYTIC_FF) | (t.first == BASE)
    implies(t, m1, analytic, "mode 1 differences analytic jacobians only")
    implies(t, t.eq == EQ_CHAIN, (t.eq_second != E_MODE1_SMALL) & (t.eq_second != E_MODE1_WAVE), "Chain has no mode-1 tensors")
    implies(t, t.eq_second == E_MODE1_SMALL, (t.eq == EQ_PER_LANE) & (t.nj <= 6), "one-lane mode-1 constraint tensors")
    implies(t, t.eq_second == E_MODE1_WAVE, t.eq == EQ_ANALYTIC, "wave mode-1 constraint tensors")
    implies(t, t.first == ANALYTIC_FF, ~m1 & ((t.eq == EQ_NONE) | (t.eq == EQ_CHAIN)), "free flyer: first order only")
    # the one-lane kernels exist for NJ <= 6 only
    small_leg = (t.first == ANALYTIC_SMALL) | (t.second == S_MODE1_SMALL) | (t.eq == EQ_PER_LANE) | (t.eq_second == E_MODE1_SMALL)
    implies(t, small_leg, t.nj <= 6, "one-lane kernels")
    implies(t, t.nj > 0, t.nj == np.where(t.nv <= 1, 1, np.where((t.nv <= 6) & (t.ff == 0), 6, np.where(t.nv <= 38, 38, 64))), "NJ")
    implies(t, t.tensors == 0, (t.second == S_NONE) & (t.eq_second == E_NONE) & (t.has_tensors == 0), "tensor-free")
    implies(t, t.tensors == 1, (t.second != S_NONE) & (t.has_tensors == 1), "tensors")


def test_structural_marks(table):
    t = table
    implies(t, t.skip_top == 1, (t.topo > 0) & (t.mode == 2) & (t.tensors == 1), "skip_top")
    implies(t, t.skip_qv_mirror == 1, (t.sym_ok == 1) & (t.skip_top == 1), "skip_qv_mirror")
    implies(t, t.accel_static == 1, (t.matched == 1) & (t.mode == 1) & (t.tensors == 1) & (t.ff == 0), "static accelerations")
    # (the stencil's caches: the static stencil is the one with a full-ABA configuration level)
    implies(t, t.ws_qws2 == 1, t.on("cfg_full_aba") & (t.second == S_MODE2_STATIC), "lin_qws2")
    implies(t, t.on("cfg_full_aba") & (t.second == S_MODE2_STATIC), t.ws_qws2 == 1, "lin_qws2")
    implies(t, t.m1_fused == 1, (t.first == ANALYTIC_WAVE) & (t.second == S_MODE1_WAVE) & (t.mode == 1) & (t.etot == 1), "m1_fused")
    implies(t, t.ncfg > 1, (t.mode == 2) & (t.tensors == 1) & (t.kind == 1) & (t.ff == 0), "ncfg > 1")
    implies(t, t.topo > 0, (t.matched == 1) & ~t.on("no_static") & (t.kind == 1), "static topology")
    assert np.any(t.live & (t.skip_qv_mirror == 1)) and np.any(t.live & (t.m1_fused == 1)) and np.any(t.live & (t.ws_qws2 == 1))


def test_every_leg_is_reached_and_every_refusal_is_there(table):
    t = table
    for col, count in (("first", 6), ("second", 7), ("eq", 4), ("eq_jac", 3), ("eq_second", 5)):
        assert set(np.unique(getattr(t, col)[t.live])) == set(range(count)), col
    created = t.created == 1
    # lin_setup's refusals (ddp_hip_create returns DDP_HIP_E_UNSUPPORTED): mode 1 on forward-differenced jacobians; more than two
    # look-ahead steps on the analytic constraint chain; a free flyer past the 38-joint instantiation of its analytic kernel
    wave = (t.kind == 1) & (t.fo_fd == 0) & (t.ff == 0) & (t.nv > 6)
    expect = ((t.mode == 1) & (t.fo_fd == 1) & (t.tensors == 1)) | (wave & (t.etot == 1) & (t.K > 2)) | \
             ((t.kind == 1) & (t.fo_fd == 0) & (t.ff == 1) & (t.nv > 38))
    assert np.array_equal(t.refuse[created] == 1, expect[created])


def test_pinned_paths(table):
    """what the GPU suite pins of ddp_hip_ctx_info, at the table's sizes (a matched topology has id 1 here: lin_path 2)"""
    t = table

    def rows(**kw):
        sel = t.live & t.on(kw.pop("switch", "none"))
        for k, v in kw.items():
            sel = sel & (getattr(t, k) == v)
        assert np.any(sel)
        return sel

    tree38 = dict(kind=1, nv=38, ff=0, matched=1, tensors=1)
    # tests/test_at_size.py: tree38, mode 2, default (forward-differenced) first order: static TopoTalos38
    assert np.all(t.lin_path[rows(mode=2, fo_fd=1, **tree38)] == 2)
    # tests/test_analytic_derivs.py: tree38, mode 1, analytic: first_order 2; lin_path 2 (the static accelerations), 1 under ANA_OWN_ABA
    sel = rows(mode=1, fo_fd=0, **tree38)
    assert np.all(t.first_order[sel] == 2) and np.all(t.lin_path[sel] == 2) and np.all(t.accel_static[sel] == 1)
    sel = rows(mode=1, fo_fd=0, switch="ana_own_aba", **tree38)
    assert np.all(t.lin_path[sel] == 1) and np.all(t.accel_static[sel] == 0)
    # tests/test_generated_topology.py: a 7-joint tree with a compiled-in topology: 1 + its id; TREE44 (no topology, the 64
    # instantiation): lin_path 1; analytic mode 1 on both: first_order 2
    sel = rows(kind=1, nv=7, ff=0, matched=1, tensors=1, mode=1, fo_fd=0)
    assert np.all(t.lin_path[sel] == 1 + t.topo[sel]) and np.all(t.topo[sel] == 1) and np.all(t.first_order[sel] == 2)
    sel = rows(kind=1, nv=39, ff=0, matched=0, tensors=1, mode=1, fo_fd=0)
    assert np.all(t.lin_path[sel] == 1) and np.all(t.first_order[sel] == 2) and np.all(t.nj[sel] == 64)
    # tests/test_ff_analytic.py: tree38ff, mode 0, analytic: first_order 2
    assert np.all(t.first_order[rows(kind=1, nv=38, ff=1, mode=0, fo_fd=0)] == 2)
    # tests/test_cfg_splice.py: chain6 / tree38 in mode 2: a static topology (lin_path >= 2)
    assert np.all(t.lin_path[rows(kind=1, nv=6, ff=0, matched=1, tensors=1, mode=2, fo_fd=1)] >= 2)
    # include/ddp_hip/ddp_hip.h: the pendulum reports 0 / 0
    sel = rows(kind=0)
    assert np.all(t.lin_path[sel] == 0) and np.all(t.first_order[sel] == 0)
