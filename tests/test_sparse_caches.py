"""The static stencil's q-cache as a base block and deltas (lin_static.hip: QcLayout, LinPlan::qc_sparse).

In the local-frame ABA, record K of configuration 1+g (q_g stepped) differs from the base record only in E | r if K == g
and in U | 1/D | Ia if K is a strict ancestor of g; of the v-cache records a q_g step changes those of g's strict ancestors
and of its subtree, a v_g step those of its subtree.  The cache therefore keeps the base block and, per stepped joint, the
records the step changes; every reader selects between the two sources word by word and leaves the LDS image it left before.

The CPU part restates the kernels' tables and offsets in Python against a brute-force ancestor / subtree walk for every
compiled-in topology, checks in numpy that the q-part and the v-part are bit-equal outside the changed sets, and asserts the
counts the layout was sized by.  The GPU part requires np.array_equal between a default context and one created under
DDP_HIP_QCACHE_DENSE (whole blocks, the kernels as they were) for every output of a linearisation: F_VAL, FX, FU, FXX, FUX,
FUU and the cost's LFX, LFXX (the context has no sequences named LFU, LFUX or LFUU: the jacobians and tensors of f are FX ...
FUU)."""
import os
import subprocess

import numpy as np
import pytest

from problems import make
from robots import ARM7, BIPED12, seeded_tree
from test_cfg_splice import TOPOS, _Tree, _skew, spine_tables, strict_ancestors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddp_pinocchio_amd", "csrc")
QC_STRIDE, ER, UD, VC_STRIDE = 40, 12, 28, 18
SWITCHES = ("DDP_HIP_QCACHE_DENSE", "DDP_HIP_LIN_SERIAL", "DDP_HIP_LIN_FORKS", "DDP_HIP_K3_NO_PACK", "DDP_HIP_FXX_FULL",
            "DDP_HIP_K3_NO_SYM", "DDP_HIP_CFG_FULL_ABA", "DDP_HIP_NO_STATIC", "DDP_HIP_NO_QCACHE", "DDP_HIP_QWS_BT")


# ---- CPU: the tables and the layout, restated ------------------------------------------------------------------------------
def subtree_or_self(parent, g):
    """brute force: g and every joint that reaches g by walking up"""
    out = set()
    for k in range(len(parent)):
        a = k
        while a >= 0 and a != g:
            a = parent[a]
        if a == g:
            out.add(k)
    return out


def layout(parent):
    """QcLayout: the base block, then one delta block per stepped joint: E | r, then U | 1/D | Ia by ancestor depth"""
    N = len(parent)
    depth = spine_tables(parent)["depth"]
    maxd = max(1, max(depth))
    dw = ER + maxd * UD
    return dict(N=N, MAXD=maxd, DW=dw, DELTA=N * QC_STRIDE, PATH0=N * QC_STRIDE + ER, WORDS=N * QC_STRIDE + N * dw)


def qc_word(L, g, anc, K, e):
    """lin_static.hip: qc_word -- where word e of joint K's record at configuration 1+g lives (g = -1, anc = 0: the base)"""
    d = bin(anc & ((1 << K) - 1)).count("1")
    base = K * QC_STRIDE + e
    own = L["DELTA"] + g * L["DW"] + e
    path = L["PATH0"] + g * L["DW"] + d * UD + (e - ER)
    w_own = int(e < ER) & int(K == g)
    w_path = int(e >= ER) & ((anc >> K) & 1)
    return base + w_own * (own - base) + w_path * (path - base)


COUNTS = {  # topology: (q records a q step changes, v records a q step changes, v records a v step changes, N^2)
    "TopoTalos38": (369, 700, 369, 1444),
    "TopoChain6": (21, 36, 21, 36),
    "TopoArm7": (28, 49, 28, 49),
    "TopoBiped12": (48, 84, 48, 144),
}


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_changed_sets_and_layout_against_brute_force(name):
    parent, _ = TOPOS[name]
    N = len(parent)
    tab = spine_tables(parent)
    L = layout(parent)
    SA = [strict_ancestors(parent, g) for g in range(N)]
    SUB = [subtree_or_self(parent, g) for g in range(N)]
    nq = nvq = nvv = 0
    seen = {}
    for g in range(N):
        anc = tab["anc"][g]
        # a joint's subtree is one contiguous index range, and its ancestors have smaller indices (what the depth-by-popcount
        # rule and the v-cache's range rule rest on)
        assert SUB[g] == set(range(g, g + len(SUB[g]))), (name, g)
        assert all(a < g for a in SA[g])
        assert {K for K in range(N) if (anc >> K) & 1} == SA[g]
        for K in range(N):
            for e in range(QC_STRIDE):
                w = qc_word(L, g, anc, K, e)
                changed = (K == g) if e < ER else (K in SA[g])
                if not changed:
                    assert w == K * QC_STRIDE + e                       # the base record
                    continue
                assert L["DELTA"] + g * L["DW"] <= w < L["DELTA"] + (g + 1) * L["DW"] <= L["WORDS"]   # inside g's delta block
                if e >= ER:
                    assert w == L["PATH0"] + g * L["DW"] + tab["depth"][K] * UD + (e - ER) and tab["depth"][K] < L["MAXD"]
                assert seen.setdefault(w, (g, K, e)) == (g, K, e)       # no two words share a slot
        # the base configuration's rows (g = -1, no ancestors): the base block, every word
        assert all(qc_word(L, -1, 0, K, e) == K * QC_STRIDE + e for K in range(N) for e in range(QC_STRIDE))
        nq += 1 + len(SA[g])                  # records with a changed half
        nvq += len(SA[g] | SUB[g])
        nvv += len(SUB[g])
    assert (nq, nvq, nvv, N * N) == COUNTS[name]
    assert nq == N + sum(tab["depth"])
    if name == "TopoTalos38":
        assert max(tab["depth"]) == 15 and sum(tab["depth"]) == 331
        words = N * ER + sum(tab["depth"]) * UD
        assert round(100.0 * words / (N * N * QC_STRIDE)) == 17           # 17 % of the words of the 38 stepped blocks
        assert L["WORDS"] * 8 == 143_488 and (N + 1) * N * QC_STRIDE * 8 == 474_240


def _motion_cross(v):
    w, u = v[:3], v[3:]
    X = np.zeros((6, 6))
    X[:3, :3] = _skew(w)
    X[3:, 3:] = _skew(w)
    X[3:, :3] = _skew(u)
    return X


def _vpart(tr, X, rec, v):
    """rbd::aba_vpart_cached in numpy: per joint cb | pA0 | Ia cb from the q-part's records and the velocities"""
    vel, out = [None] * tr.N, [None] * tr.N
    for K in range(tr.N):
        vJ = tr.S[K] * v[K]
        vel[K] = vJ if tr.parent[K] < 0 else X[K] @ vel[tr.parent[K]] + vJ
        cb = _motion_cross(vel[K]) @ vJ
        pA = -_motion_cross(vel[K]).T @ (tr.I6[K] @ vel[K])
        out[K] = (cb, pA, rec[K][2] @ cb)
    return out


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_records_outside_the_changed_sets_are_bit_equal(name):
    """numpy q-part and v-part at every stepped point against the base point: np.array_equal outside the changed sets.  (Inside
    them a record need not move -- velocities are local, so a step of the root joint's position moves no v record at all -- but
    the q-part's sets are tight for a generic model.)"""
    parent, pris = TOPOS[name]
    tr = _Tree(parent, pris, seed=11)
    N, eps = tr.N, 2.0 ** -13
    v0 = np.random.default_rng(12).normal(size=N)
    X0, R0 = tr.qpart(tr.q0)
    V0 = _vpart(tr, X0, R0, v0)
    eq = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    moved = 0
    for g in range(N):
        SA, SUB = strict_ancestors(parent, g), subtree_or_self(parent, g)
        q = tr.q0.copy()
        q[g] += eps
        Xg, Rg = tr.qpart(q)
        Vq = _vpart(tr, Xg, Rg, v0)
        v = v0.copy()
        v[g] += eps
        Vv = _vpart(tr, X0, R0, v)
        for K in range(N):
            assert np.array_equal(Xg[K], X0[K]) == (K != g), (g, K)                 # E | r
            assert eq(Rg[K], R0[K]) == (K not in SA), (g, K)                          # U | 1/D | Ia
            assert eq(Vq[K], V0[K]) or K in SA | SUB, (g, K)                          # v records, q_g stepped
            assert eq(Vv[K], V0[K]) or K in SUB, (g, K)                               # v records, v_g stepped
        moved += sum(not eq(Vq[K], V0[K]) for K in range(N)) + sum(not eq(Vv[K], V0[K]) for K in range(N))
    assert moved > 0


def test_plan_reports_the_layout():
    """the flagship plan through read_switches and lin_plan_decide (a host program: no device)"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_table"])

    def caches(env):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        out = subprocess.run([os.path.join(ROOT, "build", "lin_plan_table"), "caches"], capture_output=True, text=True, check=True, env=e).stdout.split()
        return dict(zip(out[0::2], (int(v) for v in out[1::2])))
    assert caches({}) == {"qc_sparse": 1, "ncfg": 39, "nvcfg": 77}
    assert caches({"DDP_HIP_QCACHE_DENSE": "1"})["qc_sparse"] == 0
    assert caches({"DDP_HIP_CFG_FULL_ABA": "1"})["qc_sparse"] == 0          # cfg_up / cfg_down read whole blocks
    assert caches({"DDP_HIP_NO_STATIC": "1"})["qc_sparse"] == 0             # the run-time-tree kernels know whole blocks only
    assert caches({"DDP_HIP_LIN_SERIAL": "1"})["qc_sparse"] == 1


# ---- GPU: base + deltas against whole blocks, bit for bit ------------------------------------------------------------------
SEQS = ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU", "LFX", "LFXX")
T, B = 3, 3        # 9 (instance, t): 351 configuration lanes, 9 x 38 step lanes -- both cache kernels end in a partial wave


def _problem(capi, name):
    """(spec, X, U): a posture held under computed-torque control from a moving start (non-zero velocities at every t), random
    u on top"""
    from oracle.binding import Oracle
    if name in ("tree38", "chain6"):
        model, spec, o = make(name, T, batch=B, fd_mode=2, first_order_fd=1)
    else:
        parents = {"arm7": ARM7, "biped12": BIPED12}[name]
        model = seeded_tree(parents, seed=len(parents))
        kw = dict(dt=0.01, c=1.0, fd_mode=2, first_order_fd=1, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
        spec = capi.ProblemSpec(model, T, batch=B, **kw)
        o = Oracle(model, T, **kw)
    nv = model.nv
    X, U = [], []
    for b in range(B):
        rng = np.random.default_rng(40 + b)
        q0 = 0.3 * rng.normal(size=nv)
        x = np.concatenate([q0, 0.2 * rng.normal(size=nv)])
        x0, us = x.copy(), np.zeros(T * nv)
        for t in range(T):
            us[t * nv:(t + 1) * nv] = o.rnea(x[:nv], x[nv:], -100.0 * (x[:nv] - q0) - 20.0 * x[nv:]) + 0.3 * rng.normal(size=nv)
            x = o.eval_f(x, us[t * nv:(t + 1) * nv])
        xs = o.rollout(x0, us)
        assert np.all(np.isfinite(xs)) and all(np.max(np.abs(xs[t * 2 * nv + nv:(t + 1) * 2 * nv])) > 0 for t in range(T))
        X.append(xs)
        U.append(us)
    return spec, np.stack(X), np.stack(U)


def _pair(capi, monkeypatch, spec, env=(), dense_env=(("DDP_HIP_QCACHE_DENSE", "1"),)):
    """(default context, its partner): the switches are read once, by ddp_hip_create"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env:
        monkeypatch.setenv(k, v)
    new = capi.Context(spec)
    for k, v in dense_env:
        monkeypatch.setenv(k, v)
    old = capi.Context(spec)
    for k, _ in tuple(env) + tuple(dense_env):
        monkeypatch.delenv(k, raising=False)
    return new, old


def _equal(new, old):
    for s in SEQS:
        if not new.seq_size(s):
            continue
        a, r = new.download(s), old.download(s)
        assert a.shape == r.shape and a.size > 0, s
        assert np.all(np.isfinite(r)), s
        assert np.array_equal(a, r), (s, int(np.sum(a != r)), a.size)


def _run(capi, monkeypatch, name, lin_path, env=(), dense_env=(("DDP_HIP_QCACHE_DENSE", "1"),), asynchronous=False):
    spec, X, U = _problem(capi, name)
    new, old = _pair(capi, monkeypatch, spec, env, dense_env)
    with new, old:
        assert new.info()["lin_path"] == lin_path and old.info()["lin_path"] == lin_path      # the static kernels of that topology
        for ctx in (new, old):
            ctx.upload("X", X)
            ctx.upload("U", U)
            if asynchronous:
                ctx.set_async(True)
            ctx.linearize()
            if asynchronous:
                ctx.linearize()          # the caches written again behind their readers, no host synchronisation in between
        _equal(new, old)
        if asynchronous:
            for ctx in (new, old):
                ctx.set_async(False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lin_path", [("tree38", 2), ("chain6", 3), ("arm7", 4), ("biped12", 5)])
def test_sparse_against_dense(gpu, monkeypatch, name, lin_path):
    _run(gpu, monkeypatch, name, lin_path)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [
    (("DDP_HIP_LIN_SERIAL", "1"),),          # the single-stream order
    (("DDP_HIP_K3_NO_PACK", "1"),),          # the contract layout
], ids=["serial", "contract_layout"])
def test_sparse_against_dense_under_switch(gpu, monkeypatch, env):
    _run(gpu, monkeypatch, "tree38", 2, env=env, dense_env=env + (("DDP_HIP_QCACHE_DENSE", "1"),))


@pytest.mark.gpu
def test_sparse_against_dense_across_workspace_slices(gpu, monkeypatch):
    """more than one workspace slice, forced the way test_cfg_splice.py forces it (DDP_HIP_QWS_BT): T = 24, batch 3 is 72
    (instance, t) on a 16-entry workspace -- the first order's q columns run five slices, the spine sets two"""
    capi = gpu
    Tn = 24
    model, spec, _ = make("tree38", Tn, batch=B, fd_mode=2, first_order_fd=1)
    rng = np.random.default_rng(50)
    X, U = 0.1 * rng.normal(size=(B, (Tn + 1) * 2 * model.nv)), 0.1 * rng.normal(size=(B, Tn * model.nv))
    env = (("DDP_HIP_QWS_BT", "16"),)
    new, old = _pair(capi, monkeypatch, spec, env, env + (("DDP_HIP_QCACHE_DENSE", "1"),))
    with new, old:
        for ctx in (new, old):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.linearize()
        _equal(new, old)


@pytest.mark.gpu
def test_sparse_against_dense_async(gpu, monkeypatch):
    _run(gpu, monkeypatch, "tree38", 2, asynchronous=True)


@pytest.mark.gpu
def test_full_aba_implies_whole_blocks(gpu, monkeypatch):
    """DDP_HIP_CFG_FULL_ABA alone (cfg_up / cfg_down read whole blocks, so the plan keeps them) against the same switch with
    DDP_HIP_QCACHE_DENSE spelled out: the implied layout works, and is the dense one"""
    env = (("DDP_HIP_CFG_FULL_ABA", "1"),)
    _run(gpu, monkeypatch, "tree38", 2, env=env, dense_env=env + (("DDP_HIP_QCACHE_DENSE", "1"),))
