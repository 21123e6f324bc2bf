"""The static stencil's v-cache as base blocks and deltas (lin_static.hip: VcLayout, vc_word, LinPlan::vc_sparse).

Of the v records (cb | pA0 | Ia cb) a q_g step changes those of g's strict ancestors and of g's subtree, a v_g step those of g's
subtree (test_sparse_caches.py states the sets and checks them in numpy).  Per (instance, t) the cache keeps entry 0 (the base
(q, v), written by the configuration fill), a v-step base block (the unstepped point as the v-step fill's own instruction stream
forms it: lane nv of that kernel), and per stepped joint the records its step changes, packed exactly.  A fill lane stores a
record its step does not change onto the base block of its own kernel, where another lane of the same kernel stores the same
bits; the torque rows select between base block and deltas word by word and leave the LDS image they left before.

The CPU part restates the offset tables and vc_word in Python against a brute-force ancestor / subtree walk for every compiled-in
topology.  The GPU part requires np.array_equal between a default context and one created under DDP_HIP_VCACHE_DENSE (77 whole
entries, the kernels as they were) for every output of a linearisation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from problems import make
from test_cfg_splice import TOPOS, spine_tables, strict_ancestors
from test_sparse_caches import B, COUNTS, CSRC, ROOT, VC_STRIDE, _equal, _pair, _run, subtree_or_self

SWITCHES = ("DDP_HIP_VCACHE_DENSE", "DDP_HIP_QCACHE_DENSE", "DDP_HIP_LIN_SERIAL", "DDP_HIP_LIN_FORKS", "DDP_HIP_K3_NO_PACK",
            "DDP_HIP_FXX_FULL", "DDP_HIP_K3_NO_SYM", "DDP_HIP_CFG_FULL_ABA", "DDP_HIP_NO_STATIC", "DDP_HIP_NO_QCACHE", "DDP_HIP_QWS_BT")
TOPO_ID = {"TopoTalos38": 1, "TopoChain6": 2, "TopoArm7": 3, "TopoBiped12": 4}     # lin_static_supported: lin_path - 1
DENSE = (("DDP_HIP_VCACHE_DENSE", "1"),)
R = VC_STRIDE


# ---- CPU: the tables and the address function, restated ---------------------------------------------------------------------
def vc_tab(parent):
    """make_vc_tab: entry 0 | the v-step base block | q-step deltas of g = 0 .. N-1 (strict ancestors root first, then the subtree)
    | v-step deltas of g = 0 .. N-1 (the subtree); offsets in doubles"""
    N = len(parent)
    depth, sub = [0] * N, [1] * N
    for k in range(N):
        a = parent[k]
        while a >= 0:
            depth[k] += 1
            sub[a] += 1
            a = parent[a]
    off, qoff, voff = 2 * N * R, [], []
    for g in range(N):
        qoff.append(off)
        off += (depth[g] + sub[g]) * R
    for g in range(N):
        voff.append(off)
        off += sub[g] * R
    return dict(N=N, VB=N * R, qoff=qoff, voff=voff, sub=sub, words=off)


def vc_word(L, kind, g, anc, K, e):
    """lin_static.hip: vc_word -- where word e of joint K's v record lives with q_g (kind 0; g = -1: entry 0) or v_g (kind 1) stepped"""
    gi = max(g, 0)
    nsub = 0 if g < 0 else L["sub"][gi]
    off = L["voff"][gi] if kind else L["qoff"][gi]
    a = 0 if kind else anc
    dg, d = bin(a).count("1"), bin(a & ((1 << K) - 1)).count("1")
    base = kind * L["VB"] + K * R + e
    below = off + (dg + K - g) * R + e
    path = off + d * R + e
    w_below = int(K >= g) & int(K < g + nsub)
    w_path = (a >> K) & 1
    return base + w_below * (below - base) + w_path * (path - base)


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_layout_against_brute_force(name):
    parent, _ = TOPOS[name]
    N = len(parent)
    tab = spine_tables(parent)
    L = vc_tab(parent)
    SA = [strict_ancestors(parent, g) for g in range(N)]
    SUB = [subtree_or_self(parent, g) for g in range(N)]
    seen = {}
    nchanged = [0, 0]
    for kind in (0, 1):
        for g in range(N):
            anc = tab["anc"][g]
            changed = (SA[g] | SUB[g]) if kind == 0 else SUB[g]
            assert not SA[g] & SUB[g]
            lo = (L["qoff"] if kind == 0 else L["voff"])[g]
            hi = lo + len(changed) * R                                   # packed exactly: as many slots as changed records
            for K in range(N):
                # the row of a v step hands vc_word whatever ancestors it has at hand: they must not matter
                words = [vc_word(L, kind, g, anc, K, e) for e in range(R)]
                if kind == 1:
                    assert words == [vc_word(L, kind, g, 0, K, e) for e in range(R)]
                assert words == list(range(words[0], words[0] + R))      # a record stays one run of 18 words
                if K not in changed:
                    assert words[0] == kind * L["VB"] + K * R            # its own base block
                    continue
                assert lo <= words[0] and words[-1] < hi <= L["words"]
                assert (words[0] - lo) % R == 0
                assert seen.setdefault(words[0], (kind, g, K)) == (kind, g, K)      # no two records share a slot
                nchanged[kind] += 1
                if kind == 0 and K in SA[g]:
                    assert words[0] == lo + tab["depth"][K] * R           # ancestors root first
                else:
                    assert words[0] == lo + ((tab["depth"][g] if kind == 0 else 0) + K - g) * R
    # the delta blocks tile their region: nothing between them
    assert L["qoff"][0] == 2 * N * R and L["voff"][0] == L["qoff"][0] + nchanged[0] * R and L["words"] == L["voff"][0] + nchanged[1] * R
    assert len(seen) == nchanged[0] + nchanged[1] and min(seen) == 2 * N * R and max(seen) == L["words"] - R
    # entry 0 (the base configuration's rows: g = -1, no ancestors), every word
    assert all(vc_word(L, 0, -1, 0, K, e) == K * R + e for K in range(N) for e in range(R))
    assert (nchanged[0], nchanged[1], N * N) == COUNTS[name][1:]
    if name == "TopoTalos38":
        assert nchanged == [700, 369]
        assert L["words"] * 8 == 164_880 and (2 * N + 1) * N * R * 8 == 421_344


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_bytes_match_the_library(name):
    """lin_static_vc_per_bt (what lin_ws is sized by and LinParams::vc_bt holds) against the restated tables: a host function"""
    from ddp_pinocchio_amd import capi
    capi.lib()
    fn = ctypes.CDLL(capi.LIB_PATH)._Z20lin_static_vc_per_bti
    fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_int]
    assert fn(TOPO_ID[name]) == vc_tab(TOPOS[name][0])["words"]
    assert fn(0) == 0


def test_plan_reports_the_layout():
    """the flagship plan through read_switches and lin_plan_decide (a host program: no device)"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_table"])

    def vcaches(env):
        e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        e.update(env)
        out = subprocess.run([os.path.join(ROOT, "build", "lin_plan_table"), "vcaches"], capture_output=True, text=True, check=True, env=e).stdout.split()
        return dict(zip(out[0::2], (int(v) for v in out[1::2])))
    assert vcaches({}) == {"vc_sparse": 1, "qc_sparse": 1, "nvcfg": 77}
    assert vcaches({"DDP_HIP_VCACHE_DENSE": "1"}) == {"vc_sparse": 0, "qc_sparse": 1, "nvcfg": 77}
    assert vcaches({"DDP_HIP_QCACHE_DENSE": "1"})["vc_sparse"] == 0          # the sparse v-cache comes with the sparse q-cache
    assert vcaches({"DDP_HIP_CFG_FULL_ABA": "1"})["vc_sparse"] == 0
    assert vcaches({"DDP_HIP_NO_STATIC": "1"})["vc_sparse"] == 0             # the run-time-tree kernels know whole entries only
    assert vcaches({"DDP_HIP_LIN_SERIAL": "1"})["vc_sparse"] == 1


# ---- GPU: base blocks + deltas against whole entries, bit for bit -------------------------------------------------------------
# (inputs: test_sparse_caches._problem -- non-zero velocities at every t; T = 3, batch 3: 9 (instance, t), 351 configuration lanes,
# so the configuration fill ends in a partial wave and the v-step fill runs 39 of a wave's 64 lanes)
def _clear(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lin_path", [
    ("tree38", 2),
    ("chain6", 3),           # a single chain: the leaf is in every lane's subtree, so no v row selects its base slot (lane nv writes it)
    ("arm7", 4),
    ("biped12", 5),
])
def test_sparse_against_dense(gpu, monkeypatch, name, lin_path):
    _clear(monkeypatch)
    _run(gpu, monkeypatch, name, lin_path, dense_env=DENSE)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [
    (("DDP_HIP_LIN_SERIAL", "1"),),          # the single-stream order
    (("DDP_HIP_K3_NO_PACK", "1"),),          # the contract layout
], ids=["serial", "contract_layout"])
def test_sparse_against_dense_under_switch(gpu, monkeypatch, env):
    _clear(monkeypatch)
    _run(gpu, monkeypatch, "tree38", 2, env=env, dense_env=env + DENSE)


@pytest.mark.gpu
def test_sparse_against_dense_across_workspace_slices(gpu, monkeypatch):
    """more than one workspace slice (DDP_HIP_QWS_BT = 16, T = 24, batch 3: 72 (instance, t)): the spine pre-pass reads entry 0 at
    the new per-(instance, t) stride in every slice"""
    capi = gpu
    _clear(monkeypatch)
    Tn = 24
    model, spec, _ = make("tree38", Tn, batch=B, fd_mode=2, first_order_fd=1)
    rng = np.random.default_rng(50)
    X, U = 0.1 * rng.normal(size=(B, (Tn + 1) * 2 * model.nv)), 0.1 * rng.normal(size=(B, Tn * model.nv))
    env = (("DDP_HIP_QWS_BT", "16"),)
    new, old = _pair(capi, monkeypatch, spec, env, env + DENSE)
    with new, old:
        for ctx in (new, old):
            ctx.upload("X", X)
            ctx.upload("U", U)
            ctx.linearize()
        _equal(new, old)


@pytest.mark.gpu
def test_sparse_against_dense_async(gpu, monkeypatch):
    """two linearisations back to back: the caches written again behind their readers, no host synchronisation in between"""
    _clear(monkeypatch)
    _run(gpu, monkeypatch, "tree38", 2, dense_env=DENSE, asynchronous=True)
