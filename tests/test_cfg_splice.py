"""The (q_i, q_j) points of the mode-2 stencil from cached q-parts (lin_static.hip: lin_static_spine_kernel,
lin_static_cfg_pair_kernel).

In the local-frame ABA the record of joint K is E | r (a function of q_K alone) and U | 1/D | Ia (functions of the q of the
strict descendants of K alone).  At q + eps e_i + eps e_j the record of K is therefore the base record, the record of the
single-step configuration 1+i or 1+j, or -- only on the spine S_i & S_j, the common strict ancestors -- recomputed from the
children's records.  The CPU part checks that rule bit for bit in numpy, for every pair of every compiled-in topology, and the
compile-time tables of the kernels restated in Python against a brute-force ancestor walk.  The GPU part checks the (q, q)
block of f_xx against the oracle and against the full-ABA path kept behind DDP_HIP_CFG_FULL_ABA."""
import json
import os
import re

import numpy as np
import pytest

from problems import held_trajectory, make

EPS, E1, E2 = 2.220446049250313e-16, 1.4901161193847656e-08, 1.220703125e-04
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ddp_pinocchio_amd", "csrc")


# ---- the topologies the kernels are compiled for, parsed from the sources ------------------------------------------------
def _ints(body):
    return [int(x) for x in re.sub(r"//[^\n]*", "", body).replace("\n", " ").split(",") if x.strip()]


def _topologies():
    topos = {}
    src = open(os.path.join(CSRC, "lin_static.hip")).read()
    for name in ("TopoTalos38", "TopoChain6"):
        m = re.search(r"struct %s \{(.*?)\n\};" % name, src, re.S)
        assert m, name
        par = re.search(r"parent\[N\] = \{(.*?)\};", m.group(1), re.S).group(1)
        pri = re.search(r"prismatic\[N\] = \{(.*?)\};", m.group(1), re.S).group(1)
        topos[name] = (_ints(par), _ints(pri))
    extra = open(os.path.join(CSRC, "topo_extra.h")).read()
    reg = re.search(r"^// REGISTRY (.*)$", extra, re.M)
    assert reg
    for e in json.loads(reg.group(1)):
        topos["Topo" + e["name"]] = (list(e["parents"]), list(e["prismatic"]))
        assert "struct Topo%s " % e["name"] in extra
    for name, (par, pri) in topos.items():
        assert len(par) == len(pri) >= 2 and par[0] == -1 and all(-1 <= p < k for k, p in enumerate(par)), name
    return topos


TOPOS = _topologies()


# ---- the compile-time tables (make_spine_tab), restated ------------------------------------------------------------------
def spine_tables(parent):
    """mask[K]: bit i set <=> K is a strict ancestor of i; anc[i]: the transpose; depth; per pair (tri_index order: row by
    row, i < j) the deepest spine joint, the spine length and the exclusive prefix of the lengths; and make_spine_tab's
    per-slot tables."""
    N = len(parent)
    mask, anc, depth = [0] * N, [0] * N, [0] * N
    for k in range(N):
        a = parent[k]
        while a >= 0:
            depth[k] += 1
            mask[a] |= 1 << k
            anc[k] |= 1 << a
            a = parent[a]
    top, length, off, acc = [], [], [], 0
    for i in range(N):
        for j in range(i + 1, N):
            a = parent[i]
            while a >= 0 and not (mask[a] >> j) & 1:
                a = parent[a]
            top.append(a)
            length.append(depth[a] + 1 if a >= 0 else 0)
            off.append(acc)
            acc += length[-1]
    off.append(acc)
    # the lane slots: pairs ordered by top (counting sort, ties in tri_index order); the records of one top are laid out
    # [depth][pair of that top]: the record of a pair's spine joint of depth d is rbase + d * rstride
    cnt = [0] * (N + 1)
    for a in top:
        cnt[a + 1] += 1
    start, goff = [0], [0]
    for g in range(N + 1):
        start.append(start[g] + cnt[g])
        goff.append(goff[g] + cnt[g] * (0 if g == 0 else depth[g - 1] + 1))
    fill = [0] * (N + 1)
    slots = [None] * len(top)
    q = 0
    for i in range(N):
        for j in range(i + 1, N):
            g = top[q] + 1
            slots[start[g] + fill[g]] = dict(i=i, j=j, top=top[q], rbase=goff[g] + fill[g], rstride=cnt[g], length=length[q])
            fill[g] += 1
            q += 1
    return dict(mask=mask, anc=anc, depth=depth, top=top, length=length, off=off, slots=slots, nrec=goff[N + 1])


def strict_ancestors(parent, i):
    s, k = set(), parent[i]
    while k >= 0:
        s.add(k)
        k = parent[k]
    return s


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_spine_tables_against_ancestor_walk(name):
    parent, _ = TOPOS[name]
    N = len(parent)
    assert N <= 64                                     # the masks are 64 bits wide
    tab = spine_tables(parent)
    SA = [strict_ancestors(parent, i) for i in range(N)]
    for k in range(N):
        assert tab["depth"][k] == len(SA[k])
        assert {i for i in range(N) if (tab["mask"][k] >> i) & 1} == {i for i in range(N) if k in SA[i]}
        assert {a for a in range(N) if (tab["anc"][k] >> a) & 1} == SA[k]
    q, acc = 0, 0
    for i in range(N):
        for j in range(i + 1, N):
            spine = SA[i] & SA[j]
            assert tab["length"][q] == len(spine) and tab["off"][q] == acc
            # the spine is a path that ends at the root: its deepest joint and all of that joint's ancestors
            top = tab["top"][q]
            assert spine == (set() if top < 0 else SA[top] | {top})
            # the kernel's membership tests: bit K of the two ancestor masks
            for K in range(N):
                si, sj = (tab["anc"][i] >> K) & 1, (tab["anc"][j] >> K) & 1
                assert (si & sj) == (K in spine) and si == (K in SA[i]) and sj == (K in SA[j])
            acc += len(spine)
            q += 1
    assert q == N * (N - 1) // 2 and tab["off"][q] == acc and tab["nrec"] == acc
    # the lane slots: every pair once, ordered by top; the records of all spines tile 0 .. nrec-1 without overlap
    sl = tab["slots"]
    assert sorted((e["i"], e["j"]) for e in sl) == [(i, j) for i in range(N) for j in range(i + 1, N)]
    assert all(sl[k]["top"] <= sl[k + 1]["top"] for k in range(len(sl) - 1))
    used = []
    for e in sl:
        spine = SA[e["i"]] & SA[e["j"]]
        assert e["length"] == len(spine) and (e["top"] < 0) == (not spine)
        assert sorted(tab["depth"][K] for K in spine) == list(range(len(spine)))      # one record per depth 0 .. length-1
        used += [e["rbase"] + d * e["rstride"] for d in range(len(spine))]
    assert sorted(used) == list(range(acc))
    if name == "TopoTalos38":
        assert acc == 3952 and max(tab["length"]) == 14
        hist = {n: tab["length"].count(n) for n in set(tab["length"])}
        assert hist == {0: 37, 1: 36, 2: 35, 3: 34, 4: 33, 5: 32, 6: 305, 7: 26, 8: 117, 9: 16, 10: 12, 11: 8, 12: 6, 13: 4, 14: 2}


# ---- the splice rule, bit for bit ----------------------------------------------------------------------------------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


class _Tree:
    """A random tree model on a parent table; joint_rec is the one joint step the full q-part and the splice share."""

    def __init__(self, parent, pris, seed):
        rng = np.random.default_rng(seed)
        self.parent, self.pris, self.N = parent, pris, len(parent)
        N = self.N
        self.axis = [np.eye(3)[rng.integers(3)] for _ in range(N)]
        self.Rp = [np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(N)]
        self.pp = [0.3 * rng.normal(size=3) for _ in range(N)]
        self.I6 = []
        for _ in range(N):
            A = rng.normal(size=(6, 6))
            self.I6.append(A @ A.T + 6 * np.eye(6))
        self.S = []
        for K in range(N):
            s = np.zeros(6)
            o = 3 if pris[K] else 0
            s[o:o + 3] = self.axis[K]
            self.S.append(s)
        self.children = [[c for c in range(N) if parent[c] == k] for k in range(N)]
        self.q0 = rng.normal(size=N)

    def X_of(self, K, q):
        a = self.axis[K]
        if self.pris[K]:
            E = self.Rp[K].T
            r = self.pp[K] + self.Rp[K] @ (a * q)
        else:
            Kx = _skew(a)
            RJ = np.eye(3) + np.sin(q) * Kx + (1 - np.cos(q)) * (Kx @ Kx)
            E = (self.Rp[K] @ RJ).T
            r = self.pp[K]
        X = np.zeros((6, 6))
        X[:3, :3] = E
        X[3:, 3:] = E
        X[3:, :3] = -E @ _skew(r)
        return X

    def joint_rec(self, K, X, Ia_children):
        IA = self.I6[K].copy()
        for c in sorted(self.children[K], reverse=True):        # the order of the leaf -> root loop: children descending
            IA = IA + X[c].T @ Ia_children[c] @ X[c]
        U = IA @ self.S[K]
        dinv = 1.0 / (self.S[K] @ U)
        return U, dinv, IA - np.outer(U, U) * dinv

    def qpart(self, q):
        X = [self.X_of(K, q[K]) for K in range(self.N)]
        rec = [None] * self.N
        for K in range(self.N - 1, -1, -1):
            rec[K] = self.joint_rec(K, X, {c: rec[c][2] for c in self.children[K]})
        return X, rec


@pytest.mark.parametrize("name", sorted(TOPOS))
def test_spliced_records_equal_full_qpart_bit_for_bit(name):
    """Every pair, every joint: the record chosen by the rule (base / configuration 1+i / configuration 1+j / recomputed on the
    spine) equals the record of a full q-part at q + eps e_i + eps e_j, np.array_equal.  No pair is skipped."""
    parent, pris = TOPOS[name]
    tr = _Tree(parent, pris, seed=7)
    N, eps = tr.N, 2.0 ** -13
    tab = spine_tables(parent)
    X0, R0 = tr.qpart(tr.q0)
    single = []
    for i in range(N):
        q = tr.q0.copy()
        q[i] += eps
        single.append(tr.qpart(q))
    pairs = bad = 0
    for i in range(N):
        for j in range(i + 1, N):
            q = tr.q0.copy()
            q[i] += eps
            q[j] += eps
            Xf, Rf = tr.qpart(q)
            X = list(X0)
            X[i] = single[i][0][i]
            X[j] = single[j][0][j]
            rec = [None] * N
            for K in range(N - 1, -1, -1):
                si, sj = (tab["anc"][i] >> K) & 1, (tab["anc"][j] >> K) & 1
                if si and sj:
                    rec[K] = tr.joint_rec(K, X, {c: rec[c][2] for c in tr.children[K]})
                elif si:
                    rec[K] = single[i][1][K]
                elif sj:
                    rec[K] = single[j][1][K]
                else:
                    rec[K] = R0[K]
            for K in range(N):
                ok = np.array_equal(X[K], Xf[K]) and all(np.array_equal(a, b) for a, b in zip(rec[K], Rf[K]))
                bad += not ok
            pairs += 1
    assert pairs == N * (N - 1) // 2 and bad == 0, (pairs, bad)


# ---- GPU: against the oracle ---------------------------------------------------------------------------------------------
# one pair of each kind on the Talos-like tree: (i, j, spine length)
TALOS_KINDS = [
    (0, 1, 0), (0, 37, 0),        # i = 0: empty spine
    (26, 27, 14), (34, 35, 14),   # the two longest spines: the last two joints of an arm
    (8, 14, 6),                   # leg - leg: the floating base
    (22, 30, 8),                  # arm - arm: base and torso
    (24, 37, 8),                  # arm - head
    (21, 25, 9),                  # same chain, inside an arm: S_i
]


def _qq_block(fxx_t, nv):
    n = 2 * nv
    return fxx_t.reshape(n, n, n)[:nv, :nv, :]


@pytest.mark.gpu
@pytest.mark.parametrize("name,topo", [("tree38", "TopoTalos38"), ("chain6", "TopoChain6")])
def test_qq_block_against_oracle(gpu, name, topo):
    """The (q, q) block of f_xx, every pair, against the oracle's compute_derivatives with the finite-difference noise bound of
    test_at_size.py (second-order entries) on a held trajectory."""
    capi = gpu
    T = 3
    model, spec, o = make(name, T, batch=1, fd_mode=2)
    _, us, xs = held_trajectory(o, model, seed=70, u_sigma=0.3)
    nv = model.nv
    n = 2 * nv
    with capi.Context(spec) as ctx:
        assert ctx.info()["lin_path"] >= 2                 # a static topology
        ctx.upload("X", xs)
        ctx.upload("U", us)
        ctx.linearize()
        got = ctx.download("FXX")[0]
    d = o.compute_derivatives(xs, us)
    fscale = max(1.0, float(np.max(np.abs(d["f_val"]))))
    tol1 = 8 * EPS * fscale / E1
    tol2 = 64 * EPS * fscale / (E2 * E2) + 4 * tol1 / E2
    tab = spine_tables(TOPOS[topo][0])
    if name == "tree38":
        q_of = {}
        q = 0
        for i in range(nv):
            for j in range(i + 1, nv):
                q_of[i, j] = q
                q += 1
        for i, j, ln in TALOS_KINDS:
            assert tab["length"][q_of[i, j]] == ln, (i, j)
    sz = n ** 3
    for t in range(T):
        a = _qq_block(got[t * sz:(t + 1) * sz], nv)
        r_all = d["fxx"][t * sz:(t + 1) * sz]
        r = _qq_block(r_all, nv)
        scale = max(1.0, float(np.max(np.abs(r_all))))
        assert np.all(np.isfinite(a))
        err = np.max(np.abs(a - r), axis=2)                 # per pair (both orders and the diagonal)
        print(f"{name} t={t}: worst (q, q) pair error {float(err.max()):.3e}, bound {tol2 * scale:.3e}")
        bad = np.argwhere(err > tol2 * scale)
        assert bad.size == 0, (name, t, bad[:8].tolist(), float(err.max()), tol2 * scale)
        if name == "tree38":
            for i, j, ln in TALOS_KINDS:
                assert err[i, j] <= tol2 * scale and err[j, i] <= tol2 * scale, (i, j, ln, float(err[i, j]), tol2 * scale)
                assert float(np.max(np.abs(r[i, j]))) > 0.0 or i < 3     # (a translation of the base moves nothing: an all-zero column)


@pytest.mark.gpu
def test_splice_against_full_aba_path_across_slices(gpu, monkeypatch):
    """Two contexts on the same trajectories, T = 200, batch 6 (more (instance, t) pairs than one workspace slice holds): the splice path
    and the full-ABA path behind DDP_HIP_CFG_FULL_ABA.  Everything but the (q, q) block of f_xx is bit-equal; the (q, q) block
    agrees within the finite-difference noise bound (the largest difference is printed in units of EPS fscale / E2^2)."""
    capi = gpu
    T, B = 200, 6
    model, spec, o = make("tree38", T, batch=B, fd_mode=2)
    trajs = [held_trajectory(o, model, seed=70 + b, u_sigma=0.3) for b in range(B)]
    X = np.stack([tr[2] for tr in trajs])
    U = np.stack([tr[1] for tr in trajs])
    nv = model.nv
    n = 2 * nv
    seqs = ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU")
    monkeypatch.delenv("DDP_HIP_CFG_FULL_ABA", raising=False)
    # 1 200 (instance, t) pairs: the workspace knob makes that three slices of spine records here and ten slices of sweeps there
    monkeypatch.setenv("DDP_HIP_QWS_BT", "128")
    with capi.Context(spec) as ctx_new:
        monkeypatch.setenv("DDP_HIP_CFG_FULL_ABA", "1")
        with capi.Context(spec) as ctx_old:
            monkeypatch.delenv("DDP_HIP_CFG_FULL_ABA")
            for ctx in (ctx_new, ctx_old):
                assert ctx.info()["lin_path"] == 2
                ctx.upload("X", X)
                ctx.upload("U", U)
                ctx.linearize()
            worst, qq_equal = 0.0, True
            for b in range(B):
                fscale = 1.0
                for seq in seqs:
                    a = ctx_new.download(seq, b, 1)[0]
                    r = ctx_old.download(seq, b, 1)[0]
                    if seq == "F_VAL":
                        fscale = max(1.0, float(np.max(np.abs(r))))
                    if seq != "FXX":
                        assert np.array_equal(a, r), (seq, b)
                        continue
                    a = a.reshape(T, n, n, n)
                    r = r.reshape(T, n, n, n)
                    assert np.all(np.isfinite(a))
                    for blk in ((slice(0, nv), slice(nv, n)), (slice(nv, n), slice(0, nv)), (slice(nv, n), slice(nv, n))):
                        assert np.array_equal(a[:, blk[0], blk[1], :], r[:, blk[0], blk[1], :]), (b, blk)
                    aq, rq = a[:, :nv, :nv, :], r[:, :nv, :nv, :]
                    qq_equal = qq_equal and np.array_equal(aq, rq)
                    tol1 = 8 * EPS * fscale / E1
                    tol2 = 64 * EPS * fscale / (E2 * E2) + 4 * tol1 / E2
                    diff = float(np.max(np.abs(aq - rq)))
                    unit = EPS * fscale / (E2 * E2)
                    print(f"instance {b}: largest (q, q) difference {diff:.3e} = {diff / unit:.2f} EPS fscale / E2^2 (bound {tol2 / unit:.0f})")
                    if diff / unit > worst:
                        worst = diff / unit
                    assert diff <= tol2, (b, diff, tol2)
                    del a, r, aq, rq
            print(f"(q, q) block bit-equal: {qq_equal}; largest difference {worst:.2f} EPS fscale / E2^2")
