"""Bit-identity of the static-topology stencil (csrc/lin_static.hip) between two builds of the library: the acceptance test of a
change to the joint steps its sweeps share.

    DDP_HIP_LIB=<lib.so> python tools/lin_static_ab.py --dump DIR     one process: every case below under that library -> DIR/lin_static.npz
    python tools/lin_static_ab.py --compare A.npz B.npz               every entry np.array_equal(..., equal_nan=True), else exit 1

The smallest shapes that reach every instantiation and lane pattern.  Base shape: batch 2, T 3, fd_mode 2 on finite-difference
jacobians, one linearize() -- 39 configurations per (instance, t) at 38 joints are 234 cache evaluations, four waves, the last
partly filled, waves straddling (instance, t) boundaries -- on tree38, chain6 and the 7- and 12-joint compiled-in robots (ARM7,
BIPED12 of tests/robots.py), each under no switch, DDP_HIP_QCACHE_DENSE, DDP_HIP_CFG_FULL_ABA, DDP_HIP_LIN_SERIAL,
DDP_HIP_K3_NO_PACK and DDP_HIP_FXX_FULL.  tree38 again: batch 3, T 7 under DDP_HIP_QWS_BT=16 (two configuration-level slices, the
second partial), with and without DDP_HIP_QCACHE_DENSE; stage by stage (LIN_COST | LIN_FIRST, then LIN_SECOND); a first-order-only
context (the cache fill on one configuration per (instance, t)); fd_mode 1 (the first-order kernels' accelerations feed the
analytic pass; every derivative sequence).  The switches are set before the context that reads them is created."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEQS = ("F_VAL", "FX", "FU", "FXX", "FUX", "FUU", "LFX", "LFXX")
SWITCHES = (None, "DDP_HIP_QCACHE_DENSE", "DDP_HIP_CFG_FULL_ABA", "DDP_HIP_LIN_SERIAL", "DDP_HIP_K3_NO_PACK", "DDP_HIP_FXX_FULL")


class switches:
    """development switches of the library in the environment while a context is created (lin_plan.cpp: read_switches)"""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            del os.environ[k]


def dump(path):
    import problems
    import robots
    from ddp_pinocchio_amd import capi
    from oracle.binding import Oracle
    from test_dynamics_parity import DERIV_SEQS, TENSOR_SEQS
    out = {}

    def problem(name, T, B, fd_mode=2, first_order_fd=1):
        if name in ("arm7", "biped12"):
            parents = {"arm7": robots.ARM7, "biped12": robots.BIPED12}[name]
            model = robots.seeded_tree(parents, seed=len(parents))
            kw = dict(dt=0.01, c=1.0, fd_mode=fd_mode, first_order_fd=first_order_fd, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
            return model, capi.ProblemSpec(model, T, batch=B, **kw), Oracle(model, T, **kw)
        return problems.make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=first_order_fd)

    def held_posture(model, o, T, B):
        """a posture held under computed-torque control from a moving start (non-zero velocities at every t), random u on top"""
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
            X.append(o.rollout(x0, us))
            U.append(us)
        return np.stack(X), np.stack(U)

    def linearize(prefix, spec, X, U, env, seqs=SEQS, flags=0, stages=(None,), static=True):
        with switches(**env):
            ctx = capi.Context(spec, flags=flags)
        with ctx:
            assert not static or ctx.info()["lin_path"] >= 2, ctx.info()        # the static kernels of the topology
            ctx.upload("X", X)
            ctx.upload("U", U)
            for st in stages:
                ctx.linearize(st)
            got = {s: ctx.download(s) for s in seqs if ctx.seq_size(s)}
        assert got and all(np.all(np.isfinite(v)) for v in got.values()), prefix
        for s, v in got.items():
            out[f"{prefix}/{s}"] = np.asarray(v)

    for name in ("tree38", "chain6", "arm7", "biped12"):
        model, spec, o = problem(name, 3, 2)
        X, U = held_posture(model, o, 3, 2)
        for sw in SWITCHES:
            linearize(f"{name}/{sw or 'default'}", spec, X, U, {sw: "1"} if sw else {})
        if name == "tree38":
            linearize("tree38/staged", spec, X, U, {}, stages=(capi.LIN_COST | capi.LIN_FIRST, capi.LIN_SECOND))
            all_seqs = list(DERIV_SEQS.values()) + list(TENSOR_SEQS.values())
            _, spec1, _ = problem(name, 3, 2, fd_mode=1, first_order_fd=0)
            linearize("tree38/mode1", spec1, X, U, {}, seqs=all_seqs)
            _, spec0, _ = problem(name, 3, 2, fd_mode=0)
            linearize("tree38/first_order_only", spec0, X, U, {}, seqs=("F_VAL", "FX", "FU", "LFX"), flags=capi.FLAG_NO_TENSORS)

    Tn, B = 7, 3
    model, spec, _ = problem("tree38", Tn, B)
    rng = np.random.default_rng(50)
    X, U = 0.1 * rng.normal(size=(B, (Tn + 1) * 2 * model.nv)), 0.1 * rng.normal(size=(B, Tn * model.nv))
    linearize("tree38/two_slices", spec, X, U, {"DDP_HIP_QWS_BT": "16"})
    linearize("tree38/two_slices_dense", spec, X, U, {"DDP_HIP_QWS_BT": "16", "DDP_HIP_QCACHE_DENSE": "1"})

    os.makedirs(path, exist_ok=True)
    np.savez(os.path.join(path, "lin_static.npz"), **out)
    print(f"lin_static_ab: {len(out)} entries under {os.path.basename(capi.LIB_PATH)} -> {os.path.join(path, 'lin_static.npz')}")


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    differ = sorted(set(A.files) ^ set(Bz.files))
    for k in sorted(set(A.files) & set(Bz.files)):
        if not np.array_equal(A[k], Bz[k], equal_nan=True):
            differ.append(k)
    print(f"lin_static_ab: {len(A.files)} entries, {len(differ)} differ" + ("" if not differ else ": " + ", ".join(differ[:20])))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
    elif a.compare:
        sys.exit(compare(*a.compare))
    else:
        ap.error("--dump DIR or --compare A B")


if __name__ == "__main__":
    main()
