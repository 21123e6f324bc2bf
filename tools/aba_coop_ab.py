"""Bit-identity of the wave-cooperative articulated-body traversals (rbd.h: aba_tree_coop, aba_tree_coop2w, aba_pipe_q / aba_pipe_x)
between two builds of the library: the acceptance test of a change to their shared joint steps.

    DDP_HIP_LIB=<lib.so> python tools/aba_coop_ab.py --dump DIR     one process: every case below under that library -> DIR/aba_coop.npz
    python tools/aba_coop_ab.py --compare A.npz B.npz               every entry np.array_equal(..., equal_nan=True), else exit 1

Forward (X_NEW, U_NEW, step, dcost, rc; the inputs of tests/test_fwd_pipeline.py), each case in the pipelined form and again under
DDP_HIP_FWD_NO_PIPE (the four-candidate form): tree38 and tree38ff at batch 3, T 1 / 2 / 5, n_alpha 1 / 3 / 8; tree38 with the
tracking cost and control bounds; tree38_frame at mu = 100; wide38 of tests/robots.py (level width 8); ctx.rollout() on tree38 and
tree38ff.  Analytic (every derivative sequence linearise leaves): tree38, tree38_frame, tree38_config in mode 1, tree39 of the
catalogue (the <64> instantiations), tree38 in mode 2; tree38 again under DDP_HIP_ANA_OWN_ABA and DDP_HIP_ANA_SPLIT, where every
evaluation runs the traversal itself.  The switches are set before the context that reads them is created."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class switch:
    """a development switch of the library in the environment while a context is created (lin_plan.cpp: read_switches)"""

    def __init__(self, name=None):
        self.name = name

    def __enter__(self):
        if self.name:
            os.environ[self.name] = "1"

    def __exit__(self, *exc):
        if self.name:
            del os.environ[self.name]


def dump(path):
    import problems
    import robots
    import test_fwd_pipeline as fp
    from ddp_pinocchio_amd import capi
    from test_dynamics_parity import DERIV_SEQS, TENSOR_SEQS
    out = {}

    def make(name, T, batch=1, fd_mode=2, **kw):
        if name in robots.CATALOGUE:
            return robots.problem(name, T, batch=batch, fd_mode=fd_mode, **kw)
        return problems.make(name, T, batch=batch, fd_mode=fd_mode, **kw)
    fp.make = make                                  # _inputs on the robots of the catalogue as well

    def put(prefix, d):
        for k, v in d.items():
            out[f"{prefix}/{k}"] = np.asarray(v)

    def both_forms(prefix, run):
        for form, sw in (("pipe", None), ("nopipe", "DDP_HIP_FWD_NO_PIPE")):
            with switch(sw):
                put(f"{prefix}/{form}", run())

    # ---- forward
    B = 3
    for name in ("tree38", "tree38ff"):
        for T in (1, 2, 5):
            model, spec, o, inp = fp._inputs(name, T, B, seed=100 + T)
            for na in (1, 3, 8):
                both_forms(f"fwd/{name}/T{T}/na{na}", lambda: fp._forward(capi, spec, inp, na))

    T = 5
    model, spec, o, inp = fp._inputs("tree38", T, B, seed=9)
    rng = np.random.default_rng(90)
    xref = inp["X"].reshape(B, T + 1, o.nx) + 0.1 * rng.normal(size=(B, T + 1, o.nx))
    wx, wu = rng.uniform(0.5, 2.0, size=(B, T + 1, o.n)), rng.uniform(0.5, 2.0, size=(B, T, model.nv))
    uref = 0.1 * rng.normal(size=(B, T, model.nv))

    def tracking_and_bounds(ctx):
        ctx.set_tracking_cost(xref=xref, wx=wx, uref=uref, wu=wu)
        ctx.set_control_bounds(lo=-0.25, hi=0.25)
    both_forms("fwd/tree38/tracking_bounds", lambda: fp._forward(capi, spec, inp, 8, flags=capi.FLAG_TRACKING_COST | capi.FLAG_CONTROL_BOUNDS,
                                                                  setup=tracking_and_bounds))

    model, spec, o, inp = fp._inputs("tree38_frame", 5, B, seed=10)
    both_forms("fwd/tree38_frame/mu100", lambda: fp._forward(capi, spec, inp, 8, mu=100.0))

    model, spec, o, inp = fp._inputs("wide38", 2, B, seed=13)
    both_forms("fwd/wide38/T2", lambda: fp._forward(capi, spec, inp, 8))

    for name in ("tree38", "tree38ff"):
        model, spec, o, inp = fp._inputs(name, 5, B, seed=8)

        def rollout():
            with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
                bad = np.full_like(inp["X"], np.nan); bad[:, :o.nx] = inp["X"][:, :o.nx]
                ctx.upload("X", bad); ctx.upload("U", inp["U"])
                ctx.rollout()
                return {"X": ctx.download("X")}
        both_forms(f"rollout/{name}", rollout)

    # ---- analytic linearisation
    def linearize(prefix, name, T, batch, fd_mode, sw=None):
        model, spec, o = make(name, T, batch=batch, fd_mode=fd_mode, first_order_fd=0)
        rng = np.random.default_rng(17)
        us = 0.3 * rng.normal(size=(batch, T * model.nv))
        xs = np.stack([o.rollout(problems.random_state(model, rng, 0.3), us[b]) for b in range(batch)])
        with switch(sw):
            with capi.Context(spec) as ctx:
                assert ctx.info()["first_order"] == 2
                ctx.upload("X", xs); ctx.upload("U", us)
                ctx.linearize()
                put(prefix, {s: ctx.download(s) for s in list(DERIV_SEQS.values()) + list(TENSOR_SEQS.values()) if ctx.seq_size(s)})

    for name in ("tree38", "tree38_frame", "tree38_config"):
        linearize(f"ana/{name}/mode1", name, 3, 2, 1)
    linearize("ana/tree39/mode1", "tree39", 2, 1, 1)
    linearize("ana/tree38/mode2", "tree38", 3, 2, 2)
    linearize("ana/tree38/mode1_own_aba", "tree38", 3, 2, 1, sw="DDP_HIP_ANA_OWN_ABA")
    linearize("ana/tree38/mode1_split", "tree38", 3, 2, 1, sw="DDP_HIP_ANA_SPLIT")

    os.makedirs(path, exist_ok=True)
    np.savez(os.path.join(path, "aba_coop.npz"), **out)
    print(f"aba_coop_ab: {len(out)} entries under {os.path.basename(capi.LIB_PATH)} -> {os.path.join(path, 'aba_coop.npz')}")


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    differ = sorted(set(A.files) ^ set(Bz.files))
    for k in sorted(set(A.files) & set(Bz.files)):
        if not np.array_equal(A[k], Bz[k], equal_nan=True):
            differ.append(k)
    print(f"aba_coop_ab: {len(A.files)} entries, {len(differ)} differ" + ("" if not differ else ": " + ", ".join(differ[:20])))
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
