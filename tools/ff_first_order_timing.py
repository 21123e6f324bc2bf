"""Linearise time of the free-flyer first order, forward differences against analytic (lin_analytic.hip:
ana_ff_first_kernel), at the BASELINE config-5 shape: tree38ff_frame (nq 39, nv 38, frame constraint at t = T-2),
T = 200, batch 64, tensor-free.  Times the LIN_FIRST class with the ddp_hip_profile_* events and the whole
linearisation (constraint chain included) by the wall clock, after a warm-up.  Prints one JSON line per path."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from ddp_pinocchio_amd import capi  # noqa: E402
from problems import make, neutral_state  # noqa: E402

T, B, REPS = 200, 64, 10


def main():
    model, _, o = make("tree38ff_frame", T, batch=1, fd_mode=0)
    us = 0.1 * np.random.default_rng(0).normal(size=(B, T * model.nv))
    xs = np.stack([o.rollout(neutral_state(model), us[b]) for b in range(B)])
    for fo in (1, 0):
        _, spec, _ = make("tree38ff_frame", T, batch=B, fd_mode=0, first_order_fd=fo)
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
            ctx.upload("X", xs); ctx.upload("U", us)
            for _ in range(3):
                ctx.linearize()
            ctx.profile_enable(True)
            ctx.profile_reset()
            t0 = time.perf_counter()
            for _ in range(REPS):
                ctx.linearize()
                ctx.download("FX", 0, 1)                      # (a synchronising read: the wall time covers the whole call)
            wall = (time.perf_counter() - t0) * 1e3 / REPS
            first_ms, n = ctx.profile_get(capi.K_LIN_FIRST)
            print(json.dumps({"path": "fd" if fo else "analytic", "first_order": ctx.info()["first_order"], "T": T, "batch": B,
                              "lin_first_ms": round(first_ms / max(n, 1), 3), "linearize_wall_ms": round(wall, 3)}))


if __name__ == "__main__":
    main()
