"""Cost of the per-instance tracking cost (DDP_HIP_FLAG_TRACKING_COST) at the benchmark shape: the Talos-like tree38,
T = 200, batch 64, in mode 2 (forward-differenced first order, static mode-2 stencil) and mode 1 (analytic first order).
For each mode, a context without the flag and one with it and non-zero weights (every instance its own reference) run
linearise, backward and forward on the same inputs; each call is synchronous, timed by the wall clock after a warm-up.
Prints one JSON line per (mode, flag) with the mean ms of each phase.

Linearise is timed with every weight non-zero.  Backward and forward of the tracking context are timed with the state weights
at 0 and the controls tracking the held torques (non-zero weights): at T = 200 no full-DDP sweep of this tree with V != 0
stays positive definite in double (the oracle exhausts its restarts as well), a sweep that restarts is not one
sweep.  The sweep's kernels and bytes do not depend on the values.  The forward's wall time counts line-search rounds: on these
inputs a step that leaves the held trajectory diverges open loop and the tracking context's search runs to its floor (five
rounds where the flag-off run, whose cost ignores the state, takes one), so the rollout kernel is also timed per round with
the ddp_hip_profile_* events (rollout_ms_per_round)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from ddp_pinocchio_amd import capi  # noqa: E402
from problems import held_trajectory, make  # noqa: E402

T, B, WARM, REPS = 200, 64, 2, 5


def main():
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    rng = np.random.default_rng(1)
    n, m, nx = o.n, o.m, o.nx
    xref = xs.reshape(B, T + 1, nx) + 0.05 * rng.normal(size=(B, T + 1, nx))
    wx = rng.uniform(0.01, 0.1, size=(B, T + 1, n))
    uref = us.reshape(B, T, m) + 0.05 * rng.normal(size=(B, T, m))
    wu = rng.uniform(0.0, 0.1, size=(B, T, m))
    wu_sweep = rng.uniform(1e3, 2e3, size=(B, T, m))  # toward the held torques: the full step keeps the rollout near the held one
    for fd_mode, fo in ((2, 1), (1, 0)):
        _, spec, _ = make("tree38", T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
        for on in (False, True):
            with capi.Context(spec, flags=capi.FLAG_TRACKING_COST if on else 0) as ctx:
                ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
                if on:
                    ctx.set_tracking_cost(xref=xref, wx=wx, uref=uref, wu=wu)
                ctx.linearize()
                ms = {"linearize": [], "backward": [], "forward": []}
                restarts = 0
                ctx.profile_enable(kernels=[capi.K_FWD_ROLLOUT])   # event pairs around every rollout launch (one per line-search round)
                for r in range(WARM + REPS):
                    if r == WARM:
                        ctx.profile_reset()
                    if on:
                        ctx.set_tracking_cost(wx=wx, uref=uref, wu=wu)
                    t0 = time.perf_counter()
                    ctx.linearize()
                    t1 = time.perf_counter()
                    if on:
                        ctx.set_tracking_cost(wx=np.zeros_like(wx), uref=us.reshape(B, T, m), wu=wu_sweep)
                        ctx.linearize()
                    t2 = time.perf_counter()
                    _, _, mu, rs = ctx.backward(0.0, 1.0)
                    t3 = time.perf_counter()
                    _, step, _ = ctx.forward(mu, n_alpha=8)
                    t4 = time.perf_counter()
                    if r >= WARM:
                        ms["linearize"].append((t1 - t0) * 1e3); ms["backward"].append((t3 - t2) * 1e3)
                        ms["forward"].append((t4 - t3) * 1e3)
                        restarts += int(rs.sum())
                roll_ms, launches = ctx.profile_get(capi.K_FWD_ROLLOUT)
                info = ctx.info()
                print(json.dumps({"fd_mode": fd_mode, "first_order": info["first_order"], "tracking": on, "T": T, "batch": B,
                                  "bwd_stream_bytes": ctx.bwd_stream_bytes(), "fwd_path": info["fwd_path"],
                                  **{f"{k}_ms": round(float(np.mean(v)), 3) for k, v in ms.items()},
                                  **{f"{k}_ms_min": round(float(np.min(v)), 3) for k, v in ms.items()},
                                  "rollout_ms_per_round": round(roll_ms / max(launches, 1), 3), "rounds_per_forward": launches / REPS,
                                  "restarts": restarts, "mean_step": float(np.mean(step))}), flush=True)


if __name__ == "__main__":
    main()
