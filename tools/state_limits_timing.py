"""Cost of the per-instance soft state limits (DDP_HIP_FLAG_STATE_LIMITS) at the benchmark shape: the Talos-like tree38,
T = 200, batch 64, in mode 2 (forward-differenced first order, static mode-2 stencil) and mode 1 (analytic first order).

    python tools/state_limits_timing.py                      flag off, then flag on with binding limits, in one process, per mode
    python tools/state_limits_timing.py --off                flag off only (one process per library when comparing two)
    python tools/state_limits_timing.py --compare OTHER.so   flag off, this tree's library against OTHER.so (the parent commit's
                                                             build), --runs alternating processes each

Every call is synchronous and timed by the wall clock: median [min - max] of 20 samples after 3 warm-ups, one JSON line per
(mode, limits).  With the flag on every (instance, t, row) carries a non-zero weight and bounds of its own around the instance's
trajectory; they bind (e != 0) on roughly a third of the rows, half of those below and half above.  Linearise is timed with
weights of order 1.  Backward and forward are timed with the same weights scaled by 1e-12, as tools/frame_cost_timing.py does
and for its reason: at T = 200 no full-DDP sweep of this tree with a V_x of order 1 stays positive definite in double (DESIGN.md
4d), and a sweep that restarts is not one sweep; the kernels and their bytes do not depend on the values.  The forward's wall time
counts line-search rounds, so the rollout kernel is also timed per round with the ddp_hip_profile_* events (rollout_ms_per_round)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, B, WARM, REPS = 200, 64, 3, 20


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def measure(settings):
    import numpy as np

    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    rng = np.random.default_rng(1)
    S = xs.reshape(B, T + 1, o.nx)                   # nq == nv: the state coordinates are the tangent rows
    kind = rng.integers(0, 6, size=S.shape)          # 0: violated below, 1: above, 2 .. 5: inside
    gap, width = rng.uniform(0.05, 0.3, size=S.shape), rng.uniform(0.1, 1.0, size=S.shape)
    lo = np.where(kind == 0, S + gap, np.where(kind == 1, S - gap - width, S - width))
    hi = np.where(kind == 0, S + gap + width, np.where(kind == 1, S - gap, S + width))
    w = rng.uniform(0.5, 2.0, size=S.shape)
    binding = float(np.mean((S < lo) | (S > hi)))
    for fd_mode, fo in ((2, 1), (1, 0)):
        _, spec, _ = make("tree38", T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
        for on in settings:
            with capi.Context(spec, flags=capi.FLAG_STATE_LIMITS if on else 0) as ctx:
                ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
                if on:
                    ctx.set_state_limits(lo=lo, hi=hi, weight=w)
                ctx.linearize()
                ms = {"linearize": [], "backward": [], "forward": []}
                restarts = 0
                ctx.profile_enable(kernels=[capi.K_FWD_ROLLOUT])   # event pairs around every rollout launch (one per line-search round)
                for r in range(WARM + REPS):
                    if r == WARM:
                        ctx.profile_reset()
                    if on:
                        ctx.set_state_limits(weight=w)
                    t0 = time.perf_counter()
                    ctx.linearize()
                    t1 = time.perf_counter()
                    if on:
                        ctx.set_state_limits(weight=1e-12 * w)
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
                print(json.dumps({"lib": os.path.basename(capi.LIB_PATH), "fd_mode": fd_mode, "first_order": info["first_order"],
                                  "limits": bool(on), "binding_rows": round(binding, 3) if on else 0.0,
                                  "T": T, "batch": B, "bwd_stream_bytes": ctx.bwd_stream_bytes(), "fwd_path": info["fwd_path"],
                                  **{f"{k}_ms": stats(v) for k, v in ms.items()},
                                  "rollout_ms_per_round": round(roll_ms / max(launches, 1), 3), "rounds_per_forward": launches / REPS,
                                  "restarts": restarts, "mean_step": float(np.mean(step))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off", action="store_true", help="flag off only")
    ap.add_argument("--compare", metavar="LIB", help="flag off: this tree's library against LIB, alternating processes")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if a.compare:
        for r in range(a.runs):
            for lib in (os.path.abspath(a.compare), None):
                env = dict(os.environ)
                env.pop("DDP_HIP_LIB", None)
                if lib:
                    env["DDP_HIP_LIB"] = lib
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--off"], env=env, timeout=600).returncode
                if rc != 0:                        # a failed run ends the comparison: nothing more is started
                    sys.exit(rc)
        return
    measure([False] if a.off else [False, True])


if __name__ == "__main__":
    main()
