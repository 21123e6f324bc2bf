"""Cost of the per-instance joint-acceleration cost (DDP_HIP_FLAG_JOINT_ACCEL_COST) at the benchmark shape: the Talos-like tree38,
T = 200, batch 64, mode 2 (forward-differenced first order, static mode-2 stencil), on held trajectories.

    python tools/joint_accel_timing.py                      the three states in one process
    python tools/joint_accel_timing.py --off                flag off only (one process per library when comparing two)
    python tools/joint_accel_timing.py --compare OTHER.so   flag off, this tree's library against OTHER.so (the parent commit's
                                                             build), --runs alternating processes each
    python tools/joint_accel_timing.py --compare OTHER.so --out profiles/joint_accel_cost.json
                                                             the comparison, then the three states, and every line of both in
                                                             the file: {"states": [...], "compare": [...]}

The three states, one JSON line each:
    joint_accel 0            flag off
    joint_accel 1 zero       flag on, every weight 0 (uploaded in two half-batch ranges: the kernels stay launched and return at
                             their first test, the live rule of DESIGN.md 4p) -- the same context the live state is held against
    joint_accel 1 full       flag on, all 38 weights live at every (instance, t < T)
Every call is synchronous and timed by the wall clock: median [min - max] of 20 samples after 3 warm-ups.  The cost stage is
ddp_hip_linearize_stages(LIN_COST) (lin_joint_accel_cost_kernel: batch x T waves, the analytic recursion and the dense products) and ddp_hip_cost_seq_aug
(joint_accel_cost_kernel over batch x (T+1) states); the forward counts line-search rounds, so it is also given per round
(rollout + joint_accel_cost_kernel over the batch x 8 x (T+1) candidate states + com_sum_kernel + select), beside the rollout
kernel alone from the ddp_hip_profile_* events.  The backward sweep that provides the forward's gains runs on the flag-off
derivatives (the weights zeroed as above), as in tools/control_grav_timing.py; the weights are back in place for the forward."""
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


def measure(states):
    """one JSON line per state, printed; returns the records"""
    import numpy as np

    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    rng = np.random.default_rng(1)
    _, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    m = spec.m
    records = []
    for state in states:
        on = state != "off"
        with capi.Context(spec, flags=capi.FLAG_JOINT_ACCEL_COST if on else 0) as ctx:
            ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
            w = 1e-3 * rng.uniform(0.5, 2.0, size=(B, T, m)) if on else None

            def zero():
                ctx.set_joint_accel_cost(weight=0.0, first=0, count=B // 2)
                ctx.set_joint_accel_cost(weight=0.0, first=B // 2, count=B - B // 2)

            def live():
                ctx.set_joint_accel_cost(weight=w)  # targets 0: the residuals are the held trajectories' accelerations
                if state == "zero":
                    zero()
            if on:
                live()
            ctx.linearize()
            ms = {"linearize": [], "lin_cost": [], "cost_seq": [], "backward": [], "forward": []}
            restarts = 0
            ctx.profile_enable(kernels=[capi.K_FWD_ROLLOUT])   # event pairs around every rollout launch (one per line-search round)
            mu1 = np.ones(B)
            for r in range(WARM + REPS):
                if r == WARM:
                    ctx.profile_reset()
                if on:
                    live()
                t0 = time.perf_counter()
                ctx.linearize()
                t1 = time.perf_counter()
                ctx.linearize(capi.LIN_COST)
                t1b = time.perf_counter()
                ctx.cost_seq_aug(0, mu1)
                t1c = time.perf_counter()
                if on:
                    zero()
                    ctx.linearize()
                t2 = time.perf_counter()
                _, _, mu, rs = ctx.backward(0.0, 1.0)
                t2b = time.perf_counter()
                if on:
                    live()
                t3 = time.perf_counter()
                _, step, _ = ctx.forward(mu, n_alpha=8)
                t4 = time.perf_counter()
                if r >= WARM:
                    ms["linearize"].append((t1 - t0) * 1e3); ms["lin_cost"].append((t1b - t1) * 1e3)
                    ms["cost_seq"].append((t1c - t1b) * 1e3); ms["backward"].append((t2b - t2) * 1e3)
                    ms["forward"].append((t4 - t3) * 1e3)
                    restarts += int(rs.sum())
            roll_ms, launches = ctx.profile_get(capi.K_FWD_ROLLOUT)
            info = ctx.info()
            records.append({"lib": os.path.basename(capi.LIB_PATH), "joint_accel": int(on), "state": state, "T": T, "batch": B,
                            "fwd_path": info["fwd_path"], **{f"{k}_ms": stats(v) for k, v in ms.items()},
                            "rollout_ms_per_round": round(roll_ms / max(launches, 1), 3), "rounds_per_forward": launches / REPS,
                            "forward_ms_per_round": round(float(np.median(ms["forward"])) * REPS / max(launches, 1), 3),
                            "restarts": restarts, "mean_step": float(np.mean(step))})
            print(json.dumps(records[-1]), flush=True)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off", action="store_true", help="flag off only")
    ap.add_argument("--compare", metavar="LIB", help="flag off: this tree's library against LIB, alternating processes")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", metavar="FILE", help="write every line of this call to FILE; with --compare the three states are measured as well")
    a = ap.parse_args()
    out = {"states": [], "compare": []}
    if a.compare:                                  # first: the children start before this process has opened the GPU
        for r in range(a.runs):
            for lib in (os.path.abspath(a.compare), None):
                env = dict(os.environ)
                env.pop("DDP_HIP_LIB", None)
                if lib:
                    env["DDP_HIP_LIB"] = lib
                run = subprocess.run([sys.executable, os.path.abspath(__file__), "--off"], env=env, timeout=600, stdout=subprocess.PIPE, text=True)
                sys.stdout.write(run.stdout); sys.stdout.flush()
                if run.returncode != 0:            # a failed run ends the comparison: nothing more is started
                    sys.exit(run.returncode)
                out["compare"] += [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    if not a.compare or a.out:
        out["states"] = measure(["off"] if a.off else ["off", "zero", "full"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
