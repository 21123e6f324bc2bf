"""Cost of the per-instance centre-of-mass cost (DDP_HIP_FLAG_COM_COST) at the benchmark shape: the Talos-like tree38, T = 200,
batch 64, in mode 2 (forward-differenced first order, static mode-2 stencil) and mode 1 (analytic first order).

    python tools/com_cost_timing.py                      flag off and flag on in one process, per mode
    python tools/com_cost_timing.py --off                flag off only (one process per library when comparing two)
    python tools/com_cost_timing.py --compare OTHER.so   flag off, this tree's library against OTHER.so (the parent commit's
                                                         build), --runs alternating processes each

Every call is synchronous and timed by the wall clock: median [min - max] of 20 samples after 3 warm-ups, one JSON line per
(mode, flag).  With the flag on every (instance, t, axis) carries a non-zero weight and every instance its own targets.
Linearise is timed with weights of order 1.  The backward sweep is timed on the flag-off derivatives: at T = 200 the full-DDP
sweep of this tree does not stay positive definite once the dense CoM block enters V_xx, not even with the weights scaled by
1e-12 (the CPU oracle exhausts its restarts on the same derivatives), and a sweep that restarts is not one
sweep.  So before it the weights are zeroed in two half-batch uploads, which leaves the CoM kernels launched (the live rule)
with nothing to add; the sweep's kernels and bytes do not depend on the values.  The forward is then timed with the weights
of order 1 back in place, on those gains: com_cost_kernel does its full work on every candidate.  The forward's wall time
counts line-search rounds, so it is also given per round (forward_ms_per_round: rollout + com_cost_kernel over the
batch x 8 x (T+1) candidate states + com_sum_kernel + select), beside the rollout kernel alone from the ddp_hip_profile_* events
(rollout_ms_per_round).  The two new kernels on their own are the differences on against off of
    lin_cost_ms   ddp_hip_linearize_stages(LIN_COST)   lin_com_cost_kernel, batch x (T+1) waves
    cost_seq_ms   ddp_hip_cost_seq_aug                 com_cost_kernel over batch x (T+1) states
    forward_ms_per_round - rollout_ms_per_round        com_cost_kernel over batch x 8 x (T+1) states, com_sum_kernel"""
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


def measure(flag_states):
    import numpy as np

    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    rng = np.random.default_rng(1)
    mass = np.asarray(model.mass_j)
    for fd_mode, fo in ((2, 1), (1, 0)):
        _, spec, _ = make("tree38", T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
        for on in flag_states:
            with capi.Context(spec, flags=capi.FLAG_COM_COST if on else 0) as ctx:
                ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
                if on:
                    X = xs.reshape(B, T + 1, o.nx)
                    tgt = np.zeros((B, T + 1, 3))
                    for s in range(seeds):                  # targets near the CoM's own positions, per instance
                        for t in range(T + 1):
                            q = X[s][t][:o.nq]
                            tgt[s::seeds, t] = sum(mass[j] * o.frame_position(j, model.com[j], q) for j in range(len(mass))) / mass.sum()
                    tgt += 0.02 * rng.normal(size=tgt.shape)
                    w = rng.uniform(0.5, 2.0, size=(B, T + 1, 3))
                    ctx.set_com_cost(target=tgt, weight=w)
                ctx.linearize()
                ms = {"linearize": [], "lin_cost": [], "cost_seq": [], "backward": [], "forward": []}
                restarts = 0
                ctx.profile_enable(kernels=[capi.K_FWD_ROLLOUT])   # event pairs around every rollout launch (one per line-search round)
                mu1 = np.ones(B)
                for r in range(WARM + REPS):
                    if r == WARM:
                        ctx.profile_reset()
                    if on:
                        ctx.set_com_cost(weight=w)
                    t0 = time.perf_counter()
                    ctx.linearize()
                    t1 = time.perf_counter()
                    ctx.linearize(capi.LIN_COST)
                    t1b = time.perf_counter()
                    ctx.cost_seq_aug(0, mu1)
                    t1c = time.perf_counter()
                    if on:
                        ctx.set_com_cost(weight=0.0, first=0, count=B // 2)
                        ctx.set_com_cost(weight=0.0, first=B // 2, count=B - B // 2)
                        ctx.linearize()
                    t2 = time.perf_counter()
                    _, _, mu, rs = ctx.backward(0.0, 1.0)
                    t2b = time.perf_counter()
                    if on:
                        ctx.set_com_cost(weight=w)
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
                print(json.dumps({"lib": os.path.basename(capi.LIB_PATH), "fd_mode": fd_mode, "first_order": info["first_order"], "com": int(on),
                                  "T": T, "batch": B, "bwd_stream_bytes": ctx.bwd_stream_bytes(), "fwd_path": info["fwd_path"],
                                  **{f"{k}_ms": stats(v) for k, v in ms.items()},
                                  "rollout_ms_per_round": round(roll_ms / max(launches, 1), 3), "rounds_per_forward": launches / REPS,
                                  "forward_ms_per_round": round(float(np.median(ms["forward"])) * REPS / max(launches, 1), 3),
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
