"""Cost of the per-instance self-collision cost (DDP_HIP_FLAG_SELF_COLLISION_COST) at the benchmark shape: the Talos-like tree38,
T = 200, batch 64, mode 2 (forward-differenced first order, static mode-2 stencil), 12 spheres spread over the tree and 20 pairs
of them on different joints.

    python tools/self_collision_timing.py                      the three states in one process
    python tools/self_collision_timing.py --off                flag off only (one process per library when comparing two)
    python tools/self_collision_timing.py --compare OTHER.so   flag off, this tree's library against OTHER.so (the parent commit's
                                                               build), --runs alternating processes each

The three states, one JSON line each:
    self_collision 0         flag off
    self_collision 1 clear   flag on, every weight non-zero, every margin -10 m: the kernels run and find no active pair
    self_collision 1 tenth   flag on, every weight non-zero; in about a tenth of the (instance, t) blocks one pair's margin puts it
                             5 cm inside, elsewhere every margin is -10 m
Every call is synchronous and timed by the wall clock: median [min - max] of 20 samples after 3 warm-ups.  The cost stage is
ddp_hip_linearize_stages(LIN_COST) (lin_self_collision_cost_kernel: batch x (T+1) waves) and ddp_hip_cost_seq_aug
(self_collision_cost_kernel over batch x (T+1) states); the forward counts line-search rounds, so it is also given per round
(rollout + self_collision_cost_kernel over the batch x 8 x (T+1) candidate states + com_sum_kernel + select), beside the rollout
kernel alone from the ddp_hip_profile_* events.  The backward sweep that provides the forward's gains runs on the flag-off
derivatives (the weights are zeroed in two half-batch uploads, which leaves the kernels launched with nothing to add: the live
rule), as in tools/obstacle_cost_timing.py; the weights are back in place for the forward.  The expectation: the
"clear" line sits near the flag-off line."""
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
NS, NPAIR = 12, 20


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def spheres_and_pairs(model):
    """NS spheres on joints spread evenly over the tree and the first NPAIR pairs (a, b), a < b, by the stride that mixes near and
    far joints: (k, k + s) for s = NS / 2, NS / 2 - 1, ..."""
    nj = len(model.parent)
    pts = [(int(round(k * (nj - 1) / (NS - 1))), (0.02, -0.03, 0.1), 0.05) for k in range(NS)]
    pairs = []
    for s in range(NS // 2, 0, -1):
        for k in range(NS - s):
            if len(pairs) < NPAIR and pts[k][0] != pts[k + s][0]:
                pairs.append((k, k + s))
    assert len(pairs) == NPAIR
    return pts, pairs


def scene(o, pts, pairs, xs, state, rng):
    """margins and weights (B, T+1, NPAIR) of a state ("clear" / "tenth"), and the share of blocks with a pair put inside"""
    import numpy as np
    m = np.full((B, T + 1, NPAIR), -10.0)
    w = rng.uniform(0.5, 2.0, size=(B, T + 1, NPAIR))
    hit = np.zeros((B, T + 1), dtype=bool)
    if state == "tenth":
        hit = rng.uniform(size=(B, T + 1)) < 0.1
        X = xs.reshape(B, T + 1, o.nx)
        for b, t in zip(*np.nonzero(hit)):
            i = int(rng.integers(NPAIR))
            (ja, offa, ra), (jb, offb, rb) = pts[pairs[i][0]], pts[pairs[i][1]]
            q = X[b, t][:o.nq]
            D = float(np.linalg.norm(o.frame_position(ja, offa, q) - o.frame_position(jb, offb, q)))
            m[b, t, i] = D - ra - rb + 0.05
    return m, w, float(hit.mean())


def measure(states):
    import numpy as np

    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    rng = np.random.default_rng(1)
    pts, pairs = spheres_and_pairs(model)
    _, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    for state in states:
        on = state != "off"
        with capi.Context(spec, flags=capi.FLAG_SELF_COLLISION_COST if on else 0) as ctx:
            ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
            share = 0.0
            if on:
                m, w, share = scene(o, pts, pairs, xs, state, rng)
                ctx.set_self_collision_pairs(points=pts, pairs=pairs)
                ctx.set_self_collision_cost(margin=m, weight=w)
            ctx.linearize()
            ms = {"linearize": [], "lin_cost": [], "cost_seq": [], "backward": [], "forward": []}
            restarts = 0
            ctx.profile_enable(kernels=[capi.K_FWD_ROLLOUT])   # event pairs around every rollout launch (one per line-search round)
            mu1 = np.ones(B)
            for r in range(WARM + REPS):
                if r == WARM:
                    ctx.profile_reset()
                if on:
                    ctx.set_self_collision_cost(weight=w)
                t0 = time.perf_counter()
                ctx.linearize()
                t1 = time.perf_counter()
                ctx.linearize(capi.LIN_COST)
                t1b = time.perf_counter()
                ctx.cost_seq_aug(0, mu1)
                t1c = time.perf_counter()
                if on:
                    ctx.set_self_collision_cost(weight=np.zeros(NPAIR), first=0, count=B // 2)
                    ctx.set_self_collision_cost(weight=np.zeros(NPAIR), first=B // 2, count=B - B // 2)
                    ctx.linearize()
                t2 = time.perf_counter()
                _, _, mu, rs = ctx.backward(0.0, 1.0)
                t2b = time.perf_counter()
                if on:
                    ctx.set_self_collision_cost(weight=w)
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
            worst = float(np.min(ctx.self_collision_clearance(0))) if on else None
            print(json.dumps({"lib": os.path.basename(capi.LIB_PATH), "self_collision": int(on), "state": state, "active_share": round(share, 4),
                              "min_clearance": worst, "T": T, "batch": B, "spheres": NS, "pairs": NPAIR, "fwd_path": info["fwd_path"],
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
    measure(["off"] if a.off else ["off", "clear", "tenth"])


if __name__ == "__main__":
    main()
