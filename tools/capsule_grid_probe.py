"""What a capsule pair against the voxel grid (DDP_HIP_CAPSULE_VS_GRID) costs on the device -> profiles/capsule_grid.json.

    python tools/capsule_grid_probe.py [--out profiles/capsule_grid.json]

The Talos-like tree, T = 200, batch 64; a field of 64^3 nodes of 3 cm around the robot, built by set_occupancy from random
occupied blocks; 8 robot capsules of 48 cm (16 cells: 17 samples each) on joints spread over the tree, each in one grid pair.
Three arms, measured in three rounds that alternate between them; a round's figure is the median of REPS synchronous calls after
WARM warm-ups, timed by the wall clock (every call ends in a stream synchronise); the file holds the median of the three rounds and
their range.

  live      the 8 grid pairs with weight 1 and a margin that makes about a tenth of the (pair, t, instance) terms active
  zero      the same context with the pairs' weights 0: the capsule kernels are not launched
  spheres   the yardstick: the obstacle flag with 16 collision spheres, the capsules' two ends, against one grid slot on the same
            field with the same margin

Timed: ddp_hip_linearize_stages(DDP_HIP_LIN_COST) and ddp_hip_forward with n_alpha = 8 (after one full linearise and one sweep,
outside the clock).  The sample loop is the dealt one (the samples of the grid pairs over the lanes); no one-lane form was built."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS, WARM, REPS = 3, 2, 10
T, B, NC, SHARE = 200, 64, 8, 0.10
N_GRID, CELL, SPAN = 64, 0.03, 16


def timed(fn):
    for _ in range(WARM):
        fn()
    v = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(v))


def blocks(rng, n, count, size):
    occ = np.zeros((n, n, n), dtype=np.uint8)
    for _ in range(count):
        i = rng.integers(0, n - size, size=3)
        occ[i[0]:i[0] + size, i[1]:i[1] + size, i[2]:i[2] + size] = 1
    return occ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "capsule_grid.json"))
    a = ap.parse_args()
    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    assert capi.lib().ddp_hip_device_count() > 0, "the probe measures on an MI355X: there is no CPU fallback"
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    nj = len(model.parent)
    radius, length = 0.05, SPAN * CELL
    caps = [(int(round(k * (nj - 1) / (NC - 1))), (0.0, 0.0, 0.0), (0.0, 0.0, length), radius) for k in range(NC)]
    pairs = [(k, capi.CAPSULE_VS_GRID) for k in range(NC)]
    pts = [(j, e, radius) for j, e0, e1, _ in caps for e in (e0, e1)]
    E = np.array([[[np.concatenate([o.frame_position(j, e0, trajs[s][2].reshape(T + 1, o.nx)[t][:o.nq]),
                                    o.frame_position(j, e1, trajs[s][2].reshape(T + 1, o.nx)[t][:o.nq])]) for j, e0, e1, _ in caps]
                   for t in range(T + 1)] for s in range(seeds)])                 # (seeds, T+1, NC, 6)
    centre = E.reshape(-1, 3).mean(axis=0)
    origin = centre - CELL * (N_GRID - 1) / 2.0
    occ = blocks(np.random.default_rng(3), N_GRID, 24, 8)
    _, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    res = {"rounds": ROUNDS, "warm": WARM, "reps": REPS, "clock": "wall clock around synchronous calls, ms", "T": T, "batch": B,
           "capsules": NC, "capsule_length": length, "grid": [N_GRID] * 3, "cell": CELL, "occupied_share": round(float(occ.mean()), 4),
           "sample_loop": "dealt over lanes (no one-lane form was built)"}
    mu1 = np.ones(B)
    got = {}

    def prepare(ctx):
        ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
        ctx.set_obstacle_occupancy(occ, origin, CELL)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu1)
        return mu_o
    with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST) as cc, capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as oc:
        mu_c, mu_s = prepare(cc), prepare(oc)
        phi, j, _, _ = cc.obstacle_grid_segment_query(E.reshape(-1, 6), SPAN)
        d = phi - radius
        fin = np.isfinite(d)
        margin = float(np.quantile(d[fin], min(1.0, SHARE * d.size / fin.sum())))
        res["pairs"] = {"margin": margin, "active_share": round(float(np.mean(d - margin < 0)), 4),
                        "outside_share": round(float(np.mean(~fin)), 4), "middle_sample_share": round(float(np.mean((j > 0) & (j < SPAN))), 4)}
        geom = np.zeros((NC, 8)); geom[:, 7] = margin
        cc.set_capsule_pairs(capsules=caps, pairs=pairs)
        cc.set_capsule_cost(geom=geom, weight=np.ones(NC))
        oc.set_obstacle_points(points=pts, kinds=[capi.OBSTACLE_GRID])
        oc.set_obstacle_cost(geom=np.array([[0.0, 0.0, 0.0, margin]]), weight=np.ones(1))
        cc.linearize(capi.LIN_COST); oc.linearize(capi.LIN_COST)
        res["pairs"]["min_clearance"] = float(np.min(cc.capsule_clearance(0)))
        res["spheres"] = {"points": len(pts), "min_clearance": float(np.min(oc.obstacle_clearance(0)))}
        arms = {"live": (cc, mu_c, lambda: cc.set_capsule_cost(weight=np.ones(NC))),
                "zero": (cc, mu_c, lambda: cc.set_capsule_cost(weight=np.zeros(NC))),
                "spheres": (oc, mu_s, lambda: None)}
        for _ in range(ROUNDS):
            for arm, (ctx, mu_o, use) in arms.items():
                use()                                                             # (outside the clock)
                got.setdefault(f"lin_cost_{arm}", []).append(timed(lambda: ctx.linearize(capi.LIN_COST)))
                got.setdefault(f"forward_{arm}", []).append(timed(lambda: ctx.forward(mu_o, n_alpha=8)))
    res.update({k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                    "rounds_ms": [round(x, 4) for x in v]} for k, v in got.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
