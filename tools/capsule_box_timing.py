"""Cost of the capsule pairs of kind DDP_HIP_CAPSULE_VS_BOX at the benchmark shape, in the manner of capsule_cost_timing.py: the
Talos-like tree38, T = 200, batch 64, mode 2, on held trajectories; 8 capsules in 16 pairs (4 robot pairs, 2 world capsules, 2
half-spaces and 8 box pairs on 4 shapes), half of the pairs 2 cm inside their margin at every (instance, t), the other half 5 cm clear.

    python tools/capsule_box_timing.py [--runs 3] [--out profiles/capsule_box.json] [--bench LINES.jsonl]

Three contexts, one after the other: "box" as described; "world", the same context with its 8 box pairs replaced by world-capsule
pairs at the same places (what the kind itself costs is the difference); and a flag-off context.  In the first two the weights are
live and 0 (uploaded in two half-batch ranges: the kernels stay launched) in --runs alternating runs.  Every call is synchronous and
timed by the wall clock: per run the median of 10 samples after 2 warm-ups, and over the runs the median [min - max] of those.
--bench: JSON lines of bench.py runs made beside it (this tree's library and the parent commit's, flag off), copied into the file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, B, WARM, REPS = 200, 64, 2, 10
ROBOT, WORLD, HALF, BOX = 0, 1, 2, 4


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def task(o, model, trajs, variant):
    """8 capsules on joints spread over the tree, 16 pairs, 4 box shapes, and per distinct trajectory geom (T+1, 16, 8): a box rides
    with a random orientation, its centre 25 cm beside its capsule's middle; the world capsule that stands in for it in the
    "world" variant rides 10 cm beside it; the margins put the even pairs 2 cm inside and the odd pairs 5 cm clear"""
    import numpy as np

    import test_capsule_box as tb
    cc = tb.cc
    nj = len(model.parent)
    joints = [int(round(k * (nj - 1) / 7.0)) for k in range(8)]
    caps = [(j, (0.0, 0.0, 0.0), (0.03, 0.02, 0.12) if k != 3 else (0.0, 0.0, 0.0), 0.04) for k, j in enumerate(joints)]   # capsule 3: a sphere
    kind8 = BOX if variant == "box" else WORLD
    pairs = [(a, ROBOT, a + 4) for a in range(4)] + [(a, WORLD, 0) for a in (0, 4)] + [(a, HALF, 0) for a in (1, 5)] + [(a, kind8, a % 4) for a in range(8)]
    assert len(pairs) == 16 and all(caps[a][0] != caps[b][0] for a, k, b in pairs if k == ROBOT)
    shapes = np.array([[0.3, 0.2, 0.02], [0.05, 0.05, 0.4], [0.15, 0.15, 0.15], [0.4, 0.03, 0.1]])
    ev = tb.box_eval(shapes, tb.cg._SIBLING_EVAL)
    rng = np.random.default_rng(2)
    geoms = []
    for xs in trajs:
        X = xs.reshape(T + 1, o.nx)
        g = np.zeros((T + 1, 16, 8))
        for t in range(T + 1):
            E = cc.ends(o, caps, X[t][:o.nq])
            for i, pair in enumerate(pairs):
                mid = 0.5 * (E[pair[0]][0] + E[pair[0]][1])
                if pair[1] == WORLD:
                    c, half = mid + 0.1 * cc._unit(rng), 0.1 * cc._unit(rng)
                    g[t, i, 0:3], g[t, i, 3:6], g[t, i, 6] = c - half, c + half, 0.03
                elif pair[1] == HALF:
                    n = cc._unit(rng)
                    g[t, i, 0:3], g[t, i, 3] = n, float(n @ mid) - 0.2
                elif pair[1] == BOX:
                    q = rng.normal(size=4)
                    g[t, i, 0:3], g[t, i, 3:7] = mid + 0.25 * cc._unit(rng), q / np.sqrt(q @ q)
                g[t, i, 7] = ev(caps, E, pair, g[t, i])["d"] + (0.02 if i % 2 == 0 else -0.05)
        geoms.append(g)
    return caps, pairs, shapes, geoms


def measure(runs):
    import numpy as np

    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    weight = np.random.default_rng(1).uniform(0.5, 5.0, size=(B, T + 1, 16))
    _, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    records = []

    def timed(ctx, mu):
        lin, fwd = [], []
        for r in range(WARM + REPS):
            t0 = time.perf_counter()
            ctx.linearize()
            t1 = time.perf_counter()
            _, step, _ = ctx.forward(mu, n_alpha=8)
            t2 = time.perf_counter()
            if r >= WARM:
                lin.append((t1 - t0) * 1e3); fwd.append((t2 - t1) * 1e3)
        return float(np.median(lin)), float(np.median(fwd)), float(np.mean(step))

    for variant in ("box", "world", "off"):
        on = variant != "off"
        if on:
            caps, pairs, shapes, geoms = task(o, model, [tr[2] for tr in trajs], variant)
            geom = np.stack([geoms[b % seeds] for b in range(B)])
        with capi.Context(spec, flags=capi.FLAG_CAPSULE_COST if on else 0) as ctx:
            ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
            if on:
                ctx.set_capsule_boxes(shapes)
                ctx.set_capsule_pairs(capsules=caps, pairs=pairs)
                ctx.set_capsule_cost(geom=geom, weight=weight)

            def zero():
                ctx.set_capsule_cost(weight=0.0 * weight[:B // 2], first=0, count=B // 2)
                ctx.set_capsule_cost(weight=0.0 * weight[B // 2:], first=B // 2, count=B - B // 2)
            if on:
                zero()
            ctx.linearize()
            _, _, mu, _ = ctx.backward(0.0, 1.0)
            res = {}
            for r in range(runs):
                for state in (("live", "zero") if on else ("off",)):
                    if state == "live":
                        ctx.set_capsule_cost(weight=weight)
                    elif state == "zero":
                        zero()
                    res.setdefault(state, []).append(timed(ctx, mu))
            clear = None
            if on:                                   # (with the weights live: a zero weight measures nothing)
                ctx.set_capsule_cost(weight=weight)
                clear = float(np.min(ctx.capsule_clearance(0)))
            for state, v in res.items():
                records.append({"lib": os.path.basename(capi.LIB_PATH), "variant": variant, "state": state, "T": T, "batch": B,
                                "capsules": 8, "pairs": 16, "box_pairs": 8 if variant == "box" else 0, "runs": runs,
                                "fwd_path": ctx.info()["fwd_path"], "linearize_ms": stats([x[0] for x in v]),
                                "forward_ms": stats([x[1] for x in v]), "mean_step": v[-1][2], "least_clearance": clear})
                print(json.dumps(records[-1]), flush=True)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", metavar="FILE")
    ap.add_argument("--bench", metavar="FILE", help="JSON lines of bench.py runs to copy into --out")
    a = ap.parse_args()
    out = {"states": measure(a.runs)}
    if a.bench:
        out["bench_flag_off"] = [json.loads(line) for line in open(a.bench) if line.startswith("{")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
