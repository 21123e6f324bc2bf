"""Cost of the per-instance balance-region cost (DDP_HIP_FLAG_BALANCE_REGION_COST) at the benchmark shape: the Talos-like tree38,
T = 200, batch 64, mode 2 (forward-differenced first order, static mode-2 stencil), on held trajectories, eight plane slots:
a box about the CoM (four slots, tau = 0) and a box about the capture point (four slots, tau = 0.3).

    python tools/balance_region_timing.py                      the four states in one process
    python tools/balance_region_timing.py --off                flag off only (one process per library when comparing two)
    python tools/balance_region_timing.py --compare OTHER.so   flag off, this tree's library against OTHER.so (the parent commit's
                                                               build), --runs alternating processes each
    python tools/balance_region_timing.py --compare OTHER.so --out profiles/balance_region_cost.json
                                                               the comparison, then the four states, and every line of both in
                                                               the file: {"states": [...], "compare": [...], "added": {...},
                                                               "added_clear": {...}, "momentum_for_scale": {...}}

The four states, one JSON line each:
    balance_region 0           flag off
    balance_region 1 zero      flag on, every weight 0 (uploaded in two half-batch ranges: the kernels stay launched and return at
                               their first test, the live rule of DESIGN.md 4p) -- the same context the live states are held against
    balance_region 1 clear     flag on, eight live planes, the tested points 2 cm inside both boxes: the usual case of a one-sided
                               term -- values formed, nothing active, no jacobian
    balance_region 1 full      flag on, eight live planes, every (instance, t) 2 cm outside one plane of each box: the CoM's and the
                               capture point's jacobians formed at every (instance, t)
Every call is synchronous and timed by the wall clock: median [min - max] of 20 samples after 3 warm-ups.  The cost stage is
ddp_hip_linearize_stages(LIN_COST) (lin_balance_region_cost_kernel: batch x (T+1) waves) and ddp_hip_cost_seq_aug
(balance_region_cost_kernel over batch x (T+1) states); the forward counts line-search rounds, so it is also given per round
(rollout + balance_region_cost_kernel over the batch x 8 x (T+1) candidate states + com_sum_kernel + select).  The backward sweep
that provides the forward's gains runs on the flag-off derivatives (the weights zeroed as above), as in
tools/frame_aim_timing.py; the weights are back in place for the forward.  "added": full minus zero, of the medians -- the whole
linearisation, its cost stage alone (the same difference without the stencil's spread on top) and a forward round -- with the
noise = the larger of the two states' (max - min) / 2; "added_clear": the same for the clear state; "momentum_for_scale": the
momentum term's differences (all six weights against flag off) from profiles/momentum_cost.json, as that file holds them."""
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
NP, TAU, HALF = 8, 0.3, 0.03                        # plane slots; the capture-point slots' time constant; the boxes' half width


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def boxes(xi0, xi1, shift):
    """eight planes (n, h, tau): a box of half width HALF about xi0 + shift e_x (tau = 0) and one about xi1 + shift e_y (tau = TAU).
    shift = 0: the points sit in the middle, every plane clear by HALF; shift = HALF + 0.02: 2 cm outside one plane of each box"""
    import numpy as np
    out = []
    for centre, tau in ((xi0 + np.array([shift, 0.0, 0.0]), 0.0), (xi1 + np.array([0.0, shift, 0.0]), TAU)):
        for n in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)):
            out.append(list(n) + [float(np.dot(n, centre)) - HALF, tau])
    return np.array(out)


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
    records = []
    geoms = {}
    if any(s != "off" for s in states):
        # the boxes follow the tested points of each trajectory, t by t (a held trajectory stands almost still)
        for name, shift in (("zero", HALF + 0.02), ("clear", 0.0), ("full", HALF + 0.02)):
            geoms[name] = np.zeros((B, T + 1, NP, 5))
        with capi.ModelHandle(model) as h:
            for s in range(seeds):
                X = trajs[s][2].reshape(T + 1, o.nx)
                for t in range(T + 1):
                    q, v = X[t][:o.nq], X[t][o.nq:]
                    xi0, xi1 = h.capture_point(q, v, 0.0), h.capture_point(q, v, TAU)
                    for name, shift in (("zero", HALF + 0.02), ("clear", 0.0), ("full", HALF + 0.02)):
                        geoms[name][s::seeds, t] = boxes(xi0, xi1, shift)
    for state in states:
        on = state != "off"
        with capi.Context(spec, flags=capi.FLAG_BALANCE_REGION_COST if on else 0) as ctx:
            ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
            w = None
            if on:
                ctx.set_balance_region_planes(NP)
                w = 100.0 * rng.uniform(0.5, 2.0, size=(B, T + 1, NP))
                ctx.set_balance_region_cost(geom=geoms[state])

            def zero():
                ctx.set_balance_region_cost(weight=np.zeros(NP), first=0, count=B // 2)
                ctx.set_balance_region_cost(weight=np.zeros(NP), first=B // 2, count=B - B // 2)

            def live():
                ctx.set_balance_region_cost(weight=w)
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
            margin = float(np.min(ctx.balance_region_margin(0))) if on and state != "zero" else None
            fwd = np.asarray(ms["forward"]) * REPS / max(launches, 1)
            records.append({"lib": os.path.basename(capi.LIB_PATH), "balance_region": int(on), "state": state, "T": T, "batch": B, "planes": NP,
                            "fwd_path": info["fwd_path"], **{f"{k}_ms": stats(v) for k, v in ms.items()},
                            "rollout_ms_per_round": round(roll_ms / max(launches, 1), 3), "rounds_per_forward": launches / REPS,
                            "forward_ms_per_round": round(float(np.median(fwd)), 3),
                            "forward_ms_per_round_range": [round(float(np.min(fwd)), 3), round(float(np.max(fwd)), 3)],
                            "restarts": restarts, "mean_step": float(np.mean(step)), "least_margin": margin})
            print(json.dumps(records[-1]), flush=True)
    return records


def added(records, live_state="full"):
    """what the live state adds to the zero state: the linearisation and a forward round, each with its noise"""
    by = {r["state"]: r for r in records}
    if live_state not in by or "zero" not in by:
        return {}
    a, z = by[live_state], by["zero"]

    def half(r, k):
        return (r[k]["max"] - r[k]["min"]) / 2
    fr = "forward_ms_per_round_range"
    return {"state": live_state,
            "linearize_ms": round(a["linearize_ms"]["median"] - z["linearize_ms"]["median"], 3),
            "linearize_noise_ms": round(max(half(a, "linearize_ms"), half(z, "linearize_ms")), 3),
            "lin_cost_ms": round(a["lin_cost_ms"]["median"] - z["lin_cost_ms"]["median"], 3),
            "lin_cost_noise_ms": round(max(half(a, "lin_cost_ms"), half(z, "lin_cost_ms")), 3),
            "forward_round_ms": round(a["forward_ms_per_round"] - z["forward_ms_per_round"], 3),
            "forward_round_noise_ms": round(max(a[fr][1] - a[fr][0], z[fr][1] - z[fr][0]) / 2, 3)}


def momentum_scale():
    """the momentum term's figures, from the committed file: its full state minus its flag-off state"""
    path = os.path.join(ROOT, "profiles", "momentum_cost.json")
    if not os.path.exists(path):
        return {}
    by = {r["state"]: r for r in json.load(open(path))["states"]}
    if "full" not in by or "off" not in by:
        return {}
    a, z = by["full"], by["off"]
    return {"source": "profiles/momentum_cost.json",
            "linearize_ms": round(a["linearize_ms"]["median"] - z["linearize_ms"]["median"], 3),
            "lin_cost_ms": round(a["lin_cost_ms"]["median"] - z["lin_cost_ms"]["median"], 3),
            "forward_round_ms": round(a["forward_ms_per_round"] - z["forward_ms_per_round"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off", action="store_true", help="flag off only")
    ap.add_argument("--compare", metavar="LIB", help="flag off: this tree's library against LIB, alternating processes")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", metavar="FILE", help="write every line of this call to FILE; with --compare the four states are measured as well")
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
                out["compare"] += [json.loads(line) for line in run.stdout.splitlines() if line.startswith('{"lib"')]
    if not a.compare or a.out:
        out["states"] = measure(["off"] if a.off else ["off", "zero", "clear", "full"])
        if not a.off:
            out["added"] = added(out["states"])
            out["added_clear"] = added(out["states"], "clear")
            out["momentum_for_scale"] = momentum_scale()
            print(json.dumps({k: out[k] for k in ("added", "added_clear", "momentum_for_scale")}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
