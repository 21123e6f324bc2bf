"""Time of the receding-horizon advance (ddp_hip_advance) against the composed path of the same library -- download every per-step
array, roll it with numpy, upload it again, forward(n_alpha=0) + swap_traj (or rollout) -- which is what a caller had before the
entry point existed.  The benchmark shape: the Talos-like tree38, T = 200, batch 64, tracking, control bounds and four add-on terms
resident and live (frame positions on 3 frames, state limits, centre of mass, obstacles on 3 slots); shift s = 1, the overlap case.
The context is tensor-free (the second-order tensors play no part in an advance).

    python tools/advance_probe.py                                   prints one JSON line per mode
    python tools/advance_probe.py --out profiles/bench_advance.json  ... and writes them to the file

Two contexts hold the same data; one is advanced, the other goes the composed way, alternating, RUNS times per mode, every call
ending in a device synchronise and timed by the wall clock.  After every pair X, U and FB_JAC of the two are compared bit for bit
(a probe that times two different computations says nothing).  NO_ROLL reports the bytes moved per second against twice the
shifted bytes (every word of a walked row is read once and written once); the rolling modes stand beside one
ddp_hip_forward(n_alpha=0) and one ddp_hip_rollout of the same context."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T, B, S, RUNS, INNER = 200, 64, 1, 3, 3


def roll(a, s, rule="hold", terminal=False):
    """the header's row rules on (B, rows, ...): the composed path's numpy part"""
    import numpy as np
    out = a.copy()
    R = a.shape[1] - (1 if terminal else 0)
    keep = max(R - s, 0)
    if rule == "zero":
        out[:, :R] = 0.0
        return out
    out[:, :keep] = a[:, s:R]
    out[:, keep:R] = 0.0 if rule == "zero_tail" else a[:, R - 1:R]
    return out


def stats(v):
    import numpy as np
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3), "runs": [round(float(x), 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", metavar="FILE")
    a = ap.parse_args()
    import numpy as np

    import test_frame_cost as fc
    import test_obstacle_cost as ob
    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    assert capi.lib().ddp_hip_device_count() > 0, "advance_probe needs an MI355X: there is no CPU fallback"
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8
    trajs = [held_trajectory(o, model, seed=k, q0_sigma=0.3) for k in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    _, spec, _ = make("tree38", T, batch=B, fd_mode=0)
    n, m, nx = spec.n, spec.m, spec.nx
    rng = np.random.default_rng(1)
    flags = (capi.FLAG_NO_TENSORS | capi.FLAG_TRACKING_COST | capi.FLAG_CONTROL_BOUNDS | capi.FLAG_FRAME_COST | capi.FLAG_STATE_LIMITS |
             capi.FLAG_COM_COST | capi.FLAG_OBSTACLE_COST)
    frames, pts = fc.pick_frames(model, 3), ob.pick_points(model)
    kinds = (capi.OBSTACLE_SPHERE, capi.OBSTACLE_HALFSPACE, capi.OBSTACLE_SPHERE)
    geom = rng.normal(size=(B, T + 1, 3, 4)) + np.array([5.0, 5.0, 5.0, 0.0])      # far away: live weights, nothing touched
    geom[..., 3] = 0.1
    geom[:, :, 1, :3] = np.array([0.0, 0.0, 1.0]); geom[:, :, 1, 3] = -50.0
    data = dict(xref=xs.reshape(B, T + 1, nx), wx=rng.uniform(0.1, 1, size=(B, T + 1, n)), uref=us.reshape(B, T, m), wu=rng.uniform(0.1, 1, size=(B, T, m)),
                lo=us.reshape(B, T, m) - 50.0, hi=us.reshape(B, T, m) + 50.0, K=1e-3 * rng.normal(size=(B, T, m * n)))

    def fresh():
        ctx = capi.Context(spec, flags=flags)
        ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
        ctx.set_tracking_cost(xref=data["xref"], wx=data["wx"], uref=data["uref"], wu=data["wu"])
        ctx.set_control_bounds(lo=data["lo"], hi=data["hi"])
        ctx.set_frame_cost(frames=frames, target=rng.normal(size=(B, T + 1, 3, 3)), weight=np.full((B, T + 1, 3, 3), 0.5))
        ctx.set_state_limits(lo=np.full((B, T + 1, n), -100.0), hi=np.full((B, T + 1, n), 100.0), weight=np.full((B, T + 1, n), 0.5))
        ctx.set_com_cost(target=rng.normal(size=(B, T + 1, 3)), weight=np.full((B, T + 1, 3), 0.5))
        ob.set_task(ctx, pts, kinds, geom, np.full((B, T + 1, 3), 0.5))
        ctx.upload("FB_JAC", data["K"]); ctx.upload("FB_VAL", np.zeros((B, T * m)))
        ctx.upload("FB_ORIGIN", xs[:, :T * nx]); ctx.upload("MULT_ORIGIN", xs[:, :T * nx])
        return ctx

    def seq(ctx, name, rows):
        return ctx.download(name).reshape(B, rows, -1)

    def composed(ctx, mode):
        """the caller's recipe; returns the bytes it rolled"""
        moved = 0
        X = roll(seq(ctx, "X", T + 1), S)
        U = roll(seq(ctx, "U", T), S)
        K = roll(seq(ctx, "FB_JAC", T), S, "zero_tail")
        moved += X.nbytes + U.nbytes + K.nbytes + U.nbytes            # (+ FB_VAL)
        ctx.upload("X", X); ctx.upload("U", U); ctx.upload("FB_JAC", K); ctx.upload("FB_VAL", np.zeros((B, T * m)))
        for name, rows, terminal in (("COST_XREF", T + 1, True), ("COST_WX", T + 1, True), ("COST_UREF", T, False), ("COST_WU", T, False),
                                     ("CTRL_LO", T, False), ("CTRL_HI", T, False)):
            v = roll(seq(ctx, name, rows), S, terminal=terminal)
            moved += v[:, :T].nbytes
            ctx.upload(name, v)
        for get, put, keys in ((ctx.frame_cost, ctx.set_frame_cost, ("target", "weight")), (ctx.state_limits, ctx.set_state_limits, ("lo", "hi", "weight")),
                               (ctx.com_cost, ctx.set_com_cost, ("target", "weight")), (ctx.obstacle_cost, ctx.set_obstacle_cost, ("geom", "weight"))):
            sides = [roll(v, S, terminal=True) for v in get()]
            moved += sum(v[:, :T].nbytes for v in sides)
            put(**dict(zip(keys, sides)))
        if mode == capi.ADVANCE_OPEN_LOOP:
            ctx.rollout()
        elif mode == capi.ADVANCE_CLOSED_LOOP:
            ctx.upload("X_NEW", X)
            ctx.forward(np.ones(B), n_alpha=0)
            ctx.swap_traj()
        X = ctx.download("X")
        ctx.upload("X_NEW", X); ctx.upload("U_NEW", ctx.download("U"))
        ctx.upload("FB_ORIGIN", X[:, :T * nx]); ctx.upload("MULT_ORIGIN", X[:, :T * nx])
        return moved

    records = []
    names = {capi.ADVANCE_NO_ROLL: "NO_ROLL", capi.ADVANCE_OPEN_LOOP: "OPEN_LOOP", capi.ADVANCE_CLOSED_LOOP: "CLOSED_LOOP"}
    with fresh() as ca, fresh() as cb:
        for mode in names:                                            # warm-up: every kernel and every copy shape once
            ca.advance(S, None, mode); composed(cb, mode)
        for ctx in (ca, cb):
            ctx.upload("FB_JAC", data["K"])
        fwd, rol = [], []
        for _ in range(RUNS):
            ca.upload("X_NEW", ca.download("X"))
            t0 = time.perf_counter(); ca.forward(np.ones(B), n_alpha=0); t1 = time.perf_counter(); ca.rollout(); t2 = time.perf_counter()
            fwd.append((t1 - t0) * 1e3); rol.append((t2 - t1) * 1e3)
        cb.upload("X", ca.download("X")); cb.upload("X_NEW", ca.download("X_NEW")); cb.upload("U_NEW", ca.download("U_NEW"))
        for mode, label in names.items():
            adv, comp, moved = [], [], 0
            for _ in range(RUNS):
                for ctx in (ca, cb):                                  # the same gains in both: an advance zeroes one row more each time
                    ctx.upload("FB_JAC", data["K"])
                ts = []
                for _ in range(INNER):
                    t0 = time.perf_counter(); ca.advance(S, None, mode); ts.append((time.perf_counter() - t0) * 1e3)
                adv.append(float(np.median(ts)))
                t0 = time.perf_counter(); moved = composed(cb, mode); comp.append((time.perf_counter() - t0) * 1e3)
                for _ in range(INNER - 1):                            # (untimed: the two contexts stay in step)
                    composed(cb, mode)
                for k in ("X", "U", "FB_JAC"):
                    assert np.array_equal(ca.download(k), cb.download(k), equal_nan=True), (label, k)
            rec = {"mode": label, "T": T, "batch": B, "shift": S, "advance_ms": stats(adv), "composed_ms": stats(comp),
                   "speedup_median": round(float(np.median(comp) / np.median(adv)), 1), "shifted_bytes": int(moved),
                   "forward_n_alpha0_ms": stats(fwd), "rollout_ms": stats(rol), "fwd_path": ca.info()["fwd_path"]}
            if mode == capi.ADVANCE_NO_ROLL:
                rec["gbytes_per_s"] = round(2 * moved / (float(np.median(adv)) * 1e-3) / 1e9, 1)
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"runs": records}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
