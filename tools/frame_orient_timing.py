"""Cost of the per-instance frame-orientation costs (DDP_HIP_FLAG_FRAME_ORIENT_COST) at the benchmark shape: the Talos-like
tree38, T = 200, batch 64, in mode 2 (forward-differenced first order, static mode-2 stencil) and mode 1 (analytic first order).

    python tools/frame_orient_timing.py                      per mode and for 1 and 4 frames, in one process: frame positions
                                                             alone (DDP_HIP_FLAG_FRAME_COST), then positions + orientations
    python tools/frame_orient_timing.py --off                no flag at all (one process per library when comparing two)
    python tools/frame_orient_timing.py --compare OTHER.so   no flag, this tree's library against OTHER.so (the parent commit's
                                                             build), --runs alternating processes each

Every call is synchronous and timed by the wall clock: median [min - max] of 20 samples after 3 warm-ups, one JSON line per
(mode, frames, orientation).  With the flags on every (instance, t, frame) carries non-zero position and orientation weights, a
target 0.1 away from the frame and a reference rotation 0.05 .. 2.5 rad away from it.  Linearise is timed with weights of order
1.  Backward and forward are timed with the same weights scaled by 1e-12, as tools/frame_cost_timing.py does and for its reason:
at T = 200 no full-DDP sweep of this tree with a V_x of order 1 stays positive definite in double, and a sweep that
restarts is not one sweep; the kernels and their bytes do not depend on the values.  The forward's wall time counts line-search
rounds, so the rollout kernel is also timed per round with the ddp_hip_profile_* events (rollout_ms_per_round)."""
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


def rot(axis, ang):
    import numpy as np
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def quat_of(M):
    """x y z w of a rotation matrix (the branch of the largest diagonal entry / trace), normalised"""
    import numpy as np
    d = [M[0, 0], M[1, 1], M[2, 2], M[0, 0] + M[1, 1] + M[2, 2]]
    k = int(np.argmax(d))
    if k == 3:
        s = 2 * np.sqrt(d[3] + 1)
        qt = [(M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s, 0.25 * s]
    else:
        i, j, l = k, (k + 1) % 3, (k + 2) % 3
        s = 2 * np.sqrt(1 + M[i, i] - M[j, j] - M[l, l])
        qt = [0.0, 0.0, 0.0, (M[l, j] - M[j, l]) / s]
        qt[i], qt[j], qt[l] = 0.25 * s, (M[i, j] + M[j, i]) / s, (M[i, l] + M[l, i]) / s
    qt = np.array(qt)
    return qt / np.linalg.norm(qt)


def measure(settings):
    """settings: (frames, orientation) pairs; frames 0: no flag"""
    import numpy as np

    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    from test_frame_cost import pick_frames
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    rng = np.random.default_rng(1)
    task = {}
    for F in sorted({f for f, _ in settings if f}):
        frames = [fr for fr in pick_frames(model, 4)[4 - F:]]          # 1: a leaf; 4: joint 0, a mid-tree joint, two leaves
        tgt, quat = np.zeros((seeds, T + 1, F, 3)), np.zeros((seeds, T + 1, F, 4))
        for s in range(seeds):
            X = trajs[s][2].reshape(T + 1, o.nx)
            for t in range(T + 1):
                for f, (j, off) in enumerate(frames):
                    q = X[t][:o.nq]
                    p0 = o.frame_position(j, (0.0, 0.0, 0.0), q)
                    R = np.stack([o.frame_position(j, tuple(e), q) - p0 for e in np.eye(3)], axis=1)
                    tgt[s, t, f] = o.frame_position(j, off, q) + 0.1 * rng.normal(size=3) / np.sqrt(3)
                    quat[s, t, f] = quat_of(R @ rot(rng.normal(size=3), -rng.uniform(0.05, 2.5)))
        idx = np.arange(B) % seeds
        task[F] = (frames, tgt[idx], quat[idx], rng.uniform(0.5, 2.0, size=(B, T + 1, F, 3)), rng.uniform(0.5, 2.0, size=(B, T + 1, F, 3)))
    for fd_mode, fo in ((2, 1), (1, 0)):
        _, spec, _ = make("tree38", T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
        for F, orient in settings:
            flags = (capi.FLAG_FRAME_COST if F else 0) | (capi.FLAG_FRAME_ORIENT_COST if orient else 0)
            with capi.Context(spec, flags=flags) as ctx:
                ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
                if F:
                    frames, tgt, quat, w, ow = task[F]
                    ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
                    if orient:
                        ctx.set_frame_orient_cost(quat=quat, weight=ow)

                def weights(scale):
                    if F:
                        ctx.set_frame_cost(weight=scale * w)
                        if orient:
                            ctx.set_frame_orient_cost(weight=scale * ow)
                ctx.linearize()
                ms = {"linearize": [], "backward": [], "forward": []}
                restarts = 0
                ctx.profile_enable(kernels=[capi.K_FWD_ROLLOUT])   # event pairs around every rollout launch (one per line-search round)
                for r in range(WARM + REPS):
                    if r == WARM:
                        ctx.profile_reset()
                    weights(1.0)
                    t0 = time.perf_counter()
                    ctx.linearize()
                    t1 = time.perf_counter()
                    if F:
                        weights(1e-12)
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
                                  "frames": F, "orientation": bool(orient),
                                  "T": T, "batch": B, "bwd_stream_bytes": ctx.bwd_stream_bytes(), "fwd_path": info["fwd_path"],
                                  **{f"{k}_ms": stats(v) for k, v in ms.items()},
                                  "rollout_ms_per_round": round(roll_ms / max(launches, 1), 3), "rounds_per_forward": launches / REPS,
                                  "restarts": restarts, "mean_step": float(np.mean(step))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--off", action="store_true", help="no flag only")
    ap.add_argument("--compare", metavar="LIB", help="no flag: this tree's library against LIB, alternating processes")
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
    measure([(0, False)] if a.off else [(1, False), (1, True), (4, False), (4, True)])


if __name__ == "__main__":
    main()
