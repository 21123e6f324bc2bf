"""Cost of the control bounds (DDP_HIP_FLAG_CONTROL_BOUNDS) in the backward sweep at the benchmark shape: the Talos-like
tree38, T = 200, batch 64, with the second-order tensors (K5 -> K3h -> K4' as one graph launch).  One synchronous
ddp_hip_backward per sample, timed by the wall clock after a warm-up; every sample is printed, so the spread shows.

  (a) the flag-off sweep of the in-tree library against the parent commit's library, if build_ab/libddp_hip_parent.so exists
      (the parent's ddp_pinocchio_amd/csrc built beside the tree), alternating: the same kernels, so a difference beyond the
      spread of the parent's own repeats is a defect;
  (b) flag on, bounds +-inf;
  (c) flag on, lo = u - w U(0,1), hi = u + w U(0,1) for w = 0.2 and 0.05, with the mean of BOX_STAT[:, 1] (projected-Newton
      iterations per step) and of BOX_STAT[:, 0] (clamped controls) beside each.

Every measurement is a child process of its own (a library is chosen at load time) under its own time limit; the first
failure stops the run.  usage: python tools/control_bounds_timing.py            (from the repository root, on the GPU)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, B, WARM, REPS = 200, 64, 3, 20
PARENT_LIB = os.path.join(ROOT, "build_ab", "libddp_hip_parent.so")
CHILD_LIMIT_S = 280


def child(kind):
    import time
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    from ddp_pinocchio_amd import capi
    from problems import held_trajectory, make
    model, _, o = make("tree38", T, batch=1, fd_mode=2)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    _, spec, _ = make("tree38", T, batch=B, fd_mode=2)
    flags = 0 if kind == "off" else getattr(capi, "FLAG_CONTROL_BOUNDS")
    with capi.Context(spec, flags=flags) as ctx:
        ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
        if kind.startswith("w"):
            w = float(kind[1:])
            rng = np.random.default_rng(1)
            U = us.reshape(B, T, o.m)
            ctx.set_control_bounds(lo=U - w * rng.uniform(0, 1, size=U.shape), hi=U + w * rng.uniform(0, 1, size=U.shape))
        ctx.linearize()
        ms, restarts = [], 0
        for r in range(WARM + REPS):
            t0 = time.perf_counter()
            _, _, _, rs = ctx.backward(0.0, 1.0)
            t1 = time.perf_counter()
            if r >= WARM:
                ms.append(round((t1 - t0) * 1e3, 3))
                restarts += int(rs.sum())
        out = {"kind": kind, "lib": os.path.relpath(capi.LIB_PATH, ROOT), "T": T, "batch": B, "bwd_path": ctx.info()["bwd_path"],
               "bwd_stream_bytes": ctx.bwd_stream_bytes(), "sweep_ms": ms, "sweep_ms_median": float(np.median(ms)),
               "sweep_ms_min": min(ms), "sweep_ms_max": max(ms), "restarts": restarts}
        if kind != "off":
            st = ctx.download("BOX_STAT").reshape(B, T, 2)
            out["mean_clamped"] = float(st[:, :, 0].mean())
            out["mean_iterations"] = float(st[:, :, 1].mean())
            out["max_iterations"] = float(st[:, :, 1].max())
        print(json.dumps(out), flush=True)


def main():
    runs = []
    if os.path.exists(PARENT_LIB):
        runs += [("off", PARENT_LIB), ("off", None)] * 3
    else:
        print(f"# {os.path.relpath(PARENT_LIB, ROOT)} is missing: (a) is skipped", flush=True)
        runs += [("off", None)]
    runs += [("inf", None), ("w0.2", None), ("w0.05", None)]
    for kind, lib in runs:
        env = dict(os.environ)
        env.pop("DDP_HIP_LIB", None)
        if lib:
            env["DDP_HIP_LIB"] = lib
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind], env=env, timeout=CHILD_LIMIT_S).returncode
        if rc != 0:
            print(f"# {kind} ({lib or 'in-tree'}) ended with status {rc}: stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main())
