"""What the voxel-grid obstacle kind (DDP_HIP_OBSTACLE_GRID) costs on the device -> profiles/obstacle_grid.json.

    python tools/obstacle_grid_probe.py [--out profiles/obstacle_grid.json]

Two groups of measurements.  Each measurement is taken in three rounds that alternate between the members of its group; a round's
figure is the median of REPS synchronous calls after WARM warm-ups, timed by the wall clock (every call ends in a stream
synchronise); the file holds the median of the three rounds and their range.

  scene   what an MPC cycle pays for a new scene, at 64^3 and 128^3: ddp_hip_obstacle_set_occupancy (the upload of the voxel bytes
          and the distance transform), beside ddp_hip_obstacle_set_grid of a host-made field of the same shape (the upload of
          eight times the bytes, no transform), and a bare synchronous host-to-device copy of the voxel bytes, which is what
          "upload excluded" subtracts (derived, not measured inside the call).
  cost    one ddp_hip_linearize_stages(DDP_HIP_LIN_COST) and one ddp_hip_cost_seq_aug at T = 200, batch 64, the Talos-like tree,
          16 collision points: with one grid slot, against the same context with one sphere slot placed so that the same share of
          (point, t, instance) pairs is active.  The sphere slot is the yardstick; both shares are in the file.  The grid is 32^3
          nodes of 5 cm around the robot's root, built by set_occupancy from random occupied blocks; the margin (grid) and the
          radius (sphere) are the quantiles of the points' distances that give the share."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUNDS, WARM, REPS = 3, 2, 10
T, B, NP, SHARE = 200, 64, 16, 0.10


def timed(fn):
    for _ in range(WARM):
        fn()
    v = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        v.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(v))


def alternate(members):
    """{name: fn} -> {name: {"median_ms", "min_ms", "max_ms", "rounds_ms"}}: ROUNDS rounds, every member once per round"""
    got = {k: [] for k in members}
    for _ in range(ROUNDS):
        for k, fn in members.items():
            got[k].append(timed(fn))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "rounds_ms": [round(x, 4) for x in v]} for k, v in got.items()}


def hip_runtime():
    """the HIP runtime libddp_hip.so itself is linked against and has loaded into this process (its path from /proc/self/maps),
    not whichever copy the bare name would resolve to"""
    from ddp_pinocchio_amd import capi
    capi.lib()
    paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def bare_copy(nbytes):
    """a synchronous host-to-device copy of nbytes from pageable memory, through the HIP runtime the library uses"""
    hip = hip_runtime()
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    dst = C.c_void_p()
    assert hip.hipMalloc(C.byref(dst), nbytes) == 0
    src = np.random.default_rng(0).integers(0, 2, size=nbytes, dtype=np.uint8)

    def fn():
        assert hip.hipMemcpy(dst, src.ctypes.data, nbytes, 1) == 0
    return fn, lambda: hip.hipFree(dst)


def blocks(rng, n, count, size):
    occ = np.zeros((n, n, n), dtype=np.uint8)
    for _ in range(count):
        i = rng.integers(0, n - size, size=3)
        occ[i[0]:i[0] + size, i[1]:i[1] + size, i[2]:i[2] + size] = 1
    return occ


def scene_group(capi, make):
    _, spec, _ = make("chain6", 1, batch=1, fd_mode=0)
    rng = np.random.default_rng(2)
    out = {}
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST | capi.FLAG_NO_TENSORS) as ctx:
        members, frees = {}, []
        origin, cell = np.zeros(3), 0.02
        for n in (64, 128):
            occ = blocks(rng, n, 40, n // 8)
            ctx.set_obstacle_occupancy(occ, origin, cell)
            phi = ctx.obstacle_grid()[0]
            members[f"set_occupancy_{n}"] = lambda occ=occ: ctx.set_obstacle_occupancy(occ, origin, cell)
            members[f"set_grid_{n}"] = lambda phi=phi: ctx.set_obstacle_grid(phi, origin, cell)
            fn, free = bare_copy(n ** 3)
            members[f"copy_voxel_bytes_{n}"] = fn
            frees.append(free)
            out[f"occupied_share_{n}"] = round(float(occ.mean()), 4)
        out.update(alternate(members))
        for free in frees:
            free()
    for n in (64, 128):
        out[f"set_occupancy_{n}_upload_excluded_ms_derived"] = round(out[f"set_occupancy_{n}"]["median_ms"] - out[f"copy_voxel_bytes_{n}"]["median_ms"], 4)
    return out


def cost_group(capi, make):
    from problems import held_trajectory
    model, _, o = make("tree38", T, batch=1, fd_mode=0)
    seeds = 8                                        # distinct held trajectories, tiled over the batch
    trajs = [held_trajectory(o, model, seed=s, q0_sigma=0.3) for s in range(seeds)]
    xs = np.stack([trajs[b % seeds][2] for b in range(B)])
    us = np.stack([trajs[b % seeds][1] for b in range(B)])
    nj = len(model.parent)
    pts = [(int(round(k * (nj - 1) / (NP - 1))), (0.02, -0.03, 0.1), 0.05) for k in range(NP)]
    radius = np.array([p[2] for p in pts])
    P = np.array([[[o.frame_position(j, off, trajs[s][2].reshape(T + 1, o.nx)[t][:o.nq]) for j, off, _ in pts] for t in range(T + 1)]
                  for s in range(seeds)])                                            # (seeds, T+1, NP, 3)
    n, cell = 32, 0.05
    centre = P.reshape(-1, 3).mean(axis=0)
    origin = centre - cell * (n - 1) / 2.0
    occ = blocks(np.random.default_rng(3), n, 12, 5)
    _, spec, _ = make("tree38", T, batch=B, fd_mode=2, first_order_fd=1)
    out = {"T": T, "batch": B, "points": NP, "grid": [n, n, n], "cell": cell, "occupied_share": round(float(occ.mean()), 4)}
    mu1 = np.ones(B)
    with capi.Context(spec, flags=capi.FLAG_OBSTACLE_COST) as ctx:
        ctx.upload("X", xs); ctx.upload("U", us); ctx.upload("X_NEW", xs); ctx.upload("U_NEW", us)
        ctx.set_obstacle_occupancy(occ, origin, cell)
        phi = ctx.obstacle_grid_query(P.reshape(-1, 3), grad=False).reshape(seeds, T + 1, NP)
        dg = phi - radius                                                            # +inf outside the grid
        margin = float(np.quantile(dg[np.isfinite(dg)], SHARE * dg.size / np.isfinite(dg).sum()))
        ds = np.linalg.norm(P - centre, axis=-1) - radius
        rho = float(np.quantile(ds, SHARE))
        assert rho > 0.0, rho
        out["grid_slot"] = {"margin": margin, "active_share": round(float(np.mean(dg - margin < 0)), 4), "outside_share": round(float(np.mean(np.isinf(dg))), 4)}
        out["sphere_slot"] = {"rho": rho, "active_share": round(float(np.mean(ds - rho < 0)), 4)}
        w = np.ones(1)
        slots = {"grid": ((capi.OBSTACLE_GRID,), np.array([[0.0, 0.0, 0.0, margin]])),
                 "sphere": ((capi.OBSTACLE_SPHERE,), np.array([np.concatenate([centre, [rho]])]))}
        ctx.linearize()

        def use(kind):
            ctx.set_obstacle_points(points=pts, kinds=slots[kind][0])
            ctx.set_obstacle_cost(geom=slots[kind][1], weight=w)
        for kind in slots:
            use(kind)
            ctx.linearize(capi.LIN_COST)
            out[f"{kind}_slot"]["min_clearance"] = float(np.min(ctx.obstacle_clearance(0)))
        members = {}
        for kind in slots:                           # (set_points with another kind resets the block: set per member, outside the clock)
            members[f"lin_cost_{kind}"] = lambda kind=kind: ctx.linearize(capi.LIN_COST)
            members[f"cost_seq_aug_{kind}"] = lambda kind=kind: ctx.cost_seq_aug(0, mu1)
        got = {k: [] for k in members}
        for _ in range(ROUNDS):
            for kind in slots:
                use(kind)
                for k in (f"lin_cost_{kind}", f"cost_seq_aug_{kind}"):
                    got[k].append(timed(members[k]))
        out.update({k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                        "rounds_ms": [round(x, 4) for x in v]} for k, v in got.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacle_grid.json"))
    a = ap.parse_args()
    from ddp_pinocchio_amd import capi
    from problems import make
    assert capi.lib().ddp_hip_device_count() > 0, "the probe measures on an MI355X: there is no CPU fallback"
    res = {"rounds": ROUNDS, "warm": WARM, "reps": REPS, "clock": "wall clock around synchronous calls, ms",
           "scene": scene_group(capi, make), "cost": cost_group(capi, make)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
