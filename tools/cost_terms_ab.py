"""Bit-identity of the per-instance cost terms between two builds of the library (a refactor's acceptance test).

    DDP_HIP_LIB=<lib.so> python tools/cost_terms_ab.py --dump DIR     one process: every case below under that library -> DIR/cost_terms.npz
    python tools/cost_terms_ab.py --compare A.npz B.npz               every entry np.array_equal(..., equal_nan=True), else exit 1

The cases are those of tests/test_cost_terms_together.py (three models, batch 3, T = 4, n_alpha 1 / 3 / 8, all seven cost flags
live; the zero-weight uploads of its upload rules), each term alone, a list of refused calls with their return codes, the model
entry points com and frame_velocity with their jacobians, and each term alone on the prismatic tree table7.  What
is written: every derivative sequence linearise leaves, COSTS_OLD / COSTS_NEW, step, dcost, X_NEW, U_NEW, the clearances, what
the getters hand back, and the return codes."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def model_entry_points(capi, model, o, frames):
    """com and frame_velocity with their jacobians at two states: the staging and column lanes of the CoM and frame-velocity
    kernels on their own (ddp_hip_model_com, ddp_hip_model_frame_velocity)"""
    out = {}
    rng = np.random.default_rng(5)
    with capi.ModelHandle(model) as h:
        for k in range(2):
            q, v = rng.normal(size=o.nq), rng.normal(size=o.nv)
            if o.nq != o.nv:
                q[3:7] /= np.linalg.norm(q[3:7])
            out[f"com_c{k}"], out[f"com_J{k}"] = h.com(q, jacobian=True)
            for f, (j, off) in enumerate(frames):
                for key, val in zip(("vel", "Jq", "Jv"), h.frame_velocity(j, off, q, v, jacobian=True)):
                    out[f"fv{k}_{f}_{key}"] = val
    return out


def table7(capi, tt, put):
    """each term alone on the tree of tests/test_com_cost.py: joint 1 is prismatic and no leaf, joint 4 a prismatic leaf, so
    the prismatic step sits in the middle of a walk (of the models above only tree38's root is prismatic).  Batch 3, T = 4:
    linearise, both cost sequences, the clearances"""
    B, T = 3, 4
    cm, fc, fo, fv, ob, tc = tt.cm, tt.fc, tt.fo, tt.fv, tt.ob, tt.tc
    model, spec, o = cm.make_any("table7", T, batch=B, fd_mode=2)
    xs, us = tc._trajs(o, model, B, 61)
    xs2, us2 = tc._trajs(o, model, B, 62)
    mults, mu = tc._mults(o, xs[0], 63), np.ones(B)
    frames, pts, kinds = fc.pick_frames(model, 3), ob.pick_points(model), ob.KINDS
    t_fc, t_fo = fc.random_task(o, xs, frames, B, 64), fo.random_orient(o, xs, frames, B, 65)
    t_cm, t_fv = cm.random_task(o, model, xs, B, 66), fv.random_task(o, xs, frames, B, 67)
    t_ob = ob.random_task(o, pts, kinds, xs, B, 68)
    alone = {"frame": (capi.FLAG_FRAME_COST, lambda x: x.set_frame_cost(frames=frames, target=t_fc[0], weight=t_fc[1])),
             "orient": (capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST,
                        lambda x: (x.set_frame_cost(frames=frames), x.set_frame_orient_cost(quat=t_fo[0], weight=t_fo[1]))),
             "com": (capi.FLAG_COM_COST, lambda x: x.set_com_cost(target=t_cm[0], weight=t_cm[1])),
             "vel": (capi.FLAG_FRAME_COST | capi.FLAG_FRAME_VEL_COST,
                     lambda x: (x.set_frame_cost(frames=frames), x.set_frame_vel_cost(target=t_fv[0], weight=t_fv[1]))),
             "obstacle": (capi.FLAG_OBSTACLE_COST, lambda x: ob.set_task(x, pts, kinds, t_ob[0], t_ob[1]))}
    for term, (flags, upload) in alone.items():
        with capi.Context(spec, flags=flags | capi.FLAG_NO_TENSORS) as ctx:
            tc._setup(ctx, xs, us, mults, o.Etot)
            upload(ctx)
            ctx.linearize()
            put(f"table7/alone/{term}", {s: ctx.download(s) for s in tt.DERIVS})
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            ctx.cost_seq_aug(0, mu); ctx.cost_seq_aug(1, mu)
            put(f"table7/alone/{term}", {s: ctx.download(s) for s in ("COSTS_OLD", "COSTS_NEW")})
            if term == "obstacle":
                put(f"table7/alone/{term}", {"clear0": ctx.obstacle_clearance(0), "clear1": ctx.obstacle_clearance(1)})
    put("table7/model", model_entry_points(capi, model, o, frames))


def dump(path):
    import test_cost_terms_together as tt
    from ddp_pinocchio_amd import capi
    out = {}

    def put(prefix, d):
        for k, v in d.items():
            out[f"{prefix}/{k}"] = np.asarray(v)

    def code(fn):
        try:
            fn()
            return capi.OK
        except capi.DdpHipError as e:
            return e.code

    for name in tt.MODELS:
        c = tt.case(name)
        B, T, o = tt.B, tt.T, c["o"]
        # all terms together, per n_alpha and flag set; the upload rules
        for na in tt.N_ALPHA:
            for which in ("base", "inline", "all"):
                put(f"{name}/{which}/na{na}", tt.run(capi, c, which, na))
        put(f"{name}/all/stages", tt.run(capi, c, "all", 3, stages=1))
        nz = np.zeros(len(c["kinds"]))

        def halves(ctx):
            for first, count in ((0, 1), (1, B - 1)):
                ctx.set_com_cost(weight=0.0, first=first, count=count)
                ctx.set_frame_vel_cost(weight=0.0, first=first, count=count)
                ctx.set_obstacle_cost(weight=nz, first=first, count=count)

        def off_and_on(ctx):
            ctx.set_com_cost(weight=0.0); ctx.set_frame_vel_cost(weight=0.0); ctx.set_obstacle_cost(weight=nz)
            ctx.set_com_cost(weight=c["cm"][1]); ctx.set_frame_vel_cost(weight=c["fv"][1]); ctx.set_obstacle_cost(weight=c["ob"][1])
        put(f"{name}/all/halves", tt.run(capi, c, "all", 3, before=halves))
        put(f"{name}/all/off_and_on", tt.run(capi, c, "all", 3, before=off_and_on))

        # each term alone
        alone = {"frame": (capi.FLAG_FRAME_COST, lambda x: x.set_frame_cost(frames=c["frames"], target=c["fc"][0], weight=c["fc"][1])),
                 "orient": (capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST,
                            lambda x: (x.set_frame_cost(frames=c["frames"]), x.set_frame_orient_cost(quat=c["fo"][0], weight=c["fo"][1]))),
                 "limits": (capi.FLAG_STATE_LIMITS, lambda x: x.set_state_limits(lo=c["sl"][0], hi=c["sl"][1], weight=c["sl"][2])),
                 "com": (capi.FLAG_COM_COST, lambda x: x.set_com_cost(target=c["cm"][0], weight=c["cm"][1])),
                 "vel": (capi.FLAG_FRAME_COST | capi.FLAG_FRAME_VEL_COST,
                         lambda x: (x.set_frame_cost(frames=c["frames"]), x.set_frame_vel_cost(target=c["fv"][0], weight=c["fv"][1]))),
                 "obstacle": (capi.FLAG_OBSTACLE_COST, lambda x: tt.ob.set_task(x, c["pts"], c["kinds"], c["ob"][0], c["ob"][1]))}
        for term, (flags, upload) in alone.items():
            with capi.Context(c["spec"], flags=flags | capi.FLAG_NO_TENSORS) as ctx:
                tt.setup(ctx, c)
                upload(ctx)
                ctx.linearize()
                put(f"{name}/alone/{term}", {s: ctx.download(s) for s in tt.DERIVS})
                put(f"{name}/alone/{term}", tt.costs_and_forward(ctx, c, 3))
                if term == "obstacle":
                    put(f"{name}/alone/{term}", {"clear0": ctx.obstacle_clearance(0), "clear1": ctx.obstacle_clearance(1)})

        # getters, layout changes and refused calls on one context with everything on
        with capi.Context(c["spec"], flags=tt.flag_sets(capi)["all"]) as ctx:
            rc = []
            tt.setup(ctx, c)
            rc.append(code(lambda: ctx.set_frame_orient_cost(weight=1.0)))          # no frames yet
            rc.append(code(lambda: ctx.set_frame_vel_cost(weight=1.0)))
            rc.append(code(lambda: ctx.obstacle_clearance(0)))                       # no points yet
            ctx.n_obstacles = len(c["kinds"])
            rc.append(code(lambda: ctx.set_obstacle_cost(weight=nz)))                # no slots yet (the wrapper believes there are)
            ctx.n_obstacles = 0
            tt.upload_tasks(ctx, c, "all")
            put(f"{name}/get", dict(zip(("fc_t", "fc_w"), ctx.frame_cost())))
            put(f"{name}/get", dict(zip(("fo_q", "fo_w"), ctx.frame_orient_cost(first=1, count=2))))
            put(f"{name}/get", dict(zip(("sl_lo", "sl_hi", "sl_w"), ctx.state_limits())))
            put(f"{name}/get", dict(zip(("cm_t", "cm_w"), ctx.com_cost(first=2))))
            put(f"{name}/get", dict(zip(("fv_t", "fv_w"), ctx.frame_vel_cost())))
            put(f"{name}/get", dict(zip(("ob_g", "ob_w"), ctx.obstacle_cost())))
            put(f"{name}/get", {"clear0": ctx.obstacle_clearance(0), "clear1": ctx.obstacle_clearance(1)})
            n, F, no = o.n, len(c["frames"]), len(c["kinds"])
            bad_q = c["fo"][0].copy(); bad_q[B - 1, T, F - 1, 3] += 1e-8
            bad_g = c["ob"][0].copy(); bad_g[B - 1, T, 0, 3] = -1.0               # slot 0 is a sphere
            bad_n = c["ob"][0].copy(); bad_n[0, 0, 1, :3] *= 1.0 + 1e-8            # slot 1 a half-space
            pose_w = np.zeros(n); pose_w[0] = 1.0
            for fn in (lambda: ctx.set_com_cost(weight=1.0, first=1, count=B),     # one beyond the batch
                       lambda: ctx.set_com_cost(weight=1.0, first=-1, count=1),
                       lambda: ctx.set_com_cost(weight=1.0, first=B, count=0),     # nothing to do
                       lambda: ctx.set_com_cost(weight=-1.0),
                       lambda: ctx.set_com_cost(target=np.full((T + 1, 3), np.nan)),
                       lambda: ctx.set_frame_cost(weight=np.inf),
                       lambda: ctx.set_frame_vel_cost(target=np.full((T + 1, F, 6), np.inf)),
                       lambda: capi._check(capi.lib().ddp_hip_frame_orient_upload(ctx._h, capi._ptr(bad_q), None, 0, B), "orient"),
                       lambda: ctx.set_obstacle_cost(geom=bad_g),
                       lambda: ctx.set_obstacle_cost(geom=bad_n),
                       lambda: ctx.set_obstacle_cost(weight=np.full(no, -1.0)),
                       lambda: ctx.set_state_limits(lo=np.inf),
                       lambda: ctx.set_state_limits(hi=-np.inf),
                       lambda: ctx.set_state_limits(lo=1e9),                       # above the resident hi somewhere
                       lambda: ctx.set_state_limits(hi=-1e9),
                       lambda: ctx.set_state_limits(weight=pose_w),                # refused on a free-flyer root only
                       lambda: ctx.set_state_limits(weight=np.nan),
                       lambda: ctx.frame_cost(first=1, count=B),
                       lambda: ctx.state_limits(first=0, count=-1),
                       lambda: ctx.obstacle_clearance(2)):
                rc.append(code(fn))
            # nothing of the refused uploads was written
            put(f"{name}/after_refusals", dict(zip(("sl_lo", "sl_hi", "sl_w"), ctx.state_limits())))
            put(f"{name}/after_refusals", dict(zip(("ob_g", "ob_w"), ctx.obstacle_cost())))
            put(f"{name}/after_refusals", dict(zip(("fo_q", "fo_w"), ctx.frame_orient_cost())))
            ctx.set_frame_cost(frames=c["frames"][:2])
            ctx.set_obstacle_points(points=c["pts"], kinds=(c["kinds"][1], c["kinds"][0]) + tuple(c["kinds"][2:]))
            put(f"{name}/reset", dict(zip(("fc_t", "fc_w"), ctx.frame_cost())))
            put(f"{name}/reset", dict(zip(("fo_q", "fo_w"), ctx.frame_orient_cost())))
            put(f"{name}/reset", dict(zip(("fv_t", "fv_w"), ctx.frame_vel_cost())))
            put(f"{name}/reset", dict(zip(("ob_g", "ob_w"), ctx.obstacle_cost())))
            ctx.linearize()
            put(f"{name}/reset", {s: ctx.download(s) for s in tt.DERIVS})
            put(f"{name}/reset", tt.costs_and_forward(ctx, c, 3))
        with capi.Context(c["spec"], flags=capi.FLAG_NO_TENSORS) as ctx:           # no flag: every entry point refuses
            for fn in (lambda: ctx.set_frame_cost(frames=c["frames"]), lambda: ctx.set_frame_cost(weight=1.0), lambda: ctx.frame_cost(),
                       lambda: ctx.set_frame_orient_cost(weight=1.0), lambda: ctx.frame_orient_cost(),
                       lambda: ctx.set_frame_vel_cost(weight=1.0), lambda: ctx.frame_vel_cost(),
                       lambda: ctx.set_com_cost(weight=1.0, first=-1, count=1), lambda: ctx.com_cost(),
                       lambda: ctx.set_state_limits(weight=1.0), lambda: ctx.state_limits(),
                       lambda: ctx.set_obstacle_points(points=c["pts"], kinds=c["kinds"]), lambda: ctx.obstacle_cost(),
                       lambda: ctx.obstacle_clearance(0)):
                rc.append(code(fn))
        L = capi.lib()
        for fn in (L.ddp_hip_frame_cost_upload, L.ddp_hip_frame_orient_upload, L.ddp_hip_frame_vel_upload, L.ddp_hip_com_cost_upload,
                   L.ddp_hip_obstacle_upload, L.ddp_hip_frame_cost_download, L.ddp_hip_com_cost_download):
            rc.append(fn(None, None, None, 0, 0))                                    # a null context
        rc.append(L.ddp_hip_state_limits_upload(None, None, None, None, 0, 0))
        out[f"{name}/return_codes"] = np.array(rc, dtype=np.int64)
        put(f"{name}/model", model_entry_points(capi, c["model"], c["o"], c["frames"]))
    table7(capi, tt, put)
    os.makedirs(path, exist_ok=True)
    np.savez(os.path.join(path, "cost_terms.npz"), **out)
    print(f"cost_terms_ab: {len(out)} entries under {os.path.basename(capi.LIB_PATH)} -> {os.path.join(path, 'cost_terms.npz')}")


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    differ = sorted(set(A.files) ^ set(Bz.files))
    for k in sorted(set(A.files) & set(Bz.files)):
        if not np.array_equal(A[k], Bz[k], equal_nan=True):
            differ.append(k)
    print(f"cost_terms_ab: {len(A.files)} entries, {len(differ)} differ" + ("" if not differ else ": " + ", ".join(differ[:20])))
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
    elif a.compare:
        sys.exit(compare(*a.compare))
    else:
        ap.error("--dump DIR or --compare A B")


if __name__ == "__main__":
    main()
