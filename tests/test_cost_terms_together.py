"""Every per-instance cost term live at once: tracking, frame positions, frame orientations, state limits, centre of mass, frame
velocities and obstacles in one context.  The single-term modules check each term's arithmetic; this one checks what they share
-- the order of additions in linearise, cost_seq_aug and the forward's line search (three terms formed out of line, each summed
onto the candidates' cost differences), the rule by which a term's kernels are switched on and off, and the reset of a term's
data when its layout changes.

Batch 3, T = 4: 15 (instance, t) pairs, a multiple of neither 8, 16 nor 4, so com_cost_kernel, frame_vel_cost_kernel and
obstacle_cost_kernel each end on a partly filled workgroup.  chain6 has 8 lanes per CoM evaluation, tree38 64 (more than half a
wave), chain6ff a free-flyer root.  Instance 1 carries zero weights in the three out-of-line terms, instance 2 is frozen
(set_active) during the forward.

The feedback of the forward comes from the CPU oracle (its backward sweep on the plain problem, the feed-forward tripled so
that the halving runs), so the whole emulation runs without a GPU: test_emulation_decides_clearly asserts there, for every
case, that each candidate tried decides by more than 1e-9 of the sum of the cost terms' magnitudes (the device adds the terms
in another association).  The seeds were chosen for it."""
import functools

import numpy as np
import pytest

import test_com_cost as cm
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_frame_vel_cost as fv
import test_obstacle_cost as ob
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err

MODELS = ("chain6", "chain6ff", "tree38")
N_ALPHA = (1, 3, 8)
T, B, MU, K_SCALE = 4, 3, 1.0, 3.0
SEEDS = {"chain6": 11, "chain6ff": 11, "tree38": 11}
DERIVS = fc.DERIVS
OUTS = ("step", "dcost", "X_NEW", "U_NEW", "COSTS_OLD", "COSTS_NEW")


def flag_sets(capi):
    base = capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS
    inline = base | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_STATE_LIMITS
    return {"base": base, "inline": inline, "all": inline | capi.FLAG_COM_COST | capi.FLAG_FRAME_VEL_COST | capi.FLAG_OBSTACLE_COST}


@functools.lru_cache(maxsize=None)
def case(name):
    """everything a case needs that the CPU can compute, once per model"""
    seed = SEEDS[name]
    model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=0 if name.endswith("ff") else None)
    xs, us = tc._trajs(o, model, B, seed, held=True)
    xs2, us2 = tc._trajs(o, model, B, seed + 20)
    c = dict(name=name, model=model, spec=spec, o=o, xs=xs, us=us, xs2=xs2, us2=us2, mults=tc._mults(o, xs[0], seed + 1),
             frames=fc.pick_frames(model, 3), pts=ob.pick_points(model), kinds=ob.KINDS)
    c["ref"] = tc.random_ref(o, model, xs, us, B, seed + 2)
    c["fc"] = fc.random_task(o, xs, c["frames"], B, seed + 3)
    c["fo"] = fo.random_orient(o, xs, c["frames"], B, seed + 4)
    c["sl"] = sl.random_limits(o, xs, B, seed + 5)
    c["cm"] = cm.random_task(o, model, xs, B, seed + 6, wscale=20.0, spread=0.02)
    c["fv"] = fv.random_task(o, xs, c["frames"], B, seed + 7, wscale=5.0, spread=0.02)
    c["ob"] = ob.random_task(o, c["pts"], c["kinds"], xs, B, seed + 8)
    for k in ("cm", "fv", "ob"):
        c[k][1][1] = 0.0                                  # instance 1: no weight in the three out-of-line terms
    ob.check_task(o, c["pts"], c["kinds"], xs, c["ob"][0], c["ob"][1], fractions=False)
    # the forward's feedback and mu: the oracle's sweep on the plain problem, per instance; the feed-forward overshoots
    fbs, mus = [], []
    for b in range(B):
        r = o.backward(o.compute_derivatives(xs[b], us[b]), xs[b], c["mults"], 0.0, MU)
        assert r["restarts"] == 0
        r["fb"]["val"] = K_SCALE * r["fb"]["val"]
        fbs.append(r["fb"]); mus.append(r["mu"])
    c["fb"], c["mu"] = fbs, np.array(mus)
    return c


def inline_terms(c, b, X, U):
    """tracking + frame positions + frame orientations + limits of instance b's data along (X, U), per t"""
    o, fr = c["o"], c["frames"]
    return (tc.track_terms(o, 1.0, X, U, c["ref"], b) + fc.frame_terms(o, X, fr, c["fc"][0][b], c["fc"][1][b])
            + fo.orient_terms(o, X, fr, c["fo"][0][b], c["fo"][1][b]) + sl.limit_terms(o, X, *(s[b] for s in c["sl"])))


def addon_terms(c, b, X):
    """CoM + frame velocities + obstacles, per t"""
    o = c["o"]
    return (cm.com_terms(o, c["model"], X, c["cm"][0][b], c["cm"][1][b]) + fv.vel_terms(o, X, c["frames"], c["fv"][0][b], c["fv"][1][b])
            + ob.ob_terms(o, c["pts"], c["kinds"], X, c["ob"][0][b], c["ob"][1][b]))


@functools.lru_cache(maxsize=None)
def emulation(name, b, n_alpha):
    c = case(name)
    o = c["o"]

    def cost(X, U):
        return o.cost_seq_aug(X, U, c["mults"], c["mu"][b]) + inline_terms(c, b, X, U) + addon_terms(c, b, X)
    em = ob._emulate_forward(o, c["xs"][b], c["us"][b], c["mults"], c["fb"][b], c["mu"][b], n_alpha, cost)
    assert em is not None
    return em


def upload_tasks(ctx, c, which):
    """the tasks of the flag set `which` ("base" / "inline" / "all")"""
    tc.upload_ref(ctx, c["ref"])
    if which == "base":
        return
    ctx.set_frame_cost(frames=c["frames"], target=c["fc"][0], weight=c["fc"][1])
    ctx.set_frame_orient_cost(quat=c["fo"][0], weight=c["fo"][1])
    ctx.set_state_limits(lo=c["sl"][0], hi=c["sl"][1], weight=c["sl"][2])
    if which == "all":
        ctx.set_com_cost(target=c["cm"][0], weight=c["cm"][1])
        ctx.set_frame_vel_cost(target=c["fv"][0], weight=c["fv"][1])
        ob.set_task(ctx, c["pts"], c["kinds"], c["ob"][0], c["ob"][1])


def setup(ctx, c):
    o = c["o"]
    tc._setup(ctx, c["xs"], c["us"], c["mults"], o.Etot)
    for k, s in (("origin", "FB_ORIGIN"), ("val", "FB_VAL"), ("jac", "FB_JAC")):
        ctx.upload(s, np.stack([c["fb"][b][k][:ctx.seq_size(s)] for b in range(B)]))


def costs_and_forward(ctx, c, n_alpha):
    """both cost sequences (X_NEW: the second trajectory), then one forward with instance 2 frozen"""
    out = {}
    ctx.upload("X_NEW", c["xs2"]); ctx.upload("U_NEW", c["us2"])
    ctx.cost_seq_aug(0, c["mu"]); ctx.cost_seq_aug(1, c["mu"])
    out["COSTS_OLD"], out["COSTS_NEW"] = ctx.download("COSTS_OLD"), ctx.download("COSTS_NEW")
    ctx.upload("X_NEW", c["xs"]); ctx.upload("U_NEW", c["us"])   # (a rollout starts from X_NEW's first state, as the reference's does)
    ctx.set_active([1, 1, 0])
    _, step, dcost = ctx.forward(c["mu"], n_alpha=n_alpha)
    out["step"], out["dcost"] = step[:2], dcost[:2]              # (the forward writes no step for a frozen instance)
    ctx.set_active(None)
    out["X_NEW"], out["U_NEW"] = ctx.download("X_NEW"), ctx.download("U_NEW")
    return out


def run(capi, c, which, n_alpha, stages=None, before=None):
    """one context of the flag set `which`: linearise, both cost sequences, one forward.  before(ctx): further uploads"""
    with capi.Context(c["spec"], flags=flag_sets(capi)[which]) as ctx:
        setup(ctx, c)
        upload_tasks(ctx, c, which)
        if before:
            before(ctx)
        ctx.linearize(None if stages is None else capi.LIN_COST)
        out = {s: ctx.download(s) for s in DERIVS}
        out.update(costs_and_forward(ctx, c, n_alpha))
        return out


# ---- CPU: the condition on the inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_emulation_decides_clearly(name):
    """on the emulation alone: every candidate tried, of every searched instance and every n_alpha, decides by more than 1e-9 of
    the sum of the cost terms' magnitudes; the out-of-line terms are material where they carry weight, and the halving runs"""
    c = case(name)
    halved = False
    for b in (0, 1):
        add = addon_terms(c, b, c["xs"][b])
        assert np.all(add == 0.0) if b == 1 else np.all(add > 0.0)
        for na in N_ALPHA:
            step, _, _, diff, margins = emulation(name, b, na)
            print("emulation", name, b, na, "step", step, "diff", diff, "margins", margins)
            assert min(margins) > 1e-9, (b, na, margins)
            halved |= step < 1.0
    assert halved


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stages", [None, 1])
@pytest.mark.parametrize("name", MODELS)
def test_linearize_adds_every_term(gpu, name, stages):
    """LX, LXX, LFX, LFXX equal the tracking-only context's values plus the six terms' derivatives to 1e-12; LXX / LFXX symmetric
    bit for bit; LU, LUU, LUX bit for bit the tracking-only values.  Through linearize() and linearize_stages(LIN_COST)"""
    c = case(name)
    o, n = c["o"], c["o"].n
    got = {w: run(gpu, c, w, 1, stages) for w in ("base", "all")}
    for b in range(B):
        X, fr = c["xs"][b], c["frames"]
        adds = (fc.frame_derivs(o, X, fr, c["fc"][0][b], c["fc"][1][b]), fo.orient_derivs(o, X, fr, c["fo"][0][b], c["fo"][1][b]),
                sl.limit_derivs(o, X, *(s[b] for s in c["sl"])), cm.com_derivs(o, c["model"], X, c["cm"][0][b], c["cm"][1][b]),
                fv.vel_derivs(o, c["model"], X, fr, c["fv"][0][b], c["fv"][1][b]),
                ob.ob_derivs(o, c["model"], c["pts"], c["kinds"], X, c["ob"][0][b], c["ob"][1][b]))
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got["base"][s][b] + sum(a[s] for a in adds)
            e = rel_err(got["all"][s][b], ex)
            print("linearize", name, stages, s, b, e)
            assert e <= 1e-12, (s, b, e)
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got["all"][s][b], got["base"][s][b]), s
        for blk in list(got["all"]["LXX"][b].reshape(T, n, n)) + [got["all"]["LFXX"][b].reshape(n, n)]:
            assert np.array_equal(blk, blk.T)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_cost_seq_aug_adds_every_term(gpu, name):
    """COSTS_OLD / COSTS_NEW equal the tracking-only context's values plus the numpy terms of all six, to 1e-12"""
    c = case(name)
    got = {w: run(gpu, c, w, 1) for w in ("base", "all")}
    for key, Xs, Us in (("COSTS_OLD", c["xs"], c["us"]), ("COSTS_NEW", c["xs2"], c["us2"])):
        for b in range(B):
            add = inline_terms(c, b, Xs[b], Us[b]) - tc.track_terms(c["o"], 1.0, Xs[b], Us[b], c["ref"], b) + addon_terms(c, b, Xs[b])
            e = rel_err(got["all"][key][b], got["base"][key][b] + add)
            print("cost_seq_aug", name, key, b, e)
            assert np.any(add != 0.0) and e <= 1e-12, (key, b, e)


@pytest.mark.gpu
@pytest.mark.parametrize("n_alpha", N_ALPHA)
@pytest.mark.parametrize("name", MODELS)
def test_forward_matches_emulation(gpu, name, n_alpha):
    """step, X_NEW, U_NEW and dcost of the searched instances against the emulation (test_obstacle_cost's tolerances), after the
    guard on the emulation alone.  Instance 1 (zero weights in the out-of-line terms) and instance 2 (frozen) bit for bit as in
    a context created without the three flags (instance 2: X_NEW and U_NEW, which stay the uploaded trajectory)"""
    c = case(name)
    ems = {b: emulation(name, b, n_alpha) for b in (0, 1)}
    for b, em in ems.items():
        assert min(em[4]) > 1e-9, (b, em[4])               # before anything from the device is compared
    got = {w: run(gpu, c, w, n_alpha) for w in ("inline", "all")}
    for b, (step_ref, xn_ref, un_ref, new, margins) in ems.items():
        a = got["all"]
        print("forward", name, n_alpha, b, "step", a["step"][b], step_ref, "dcost", a["dcost"][b], new, "margins", margins)
        assert a["step"][b] == step_ref, (b, a["step"][b], step_ref)
        assert rel_err(a["X_NEW"][b], xn_ref) < 1e-9 and rel_err(a["U_NEW"][b], un_ref) < 1e-9
        assert abs(a["dcost"][b] - new) <= 1e-9 * max(1.0, abs(new)), (a["dcost"][b], new)
    assert not np.array_equal(got["all"]["COSTS_OLD"][0], got["inline"]["COSTS_OLD"][0])
    for k in OUTS:
        assert np.array_equal(got["all"][k][1], got["inline"][k][1], equal_nan=True), k
    # the forward writes nothing for a frozen instance: its trajectory stays (its step / dcost slots keep what the buffers held,
    # and its cost rows carry its own terms: neither is an output of this forward)
    for k in ("X_NEW", "U_NEW"):
        assert np.array_equal(got["all"][k][2], got["inline"][k][2]) and np.array_equal(got["all"][k][2], c[k[0].lower() + "s"][2]), k


@pytest.mark.gpu
def test_upload_rules(gpu):
    """zeros uploaded in two half-batch ranges leave the kernels launched and the outputs bit-equal to a context without the three
    flags; one whole-batch zero upload followed by the weights restores the earlier outputs bit for bit; another frame count
    brings the three frame terms' data back to their defaults, other slot kinds the obstacle data"""
    capi = gpu
    c = case("chain6ff")
    keys = DERIVS + OUTS
    first = run(capi, c, "all", 3)
    inline = run(capi, c, "inline", 3)

    def halves(ctx):
        for first, count in ((0, 1), (1, B - 1)):
            ctx.set_com_cost(weight=0.0, first=first, count=count)
            ctx.set_frame_vel_cost(weight=0.0, first=first, count=count)
            ctx.set_obstacle_cost(weight=np.zeros(len(c["kinds"])), first=first, count=count)
    zeroed = run(capi, c, "all", 3, before=halves)
    for k in keys:
        assert np.array_equal(zeroed[k], inline[k], equal_nan=True), k

    def off_and_on(ctx):
        ctx.set_com_cost(weight=0.0); ctx.set_frame_vel_cost(weight=0.0); ctx.set_obstacle_cost(weight=np.zeros(len(c["kinds"])))
        ctx.set_com_cost(weight=c["cm"][1]); ctx.set_frame_vel_cost(weight=c["fv"][1]); ctx.set_obstacle_cost(weight=c["ob"][1])
    again = run(capi, c, "all", 3, before=off_and_on)
    assert not np.array_equal(first["LX"], inline["LX"])
    for k in keys:
        assert np.array_equal(again[k], first[k], equal_nan=True), k

    with capi.Context(c["spec"], flags=flag_sets(capi)["all"]) as ctx:
        setup(ctx, c)
        upload_tasks(ctx, c, "all")
        assert np.array_equal(ctx.frame_vel_cost()[1], c["fv"][1]) and np.array_equal(ctx.obstacle_cost()[0], c["ob"][0])
        ctx.set_frame_cost(frames=c["frames"][:2])
        for t, w in (ctx.frame_cost(), ctx.frame_vel_cost()):
            assert t.shape[2] == 2 and not t.any() and not w.any()
        q, w = ctx.frame_orient_cost()
        assert np.array_equal(q, fo.identity_quat((B, T + 1, 2))) and not w.any()
        ctx.set_obstacle_points(points=c["pts"], kinds=(c["kinds"][1], c["kinds"][0]) + tuple(c["kinds"][2:]))   # the same count
        g, w = ctx.obstacle_cost()
        assert not g.any() and not w.any()
        # ... and the four terms that were reset are off: what is left is tracking, limits and the CoM
        ctx.linearize()
        rest = {s: ctx.download(s) for s in DERIVS}
    with capi.Context(c["spec"], flags=flag_sets(capi)["base"] | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST) as ctx:
        setup(ctx, c)
        tc.upload_ref(ctx, c["ref"])
        ctx.set_state_limits(lo=c["sl"][0], hi=c["sl"][1], weight=c["sl"][2])
        ctx.set_com_cost(target=c["cm"][0], weight=c["cm"][1])
        ctx.linearize()
        for s in DERIVS:
            assert np.array_equal(ctx.download(s), rest[s]), s
