"""The fourteen add-on cost terms on robots of other sizes and trees (tests/robots.py).  The terms' own modules run on five built-in
robots (6, 7, 7, 38, 39 joints: 8 or 64 lanes per evaluation, three tree shapes); the kernels take their shape at run time, and
this module runs every term where that shape is another one:

  sizes   pair2 (six of a group's eight lanes own no joint), fork5, tree13 (16 lanes per evaluation), tree21 (32 lanes, prismatic
          joints mid-tree), tree40 and tree64 (path and column masks with bits 39 .. 63 set, momentum_cost.h's nv >= 64 branch,
          lin_control_grav_cost_kernel's nv^2 doubles of LDS).  Batch 3 and T = horizon(name): 15 (instance, t) evaluations up to
          21 joints, which leaves the last wave partly filled at 4 and at 2 evaluations per wave
  shapes  deep38 (17 levels) and fan38 = [-1] + [0] * 37, built here with robots.seeded_tree: a root with 37 children, one level
          of 37 joints -- wider than the 32 lanes rbd::accel_group walks a level with, so its `idx += nh` loop runs a second round;
          the library accepts it (one open slot, a level of 37 <= 64), so no narrower replacement is needed.  The joint accelerations
          also on wide38x and quad38; the four inline terms also on wide38, the latency forward kernel (fwd_path == 1), whose
          pipelined form is bit for bit the DDP_HIP_FWD_NO_PIPE form

The joint accelerations stop at 38 joints (DDP_HIP_MAX_JOINT_ACCEL_NV): on tree40 creation is refused, and accepted without the flag.

Nothing of a reference is restated here: the numpy definitions of the terms' own modules (*_terms, *_derivs, random_task,
check_task, set_task, the pickers, _emulate_forward) are the yardstick, on the C oracle's kinematics of the same TableModel, at
those modules' tolerances: 1e-12 for the derivatives and the cost sequences, 1e-10 for what passes through M^-1 (the joint
accelerations' derivatives; their cost values per t within 1e-12 of the bound test_joint_accel_cost.test_cost_values states), 1e-9
for the forward.  The only picker without a valid answer is rf.pick_pairs, on pair2 (its second pair would be (1, 1)) and on fork5
(it wants three leaves, fork5 has two): HAND_JOINTS names their pairs' joints by hand.

States: the controls of test_other_robots.trajectories, rolled out by the oracle from a random state (problems.random_state, scale
0.5) -- its own rollouts start at q = v = 0, where sin and cos of a wrong joint's angle would be those of the right one.  The
forward's feedback is the oracle's sweep on its own plain derivatives plus the modules' *_derivs (a descent direction of the summed
cost), the feed-forward scaled by K_SCALE per instance, so the whole emulation runs without a GPU and the conditions on the inputs
are asserted there (test_inputs_*): every addition non-zero, the one-sided terms with violated and clear entries, a result for
every instance, every candidate deciding by more than 1e-9 of the summed magnitudes, the halving running (the instances accept 1,
1/2 and 1/16).  Instance 1 carries zero weights in the term, (instance 2, t = 1) carries zero weights inside a live instance.  SEEDS
holds the task seeds that differ from the default; they were chosen on the oracle alone, for those conditions.

All fourteen at once on tree21 (test_all_terms_at_once): what test_cost_terms_together.py does for seven terms on the built-ins,
with the sum of all modules' references, n_alpha 3 and 8, and instance 1 without a weight in the ten terms formed out of line.

No reference needed another tolerance at 64 joints.  Measured on an MI355X: the derivative sequences within 6.3e-13 of their largest
entry (LX / LFX of the momentum term, which grow with the joint count: 1.8e-13 at 21 joints, 3.2e-13 at 40, 6.3e-13 at 64; every
other term on every robot under 1e-13; 1e-12 allowed), the joint accelerations' cost
values at a fifth of their bound, the reporting calls and ModelHandle evaluations within 4e-15; no case takes 3 s, its CPU reference
included."""
import functools

import numpy as np
import pytest

import robots
import test_balance_region_cost as br
import test_com_cost as cm
import test_control_grav_cost as cg
import test_frame_aim_cost as fa
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_frame_vel_cost as fv
import test_joint_accel_cost as ja
import test_momentum_cost as mo
import test_obstacle_cost as ob
import test_relative_frame_cost as rf
import test_self_collision_cost as sc
import test_state_limits as sl
import test_tracking_cost as tc
from problems import random_state
from synth import rel_err
from test_dynamics_parity import DERIV_SEQS
from test_other_robots import B, K_SCALE, assert_info, horizon, trajectories

MU, TOL, TOL_FWD = 1.0, 1e-12, 1e-9
FAN38 = [-1] + [0] * 37
LOCAL = {"fan38": (FAN38, 242)}
SIZES = ("pair2", "fork5", "tree13", "tree21", "tree40", "tree64")
SHAPES = ("deep38", "fan38")
INLINE = ("tracking", "frame", "orient", "limits")
COST_SEQS = ("LX", "LXX", "LU", "LUU", "LUX", "LFX", "LFXX")
ALL_SEQS = tuple(s for s in DERIV_SEQS.values() if not s.startswith("EQ_"))
X_SEQS, U_SEQS = ("LX", "LXX", "LFX", "LFXX"), ("LX", "LXX", "LU", "LUU", "LUX")
OUTS = ("step", "dcost", "X_NEW", "U_NEW", "COSTS_OLD", "COSTS_NEW")
REPORT_ON = ("tree21", "tree64")
ZERO_INSTANCE, ZERO_ROW = 1, (2, 1)
SEED0 = 11
# (term, robot, together): the sphere terms draw a clear block with probability 1/4; these seeds give the terminal block of both
# live instances an active pair (LFX / LFXX non-zero) and leave some block clear
SEEDS = {("obstacle", "fork5", False): 1001, ("obstacle", "tree13", False): 1001, ("obstacle", "deep38", False): 1000,
         ("obstacle", "fan38", False): 1002, ("selfcol", "pair2", False): 1000, ("selfcol", "fork5", False): 1009,
         ("selfcol", "tree13", False): 1009, ("selfcol", "tree21", False): 1009, ("selfcol", "tree40", False): 1003,
         ("selfcol", "tree64", False): 1003, ("selfcol", "deep38", False): 1000, ("selfcol", "fan38", False): 1001}
HAND_JOINTS = {"pair2": [(0, 1), (1, 0), (0, 1)],      # the two joints in both roles
               "fork5": [(2, 4), (0, 2), (1, 3)]}      # across the two branches, the root -> a leaf, across the branches' first joints


def hand_pairs(name):
    """the frame pairs of a robot rf.pick_pairs has no answer for, in its layout: three pairs with rf.OFFS, and the first swapped"""
    pairs = [((a, rf.OFFS[k][0]), (b, rf.OFFS[k][1])) for k, (a, b) in enumerate(HAND_JOINTS[name])]
    return pairs + [(pairs[0][1], pairs[0][0])]


# ---- robots and trajectories -------------------------------------------------------------------------------------------------
def nv_of(name):
    return len(LOCAL[name][0] if name in LOCAL else robots.CATALOGUE[name].parents)


def T_of(name):
    return 3 if name in LOCAL else horizon(name)


def check_info(ctx, name):
    """assert_info, and for the robot built here what it stands for: the run-time-tree linearisation, the one-lane forward kernel
    (a level of 37 is past the latency kernel's 8), the Talos-shaped sweep at nv = 38"""
    if name not in LOCAL:
        return assert_info(ctx, name)
    info = ctx.info()
    for k, v in {"lin_path": 1, "first_order": 1, "fwd_path": 0, "bwd_path": 1}.items():
        assert info[k] == v, (name, k, info)


@functools.lru_cache(maxsize=None)
def case(name):
    """everything of a robot that no term owns: the problem, two batches of trajectories (the second one's instances in another
    order), the frames, points and pairs the pickers choose"""
    from ddp_pinocchio_amd import capi
    from oracle.binding import Oracle
    T = T_of(name)
    if name in LOCAL:
        model = robots.seeded_tree(*LOCAL[name])
        kw = dict(dt=0.01, c=1.0, fd_mode=0, first_order_fd=1, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
        spec, o = capi.ProblemSpec(model, T, batch=B, **kw), Oracle(model, T, **kw)
        rng = np.random.default_rng(10)
        controls = [[s * rng.normal(size=T * model.nv) for _ in range(B)] for s in (0.3, 0.5)]
    else:
        model, spec, o, tr = trajectories(name, T, 0, 1, None, 0.3)
        controls = [[us for _, us in tr], [us for _, us in trajectories(name, T, 0, 1, None, 0.5)[3]]]
    rng = np.random.default_rng(900 + model.nv)
    sets = []
    for k, us_k in enumerate(controls):
        us_k = us_k[k:] + us_k[:k]
        sets.append((np.stack([o.rollout(random_state(model, rng, 0.5), u) for u in us_k]), np.stack(us_k)))
    pts = ob.pick_points(model)
    return dict(name=name, T=T, model=model, spec=spec, o=o, xs=sets[0][0], us=sets[0][1], xs2=sets[1][0], us2=sets[1][1],
                mults=o.alloc_affine(0), frames=fc.pick_frames(model, 3), pts=pts, scpairs=sc.all_pairs(pts),
                rfpairs=hand_pairs(name) if name in HAND_JOINTS else rf.pick_pairs(model), aim=fa.pick_aim_frames(model))


@functools.lru_cache(maxsize=None)
def plain(name):
    """per instance: the oracle's plain-cost derivatives (raw: as the oracle holds them) and both plain cost sequences"""
    c = case(name)
    o, out = c["o"], []
    for b in range(B):
        d = o.compute_derivatives(c["xs"][b], c["us"][b])
        out.append(dict(raw=d, d={s: d[k] for k, s in DERIV_SEQS.items() if s in ALL_SEQS},
                        costs=(o.cost_seq_aug(c["xs"][b], c["us"][b], c["mults"], MU), o.cost_seq_aug(c["xs2"][b], c["us2"][b], c["mults"], MU))))
    return out


def feedback(c, raw, adds, b):
    """the oracle's sweep on its own derivatives plus the terms' additions (a descent direction of the summed cost), the
    feed-forward scaled by K_SCALE so that the instances accept different steps: (fb, mu)"""
    d = {k: np.array(v, copy=True) for k, v in raw.items()}
    for k, s in DERIV_SEQS.items():
        if s in adds:
            d[k][:adds[s].size] += adds[s]
    r = c["o"].backward(d, c["xs"][b], c["mults"], 0.0, MU)
    assert r["restarts"] == 0
    r["fb"]["val"] = K_SCALE[b] * r["fb"]["val"]
    return r["fb"], r["mu"]


# ---- the terms: each module's own task generator, upload, values and derivatives ----------------------------------------------
class Term:
    """seqs: the sequences the term adds to; tol: its module's tolerance for them; one_sided: check(c, task) returns the entries'
    activity; report(ctx, which) / report_ref(c, task, b, X, U): its reporting call, where it has one"""
    one_sided, tol, report, needs_frames = False, TOL, None, False
    seqs = X_SEQS

    def zero(self, task, b, t=None):
        task[-1][(b,) if t is None else (b, t)] = 0.0


class Tracking(Term):
    seqs = ("LX", "LXX", "LU", "LUU", "LFX", "LFXX")
    flags = staticmethod(lambda capi: capi.FLAG_TRACKING_COST)

    def task(self, c, seed):
        return (tc.random_ref(c["o"], c["model"], c["xs"], c["us"], B, seed),)

    def zero(self, task, b, t=None):
        for k in ("wx", "wu"):
            task[0][k][(b,) if t is None else (b, t)] = 0.0

    def upload(self, ctx, c, task):
        tc.upload_ref(ctx, task[0])

    def terms(self, c, task, b, X, U):
        return tc.track_terms(c["o"], 1.0, X, U, task[0], b)

    def derivs(self, c, task, b, d):
        """tc.expected_derivs holds the plain c/2 |u|^2 as well: what it adds is the rest"""
        ex = tc.expected_derivs(c["o"], 1.0, c["xs"][b], c["us"][b], task[0], b)
        return {s: ex[s] - d[s][:ex[s].size] for s in self.seqs}


class Frame(Term):
    needs_frames = True
    flags = staticmethod(lambda capi: capi.FLAG_FRAME_COST)

    def task(self, c, seed):
        return fc.random_task(c["o"], c["xs"], c["frames"], B, seed)

    def upload(self, ctx, c, task):
        ctx.set_frame_cost(target=task[0], weight=task[1])

    def terms(self, c, task, b, X, U):
        return fc.frame_terms(c["o"], X, c["frames"], task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return fc.frame_derivs(c["o"], c["xs"][b], c["frames"], task[0][b], task[1][b])


class Orient(Term):
    needs_frames = True
    flags = staticmethod(lambda capi: capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST)

    def task(self, c, seed):
        return fo.random_orient(c["o"], c["xs"], c["frames"], B, seed, hi=1.5)

    def upload(self, ctx, c, task):
        ctx.set_frame_orient_cost(quat=task[0], weight=task[1])

    def terms(self, c, task, b, X, U):
        return fo.orient_terms(c["o"], X, c["frames"], task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return fo.orient_derivs(c["o"], c["xs"][b], c["frames"], task[0][b], task[1][b])


class Limits(Term):
    one_sided = True
    flags = staticmethod(lambda capi: capi.FLAG_STATE_LIMITS)

    def task(self, c, seed):
        return sl.random_limits(c["o"], c["xs"], B, seed)

    def upload(self, ctx, c, task):
        ctx.set_state_limits(lo=task[0], hi=task[1], weight=task[2])

    def terms(self, c, task, b, X, U):
        return sl.limit_terms(c["o"], X, task[0][b], task[1][b], task[2][b])

    def derivs(self, c, task, b, d):
        return sl.limit_derivs(c["o"], c["xs"][b], task[0][b], task[1][b], task[2][b])

    def check(self, c, task):
        o = c["o"]
        e = sl.excess(sl.coords(o, c["xs"].reshape(B, o.T + 1, o.nx)), task[0], task[1])
        return (e != 0.0)[task[2] != 0.0]


class Com(Term):
    flags = staticmethod(lambda capi: capi.FLAG_COM_COST)

    def task(self, c, seed):
        return cm.random_task(c["o"], c["model"], c["xs"], B, seed)

    def upload(self, ctx, c, task):
        ctx.set_com_cost(target=task[0], weight=task[1])

    def terms(self, c, task, b, X, U):
        return cm.com_terms(c["o"], c["model"], X, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return cm.com_derivs(c["o"], c["model"], c["xs"][b], task[0][b], task[1][b])


class Vel(Term):
    needs_frames = True
    flags = staticmethod(lambda capi: capi.FLAG_FRAME_COST | capi.FLAG_FRAME_VEL_COST)

    def task(self, c, seed):
        return fv.random_task(c["o"], c["xs"], c["frames"], B, seed)

    def upload(self, ctx, c, task):
        ctx.set_frame_vel_cost(target=task[0], weight=task[1])

    def terms(self, c, task, b, X, U):
        return fv.vel_terms(c["o"], X, c["frames"], task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return fv.vel_derivs(c["o"], c["model"], c["xs"][b], c["frames"], task[0][b], task[1][b])


class Momentum(Term):
    flags = staticmethod(lambda capi: capi.FLAG_MOMENTUM_COST)

    def task(self, c, seed):
        return mo.random_task(c["o"], c["model"], c["xs"], B, seed)

    def upload(self, ctx, c, task):
        ctx.set_momentum_cost(target=task[0], weight=task[1])

    def terms(self, c, task, b, X, U):
        return mo.mom_terms(c["o"], c["model"], X, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return mo.mom_derivs(c["o"], c["model"], c["xs"][b], task[0][b], task[1][b])


class Balance(Term):
    one_sided = True
    flags = staticmethod(lambda capi: capi.FLAG_BALANCE_REGION_COST)

    def task(self, c, seed):
        return br.random_task(c["o"], c["model"], c["xs"], B, seed)

    def upload(self, ctx, c, task):
        br.set_task(ctx, task[0], task[1])

    def terms(self, c, task, b, X, U):
        return br.br_terms(c["o"], c["model"], X, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return br.br_derivs(c["o"], c["model"], c["xs"][b], task[0][b], task[1][b])

    def check(self, c, task):
        return br.check_task(c["o"], c["model"], [c["xs"]], task[0], task[1], fractions=False)[task[1] != 0.0]

    def report(self, ctx, which):
        return ctx.balance_region_margin(which)

    def report_ref(self, c, task, b, X, U):
        return br.br_margin(c["o"], c["model"], X, task[0][b], task[1][b])


class Relative(Term):
    flags = staticmethod(lambda capi: capi.FLAG_RELATIVE_FRAME_COST)

    def task(self, c, seed):
        return rf.random_task(c["o"], c["rfpairs"], c["xs"], B, seed, hi=1.5)

    def upload(self, ctx, c, task):
        rf.set_task(ctx, c["rfpairs"], *task)

    def terms(self, c, task, b, X, U):
        return rf.rf_terms(c["o"], c["rfpairs"], X, task[0][b], task[1][b], task[2][b])

    def derivs(self, c, task, b, d):
        return rf.rf_derivs(c["o"], c["model"], c["rfpairs"], c["xs"][b], task[0][b], task[1][b], task[2][b])

    def check(self, c, task):
        return rf.check_task(c["o"], c["rfpairs"], c["xs"], *task)

    def report(self, ctx, which):
        return ctx.relative_frame_error(which)

    def report_ref(self, c, task, b, X, U):
        return rf.rf_errors(c["o"], c["rfpairs"], X, task[0][b], task[1][b])


class Grav(Term):
    seqs = U_SEQS
    flags = staticmethod(lambda capi: capi.FLAG_CONTROL_GRAV_COST)

    def task(self, c, seed):
        return cg.random_task(c["o"], c["model"], B, seed)

    def upload(self, ctx, c, task):
        ctx.set_control_grav_cost(*task)

    def terms(self, c, task, b, X, U):
        return cg.cg_terms(c["o"], c["model"], X, U, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return cg.cg_derivs(c["o"], c["model"], c["xs"][b], c["us"][b], task[0][b], task[1][b])


class Aim(Term):
    flags = staticmethod(lambda capi: capi.FLAG_FRAME_AIM_COST)

    def task(self, c, seed):
        return fa.random_task(c["o"], c["aim"], c["xs"], B, seed)

    def upload(self, ctx, c, task):
        fa.set_task(ctx, c["aim"], *task)

    def terms(self, c, task, b, X, U):
        return fa.fa_terms(c["o"], c["aim"], X, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return fa.fa_derivs(c["o"], c["model"], c["aim"], c["xs"][b], task[0][b], task[1][b])

    def check(self, c, task):
        return fa.check_task(c["o"], c["aim"], c["xs"], *task)

    def report(self, ctx, which):
        return ctx.frame_aim_error(which)

    def report_ref(self, c, task, b, X, U):
        return fa.fa_errors(c["o"], c["aim"], X, task[0][b])


class Accel(Term):
    seqs, tol = U_SEQS, ja.TOL_LIN
    flags = staticmethod(lambda capi: capi.FLAG_JOINT_ACCEL_COST)

    def task(self, c, seed):
        return ja.random_task(c["o"], c["xs"], c["us"], B, seed, wscale=ja.FWD_WSCALE, spread=0.5)

    def upload(self, ctx, c, task):
        ctx.set_joint_accel_cost(target=task[0], weight=task[1])

    def terms(self, c, task, b, X, U):
        return ja.ja_terms(c["o"], X, U, task[0][b], task[1][b])

    def bound(self, c, task, b, X, U):
        return ja.ja_terms(c["o"], X, U, task[0][b], task[1][b], bound=True)

    def derivs(self, c, task, b, d):
        return ja.ja_derivs(c["o"], c["xs"][b], c["us"][b], task[0][b], task[1][b])

    def report(self, ctx, which):
        return ctx.joint_accel(which)

    def report_ref(self, c, task, b, X, U):
        return ja.ja_accels(c["o"], X, U)


class Obstacle(Term):
    one_sided = True
    flags = staticmethod(lambda capi: capi.FLAG_OBSTACLE_COST)

    def task(self, c, seed):
        return ob.random_task(c["o"], c["pts"], ob.KINDS, c["xs"], B, seed, p_clear=0.25)

    def upload(self, ctx, c, task):
        ob.set_task(ctx, c["pts"], ob.KINDS, *task)

    def terms(self, c, task, b, X, U):
        return ob.ob_terms(c["o"], c["pts"], ob.KINDS, X, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return ob.ob_derivs(c["o"], c["model"], c["pts"], ob.KINDS, c["xs"][b], task[0][b], task[1][b])

    def check(self, c, task):
        return ob.check_task(c["o"], c["pts"], ob.KINDS, c["xs"], *task, fractions=False)[np.any(task[1] != 0.0, axis=-1)]

    def report(self, ctx, which):
        return ctx.obstacle_clearance(which)

    def report_ref(self, c, task, b, X, U):
        return ob.ob_clearance(c["o"], c["pts"], ob.KINDS, X, task[0][b], task[1][b])


class SelfCollision(Term):
    one_sided = True
    flags = staticmethod(lambda capi: capi.FLAG_SELF_COLLISION_COST)

    def task(self, c, seed):
        return sc.random_task(c["o"], c["pts"], c["scpairs"], c["xs"], B, seed, p_clear=0.25)

    def upload(self, ctx, c, task):
        sc.set_task(ctx, c["pts"], c["scpairs"], *task)

    def terms(self, c, task, b, X, U):
        return sc.sc_terms(c["o"], c["pts"], c["scpairs"], X, task[0][b], task[1][b])

    def derivs(self, c, task, b, d):
        return sc.sc_derivs(c["o"], c["model"], c["pts"], c["scpairs"], c["xs"][b], task[0][b], task[1][b])

    def check(self, c, task):
        return sc.check_task(c["o"], c["pts"], c["scpairs"], c["xs"], *task, fractions=False)[np.any(task[1] != 0.0, axis=-1)]

    def report(self, ctx, which):
        return ctx.self_collision_clearance(which)

    def report_ref(self, c, task, b, X, U):
        return sc.sc_clearance(c["o"], c["pts"], c["scpairs"], X, task[0][b], task[1][b])


TERMS = {"tracking": Tracking(), "frame": Frame(), "orient": Orient(), "limits": Limits(), "com": Com(), "vel": Vel(),
         "momentum": Momentum(), "balance": Balance(), "relative": Relative(), "grav": Grav(), "aim": Aim(), "accel": Accel(),
         "obstacle": Obstacle(), "selfcol": SelfCollision()}
EVERY = tuple(TERMS)


def robots_of(key):
    if key == "accel":
        return [n for n in SIZES if nv_of(n) <= 38] + list(SHAPES) + ["wide38x", "quad38"]
    return list(SIZES) + list(SHAPES) + (["wide38"] if key in INLINE else [])


CASES = [(key, name) for key in TERMS for name in robots_of(key)]


@functools.lru_cache(maxsize=None)
def task_of(key, name, together=False):
    """the term's task on a robot.  Alone: instance 1 without a weight, (instance 2, t = 1) without a weight.  Together: instance
    1 without a weight in the terms formed out of line"""
    term, c = TERMS[key], case(name)
    task = term.task(c, SEEDS.get((key, name, together), SEED0 + 10 * list(TERMS).index(key)))
    if not together or key not in INLINE:
        term.zero(task, ZERO_INSTANCE)
    if not together:
        term.zero(task, *ZERO_ROW)
    return task


def adds_to(keys, b, s):
    """whether the terms `keys` add to sequence s of instance b: alone not for the instance without a weight, together only the
    inline terms there"""
    return b != ZERO_INSTANCE or (len(keys) > 1 and any(s in TERMS[k].seqs for k in keys if k in INLINE))


@functools.lru_cache(maxsize=None)
def reference(keys, name, n_alpha=8):
    """what the CPU can say of the terms `keys` live together on a robot: the sum of their derivatives and of their values along both
    trajectories per instance, and the emulated forward on the summed cost"""
    c, p = case(name), plain(name)
    o, together = c["o"], len(keys) > 1
    tasks = {k: task_of(k, name, together) for k in keys}
    out = []
    for b in range(B):
        adds = {}
        for k in keys:
            a = TERMS[k].derivs(c, tasks[k], b, p[b]["d"])
            for s in TERMS[k].seqs:
                adds[s] = adds.get(s, 0.0) + a[s]

        def terms(X, U):
            return sum(TERMS[k].terms(c, tasks[k], b, X, U) for k in keys)

        fb, mu = feedback(c, p[b]["raw"], adds, b)

        def cost(X, U):
            return o.cost_seq_aug(X, U, c["mults"], mu) + terms(X, U)
        out.append(dict(adds=adds, terms=(terms(c["xs"][b], c["us"][b]), terms(c["xs2"][b], c["us2"][b])), fb=fb, mu=mu,
                        em=cm._emulate_forward(o, c["xs"][b], c["us"][b], c["mults"], fb, mu, n_alpha, cost)))
    return out


def assert_inputs(keys, name, n_alpha=8):
    """the conditions on the inputs, on the yardstick alone"""
    c = case(name)
    together = len(keys) > 1
    ref = reference(keys, name, n_alpha)
    seqs = sorted({s for k in keys for s in TERMS[k].seqs})
    for b in range(B):
        for s in seqs:
            assert (np.max(np.abs(ref[b]["adds"][s])) > 0) == adds_to(keys, b, s), (s, b)
        for which in (0, 1):
            assert np.any(ref[b]["terms"][which] != 0.0) == adds_to(keys, b, "LX"), (b, which)
    for k in keys:
        if hasattr(TERMS[k], "check"):
            act = TERMS[k].check(c, task_of(k, name, together))
            if TERMS[k].one_sided:
                assert np.any(act) and not np.all(act), (k, act.sum(), act.size)
    for b in range(B):
        assert ref[b]["em"] is not None, b
        assert min(ref[b]["em"][4]) > 1e-9, (b, ref[b]["em"][4])
    assert any(ref[b]["em"][0] < 1.0 for b in range(B))


# ---- CPU: the conditions on the inputs -------------------------------------------------------------------------------------------
def test_the_robot_built_here():
    """fan38 is what the docstring says: one level of 37 joints, wider than accel_group's 32 lanes, inside what create accepts
    (robots.open_slots <= 8, a level <= 64), and none of the catalogue's trees"""
    level, width, children = robots.tree_shape(FAN38)
    assert len(FAN38) == 38 and list(width) == [1, 37] and children.max() == 37 and robots.open_slots(FAN38) <= 8
    assert all(list(r.parents) != FAN38 for r in robots.CATALOGUE.values())
    assert [nv_of(n) for n in SIZES] == [2, 5, 13, 21, 40, 64]
    for name in HAND_JOINTS:                                  # why these pairs are chosen by hand
        c = case(name)
        with pytest.raises((AssertionError, IndexError)):
            rf.pick_pairs(c["model"])
        assert all(a[0] != b[0] for a, b in c["rfpairs"]) and len(c["rfpairs"]) == 4 and len(c["scpairs"]) >= 1


@pytest.mark.parametrize("key,name", CASES)
def test_inputs_decide_clearly(key, name):
    """on the yardstick alone, per (term, robot): the additions are non-zero in every sequence the term touches (and zero for the
    instance without a weight), the one-sided terms have violated and clear entries, the emulated forward returns for every
    instance, every candidate decides by more than 1e-9 of the summed magnitudes, and the halving runs"""
    assert_inputs((key,), name)


@pytest.mark.parametrize("n_alpha", [3, 8])
def test_inputs_decide_clearly_all_terms(n_alpha):
    """the same for the fourteen terms together on tree21, each of them non-zero on the instances that carry it"""
    assert_inputs(EVERY, "tree21", n_alpha)
    ref = reference(EVERY, "tree21", n_alpha)
    c = case("tree21")
    for k in EVERY:                                           # every term is material in the sum, on the instances that carry it
        for b in (0, 2):
            assert np.any(TERMS[k].terms(c, task_of(k, "tree21", True), b, c["xs"][b], c["us"][b]) != 0.0), (k, b)
    assert all(r["em"] is not None for r in ref)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
_OFF = {}


def flags_of(capi, keys):
    fl = capi.FLAG_NO_TENSORS
    for k in keys:
        fl |= TERMS[k].flags(capi)
    return fl


def run(capi, keys, name, n_alpha=8, reports=False, fb_of=None):
    """one context with the flags of `keys`: linearise, both cost sequences (X_NEW: the second trajectory), the reporting calls,
    one forward from the feedback of reference(fb_of or keys)"""
    c, p = case(name), reference(fb_of or keys, name, n_alpha)
    together = len(keys) > 1
    out = {}
    with capi.Context(c["spec"], flags=flags_of(capi, keys)) as ctx:
        check_info(ctx, name)
        ctx.upload("X", c["xs"]); ctx.upload("U", c["us"]); ctx.upload("X_NEW", c["xs2"]); ctx.upload("U_NEW", c["us2"])
        if any(TERMS[k].needs_frames for k in keys):
            ctx.set_frame_cost(frames=c["frames"])
        for k in keys:
            TERMS[k].upload(ctx, c, task_of(k, name, together))
        ctx.linearize()
        for s in ALL_SEQS:
            out[s] = ctx.download(s)
        ctx.cost_seq_aug(0, MU); ctx.cost_seq_aug(1, MU)
        out["COSTS_OLD"], out["COSTS_NEW"] = ctx.download("COSTS_OLD"), ctx.download("COSTS_NEW")
        if reports:
            for k in keys:
                out["report", k] = (TERMS[k].report(ctx, 0), TERMS[k].report(ctx, 1))
        ctx.upload("X_NEW", c["xs"]); ctx.upload("U_NEW", c["us"])
        for k, s in (("origin", "FB_ORIGIN"), ("val", "FB_VAL"), ("jac", "FB_JAC")):
            ctx.upload(s, np.stack([p[b]["fb"][k][:ctx.seq_size(s)] for b in range(B)]))
        _, out["step"], out["dcost"] = ctx.forward(np.array([p[b]["mu"] for b in range(B)]), n_alpha=n_alpha)
        out["X_NEW"], out["U_NEW"] = ctx.download("X_NEW"), ctx.download("U_NEW")
    return out


def flag_off(capi, name):
    """the sequences of a context without a cost flag, once per robot (its forward is no part of any comparison)"""
    if name not in _OFF:
        _OFF[name] = run(capi, (), name, fb_of=("tracking",))
    return _OFF[name]


def compare(keys, name, got, off, n_alpha=8):
    """the device's sequences, costs and forward against the yardstick of `keys`; off: the flag-off context's sequences"""
    c, p, ref = case(name), plain(name), reference(keys, name, n_alpha)
    o, T, n = c["o"], c["T"], c["o"].n
    touched = {s: max(TERMS[k].tol for k in keys if s in TERMS[k].seqs) for k in keys for s in TERMS[k].seqs}
    worst = {}
    for s in ALL_SEQS:
        if s not in touched:
            assert np.array_equal(got[s], off[s]), s
    for b in range(B):
        for s, tol in touched.items():
            ex = p[b]["d"][s][:got[s][b].size] + ref[b]["adds"][s]
            if adds_to(keys, b, s):
                assert np.max(np.abs(ref[b]["adds"][s])) > 0, (s, b)
            if b != ZERO_INSTANCE:                           # (together, `off` holds the inline terms: instance 1 is all theirs)
                assert not np.array_equal(got[s][b], off[s][b]), (s, b)
            e = rel_err(got[s][b], ex)
            worst[s] = max(worst.get(s, 0.0), e)
            assert e <= tol, (name, keys, s, b, e)
        for blk in list(got["LXX"][b].reshape(T, n, n)) + [got["LFXX"][b].reshape(n, n)]:
            assert np.array_equal(blk, blk.T)
        for which, key in ((0, "COSTS_OLD"), (1, "COSTS_NEW")):
            ex = p[b]["costs"][which] + ref[b]["terms"][which]
            err = np.abs(got[key][b] - ex)
            tol = np.full(T + 1, 0.0 if keys == ("accel",) else TOL * np.max(np.abs(ex)))
            if "accel" in keys:                              # test_joint_accel_cost.test_cost_values: per t, through the square
                X, U = (c["xs"][b], c["us"][b]) if which == 0 else (c["xs2"][b], c["us2"][b])
                bound = TERMS["accel"].bound(c, task_of("accel", name, len(keys) > 1), b, X, U)
                tol += ja.TOL_ABA * bound + 4 * np.finfo(float).eps * np.abs(got[key][b])
            worst[key] = max(worst.get(key, 0.0), float(np.max(err / np.maximum(tol, 1e-300))))
            assert np.all(err <= tol), (name, keys, key, b, err, tol)
        step_ref, xn_ref, un_ref, new, margins = ref[b]["em"]
        assert min(margins) > 1e-9, margins                 # a condition on the inputs: the decisions do not hang on rounding
        assert got["step"][b] == step_ref, (name, keys, b, got["step"], step_ref)
        assert rel_err(got["X_NEW"][b], xn_ref) < TOL_FWD and rel_err(got["U_NEW"][b], un_ref) < TOL_FWD, (name, keys, b)
        assert abs(got["dcost"][b] - new) <= TOL_FWD * max(1.0, abs(new)), (name, keys, b, got["dcost"][b], new)
    assert any(ref[b]["em"][0] < 1.0 for b in range(B))
    print("compare", name, keys if len(keys) == 1 else "all", "steps", got["step"], "worst", worst)


def compare_report(key, name, got):
    """the term's reporting call along X and X_NEW against its module's reference, +inf where nothing is live"""
    c, term, task = case(name), TERMS[key], task_of(key, name)
    for which, (Xs, Us) in enumerate(((c["xs"], c["us"]), (c["xs2"], c["us2"]))):
        ex = np.stack([term.report_ref(c, task, b, Xs[b], Us[b]) for b in range(B)])
        dev = got["report", key][which]
        assert dev.shape == ex.shape and np.array_equal(np.isinf(dev), np.isinf(ex)), (key, which)
        fin = np.isfinite(ex)
        if term.one_sided:
            assert np.all(np.isinf(ex[ZERO_INSTANCE])) and fin.any()
        scale = np.maximum(1.0, np.abs(ex[fin])) if term.one_sided else 1.0 if key == "aim" else np.max(np.abs(ex[fin]))
        e = np.max(np.abs(dev[fin] - ex[fin]) / scale)      # (each as its module's own test of the call scales it)
        print("report", key, name, which, e)
        assert e <= TOL, (key, name, which, e)


@pytest.mark.gpu
@pytest.mark.parametrize("key,name", CASES)
def test_term_on_robot(gpu, key, name, monkeypatch):
    """one term on one robot: every sequence it adds to against the oracle's plain derivatives plus the module's *_derivs, every
    other one bit for bit the flag-off context's, LXX / LFXX symmetric bit for bit; both cost sequences; one forward with n_alpha =
    8 against the emulation (the step exactly); the reporting call on tree21 and tree64 (joint_accel: tree21 and deep38).  On
    wide38 the forward is the latency kernel's, in both forms bit for bit"""
    reports = TERMS[key].report is not None and name in (("tree21", "deep38") if key == "accel" else REPORT_ON)
    got = run(gpu, (key,), name, reports=reports)
    compare((key,), name, got, flag_off(gpu, name))
    if reports:
        compare_report(key, name, got)
    if name == "wide38":
        monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
        again = run(gpu, (key,), name)
        for k in OUTS:
            assert np.array_equal(got[k], again[k]), k


@pytest.mark.gpu
def test_joint_accel_refused_past_38_joints(gpu):
    """tree40: creation with the flag answers E_UNSUPPORTED (DDP_HIP_MAX_JOINT_ACCEL_NV), the same spec without it is accepted"""
    capi = gpu
    c = case("tree40")
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(c["spec"], flags=capi.FLAG_JOINT_ACCEL_COST | capi.FLAG_NO_TENSORS)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(c["spec"], flags=capi.FLAG_NO_TENSORS) as ctx:
        check_info(ctx, "tree40")


@pytest.mark.gpu
@pytest.mark.parametrize("n_alpha", [3, 8])
def test_all_terms_at_once(gpu, n_alpha):
    """tree21 (32 lanes per evaluation, prismatic joints) with every cost flag: every derivative sequence equals the oracle's plain
    one plus the sum of all fourteen *_derivs at the loosest tolerance among the modules that touch it (1e-10 where the joint
    accelerations add, 1e-12 for LFX / LFXX), both cost sequences the sum of all *_terms, the forward the emulation on the summed
    cost with every candidates' array live; instance 1, without a weight in any term formed out of line, is bit for bit that
    instance of a context created with the inline terms' flags alone"""
    got = run(gpu, EVERY, "tree21", n_alpha)
    inline = run(gpu, INLINE, "tree21", n_alpha, fb_of=EVERY)
    compare(EVERY, "tree21", got, inline, n_alpha)
    assert not np.array_equal(got["LX"][0], inline["LX"][0]) and not np.array_equal(got["COSTS_OLD"][0], inline["COSTS_OLD"][0])
    for k in COST_SEQS + OUTS:
        assert np.array_equal(got[k][ZERO_INSTANCE], inline[k][ZERO_INSTANCE]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", REPORT_ON)
def test_model_helpers(gpu, name):
    """the ModelHandle evaluations behind the targets at one random state with non-zero velocity, value and jacobians against the
    modules' references at 1e-12: com, centroidal_momentum, capture_point, gravity_torque, frame_velocity, relative_frame,
    frame_axis"""
    capi = gpu
    c = case(name)
    o, model = c["o"], c["model"]
    x = random_state(model, np.random.default_rng(77 + model.nv))
    q, v = x[:o.nq], x[o.nq:]
    assert np.all(v != 0.0)
    pairs = []
    with capi.ModelHandle(model) as hd:
        pairs.append(("com", hd.com(q, jacobian=True), (cm.com(o, model, q), cm.com_jac(o, model, q))))
        pairs.append(("momentum", hd.centroidal_momentum(q, v, jacobian=True), mo.momentum_jacobians(o, model, q, v)))
        pairs.append(("capture", hd.capture_point(q, v, 0.31, jacobian=True), br.point(o, model, x, 0.31, jacobian=True)))
        pairs.append(("gravity", hd.gravity_torque(q, jacobian=True), cg.grav_torque(o, model, q)))
        for j, off in c["frames"]:
            pairs.append((("velocity", j), hd.frame_velocity(j, off, q, v, jacobian=True), fv.vel_jacobians(o, model, j, off, q, v)))
        for pair in c["rfpairs"]:
            (ja_, offa), (jb, offb) = pair
            rel, E, _, _, _ = rf.placement(o, pair, q)
            qy = fo.R_to_quat(E)
            pairs.append((("relative", ja_, jb), hd.relative_frame(ja_, offa, jb, offb, q, jacobian=True),
                          (rel, -qy if qy[3] < 0 else qy, rf.rf_J(o, model, pair, q, np.zeros(3))[0])))
        for frame in c["aim"]:
            pairs.append((("axis", frame[0]), hd.frame_axis(*frame, q, jacobian=True), fa.eye_axis(o, frame, q) + (fa.pn_J(o, model, frame, q)[0],)))
    for what, dev, ex in pairs:
        assert len(dev) == len(ex)
        for a, e in zip(dev, ex):
            assert np.max(np.abs(e)) > 0, what
            err = rel_err(a, e)
            print("helper", name, what, err)
            assert err <= TOL, (what, err)
