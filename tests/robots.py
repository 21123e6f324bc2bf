"""A catalogue of robots other than the built-in ones: trees of 1-DoF joints given as parent tables (capi.TableModel), one per
size class, plan and limit the run-time-shaped kernels have (tests/test_other_robots.py runs them; what each entry reaches is
in its `what`).  A plain module: the same description goes to the product (capi.ProblemSpec) and to the oracle."""
import functools
from collections import namedtuple

import numpy as np

ARM7 = [-1, 0, 1, 2, 3, 4, 5]
BIPED12 = [-1, 0, 1, 2, 3, 4, 5, 0, 7, 8, 9, 10]
TREE44 = [-1, 0, 1, 2, 3, 4] + [5, 6, 7, 8, 9, 10] + [5, 12, 13, 14, 15, 16] + [5, 18] + [19, 20, 21, 22, 23, 24, 25] + \
         [19, 27, 28, 29, 30, 31, 32] + [19, 34] + [26, 36, 37] + [33, 39, 40] + [35, 42]


def seeded_tree(parents, seed, prismatic=()):
    """a random robot on a given tree: random axes / placements / inertias; revolute joints but the indices in `prismatic`
    (the draws do not depend on `prismatic`)"""
    from ddp_pinocchio_amd import capi
    rng = np.random.default_rng(seed)
    nv = len(parents)
    axis = rng.normal(size=(nv, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    Rp = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(nv)])
    for k in range(nv):
        if np.linalg.det(Rp[k]) < 0:
            Rp[k][:, 0] = -Rp[k][:, 0]
    pp = rng.uniform(0.05, 0.3, size=(nv, 3)) * rng.choice([-1.0, 1.0], size=(nv, 3))
    mass = rng.uniform(0.5, 5.0, size=nv)
    com = rng.uniform(-0.05, 0.05, size=(nv, 3))
    Ic = np.zeros((nv, 3, 3))
    for k in range(nv):
        a = rng.uniform(0.05, 0.3, size=3)                  # a box with these half sizes
        Ic[k] = np.diag(mass[k] / 3.0 * np.array([a[1] ** 2 + a[2] ** 2, a[0] ** 2 + a[2] ** 2, a[0] ** 2 + a[1] ** 2]))
        Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        Ic[k] = Q @ Ic[k] @ Q.T
    jtype = [capi.JOINT_PRISMATIC if k in prismatic else capi.JOINT_REVOLUTE for k in range(nv)]
    return capi.TableModel(parents, jtype, axis, Rp, pp, mass, com, Ic)


def branching(nv, seed):
    """a seeded tree: joint i hangs from one of the five joints before it"""
    rng = np.random.default_rng(seed)
    return [-1] + [int(rng.integers(max(0, i - 5), i)) for i in range(1, nv)]


def chains(lengths):
    """a root joint carrying one chain of each of the given lengths"""
    parents = [-1]
    for n in lengths:
        parents = parents + [0] + [len(parents) + k for k in range(n - 1)]
    return parents


def fanned(groups):
    """root -> one joint per group -> that joint's chains (their lengths), the chains of a group numbered joint by joint in turn:
    a fork's children are neighbours in the numbering and a chain's next joint is the group's width away"""
    parents = [-1] + [0] * len(groups)
    for g, lengths in enumerate(groups):
        last = [g + 1] * len(lengths)
        for depth in range(max(lengths)):
            for c, n in enumerate(lengths):
                if depth < n:
                    parents.append(last[c])
                    last[c] = len(parents) - 1
    return parents


# wide38: root -> 3 -> 8, eight chains below (levels of 1, 3, 8, 8, 8, 8, 2 joints).  Talos is numbered depth first (a fork's next
# child follows the whole subtree of the one before); here every fork's children are neighbours and its chains interleave
WIDE38 = fanned([(5, 4, 4), (5, 4, 4), (4, 4)])
WIDE38X = fanned([(4, 4, 4), (4, 4, 4), (4, 3, 3)])     # levels of 1, 3, 9, 9, 9, 7
DEEP38 = chains([16, 16, 5])       # 17 levels, at most 3 joints wide
QUAD38 = chains([9, 9, 9, 10])     # the root has four children

Robot = namedtuple("Robot", "name parents seed prismatic what")

CATALOGUE = {r.name: r for r in [
    Robot("pair2", [-1, 0], 202, (), "<6> instantiations below the template size, the one-lane plan of small models"),
    Robot("fork5", [-1, 0, 1, 0, 3], 205, (2,), "the same plan at odd n / m sizes, a prismatic joint"),
    Robot("star7", [-1, 0, 0, 0, 1, 2, 3], 207, (), "first size of the 38 class on the run-time-tree kernels"),
    Robot("tree13", [-1, 0, 1, 2, 1, 4, 5, 0, 7, 8, 7, 10, 11], 213, (), "38 class, CoM lanes 16, odd LDS leading dimension"),
    Robot("tree21", branching(21, 221), 221, (3, 9, 16), "CoM lanes 32, prismatic joints"),
    Robot("wide38", WIDE38, 238, (), "latency forward kernel at level width 8, fast sweep on run-time-tree tensors"),
    Robot("wide38x", WIDE38X, 239, (), "a level of 9: the one-lane forward kernel at nv = 38"),
    Robot("deep38", DEEP38, 240, (), "17 levels: the same fallback by depth"),
    Robot("quad38", QUAD38, 241, (), "a joint with 4 children: the same fallback by child count"),
    Robot("tree39", branching(39, 339), 339, (), "first size of the 64 class, gains LDS under 64 KB"),
    Robot("tree40", branching(40, 340), 340, (), "first size whose gains LDS passes 64 KB"),
    Robot("TREE44", TREE44, 144, (), "the 44-joint tree of test_generated_topology.py"),
    Robot("tree57", branching(57, 357), 357, (), "the largest size with a sweep under control bounds"),
    Robot("tree58", branching(58, 358), 358, (), "first size the box sweep refuses"),
    Robot("tree63", branching(63, 363), 363, (), "the largest size with a sweep, assemble LDS over 64 KB"),
    Robot("tree64", branching(64, 364), 364, (), "the limit: everything but the sweep"),
]}


def tree_shape(parents):
    """(level of every joint, joints per level, children per joint), in numpy"""
    p = np.asarray(parents)
    level = np.zeros(len(p), dtype=np.int64)
    for i in range(len(p)):
        level[i] = 0 if p[i] < 0 else level[p[i]] + 1
    return level, np.bincount(level), np.bincount(p[p >= 0], minlength=len(p))


def by_level_numbering(parents):
    """the same tree with its joints renumbered level by level (stable within a level)"""
    level = tree_shape(parents)[0]
    order = sorted(range(len(parents)), key=lambda i: (level[i], i))
    new = {old: k for k, old in enumerate(order)}
    return [-1 if parents[old] < 0 else new[parents[old]] for old in order]


def open_slots(parents):
    """The library keeps a joint's running sum of the tree traversals in one of a few slots, from the joint's largest-index child
    down to the joint itself (leaf -> root; root -> leaf alike): how many slots the numbering needs at once.  Creating a context
    answers E_UNSUPPORTED beyond 8 -- a tree numbered level by level with 8 chains side by side needs more"""
    n = len(parents)
    largest = [max([i for i in range(n) if parents[i] == j], default=-1) for j in range(n)]
    used, most = set(), 0
    slot = [-1] * n
    for i in range(n - 1, -1, -1):                      # leaf -> root: the parent's slot opens at its largest-index child
        if parents[i] >= 0 and largest[parents[i]] == i:
            slot[parents[i]] = min(k for k in range(n + 1) if k not in used)
            used.add(slot[parents[i]])
            most = max(most, slot[parents[i]] + 1)
        used.discard(slot[i])
    used, slot = set(), [-1] * n
    for i in range(n):                                  # root -> leaf: a joint's slot closes at its largest-index child
        if largest[i] >= 0:
            slot[i] = min(k for k in range(n + 1) if k not in used)
            used.add(slot[i])
            most = max(most, slot[i] + 1)
        if parents[i] >= 0 and largest[parents[i]] == i:
            used.discard(slot[parents[i]])
    return most


@functools.lru_cache(maxsize=None)
def model(name):
    r = CATALOGUE[name]
    return seeded_tree(r.parents, r.seed, r.prismatic)


def problem(name, T, batch=1, fd_mode=2, first_order_fd=1, constraint=None):
    """(model, spec, oracle) of a catalogue robot.  constraint: None, "config" (every joint to the neutral q at every step: emax =
    nv) or "frame" (3 rows at t = T - 2: a point of the last joint)"""
    from ddp_pinocchio_amd import capi
    from oracle.binding import Oracle
    m = model(name)
    nv = m.nv
    if constraint is None:
        kw = dict(eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    elif constraint == "config":
        kw = dict(eq_kind=capi.EQ_CONFIG, eq_advance=2, ne=np.full(T, nv, dtype=np.int64), eq_target=np.zeros(nv * T))
    elif constraint == "frame":
        ne = np.zeros(T, dtype=np.int64); ne[T - 2] = 3
        kw = dict(eq_kind=capi.EQ_FRAME, eq_advance=2, ne=ne, eq_target=np.array([0.2, -0.1, 0.3]), frame_joint=nv - 1,
                  frame_off=(0.0, 0.0, 0.1))
    else:
        raise ValueError(constraint)
    kw.update(dt=0.01, c=1.0, fd_mode=fd_mode, first_order_fd=first_order_fd)
    return m, capi.ProblemSpec(m, T, batch=batch, **kw), Oracle(m, T, **kw)
