"""The (v_i, v_j) and (u_i, u_j) pair kernels of the static mode-2 stencil (csrc/lin_static.hip: lin_static_vel_kernel<T, false>,
lin_static_tau_kernel<T, false>): one wave = 64 pairs on operands staged in LDS, output in two half-wave passes.

What the shapes are for.  tree38: 703 pairs = ten full waves and one of 63 lanes (an invalid lane in the second half-wave pass),
batch 3 x T 2 for the (instance, t) -> block arithmetic.  chain6: 15 pairs in one wave (the second half-wave pass has no valid
point at all), stage_split 3.  The 12-joint biped: a generated topology, 66 pairs = one full wave and one of two lanes.

Tolerance: the end-to-end bound of tests/test_dynamics_parity.py::_linearize_parity (tol_second_e2e, ulps = 8)."""
import functools

import numpy as np
import pytest

from problems import initial_trajectory, make

EPS, E1, E2 = 2.220446049250313e-16, 1.4901161193847656e-08, 1.220703125e-04
ULPS = 8
SEQS = {"fxx": "FXX", "fux": "FUX", "fuu": "FUU"}


def _builtin(name, T, batch):
    model, spec, o = make(name, T, batch=batch, fd_mode=2)
    sigma = 0.05 if name.startswith("chain6") else 0.5
    trajs = [initial_trajectory(o, model, seed=40 + b, u_sigma=sigma)[1:] for b in range(batch)]
    return model, spec, o, trajs


def _biped12(T, batch):
    from ddp_pinocchio_amd import capi
    from oracle.binding import Oracle
    from test_generated_topology import BIPED12, seeded_tree
    model = seeded_tree(BIPED12, seed=len(BIPED12))
    nv = len(BIPED12)
    kw = dict(dt=0.01, c=1.0, fd_mode=2, first_order_fd=1, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    spec = capi.ProblemSpec(model, T, batch=batch, **kw)
    o = Oracle(model, T, **kw)
    rng = np.random.default_rng(3)
    trajs = []
    for b in range(batch):
        us = 0.5 * rng.normal(size=T * nv)
        x0 = np.concatenate([0.3 * rng.normal(size=nv), 0.2 * rng.normal(size=nv)])
        trajs.append((us, o.rollout(x0, us)))
    return model, spec, o, trajs


CASES = {"tree38": (lambda: _builtin("tree38", 2, 3), 2), "chain6": (lambda: _builtin("chain6", 3, 2), 3),
         "biped12": (lambda: _biped12(2, 2), 5)}


@functools.lru_cache(maxsize=None)
def _linearized(case):
    """one linearisation per case: (nv, T, tensors as downloaded [batch][...], oracle derivatives per instance); read-only"""
    from ddp_pinocchio_amd import capi
    build, lin_path = CASES[case]
    model, spec, o, trajs = build()
    with capi.Context(spec) as ctx:
        assert ctx.info()["lin_path"] == lin_path, "the static-topology kernels must take this model"
        for b, (us, xs) in enumerate(trajs):
            ctx.upload("X", xs, b, 1); ctx.upload("U", us, b, 1)
        ctx.linearize()
        got = {k: ctx.download(s) for k, s in SEQS.items()}
    refs = [o.compute_derivatives(xs, us) for us, xs in trajs]
    for a in got.values():
        a.setflags(write=False)
    return model.nv, o.T, got, refs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tree38", "chain6", "biped12"])
def test_pair_blocks_match_the_oracle(gpu, case):
    nv, T, got, refs = _linearized(case)
    for b, d in enumerate(refs):
        fscale = max(1.0, float(np.max(np.abs(d["f_val"]))))
        tol_first = ULPS * EPS * fscale / E1
        tol = 8 * ULPS * EPS * fscale / (E2 * E2) + 4 * tol_first / E2
        for key in ("fxx", "fux", "fuu"):
            g = got[key][b]
            ref = d[key][:g.size]
            scale = max(1.0, float(np.max(np.abs(ref))))
            # per step, so that a block written for the wrong (instance, t) cannot hide behind another step's scale
            err = np.max(np.abs(g - ref).reshape(T, -1), axis=1)
            print(f"{case} instance {b} {key}: max |err| per step {err}, bound {tol * scale:.3e}")
            assert np.all(np.isfinite(g)), (case, key, b)
            assert np.all(err <= tol * scale), (case, key, b, err, tol * scale)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tree38", "chain6"])
def test_pair_blocks_are_exactly_symmetric_with_zero_configuration_rows(gpu, case):
    """one evaluation per pair i < j, written to (i, j) and (j, i): the (v, v) block of f_xx and all of f_uu are symmetric bit for
    bit; a control does not reach q+ = q + dt v within the step: rows k < nv of every f_uu column are exact zeros"""
    nv, T, got, _ = _linearized(case)
    n, B = 2 * nv, got["fxx"].shape[0]
    fxx = got["fxx"].reshape(B, T, n, n, n)          # [first direction][second direction][row of f]
    fuu = got["fuu"].reshape(B, T, nv, nv, n)
    vv = fxx[:, :, nv:, nv:, :]
    assert np.all(np.isfinite(vv)) and np.all(np.isfinite(fuu))
    assert np.array_equal(vv, vv.transpose(0, 1, 3, 2, 4))
    assert np.array_equal(fuu, fuu.transpose(0, 1, 3, 2, 4))
    assert np.all(fuu[..., :nv] == 0.0)
    # (the pairs did write something: the stencil's off-diagonal blocks are not all zeros)
    iu = np.triu_indices(nv, 1)
    assert np.any(vv[:, :, iu[0], iu[1], nv:] != 0.0)
