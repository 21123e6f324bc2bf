"""The packed K3h on full units (csrc/bwd_jobs.h, bwd_split.h: bwd_contract_units): which unit a column rides in
changes nothing in its sum, so the sweep is held bit for bit to a context created with DDP_HIP_K3H_COLUMN_JOBS (the packed K3h
on the column jobs) and to one created with DDP_HIP_K3_NO_PACK (the strided K3h on the contract layout).  The tolerance is
zero.  The fast sweep exists at n = 76, m = 38 only; batch 1 is the smallest grid, 3 takes the plain block mapping, 8 the XCD
remap ((B & 7) == 0)."""
import numpy as np
import pytest

from problems import initial_trajectory, make

COLUMN_JOBS = "DDP_HIP_K3H_COLUMN_JOBS"
NO_PACK = "DDP_HIP_K3_NO_PACK"
NAMES = ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE", "restarts", "reg", "mu")


def _context(capi, spec, monkeypatch, switch=None):
    """a traced context created with the development switch set: a context reads the switches once, at creation"""
    if switch:
        monkeypatch.setenv(switch, "1")
    try:
        return capi.Context(spec, flags=capi.FLAG_TRACE)
    finally:
        if switch:
            monkeypatch.delenv(switch)


def _linearize(ctx, o, B):
    """linearise, then a V_x that is not zero: with V = 0 the contraction is zero whatever the kernel reads"""
    ctx.linearize()
    ctx.upload("LFX", np.random.default_rng(1).normal(size=(B, o.n)))
    ctx.upload("LFXX", np.tile(np.eye(o.n).reshape(-1), (B, 1)))


def _sweep(ctx):
    rc, reg, mu, rs = ctx.backward(0.0, 1.0)
    return rc, [ctx.download(s) for s in NAMES[:4]] + [rs, reg, mu]


def _same(a, b, what):
    assert len(a) == len(b) == len(NAMES)
    for name, a_, b_ in zip(NAMES, a, b):
        assert np.array_equal(a_, b_), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 8])
def test_full_units_bit_for_bit(gpu, monkeypatch, B):
    capi = gpu
    T = 3
    model, spec, o = make("tree38", T, batch=B, fd_mode=2)
    ctxs = [_context(capi, spec, monkeypatch, sw) for sw in (None, COLUMN_JOBS, NO_PACK)]
    try:
        outs = []
        for c in ctxs:
            for b in range(B):
                x0, us, xs = initial_trajectory(o, model, seed=60 + b, u_sigma=0.4)
                c.upload("X", xs, b, 1); c.upload("U", us, b, 1)
            _linearize(c, o, B)
            rc, out = _sweep(c)
            assert rc == 0
            outs.append(out)
        _same(outs[0], outs[1], COLUMN_JOBS)
        _same(outs[0], outs[2], NO_PACK)
        assert float(np.max(np.abs(outs[0][2]))) > 0
        for a in outs[0]:
            assert np.all(np.isfinite(a))
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.gpu
def test_full_units_with_constraint_rows(gpu, monkeypatch):
    """tree38_frame: constraint rows on the fast sweep.  backward returns the partners' code and, where the sweep ran to its end,
    the partners' outputs"""
    capi = gpu
    B, T = 2, 4
    model, spec, o = make("tree38_frame", T, batch=B, fd_mode=2)
    jac = 0.01 * np.random.default_rng(2).normal(size=o.Etot * o.n)
    ctxs = [_context(capi, spec, monkeypatch, sw) for sw in (None, COLUMN_JOBS, NO_PACK)]

    def run(c):
        for b in range(B):
            x0, us, xs = initial_trajectory(o, model, seed=17 + b, u_sigma=0.4)
            c.upload("X", xs, b, 1); c.upload("U", us, b, 1)
            mults = o.alloc_affine(o.Etot)
            mults["origin"][:] = xs[:T * o.nx]
            mults["jac"][:o.Etot * o.n] = jac
            for k, sname in (("origin", "MULT_ORIGIN"), ("val", "MULT_VAL"), ("jac", "MULT_JAC")):
                if c.seq_size(sname):
                    c.upload(sname, mults[k][:c.seq_size(sname)], b, 1)
        _linearize(c, o, B)
        try:
            return _sweep(c)
        except capi.DdpHipError as e:
            return e.code, None

    try:
        res = [run(c) for c in ctxs]
        for (code, out), what in zip(res[1:], (COLUMN_JOBS, NO_PACK)):
            assert code == res[0][0], what
            if code >= 0:                                   # OK, or the restart event: the sweep ran to its end
                _same(res[0][1], out, what)
        if res[0][0] >= 0:
            assert float(np.max(np.abs(res[0][1][2]))) > 0
            for a in res[0][1]:
                assert np.all(np.isfinite(a))
    finally:
        for c in ctxs:
            c.close()
