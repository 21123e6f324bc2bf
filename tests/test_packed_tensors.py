"""Packed tensor records: the static mode-2 stencil leaves FXX / FUX / FUU as records of nv + 2 doubles per
column -- [top0, top1, rows nv .. n-1] at the front of each slab -- which the packed K3h streams; every other reader has them
unpacked into the contract layout first (lin.hip: lin_materialize_fxx).  Nothing that is computed changes, so every check here
is bit for bit against a context created with DDP_HIP_K3_NO_PACK, whose stencil writes the contract layout as before.  The
fast sweep exists at n = 76, m = 38 only: tree38 is the smallest shape at which any of this runs; batch 3 and batch 8 take the
two branches of K3h's XCD remapping ((B & 7) == 0)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from problems import initial_trajectory, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ddp_pinocchio_amd", "csrc")
NO_PACK = "DDP_HIP_K3_NO_PACK"
TENSORS = ("FXX", "FUX", "FUU")
T = 3


def _context(capi, spec, monkeypatch, switch=None):
    """a traced context created with the development switch set: a context reads the switches once, at creation"""
    if switch:
        monkeypatch.setenv(switch, "1")
    try:
        return capi.Context(spec, flags=capi.FLAG_TRACE)
    finally:
        if switch:
            monkeypatch.delenv(switch)


def _k3h_stencil_bytes(o):
    n, m = o.n, o.m
    cxx, cux, cuu = n * (n + 1) // 2, n * m, m * (m + 1) // 2
    return 8 * ((cxx + cux + cuu) * (n - m) + 2 * cxx - n + cux)


def _dense_bytes(o):
    return 8 * (o.n ** 3 + o.n * o.n * o.m + o.n * o.m * o.m)


def _inputs(ctx, model, o, B, seed=60):
    for b in range(B):
        x0, us, xs = initial_trajectory(o, model, seed=seed + b, u_sigma=0.4)
        ctx.upload("X", xs, b, 1); ctx.upload("U", us, b, 1)


def _linearize(ctx, o, B, stages=None):
    """linearise, then a V_x that is not zero: terminal cost gradient (the cost stage writes LFX / LFXX itself)"""
    ctx.linearize(stages)
    ctx.upload("LFX", np.random.default_rng(1).normal(size=(B, o.n)))
    ctx.upload("LFXX", np.tile(np.eye(o.n).reshape(-1), (B, 1)))


def _sweep(ctx):
    rc, reg, mu, rs = ctx.backward(0.0, 1.0)
    return [ctx.download(s) for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")] + [rs, reg, mu, rc]


def _same(a, b):
    assert len(a) == len(b)
    for a_, b_ in zip(a, b):
        assert np.array_equal(a_, b_)


def _pair(capi, monkeypatch, B, name="tree38", horizon=T):
    model, spec, o = make(name, horizon, batch=B, fd_mode=2)
    return model, o, _context(capi, spec, monkeypatch), _context(capi, spec, monkeypatch, NO_PACK)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 8])
def test_packed_sweep_bit_for_bit(gpu, monkeypatch, B):
    """the sweep on packed records against the strided K3h on the contract layout; the byte count names K3h in both"""
    model, o, ctx, ref = _pair(gpu, monkeypatch, B)
    with ctx, ref:
        outs = []
        for c in (ctx, ref):
            _inputs(c, model, o, B)
            _linearize(c, o, B)
            assert c.bwd_stream_bytes() == _k3h_stencil_bytes(o)
            outs.append(_sweep(c))
            assert c.bwd_stream_bytes() == _k3h_stencil_bytes(o)
        _same(outs[0], outs[1])
        assert float(np.max(np.abs(outs[0][2]))) > 0 and np.all(np.isfinite(outs[0][0]))


@pytest.mark.gpu
def test_default_context_really_holds_records(gpu, monkeypatch):
    """the bytes in FXX after a default context's linearisation, copied straight from device memory (no materialise hook), are
    the records: column j >= c of slab c is [top0, top1, rows nv .. n-1] at slab + j (nv + 2).  Every other case here compares a
    context with its partner, which would also pass if the default context never packed; this one would not"""
    capi = gpu
    B = 3
    model, o, ctx, ref = _pair(capi, monkeypatch, B)
    n, nv = o.n, o.n // 2
    R = nv + 2
    with ctx, ref:
        ptr = ctx.device_ptr("FXX")                         # taken before the linearisation: asking later would unpack
        assert ptr
        for c in (ctx, ref):
            _inputs(c, model, o, B)
            _linearize(c, o, B)
        ctx.synchronize()
        raw = np.empty(n * n * n)                           # instance 0, t = 0
        hip_memcpy = capi.lib().hipMemcpy                   # (the HIP runtime the library is linked against)
        hip_memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert hip_memcpy(raw.ctypes.data, ptr, raw.nbytes, 2) == 0   # 2: hipMemcpyDeviceToHost
        rec = raw.reshape(n, n * n)[:, :n * R].reshape(n, n, R)       # [slab c][column j][word]
        fx = ref.download("FXX")[0][:n * n * n].reshape(n, n, n)      # the contract layout: [slab c][column j][row k]
        cc, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        written = jj >= cc                                  # the symmetric stencil skips j < c
        assert np.array_equal(rec[..., 2:][written], fx[..., nv:][written])
        top0 = np.take_along_axis(fx, (cc % nv)[..., None], axis=2)[..., 0]
        top1 = np.take_along_axis(fx, (jj % nv)[..., None], axis=2)[..., 0]
        assert np.array_equal(rec[..., 0][written], top0[written])
        two = written & ((jj % nv) != (cc % nv))
        assert np.array_equal(rec[..., 1][two], top1[two])
        assert np.any(rec[..., 2:][written]) and np.any(top0[written])   # (the top1 entries of this (instance, t) are exact zeros)
        # and the download of the same context shows the contract layout, the partner's
        assert np.array_equal(ctx.download("FXX"), ref.download("FXX"))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 8])
def test_packed_life_cycle(gpu, monkeypatch, B):
    """linearise -> backward (packed) -> download FUX only (unpacks all three) -> backward (strided K3h) -> linearise (packs
    again) -> backward: every sweep is the partner's, and what the download leaves is the contract layout"""
    model, o, ctx, ref = _pair(gpu, monkeypatch, B)
    n, m, nv = o.n, o.m, o.n // 2
    with ctx, ref:
        for c in (ctx, ref):
            _inputs(c, model, o, B)
            _linearize(c, o, B)
        s1, r1 = _sweep(ctx), _sweep(ref)
        _same(s1, r1)
        assert float(np.max(np.abs(s1[2]))) > 0
        fux, fux_ref = ctx.download("FUX"), ref.download("FUX")
        assert np.array_equal(fux, fux_ref)
        assert ctx.bwd_stream_bytes() == _k3h_stencil_bytes(o)
        _same(_sweep(ctx), _sweep(ref))
        fxx, fuu = ctx.download("FXX"), ctx.download("FUU")
        assert np.array_equal(fxx, ref.download("FXX")) and np.array_equal(fuu, ref.download("FUU"))
        fx4 = fxx.reshape(B, T, n, n, n)                    # [b][t][slab c][column j][row k]
        assert np.array_equal(fx4, fx4.transpose(0, 1, 3, 2, 4)), "f_xx is symmetric bit for bit"
        # the configuration rows: zeros but the rows of the two directions
        k = np.arange(nv)
        cmod = (np.arange(n) % nv)
        named_xx = (k[None, None, :] == cmod[:, None, None]) | (k[None, None, :] == cmod[None, :, None])   # [c][j][k]
        assert not np.any(fx4[..., :nv][:, :, ~named_xx])
        assert np.any(fx4[..., :nv][:, :, named_xx])
        fu4 = fux.reshape(B, T, n, m, n)                    # [b][t][slab c (x)][column j (u)][row k]
        named_ux = np.broadcast_to(k[None, None, :] == cmod[:, None, None], (n, m, nv))
        assert not np.any(fu4[..., :nv][:, :, ~named_ux])
        assert not np.any(fuu.reshape(B, T, m, m, n)[..., :nv])
        for c in (ctx, ref):
            _linearize(c, o, B)
        _same(_sweep(ctx), _sweep(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 8])
def test_outside_writes_after_a_packed_linearisation(gpu, monkeypatch, B):
    """upload / fill / device_ptr of any of the three tensors unpack all of them first: what the caller does not overwrite is
    the contract layout's, what it writes is there as written, and the sweep reads the result as the partner does"""
    model, o, ctx, ref = _pair(gpu, monkeypatch, B)
    with ctx, ref:
        for c in (ctx, ref):
            _inputs(c, model, o, B)
        _linearize(ref, o, B)
        base = {s: ref.download(s) for s in TENSORS}        # the stencil's tensors, complete (the partner never packs)
        new_fxx = 0.5 * base["FXX"][1]
        new_fux = 0.25 * base["FUX"]

        def w_fxx(c): c.upload("FXX", new_fxx, 1, 1)
        def w_fux(c): c.upload("FUX", new_fux)
        def w_fuu(c): c.fill("FUU", 0.0)
        def w_ptr(c): assert c.device_ptr("FXX")

        def expect(which):
            e = {s: base[s].copy() for s in TENSORS}
            if which == "fxx": e["FXX"][1] = new_fxx
            if which == "fux": e["FUX"] = new_fux
            if which == "fuu": e["FUU"][:] = 0.0
            return e

        nbytes = {"fxx": _dense_bytes(o), "fuu": _dense_bytes(o), "ptr": _dense_bytes(o)}
        for which, write in (("fxx", w_fxx), ("fux", w_fux), ("fuu", w_fuu), ("ptr", w_ptr)):
            outs = []
            for c in (ctx, ref):
                _linearize(c, o, B)
                write(c)
                if which in nbytes:
                    assert c.bwd_stream_bytes() == nbytes[which]
                got = {s: c.download(s) for s in TENSORS}
                e = expect(which)
                for s in TENSORS:
                    assert np.array_equal(got[s], e[s]), (which, s)
                outs.append(_sweep(c))
            assert ctx.bwd_stream_bytes() == ref.bwd_stream_bytes()
            _same(outs[0], outs[1])
            assert float(np.max(np.abs(outs[0][2]))) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 8])
def test_first_order_alone_keeps_the_records(gpu, monkeypatch, B):
    """linearize_stages without the second-order stage leaves the tensors as they are -- packed -- and the sweep reads them so"""
    capi = gpu
    model, o, ctx, ref = _pair(capi, monkeypatch, B)
    with ctx, ref:
        outs = []
        for c in (ctx, ref):
            _inputs(c, model, o, B)
            c.linearize()
            _linearize(c, o, B, capi.LIN_COST | capi.LIN_FIRST | capi.LIN_EQ)
            assert c.bwd_stream_bytes() == _k3h_stencil_bytes(o)
            outs.append(_sweep(c))
        _same(outs[0], outs[1])
        assert float(np.max(np.abs(outs[0][2]))) > 0


@pytest.mark.gpu
def test_packed_with_constraint_rows(gpu, monkeypatch):
    """tree38_frame: constraint rows on the fast sweep.  The tensors a download shows are the partner's, backward returns the
    partner's code and, where that is OK, the partner's outputs"""
    capi = gpu
    B, T4 = 2, 4
    model, o, ctx, ref = _pair(capi, monkeypatch, B, "tree38_frame", T4)
    rng = np.random.default_rng(2)
    jac = 0.01 * rng.normal(size=o.Etot * o.n)

    def run(c):
        for b in range(B):
            x0, us, xs = initial_trajectory(o, model, seed=17 + b, u_sigma=0.4)
            c.upload("X", xs, b, 1); c.upload("U", us, b, 1)
            mults = o.alloc_affine(o.Etot)
            mults["origin"][:] = xs[:T4 * o.nx]
            mults["jac"][:o.Etot * o.n] = jac
            for k, sname in (("origin", "MULT_ORIGIN"), ("val", "MULT_VAL"), ("jac", "MULT_JAC")):
                if c.seq_size(sname):
                    c.upload(sname, mults[k][:c.seq_size(sname)], b, 1)
        _linearize(c, o, B)
        assert c.bwd_stream_bytes() == _k3h_stencil_bytes(o)
        try:
            out = _sweep(c)
            code = out[-1]
        except capi.DdpHipError as e:
            out, code = None, e.code
        return code, out, [c.download(s) for s in TENSORS]

    with ctx, ref:
        code, out, tensors = run(ctx)
        code_ref, out_ref, tensors_ref = run(ref)
        _same(tensors, tensors_ref)
        assert code == code_ref
        if code >= 0:                                       # OK, or the restart event: the sweep ran to its end
            _same(out, out_ref)
            assert float(np.max(np.abs(out[2]))) > 0


def test_plan_packs_only_the_static_stencil_for_k3h():
    """the plan table (csrc/lin_plan.cpp): pack implies the stencil skips the mirror images and runs on the static kernels; some
    combination a context can be created with packs; none with K3h or the skipped rows switched off does"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_table"])
    out = subprocess.run([os.path.join(ROOT, "build", "lin_plan_table")], capture_output=True, text=True, check=True).stdout
    head, sw, body = out.split("\n", 2)
    names, switches = head.split(), sw.split()[1:]
    rows = np.array(body.split(), dtype=np.int64).reshape(-1, len(names))
    col = {name: rows[:, k] for k, name in enumerate(names)}
    live = (col["created"] == 1) & (col["refuse"] == 0)
    pack = col["pack"] == 1
    mode2_static = 2                                        # LinSecond::Mode2Static (csrc/internal.h)
    assert not np.any(pack & ~((col["skip_qv_mirror"] == 1) & (col["second"] == mode2_static)))
    assert np.any(pack & live)
    # the headline context: the Talos tree on its static kernels, mode 2, tensors resident, a sweep that reads by halves, no switch
    talos = (live & (col["nv"] == 38) & (col["ff"] == 0) & (col["matched"] == 1) & (col["mode"] == 2) & (col["tensors"] == 1) &
             (col["sym_ok"] == 1) & (col["sw"] == switches.index("none")))
    assert np.any(talos) and np.all(pack[talos])
    for s in ("k3_no_half", "fxx_full"):
        assert not np.any(pack & (col["sw"] == switches.index(s)))
