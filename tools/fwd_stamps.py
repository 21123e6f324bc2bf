"""development: phase split of the forward latency kernel (build_ab/libddp_hip_fstamps.so: `make fstamps`, -DFWD_STAMPS):
accumulated s_memrealtime (100 MHz) of workgroup 0 over the 200 steps of one forward pass, of the leading wave and, in the
pipelined form, of the helper wave that runs one step ahead and of the assistant wave that forms the controls, the cost and the
prefetch beside pass 1.  DDP_HIP_FWD_NO_PIPE=1: the four-candidate form"""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["DDP_HIP_LIB"] = os.path.join(ROOT, "build_ab", "libddp_hip_fstamps.so")
sys.path.insert(0, ROOT)
import numpy as np
from ddp_pinocchio_amd import capi
S, T = int(sys.argv[1]) if len(sys.argv) > 1 else 4, 200
model = capi.BuiltinModel(capi.BUILTIN_TREE38, 1)
ctx = capi.Context(capi.ProblemSpec(model, T, batch=S, fd_mode=0), flags=capi.FLAG_NO_TENSORS)
us = 0.1 * np.random.default_rng(0).normal(size=(S, T * 38))
ctx.upload("X", np.zeros((S, (T + 1) * 76))); ctx.upload("U", us); ctx.rollout()
ctx.upload("X_NEW", ctx.download("X")); ctx.upload("U_NEW", us)
ctx.linearize()
ctx.backward(np.zeros(S), np.full(S, 1e2))
for _ in range(2):
    rc, step, dcost = ctx.forward(np.full(S, 1e2), n_alpha=8)
out = (C.c_ulonglong * 36)()
assert capi.lib().ddp_hip_debug_fwd_stamps(out) == 0
piped = any(out[12:])
if piped:
    lead = {4: "pass 1", 0: "wait for u_t (the hand-off)", 5: "pass 2: forces", 6: "pass 3", 7: "v update", 3: "wait at the step's barrier"}
    assist = {0: "dx + K dx + u, post", 1: "cost term", 2: "request t+1", 8: "park", 3: "wait at the step's barrier"}
    helper = {0: "q_{t+1} = q_t (+) dt v_t", 3: "placements", 9: "levels: tables + inertia sums", 10: "levels: U, D, 1/D",
              11: "levels: Ia, X^T Ia X, stores", 5: "wait at the step's barrier"}
    chains = (("leading wave (step t)", lead, out[:12]), ("helper wave (q-part of step t + 1)", helper, out[12:24]),
              ("assistant wave (controls, cost, prefetch of step t)", assist, out[24:]))
else:
    names = ["dx + K dx + u", "cost term", "request t+1", "placements", "pass 1", "pass 2: wait at the level barrier", "pass 3", "x update", "park",
             "pass 2: tables + inertia sums", "pass 2: U, D, 1/D", "pass 2: force half"]
    chains = (("leading wave", dict(enumerate(names)), out[:12]),)
for title, names, acc in chains:
    tot = sum(acc)
    print(f"-- {title}")
    for i, nme in names.items():
        print(f"{nme:36s} {acc[i] / 100.0 / T:8.2f} us / step  ({100.0 * acc[i] / tot:5.1f} %)")
    busy = tot - (acc[5] if title.startswith("helper") else acc[3] + (acc[0] if title.startswith("leading") else 0)) if piped else tot
    print(f"{'total':36s} {tot / 100.0 / T:8.2f} us / step" + (f"   (without the waits: {busy / 100.0 / T:.2f})" if piped else ""))
