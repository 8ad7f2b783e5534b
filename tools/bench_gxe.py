"""Interaction scan (pg_assoc_gxe_dev, lmm.pygemma_gxe) against the Wald scan (pg_assoc_dev, lmm.pygemma) on one GPU.

At n = 10 000, W with c = 5 columns (the interaction scan adds e: 6 shared covariates), p = 100 000 SNPs resident as genotype codes,
alternating in one process:
  kernel:  device-event time of one pg_assoc_gxe_dev call against one pg_assoc_dev call on the same rotated block (U'X; the GxE call
           also reads U'(X o e));
  step:    two rotations (pg_rotate_auto_dev with U and with diag(e) U) + GxE against one rotation + Wald;
  e2e:     wall time of lmm.pygemma_gxe against lmm.pygemma (pinned float32 X, K given: eigensolver included).
Prints one JSON line (median, min, max of the repeats; ratio = GxE / Wald); --out also writes it to a file.
usage: bench_gxe.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygemma_amd import _lib, lmm, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--c", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--e2e-p", type=int, default=100000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p, c = a.n, a.p, a.c
L = _lib.load()
ctx = _lib.Context(0)
ldx = (n + 63) // 64 * 64
rng = np.random.default_rng(5)

# ---- inputs: eigenbasis d, W, y; a dense orthogonal U; e; raw genotype codes resident as float32 (n, p)
rp = synth.fast_rotated_panel(n, 64, c)
d, W = rp["d"].astype(np.float32), np.ascontiguousarray(rp["W"], np.float32)
y = rp["Y"].reshape(-1).astype(np.float32)
e = rng.standard_normal(n).astype(np.float32)
U = np.empty((n, n), np.float32)
synth.block_orthogonal(U, seed=3)
We = np.ascontiguousarray(np.c_[W, U.T @ e], np.float32)           # W' = [W, U'e] in the eigenbasis
G = np.empty((n, p), np.float32)
for s0 in range(0, p, 8192):
    e0 = min(p, s0 + 8192)
    thr = rng.uniform(0.05, 0.5, e0 - s0)
    u = rng.random((2, n, e0 - s0), dtype=np.float32)
    G[:, s0:e0] = (u[0] < thr).astype(np.float32) + (u[1] < thr).astype(np.float32)
dd, dW, dWe, dy, dU, dX, de = (ctx.to_device(v) for v in (d, W, We, y, U, G, e))
dUe = ctx.alloc(n * n * 4)
dXr, dXEr = ctx.alloc(p * ldx * 4), ctx.alloc(p * ldx * 4)
dprep, dprepe = ctx.alloc(L.pg_geno_prep_bytes(n)), ctx.alloc(L.pg_geno_prep_bytes(n))
dwork = ctx.alloc(L.pg_geno_work_bytes(n, p))
_lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
_lib.check(L.pg_gxe_scale_u_dev(ctx.handle, n, dU.ptr, n, de.ptr, dUe.ptr), "pg_gxe_scale_u_dev")
_lib.check(L.pg_geno_prep_dev(ctx.handle, n, dUe.ptr, n, dprepe.ptr), "pg_geno_prep_dev")
res = ctx.alloc(32 * p)
r0 = res.ptr
evs = [C.c_void_p() for _ in range(2)]
for ev in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(ev)), "pg_event_create")


def rotate(dUx=dU, dprepx=dprep, dst=dXr):
    _lib.check(L.pg_rotate_auto_dev(ctx.handle, n, p, dUx.ptr, n, dprepx.ptr, dX.ptr, p, dst.ptr, ldx, dwork.ptr, None), "pg_rotate_auto_dev")


def rotate_e():
    rotate(dUe, dprepe, dXEr)


def wald():
    _lib.check(L.pg_assoc_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, dXr.ptr, ldx, 0,
                              r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0 + 28 * p, r0, r0 + 8 * p, None), "pg_assoc_dev")


def gxe():
    _lib.check(L.pg_assoc_gxe_dev(ctx.handle, n, c + 1, p, dd.ptr, dWe.ptr, dy.ptr, dXr.ptr, ldx, dXEr.ptr, ldx,
                                  r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0 + 28 * p, r0, r0 + 8 * p, None), "pg_assoc_gxe_dev")


def timed(fn):
    L.pg_event_record(ctx.handle, evs[0])
    fn()
    L.pg_event_record(ctx.handle, evs[1])
    ms = C.c_float()
    _lib.check(L.pg_event_elapsed_ms(ctx.handle, evs[0], evs[1], C.byref(ms)), "pg_event_elapsed_ms")
    return ms.value


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


# warm-up: every launch shape once (scratch allocations, code objects)
rotate()
rotate_e()
wald()
gxe()
ctx.sync()
out = {"tool": "bench_gxe", "n": n, "p": p, "c": c, "shared_covariates_gxe": c + 1, "reps": a.reps,
       "gxe_finite": None}
ker = {"gxe": [], "wald": []}
stp = {"gxe": [], "wald": []}
rot = []
for r in range(a.reps):
    rotate()
    rotate_e()
    legs = (("gxe", gxe), ("wald", wald))
    for name, fn in (legs if r % 2 == 0 else legs[::-1]):
        ker[name].append(timed(fn))
    rot.append(timed(rotate))
    steps = (("gxe", lambda: (rotate(), rotate_e(), gxe())), ("wald", lambda: (rotate(), wald())))
    for name, fn in (steps if r % 2 == 0 else steps[::-1]):
        stp[name].append(timed(fn))
gxe()
ctx.sync()
out["gxe_finite"] = float(np.isfinite(res.download((p,), np.float64)).mean())
out["kernel"] = {"gxe_ms": summary(ker["gxe"]), "wald_ms": summary(ker["wald"]),
                 "ratio": round(float(np.median(ker["gxe"]) / np.median(ker["wald"])), 4)}
out["step"] = {"rotation_ms": summary(rot), "gxe_ms": summary(stp["gxe"]), "wald_ms": summary(stp["wald"]),
               "ratio": round(float(np.median(stp["gxe"]) / np.median(stp["wald"])), 4),
               "rotation_share_gxe": round(float(2 * np.median(rot) / np.median(stp["gxe"])), 4)}
for b in (dX, dXr, dXEr, dwork, dU, dUe):
    b.free()
ctx.sync()

# ---- end to end: lmm.pygemma_gxe against lmm.pygemma, pinned float32 X, eigensolver included (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    pe = a.e2e_p
    Xh = _lib.pinned_empty((n, pe), np.float32)
    Xh[:] = G[:, :pe]
    del G
    K = lmm.kinship(Xh[:, :2000])
    Wh = np.concatenate([np.ones((n, 1), np.float32), rng.standard_normal((n, c - 1)).astype(np.float32)], axis=1)
    Yh = (Xh[:, :30] @ rng.standard_normal(30) + rng.standard_normal(n) * 2).astype(np.float64)
    lmm.pygemma_gxe(Yh, Xh[:, :8192].copy(), Wh, K, e)                  # warm-up of both paths (kernels, allocations)
    lmm.pygemma(Yh, Xh[:, :8192].copy(), Wh, K)
    e2e = {"gxe": [], "wald": []}
    for r in range(a.e2e_reps):
        legs = (("gxe", lambda: lmm.pygemma_gxe(Yh, Xh, Wh, K, e)), ("wald", lambda: lmm.pygemma(Yh, Xh, Wh, K)))
        for name, fn in (legs if r % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            fn()
            e2e[name].append(time.perf_counter() - t0)
    out["e2e"] = {"p": pe, "gxe_s": summary(e2e["gxe"]), "wald_s": summary(e2e["wald"]),
                  "ratio": round(float(np.median(e2e["gxe"]) / np.median(e2e["wald"])), 3)}
else:
    del G
for ev in evs:
    L.pg_event_destroy(ctx.handle, ev)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
