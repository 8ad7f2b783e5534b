"""Multi-phenotype scan against t single-phenotype scans on one GPU (the loop the reference's callers write over phenotypes).

At n = 10 000, c = 5, p = 100 000 SNPs resident, Brent and grid, t in {1, 2, 4, 8}, alternating in one process:
  assoc:   device-event time of one pg_assoc_pheno_dev call (t phenotypes) against t back-to-back pg_assoc_dev calls on the same
           rotated block;
  step:    rotation (pg_rotate_auto_dev, genotype codes) + association for t phenotypes against t x (rotation + pg_assoc_dev);
  e2e:     wall time of lmm.pygemma_multi against a loop of t lmm.pygemma calls (pinned float32 X, K given: eigensolver included), t = 4.
Prints one JSON line (median, min, max of the repeats; ratio = multi / singles); --out also writes it to a file.
usage: bench_pheno.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--e2e-p", type=int, default=100000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p, c = a.n, a.p, a.c
TS = (1, 2, 4, 8)
L = _lib.load()
ctx = _lib.Context(0)
ldx = (n + 63) // 64 * 64
rng = np.random.default_rng(5)

# ---- inputs: eigenbasis d, W, 8 phenotypes; a dense orthogonal U; raw genotype codes resident as float32 (n, p)
rp = synth.fast_rotated_panel(n, 64, c)
d, W = rp["d"].astype(np.float32), np.ascontiguousarray(rp["W"], np.float32)
y0 = rp["Y"].reshape(-1).astype(np.float32)
Y = np.stack([y0] + [(rng.standard_normal() * y0 + rng.standard_normal(n)).astype(np.float32) for _ in range(7)])
U = np.empty((n, n), np.float32)
synth.block_orthogonal(U, seed=3)
G = np.empty((n, p), np.float32)
for s0 in range(0, p, 8192):
    e0 = min(p, s0 + 8192)
    thr = rng.uniform(0.05, 0.5, e0 - s0)
    u = rng.random((2, n, e0 - s0), dtype=np.float32)
    G[:, s0:e0] = (u[0] < thr).astype(np.float32) + (u[1] < thr).astype(np.float32)
dd, dW, dY, dU, dX = ctx.to_device(d), ctx.to_device(W), ctx.to_device(Y), ctx.to_device(U), ctx.to_device(G)
dXr = ctx.alloc(p * ldx * 4)
dprep = ctx.alloc(L.pg_geno_prep_bytes(n))
dwork = ctx.alloc(L.pg_geno_work_bytes(n, p))
_lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
res = ctx.alloc(32 * p * max(TS))
r0 = res.ptr
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def rotate():
    _lib.check(L.pg_rotate_auto_dev(ctx.handle, n, p, dU.ptr, n, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, None), "pg_rotate_auto_dev")


def singles(t, grid):
    for k in range(t):
        _lib.check(L.pg_assoc_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dY.ptr + 4 * n * k, dXr.ptr, ldx, grid,
                                  r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0 + 28 * p, r0, r0 + 8 * p, None), "pg_assoc_dev")


def multi(t, grid):
    tp = t * p
    _lib.check(L.pg_assoc_pheno_dev(ctx.handle, n, c, p, t, dd.ptr, dW.ptr, dY.ptr, n, dXr.ptr, ldx, grid,
                                    r0 + 16 * tp, r0 + 20 * tp, r0 + 24 * tp, r0 + 28 * tp, r0, r0 + 8 * tp, None), "pg_assoc_pheno_dev")


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
for grid in (0, 1):
    singles(1, grid)
    for t in TS:
        multi(t, grid)
ctx.sync()

out = {"tool": "bench_pheno", "n": n, "p": p, "c": c, "reps": a.reps, "assoc": {}, "step": {}}
for grid, mode in ((0, "brent"), (1, "grid")):
    acc = {t: {"multi": [], "single": []} for t in TS}
    stp = {t: {"multi": [], "single": []} for t in TS}
    one_rot = []
    for r in range(a.reps):
        rotate()
        for t in TS:                    # alternate the order of the two sides between repeats
            legs = (("multi", lambda t=t: multi(t, grid)), ("single", lambda t=t: singles(t, grid)))
            for name, fn in (legs if r % 2 == 0 else legs[::-1]):
                acc[t][name].append(timed(fn))
        one_rot.append(timed(rotate))
        s1 = timed(lambda: (rotate(), singles(1, grid)))
        for t in TS:
            stp[t]["multi"].append(timed(lambda t=t: (rotate(), multi(t, grid))))
            stp[t]["single"].append(t * s1)
    out["assoc"][mode] = {str(t): {"multi_ms": summary(acc[t]["multi"]), "singles_ms": summary(acc[t]["single"]),
                                   "ratio": round(float(np.median(acc[t]["multi"]) / np.median(acc[t]["single"])), 3)} for t in TS}
    out["step"][mode] = {"rotation_ms": summary(one_rot)}
    out["step"][mode].update({str(t): {"multi_ms": summary(stp[t]["multi"]), "t_x_single_ms": summary(stp[t]["single"]),
                                       "ratio": round(float(np.median(stp[t]["multi"]) / np.median(stp[t]["single"])), 3)} for t in TS})
for b in (dX, dXr, dwork, dU):
    b.free()
ctx.sync()

# ---- end to end: lmm.pygemma_multi against the loop over phenotypes, pinned float32 X, eigensolver included
t4, pe = 4, a.e2e_p
Xh = _lib.pinned_empty((n, pe), np.float32)
Xh[:] = G[:, :pe]
del G
Gk = Xh[:, :2000]
K = lmm.kinship(Gk)
Wh = np.concatenate([np.ones((n, 1), np.float32), rng.standard_normal((n, c - 1)).astype(np.float32)], axis=1)
Yh = (Xh[:, :30] @ rng.standard_normal((30, t4)) + rng.standard_normal((n, t4)) * 2).astype(np.float64)
lmm.pygemma_multi(Yh[:, :2], Xh[:, :8192].copy(), Wh, K)          # warm-up of both paths (kernels, allocations)
lmm.pygemma(Yh[:, 0], Xh[:, :8192].copy(), Wh, K)
e2e = {"multi": [], "loop": []}
for r in range(a.e2e_reps):
    legs = (("multi", lambda: lmm.pygemma_multi(Yh, Xh, Wh, K)), ("loop", lambda: [lmm.pygemma(Yh[:, k], Xh, Wh, K) for k in range(t4)]))
    for name, fn in (legs if r % 2 == 0 else legs[::-1]):
        t0 = time.perf_counter()
        fn()
        e2e[name].append(time.perf_counter() - t0)
out["e2e"] = {"t": t4, "p": pe, "multi_s": summary(e2e["multi"]), "loop_s": summary(e2e["loop"]),
              "ratio": round(float(np.median(e2e["multi"]) / np.median(e2e["loop"])), 3)}
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
