"""Score test (pg_score_dev, lmm.pygemma_score) against the Wald scan (pg_assoc_dev, lmm.pygemma) on one GPU.

At n = 10 000, c = 5, p = 100 000 SNPs resident, alternating in one process:
  kernel:  device-event time of one pg_score_dev call against one pg_assoc_dev call on the same rotated block, and the score call's
           achieved HBM rate: the bytes it must move (rotated X read once, 4 ldx p; outputs 32 p) over its time, as a share of
           6.0 and 6.3 TB/s (MI355X_MICROARCH: 6.29 TB/s measured float4 copy);
  step:    rotation (pg_rotate_auto_dev, genotype codes) + score against rotation + Wald;
  e2e:     wall time of lmm.pygemma_score against lmm.pygemma (pinned float32 X, K given: eigensolver included).
Prints one JSON line (median, min, max of the repeats; ratio = score / Wald); --out also writes it to a file.
usage: bench_score.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
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

# ---- inputs: eigenbasis d, W, y; a dense orthogonal U; raw genotype codes resident as float32 (n, p)
rp = synth.fast_rotated_panel(n, 64, c)
d, W = rp["d"].astype(np.float32), np.ascontiguousarray(rp["W"], np.float32)
y = rp["Y"].reshape(-1).astype(np.float32)
U = np.empty((n, n), np.float32)
synth.block_orthogonal(U, seed=3)
G = np.empty((n, p), np.float32)
for s0 in range(0, p, 8192):
    e0 = min(p, s0 + 8192)
    thr = rng.uniform(0.05, 0.5, e0 - s0)
    u = rng.random((2, n, e0 - s0), dtype=np.float32)
    G[:, s0:e0] = (u[0] < thr).astype(np.float32) + (u[1] < thr).astype(np.float32)
dd, dW, dy, dU, dX = ctx.to_device(d), ctx.to_device(W), ctx.to_device(y), ctx.to_device(U), ctx.to_device(G)
dXr = ctx.alloc(p * ldx * 4)
dprep = ctx.alloc(L.pg_geno_prep_bytes(n))
dwork = ctx.alloc(L.pg_geno_work_bytes(n, p))
_lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
res = ctx.alloc(32 * p)
r0 = res.ptr
dl = ctx.alloc(4)
_lib.check(L.pg_score_null_dev(ctx.handle, n, c, dd.ptr, dW.ptr, dy.ptr, dl.ptr), "pg_score_null_dev")
ctx.sync()
lam0 = float(dl.download((1,), np.float32)[0])
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def rotate():
    _lib.check(L.pg_rotate_auto_dev(ctx.handle, n, p, dU.ptr, n, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, None), "pg_rotate_auto_dev")


def wald():
    _lib.check(L.pg_assoc_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, dXr.ptr, ldx, 0,
                              r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0 + 28 * p, r0, r0 + 8 * p, None), "pg_assoc_dev")


def score():
    _lib.check(L.pg_score_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, lam0, dXr.ptr, ldx,
                              r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0 + 28 * p, r0, r0 + 8 * p), "pg_score_dev")


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
wald()
score()
ctx.sync()

out = {"tool": "bench_score", "n": n, "p": p, "c": c, "reps": a.reps, "lambda0": lam0}
ker = {"score": [], "wald": []}
stp = {"score": [], "wald": []}
rot = []
for r in range(a.reps):
    rotate()
    legs = (("score", score), ("wald", wald))
    for name, fn in (legs if r % 2 == 0 else legs[::-1]):
        ker[name].append(timed(fn))
    rot.append(timed(rotate))
    steps = (("score", lambda: (rotate(), score())), ("wald", lambda: (rotate(), wald())))
    for name, fn in (steps if r % 2 == 0 else steps[::-1]):
        stp[name].append(timed(fn))
ms = float(np.median(ker["score"]))
moved = 4.0 * ldx * p + 32.0 * p                       # rotated X read once + the six output columns
out["kernel"] = {"score_ms": summary(ker["score"]), "wald_ms": summary(ker["wald"]),
                 "ratio": round(ms / float(np.median(ker["wald"])), 4),
                 "bytes": int(moved), "achieved_TBps": round(moved / (ms * 1e-3) / 1e12, 3),
                 "share_of_6.0": round(moved / (ms * 1e-3) / 6.0e12, 3), "share_of_6.3": round(moved / (ms * 1e-3) / 6.3e12, 3),
                 "roof_ms_at_6.3": round(moved / 6.3e12 * 1e3, 3)}
out["step"] = {"rotation_ms": summary(rot), "score_ms": summary(stp["score"]), "wald_ms": summary(stp["wald"]),
               "ratio": round(float(np.median(stp["score"]) / np.median(stp["wald"])), 4)}
for b in (dX, dXr, dwork, dU):
    b.free()
ctx.sync()

# ---- end to end: lmm.pygemma_score against lmm.pygemma, pinned float32 X, eigensolver included (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    pe = a.e2e_p
    Xh = _lib.pinned_empty((n, pe), np.float32)
    Xh[:] = G[:, :pe]
    del G
    K = lmm.kinship(Xh[:, :2000])
    Wh = np.concatenate([np.ones((n, 1), np.float32), rng.standard_normal((n, c - 1)).astype(np.float32)], axis=1)
    Yh = (Xh[:, :30] @ rng.standard_normal(30) + rng.standard_normal(n) * 2).astype(np.float64)
    lmm.pygemma_score(Yh, Xh[:, :8192].copy(), Wh, K)                   # warm-up of both paths (kernels, allocations)
    lmm.pygemma(Yh, Xh[:, :8192].copy(), Wh, K)
    e2e = {"score": [], "wald": []}
    for r in range(a.e2e_reps):
        legs = (("score", lambda: lmm.pygemma_score(Yh, Xh, Wh, K)), ("wald", lambda: lmm.pygemma(Yh, Xh, Wh, K)))
        for name, fn in (legs if r % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            fn()
            e2e[name].append(time.perf_counter() - t0)
    out["e2e"] = {"p": pe, "score_s": summary(e2e["score"]), "wald_s": summary(e2e["wald"]),
                  "ratio": round(float(np.median(e2e["score"]) / np.median(e2e["wald"])), 3)}
else:
    del G
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
