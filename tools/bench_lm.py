"""Linear-model scan (pg_lm_x_dev / pg_lm_bed_dev, lmm.pygemma_lm) on one GPU.

At n = 10 000, c = 5, t = 1, p = 100 000 SNPs resident, alternating in one process:
  kernel:  device-event time of one scan call (p-values included) on device-resident float32 sample-major, float32 SNP-major, int8
           (both orders) and packed .bed blocks; for each the achieved HBM rate — the bytes it must move (the block read once, 28 p
           of outputs) over its time, as a share of 6.3 TB/s — and its fp64 flop rate (2 npad NP per SNP, NP = c + t padded to 16)
           as a share of what pgx_dgemm_dev sustains on the same pipe in the same run (4096^3);
           pg_score_dev on a float32 SNP-major block of the same n, c and p (the same bytes per SNP) for comparison;
  e2e:     wall time of lmm.pygemma_lm against lmm.pygemma_score (K given: eigensolver and rotation included) from pinned float32 X
           and from a PackedBed.
Prints one JSON line (median, min, max of the repeats); --out also writes it to a file.
usage: bench_lm.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygemma_amd import _lib, lmm  # noqa: E402
from pygemma_amd.bed import PackedBed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--c", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--e2e-p", type=int, default=100000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p, c, t = a.n, a.p, a.c, 1
L = _lib.load()
ctx = _lib.Context(0)
ldx = (n + 63) // 64 * 64
bpr = (n + 3) // 4
rng = np.random.default_rng(5)

# ---- inputs: genotype codes, SNP-major int8 on the host; every other image of the block is made from it
G8 = np.empty((p, n), np.int8)
for s0 in range(0, p, 8192):
    e0 = min(p, s0 + 8192)
    thr = rng.uniform(0.05, 0.5, (e0 - s0, 1)).astype(np.float32)
    u = rng.random((2, e0 - s0, n), dtype=np.float32)
    G8[s0:e0] = (u[0] < thr).astype(np.int8) + (u[1] < thr).astype(np.int8)
code = np.zeros((p, 4 * bpr), np.uint8)
code[:, :n] = G8 + (G8 > 0)                               # 0 -> 00, 1 -> 10, 2 -> 11
code = code.reshape(p, bpr, 4)
bed = np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))
del code
W = np.concatenate([np.ones((n, 1), np.float32), rng.standard_normal((n, c - 1)).astype(np.float32)], axis=1)
y = (G8[:30].T.astype(np.float32) @ rng.standard_normal(30).astype(np.float32) + 2 * rng.standard_normal(n).astype(np.float32))
d = np.abs(rng.standard_normal(n)).astype(np.float32)

dW, dy, dd = ctx.to_device(W), ctx.to_device(y), ctx.to_device(d)
d8s = ctx.to_device(G8)                                    # int8 SNP-major (p x n)
d8m = ctx.to_device(np.ascontiguousarray(G8.T))            # int8 sample-major (n x p)
dbed = ctx.to_device(bed)
dfs = ctx.alloc(p * ldx * 4)                               # float32 SNP-major (p x ldx): also the block pg_score_dev reads
dfm = ctx.alloc(n * p * 4)                                 # float32 sample-major (n x p)
_lib.check(L.pg_cast_i8_f32_dev(ctx.handle, p, n, d8s.ptr, 0, n, dfs.ptr, ldx), "pg_cast_i8_f32_dev")
_lib.check(L.pg_transpose_dev(ctx.handle, p, n, dfs.ptr, ldx, dfm.ptr, p), "pg_transpose_dev")
work = ctx.alloc(L.pg_lm_work_bytes(n, c, t))
_lib.check(L.pg_lm_setup_dev(ctx.handle, n, c, t, dW.ptr, dy.ptr, n, work.ptr), "pg_lm_setup_dev")
res = ctx.alloc(32 * p)
r0 = res.ptr
lm_out = (r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0, r0 + 8 * p)      # beta, se, tau | F, p
M = 4096
dA, dB, dC = ctx.to_device(rng.standard_normal((M, M))), ctx.to_device(rng.standard_normal((M, M))), ctx.alloc(M * M * 8)   # random operands
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def lm_x(ptr, dtype, ldX, snp_major):
    return lambda: _lib.check(L.pg_lm_x_dev(ctx.handle, n, c, t, p, ptr, dtype, ldX, snp_major, work.ptr, *lm_out, p), "pg_lm_x_dev")


legs = {
    "f32_sample_major": (lm_x(dfm.ptr, 2, p, 0), 4.0 * n * p),
    "f32_snp_major": (lm_x(dfs.ptr, 2, ldx, 1), 4.0 * n * p),
    "i8_sample_major": (lm_x(d8m.ptr, 0, p, 0), 1.0 * n * p),
    "i8_snp_major": (lm_x(d8s.ptr, 0, n, 1), 1.0 * n * p),
    "bed": (lambda: _lib.check(L.pg_lm_bed_dev(ctx.handle, n, c, t, p, dbed.ptr, bpr, 0, work.ptr, *lm_out, p), "pg_lm_bed_dev"), 1.0 * bpr * p),
    "score_f32": (lambda: _lib.check(L.pg_score_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, 1.0, dfs.ptr, ldx, r0 + 16 * p, r0 + 20 * p,
                                                    r0 + 24 * p, r0 + 28 * p, r0, r0 + 8 * p), "pg_score_dev"), 4.0 * n * p),
    "dgemm_4096": (lambda: _lib.check(L.pgx_dgemm_dev(ctx.handle, 0, M, M, M, 1.0, dA.ptr, M, dB.ptr, M, 0.0, dC.ptr, M), "pgx_dgemm_dev"), 0.0),
}


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


for fn, _ in legs.values():      # warm-up: every launch shape once
    fn()
ctx.sync()
times = {k: [] for k in legs}
names = list(legs)
for r in range(a.reps):
    for k in (names if r % 2 == 0 else names[::-1]):
        times[k].append(timed(legs[k][0]))
dg_ms = float(np.median(times["dgemm_4096"]))
dg_tf = 2.0 * M ** 3 / (dg_ms * 1e-3) / 1e12
npanel = (c + t + 15) // 16 * 16
flops = 2.0 * ldx * npanel * p
out = {"tool": "bench_lm", "n": n, "p": p, "c": c, "t": t, "reps": a.reps,
       "dgemm_4096": {"ms": summary(times["dgemm_4096"]), "fp64_TFps": round(dg_tf, 2)}, "kernel": {}}
for k in names[:-1]:
    ms = float(np.median(times[k]))
    moved = legs[k][1] + (28.0 if k != "score_f32" else 32.0) * p
    row = {"ms": summary(times[k]), "bytes": int(moved), "achieved_TBps": round(moved / (ms * 1e-3) / 1e12, 3),
           "share_of_6.3": round(moved / (ms * 1e-3) / 6.3e12, 3), "hbm_roof_ms_at_6.3": round(moved / 6.3e12 * 1e3, 3)}
    if k != "score_f32":
        row.update({"fp64_TFps": round(flops / (ms * 1e-3) / 1e12, 2), "share_of_dgemm": round(flops / (ms * 1e-3) / 1e12 / dg_tf, 3),
                    "mfma_roof_ms_at_dgemm": round(flops / (dg_tf * 1e12) * 1e3, 3)})
    out["kernel"][k] = row
out["kernel"]["f32_snp_major_over_score"] = round(float(np.median(times["f32_snp_major"]) / np.median(times["score_f32"])), 3)
for b in (d8s, d8m, dbed, dfs, dfm, dA, dB, dC, res):
    b.free()
ctx.sync()

# ---- end to end: lmm.pygemma_lm against lmm.pygemma_score (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    pe = min(a.e2e_p, p)
    Xh = _lib.pinned_empty((n, pe), np.float32)
    for s0 in range(0, pe, 8192):
        Xh[:, s0:s0 + 8192] = G8[s0:min(pe, s0 + 8192)].T
    pb = PackedBed(bed[:pe], n)
    del G8
    K = lmm.kinship(Xh[:, :2000])
    Yh = y.astype(np.float64)
    for X in (Xh[:, :8192].copy(), PackedBed(bed[:8192], n)):       # warm-up of both paths (kernels, allocations)
        lmm.pygemma_lm(Yh, X, W)
        lmm.pygemma_score(Yh, X, W, K)
    out["e2e"] = {"p": pe}
    for tag, X in (("pinned_f32", Xh), ("packed_bed", pb)):
        e2e = {"lm": [], "score": []}
        for r in range(a.e2e_reps):
            pair = (("lm", lambda: lmm.pygemma_lm(Yh, X, W)), ("score", lambda: lmm.pygemma_score(Yh, X, W, K)))
            for name, fn in (pair if r % 2 == 0 else pair[::-1]):
                t0 = time.perf_counter()
                fn()
                e2e[name].append(time.perf_counter() - t0)
        out["e2e"][tag] = {"lm_s": summary(e2e["lm"]), "score_s": summary(e2e["score"]),
                           "ratio": round(float(np.median(e2e["lm"]) / np.median(e2e["score"])), 3)}
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
