"""Polygenic scores (pg_prs_x_acc_dev / pg_prs_bed_acc_dev, lmm.prs) on one GPU.

At n = 10 000, p = 100 000 hard-call SNPs resident, alternating in one process:
  kernel:  device-event time of one score call (impute = 1: the pre-pass included) on device-resident packed .bed records, int8 and
           float32 blocks in both orders, for t = 1, 16 and 64 weight columns, with and without `called`, each next to
           pg_snp_stats_* on the same block: the pure-read yardstick.  For each leg the fp64 matrix flops it issues — 2 n p t per
           product over whole 16-column tiles — over its time, and the bytes of the block over its time.
  e2e:     wall time of lmm.prs (t = 16, counts) against lmm.snp_stats(hwe=False) from the same pinned float32 X and from the same
           PackedBed: both ride the same feed, so the ratio shows whether the score hides behind the transport.
Prints one JSON line (median, min, max of the repeats); --out also writes it to a file (profiles/prs_bench.json).
usage: bench_prs.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
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
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--e2e-reps", type=int, default=7)
ap.add_argument("--e2e-p", type=int, default=100000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p = a.n, a.p
TS = (1, 16, 64)
L = _lib.load()
ctx = _lib.Context(0)
ldx = (n + 63) // 64 * 64
bpr = (n + 3) // 4
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_prs] {msg}", file=sys.stderr, flush=True)


# ---- inputs: genotype codes, SNP-major int8 on the host; every other image of the block is made from it (as tools/bench_snp_stats.py)
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
Wt = rng.standard_normal((max(TS), p))                    # score-major weights: column k at Wt[k p + g]

note("host genotypes made")
dWt = ctx.to_device(Wt)
d8s = ctx.to_device(G8)                                    # int8 SNP-major (p x n)
d8m = ctx.to_device(np.ascontiguousarray(G8.T))            # int8 sample-major (n x p)
dbed = ctx.to_device(bed)
dfs = ctx.alloc(p * ldx * 4)                               # float32 SNP-major (p x ldx)
dfm = ctx.alloc(n * p * 4)                                 # float32 sample-major (n x p)
_lib.check(L.pg_cast_i8_f32_dev(ctx.handle, p, n, d8s.ptr, 0, n, dfs.ptr, ldx), "pg_cast_i8_f32_dev")
_lib.check(L.pg_transpose_dev(ctx.handle, p, n, dfs.ptr, ldx, dfm.ptr, p), "pg_transpose_dev")
work = ctx.alloc(L.pg_prs_work_bytes(n, p, max(TS)))
swork = ctx.alloc(L.pg_snp_stats_work_bytes(n, p))
dcnt, dmom = ctx.alloc(32 * p), ctx.alloc(32 * p)
dS, dC = ctx.alloc(8 * max(TS) * n), ctx.alloc(8 * max(TS) * n)
for b in (dS, dC):
    _lib.check(L.pg_memset(ctx.handle, b.ptr, 0, 8 * max(TS) * n), "pg_memset")
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def prs_x(ptr, dtype, ldX, snp_major):
    return lambda t, cn: _lib.check(L.pg_prs_x_acc_dev(ctx.handle, n, p, ptr, dtype, ldX, snp_major, t, dWt.ptr, p, 1, work.ptr, dS.ptr,
                                                       dC.ptr if cn else None, n), "pg_prs_x_acc_dev")


def st_x(ptr, dtype, ldX, snp_major):
    return lambda: _lib.check(L.pg_snp_stats_x_dev(ctx.handle, n, p, ptr, dtype, ldX, snp_major, swork.ptr, dcnt.ptr, dmom.ptr), "pg_snp_stats_x_dev")


# leg -> (score call (t, with counts), the statistics call on the same block, bytes of the block)
legs = {
    "bed": (lambda t, cn: _lib.check(L.pg_prs_bed_acc_dev(ctx.handle, n, p, dbed.ptr, bpr, 0, t, dWt.ptr, p, 1, work.ptr, dS.ptr,
                                                          dC.ptr if cn else None, n), "pg_prs_bed_acc_dev"),
            lambda: _lib.check(L.pg_snp_stats_bed_dev(ctx.handle, n, p, dbed.ptr, bpr, 0, swork.ptr, dcnt.ptr, dmom.ptr), "pg_snp_stats_bed_dev"),
            1.0 * bpr * p),
    "i8_snp_major": (prs_x(d8s.ptr, 0, n, 1), st_x(d8s.ptr, 0, n, 1), 1.0 * n * p),
    "i8_sample_major": (prs_x(d8m.ptr, 0, p, 0), st_x(d8m.ptr, 0, p, 0), 1.0 * n * p),
    "f32_snp_major": (prs_x(dfs.ptr, 2, ldx, 1), st_x(dfs.ptr, 2, ldx, 1), 4.0 * n * p),
    "f32_sample_major": (prs_x(dfm.ptr, 2, p, 0), st_x(dfm.ptr, 2, p, 0), 4.0 * n * p),
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


note("device blocks made")
cases = [(k, t, cn) for k in legs for t in TS for cn in (0, 1)]
for k, t, cn in cases:                     # warm-up: every launch shape once
    legs[k][0](t, cn)
for k in legs:
    legs[k][1]()
ctx.sync()
times = {c: [] for c in cases}
t_stats = {k: [] for k in legs}
for r in range(a.reps):
    for c in (cases if r % 2 == 0 else cases[::-1]):
        k, t, cn = c
        times[c].append(timed(lambda: legs[k][0](t, cn)))
    for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
        t_stats[k].append(timed(legs[k][1]))
out = {"tool": "bench_prs", "n": n, "p": p, "reps": a.reps, "kernel": {}}
for k in legs:
    st_ms = float(np.median(t_stats[k]))
    row = {"block_bytes": int(legs[k][2]), "snp_stats_ms": summary(t_stats[k]), "read_TBps_of_snp_stats": round(legs[k][2] / (st_ms * 1e-3) / 1e12, 3)}
    for t in TS:
        for cn in (0, 1):
            ms = float(np.median(times[(k, t, cn)]))
            flops = 2.0 * n * p * (-(-t // 16) * 16) * (2 if cn else 1)
            row[f"t{t}_{'called' if cn else 'score'}"] = {
                "ms": summary(times[(k, t, cn)]), "over_snp_stats": round(ms / st_ms, 2),
                "matrix_TFLOPs": round(flops / (ms * 1e-3) / 1e12, 2), "block_TBps": round(legs[k][2] / (ms * 1e-3) / 1e12, 3)}
    out["kernel"][k] = row
for b in (d8s, d8m, dbed, dfs, dfm, work, swork, dcnt, dmom, dS, dC, dWt):
    b.free()
ctx.sync()

note("kernel legs timed")

# ---- end to end: lmm.prs against lmm.snp_stats on the same sources (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    pe = min(a.e2e_p, p)
    Xh = _lib.pinned_empty((n, pe), np.float32)
    for s0 in range(0, pe, 8192):
        Xh[:, s0:s0 + 8192] = G8[s0:min(pe, s0 + 8192)].T
    rec = _lib.pinned_empty((pe, bpr), np.uint8)
    rec[:] = bed[:pe]
    pb = PackedBed(rec, n)
    del G8
    Wh = np.ascontiguousarray(Wt[:16, :pe].T)
    for X in (Xh[:, :8192].copy(), PackedBed(bed[:8192], n)):       # warm-up of both paths (kernels, allocations)
        lmm.snp_stats(X, hwe=False)
        lmm.prs(X, Wh[:8192], counts=True)
    out["e2e"] = {"p": pe, "t": 16}
    for tag, X in (("pinned_f32", Xh), ("packed_bed", pb)):
        e2e = {"prs": [], "stats": []}
        for r in range(a.e2e_reps):
            pair = (("prs", lambda: lmm.prs(X, Wh, counts=True)), ("stats", lambda: lmm.snp_stats(X, hwe=False)))
            for name, fn in (pair if r % 2 == 0 else pair[::-1]):
                t0 = time.perf_counter()
                fn()
                e2e[name].append(time.perf_counter() - t0)
        st = np.asarray(e2e["stats"])
        out["e2e"][tag] = {"prs_s": summary(e2e["prs"]), "stats_s": summary(e2e["stats"]),
                           "ratio": round(float(np.median(e2e["prs"]) / np.median(st)), 3),
                           "stats_spread": round(float((st.max() - st.min()) / np.median(st)), 3)}
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
