"""Principal components from genotypes (pg_pca_{stat,proj,back}_bed_dev, lmm.pca) on one GPU.

At n = 10 000, p = 100 000 packed hard calls of three Balding-Nichols populations (F_st = 0.1), in one process:
  kernel:  device-event time of T = Z'Q (proj), of Y += Z T (back) and of both (a pass) over the device-resident records in kernel calls
           of 16 384 SNPs (the feed's batch) and of 65 536 (what lmm.pca takes from a resident source), for l = 20 and l = 64
           columns; each as a share of the fp64 matrix peak (78.6 TF) from the 2 n p l flops a product needs.
           pg_pca_stat_bed_dev on the same records alongside.
  e2e:     wall time of lmm.pca(k = 10) at l = 20 and l = 64 from a pinned PackedBed, alternating with the route it replaces on the
           same panel: lmm.kinship (streamed, fp16 matrix pipe) plus the eigensolver (ops.syevd); and how far the two routes' top
           eigenvalues lie apart (K is float32 there).
  streamed: one lmm.pca run at n = 50 000 with snp_batch given, so that every pass rides the two-slot feed.
Prints one JSON line (median, min, max of the repeats); --out also writes it to a file (profiles/pca_bench.json).
usage: bench_pca.py [--n N] [--p P] [--reps R] [--e2e-reps R] [--stream-n N] [--stream-p P] [--out path]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygemma_amd import _lib, lmm, ops  # noqa: E402
from pygemma_amd.bed import PackedBed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--stream-n", type=int, default=50000)
ap.add_argument("--stream-p", type=int, default=40000)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p = a.n, a.p
LS, K, BATCHES, STREAM_BATCH, PEAK = (20, 64), 10, (16384, 65536), 16384, 78.6e12
bpr = (n + 3) // 4


def note(msg):
    print(f"[bench_pca] {msg}", file=sys.stderr, flush=True)


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


def packed(G8):
    """(pb, n) int8 codes 0/1/2 -> (pb, ceil(n/4)) .bed records."""
    pb, m = G8.shape
    code = np.zeros((pb, 4 * ((m + 3) // 4)), np.uint8)
    code[:, :m] = G8 + (G8 > 0)                               # 0 -> 00, 1 -> 10, 2 -> 11
    code = code.reshape(pb, -1, 4)
    return code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)


def structured_bed(n, p, seed):
    """Pinned records of three Balding-Nichols populations: ancestral frequencies U(0.1, 0.9), F_st = 0.1."""
    rng = np.random.default_rng(seed)
    rec = _lib.pinned_empty((p, (n + 3) // 4), np.uint8)
    pop = np.arange(n) * 3 // n
    for s0 in range(0, p, 8192):
        e0 = min(p, s0 + 8192)
        f = rng.uniform(0.1, 0.9, e0 - s0)
        thr = rng.beta(f * 9.0, (1 - f) * 9.0, (3, e0 - s0)).astype(np.float32).T[:, pop]
        u = rng.random((2, e0 - s0, n), dtype=np.float32)
        rec[s0:e0] = packed((u[0] < thr).astype(np.int8) + (u[1] < thr).astype(np.int8))
    return rec


def random_bed(n, p, seed):
    """Pinned records of unstructured calls, made from random bytes: the field 01 ('missing') becomes 00."""
    rng = np.random.default_rng(seed)
    lut = np.arange(256, dtype=np.uint8)
    for sh in (0, 2, 4, 6):
        lut = np.where((lut >> sh) & 3 == 1, lut & ~np.uint8(3 << sh), lut).astype(np.uint8)
    rec = _lib.pinned_empty((p, (n + 3) // 4), np.uint8)
    for s0 in range(0, p, 8192):
        e0 = min(p, s0 + 8192)
        rec[s0:e0] = lut[rng.integers(0, 256, (e0 - s0, rec.shape[1]), dtype=np.uint8)]
    return rec


L = _lib.load()
rec = structured_bed(n, p, 5)
note("host records made")
out = {"tool": "bench_pca", "n": n, "p": p, "k": K, "reps": a.reps, "fp64_matrix_peak_TF": PEAK / 1e12, "kernel": {}}

# ---- kernels on device-resident records ----------------------------------------------------------------------------------------------
ctx = _lib.Context(0)
dbed = ctx.to_device(rec)
lmax = max(LS)
work = ctx.alloc(L.pg_pca_work_bytes(n, min(p, max(BATCHES)), lmax))
dstat, dT, dQ, dY = ctx.alloc(16 * p), ctx.alloc(8 * lmax * p), ctx.alloc(8 * lmax * n), ctx.alloc(8 * lmax * n)
dQ.upload(np.linalg.qr(np.random.default_rng(0).standard_normal((n, lmax)))[0].T.copy())
_lib.check(L.pg_memset(ctx.handle, dY.ptr, 0, 8 * lmax * n), "pg_memset")
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")
WIN = {b: [(s, min(s + b, p)) for s in range(0, p, b)] for b in BATCHES}


def stat(b=BATCHES[0]):
    for s, e in WIN[b]:
        _lib.check(L.pg_pca_stat_bed_dev(ctx.handle, n, e - s, dbed.ptr + s * bpr, bpr, 0, work.ptr, dstat.ptr + 16 * s), "pg_pca_stat_bed_dev")


def proj(l, b):
    for s, e in WIN[b]:
        _lib.check(L.pg_pca_proj_bed_dev(ctx.handle, n, e - s, dbed.ptr + s * bpr, bpr, 0, dstat.ptr + 16 * s, l, dQ.ptr, n, dT.ptr + 8 * s, p),
                   "pg_pca_proj_bed_dev")


def back(l, b):
    for s, e in WIN[b]:
        _lib.check(L.pg_pca_back_bed_dev(ctx.handle, n, e - s, dbed.ptr + s * bpr, bpr, 0, dstat.ptr + 16 * s, l, dT.ptr + 8 * s, p, work.ptr, dY.ptr, n),
                   "pg_pca_back_bed_dev")


def both(l, b):
    for s, e in WIN[b]:        # as lmm.pca enqueues a pass: both products of a batch before the next
        _lib.check(L.pg_pca_proj_bed_dev(ctx.handle, n, e - s, dbed.ptr + s * bpr, bpr, 0, dstat.ptr + 16 * s, l, dQ.ptr, n, dT.ptr + 8 * s, p),
                   "pg_pca_proj_bed_dev")
        _lib.check(L.pg_pca_back_bed_dev(ctx.handle, n, e - s, dbed.ptr + s * bpr, bpr, 0, dstat.ptr + 16 * s, l, dT.ptr + 8 * s, p, work.ptr, dY.ptr, n),
                   "pg_pca_back_bed_dev")


def timed(fn):
    L.pg_event_record(ctx.handle, evs[0])
    fn()
    L.pg_event_record(ctx.handle, evs[1])
    ms = C.c_float()
    _lib.check(L.pg_event_elapsed_ms(ctx.handle, evs[0], evs[1], C.byref(ms)), "pg_event_elapsed_ms")
    return ms.value


cases = [(name, fn, l, b) for b in BATCHES for l in LS for name, fn in (("proj", proj), ("back", back), ("pass", both))]
stat()
for name, fn, l, b in cases:               # warm-up: every launch shape once
    fn(l, b)
ctx.sync()
times, t_stat = {(name, l, b): [] for name, _, l, b in cases}, []
for r in range(a.reps):
    for name, fn, l, b in (cases if r % 2 == 0 else cases[::-1]):
        times[(name, l, b)].append(timed(lambda: fn(l, b)))
    t_stat.append(timed(stat))
out["kernel"]["stat_ms"] = summary(t_stat)
for b in BATCHES:                          # SNPs per kernel call: the feed's batch, and what lmm.pca takes from a resident source
    for l in LS:
        row = {}
        for name, products in (("proj", 1), ("back", 1), ("pass", 2)):
            ms = float(np.median(times[(name, l, b)]))
            row[f"{name}_ms"] = summary(times[(name, l, b)])
            row[f"{name}_share_of_peak"] = round(products * 2.0 * n * p * l / (ms * 1e-3) / PEAK, 4)
        out["kernel"][f"l{l}_batch{b}"] = row
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
note("kernel legs timed")

# ---- end to end: lmm.pca against lmm.kinship + the eigensolver on the same panel -----------------------------------------------------------
if a.e2e_reps > 0:
    src = PackedBed(rec, n)
    warm = PackedBed(np.ascontiguousarray(rec[:4096]), n)
    lmm.pca(warm, K, iters=2)
    ops.syevd(lmm.kinship(warm))

    def kinship_route():
        w = ops.syevd(lmm.kinship(src))[0]
        return np.sort(w.astype(np.float64))[::-1][:K]

    runs = {f"pca_l{l}": [] for l in LS}
    runs["kinship_eigh"] = []
    stats, lam = {}, {}
    for r in range(a.e2e_reps):
        legs = [(f"pca_l{l}", (lambda l=l: lmm.pca(src, K, oversample=l - K, stats=stats.setdefault(l, {})).eigenvalues)) for l in LS]
        legs.append(("kinship_eigh", kinship_route))
        for name, fn in (legs if r % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            lam[name] = fn()
            runs[name].append(time.perf_counter() - t0)
    e2e = {name: summary(ts) for name, ts in runs.items()}
    for l in LS:
        st = stats[l]
        e2e[f"pca_l{l}_stats"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items()}
        # per component: the structured ones converge, those inside the bulk (no gap) are what 12 passes leave of them
        e2e[f"pca_l{l}_eigenvalues_vs_kinship_route_rel"] = [float(f"{v:.2e}") for v in np.abs(lam[f"pca_l{l}"] - lam["kinship_eigh"]) / lam["kinship_eigh"]]
    e2e["top_eigenvalues"] = [round(float(v), 4) for v in lam[f"pca_l{LS[0]}"]]
    e2e["top_eigenvalues_kinship_route"] = [round(float(v), 4) for v in lam["kinship_eigh"]]
    ratio = float(np.median(runs["kinship_eigh"]) / np.median(runs[f"pca_l{LS[0]}"]))
    e2e["kinship_eigh_over_pca_l20"] = round(ratio, 2)
    e2e["pca_is_faster"] = bool(ratio > 1)
    out["e2e"] = e2e
    note("end-to-end legs timed")
del rec

# ---- one streamed run at a larger n -----------------------------------------------------------------------------------------------------
if a.stream_n > 0:
    big = PackedBed(random_bed(a.stream_n, a.stream_p, 6), a.stream_n)
    note("streamed panel made")
    st = {}
    t0 = time.perf_counter()
    res = lmm.pca(big, K, snp_batch=STREAM_BATCH, loadings=False, stats=st)
    out["streamed"] = {"n": a.stream_n, "p": a.stream_p, "l": 20, "snp_batch": STREAM_BATCH, "wall_s": round(time.perf_counter() - t0, 3),
                       "stats": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items()},
                       "lambda_1": round(float(res.eigenvalues[0]), 4)}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
