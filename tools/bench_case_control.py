"""Case/control tests (pg_cc_count_dev, pg_cc_pack_x_dev, pg_cc_stats_dev, lmm.case_control) on one GPU.

At n = 10 000, p = 100 000 hard-call SNPs resident, alternating in one process:
  kernel:  device-event time of pg_cc_count_dev on a packed .bed block at S = 1, 4 and 16 strata, and of pg_cc_pack_x_dev +
           pg_cc_count_dev (S = 1) on float32 (both orders) and int8 (both orders) blocks, each next to pg_snp_stats_*_dev (the pure-read
           yardstick) and the linear-model scan (pg_lm_x_dev / pg_lm_bed_dev, c = 5, t = 1) on the same block.  The scan reads the same
           bytes and also drives the fp64 matrix pipe, so an S = 1 leg slower than it is a defect (`not_slower_than_lm`; the tool exits 1
           when a leg fails it).  The S = 4 and S = 16 ratios to pg_snp_stats_bed_dev are recorded, not gated.
           pg_cc_stats_dev on the p rows of counts, with and without the exact test.
  e2e:     wall time of lmm.case_control next to lmm.snp_stats from a PackedBed and from pinned float32 X.
Prints one JSON line (median, min, max of the repeats); --out also writes it to a file.
usage: bench_case_control.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
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
K = _lib.load_cc()
ctx = _lib.Context(0)
ldx = (n + 63) // 64 * 64
bpr = (n + 3) // 4
ldb = (bpr + 15) // 16 * 16                                # the pitch lmm.case_control packs an array batch at
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_case_control] {msg}", file=sys.stderr, flush=True)


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
W = np.concatenate([np.ones((n, 1), np.float32), rng.standard_normal((n, c - 1)).astype(np.float32)], axis=1)
liab = G8[:30].T.astype(np.float32) @ rng.standard_normal(30).astype(np.float32) + 2 * rng.standard_normal(n).astype(np.float32)
y = (liab > np.median(liab)).astype(np.float32)            # the 0/1 trait, also the linear model's phenotype
status = y.astype(np.int8)

note("host genotypes made")
dW, dy = ctx.to_device(W), ctx.to_device(y)
d8s = ctx.to_device(G8)                                    # int8 SNP-major (p x n)
d8m = ctx.to_device(np.ascontiguousarray(G8.T))            # int8 sample-major (n x p)
dbed = ctx.to_device(bed)
dfs = ctx.alloc(p * ldx * 4)                               # float32 SNP-major (p x ldx)
dfm = ctx.alloc(n * p * 4)                                 # float32 sample-major (n x p)
_lib.check(L.pg_cast_i8_f32_dev(ctx.handle, p, n, d8s.ptr, 0, n, dfs.ptr, ldx), "pg_cast_i8_f32_dev")
_lib.check(L.pg_transpose_dev(ctx.handle, p, n, dfs.ptr, ldx, dfm.ptr, p), "pg_transpose_dev")
work = ctx.alloc(L.pg_lm_work_bytes(n, c, t))
_lib.check(L.pg_lm_setup_dev(ctx.handle, n, c, t, dW.ptr, dy.ptr, n, work.ptr), "pg_lm_setup_dev")
res = ctx.alloc(32 * p)
r0 = res.ptr
lm_out = (r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0, r0 + 8 * p)      # beta, se, tau | F, p
swork = ctx.alloc(L.pg_snp_stats_work_bytes(n, p))
dcnt, dmom = ctx.alloc(32 * p), ctx.alloc(32 * p)
dstat, dstr = ctx.to_device(status), {}
cwork = {}
for S in (1, 4, 16):                                       # the strata: samples dealt out at random
    cwork[S] = ctx.alloc(K.pg_cc_work_bytes(n, S))
    dstr[S] = ctx.to_device(rng.integers(0, S, n).astype(np.int32))
    _lib.check(K.pg_cc_setup_dev(ctx.handle, n, S, dstat.ptr, dstr[S].ptr, cwork[S].ptr), "pg_cc_setup_dev")
drec, dhard = ctx.alloc(p * ldb), ctx.alloc(p)
dcc, dcmh, dst = ctx.alloc(64 * p), ctx.alloc(32 * p), ctx.alloc(88 * p)
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def lm_x(ptr, dtype, ldX, snp_major):
    return lambda: _lib.check(L.pg_lm_x_dev(ctx.handle, n, c, t, p, ptr, dtype, ldX, snp_major, work.ptr, *lm_out, p), "pg_lm_x_dev")


def st_x(ptr, dtype, ldX, snp_major):
    return lambda: _lib.check(L.pg_snp_stats_x_dev(ctx.handle, n, p, ptr, dtype, ldX, snp_major, swork.ptr, dcnt.ptr, dmom.ptr), "pg_snp_stats_x_dev")


def cc_bed(S):
    return lambda: _lib.check(K.pg_cc_count_dev(ctx.handle, n, p, dbed.ptr, bpr, 0, S, cwork[S].ptr, None, dcc.ptr, dcmh.ptr), "pg_cc_count_dev")


def cc_x(ptr, dtype, ldX, snp_major):
    def run():
        _lib.check(K.pg_cc_pack_x_dev(ctx.handle, n, p, ptr, dtype, ldX, snp_major, drec.ptr, ldb, dhard.ptr), "pg_cc_pack_x_dev")
        _lib.check(K.pg_cc_count_dev(ctx.handle, n, p, drec.ptr, ldb, 0, 1, cwork[1].ptr, dhard.ptr, dcc.ptr, dcmh.ptr), "pg_cc_count_dev")
    return run


st_bed = lambda: _lib.check(L.pg_snp_stats_bed_dev(ctx.handle, n, p, dbed.ptr, bpr, 0, swork.ptr, dcnt.ptr, dmom.ptr), "pg_snp_stats_bed_dev")      # noqa: E731
lm_bed = lambda: _lib.check(L.pg_lm_bed_dev(ctx.handle, n, c, t, p, dbed.ptr, bpr, 0, work.ptr, *lm_out, p), "pg_lm_bed_dev")      # noqa: E731
# leg -> (case/control call, pg_snp_stats on the same block, the linear-model call on it, bytes read, bytes written, gated)
legs = {
    "bed_S1": (cc_bed(1), st_bed, lm_bed, 1.0 * bpr * p, 96.0 * p, True),
    "bed_S4": (cc_bed(4), st_bed, lm_bed, 1.0 * bpr * p, 96.0 * p, False),
    "bed_S16": (cc_bed(16), st_bed, lm_bed, 1.0 * bpr * p, 96.0 * p, False),
    "f32_sample_major": (cc_x(dfm.ptr, 2, p, 0), st_x(dfm.ptr, 2, p, 0), lm_x(dfm.ptr, 2, p, 0), 4.0 * n * p + ldb * p, 97.0 * p + ldb * p, True),
    "f32_snp_major": (cc_x(dfs.ptr, 2, ldx, 1), st_x(dfs.ptr, 2, ldx, 1), lm_x(dfs.ptr, 2, ldx, 1), 4.0 * n * p + ldb * p, 97.0 * p + ldb * p, True),
    "i8_sample_major": (cc_x(d8m.ptr, 0, p, 0), st_x(d8m.ptr, 0, p, 0), lm_x(d8m.ptr, 0, p, 0), 1.0 * n * p + ldb * p, 97.0 * p + ldb * p, True),
    "i8_snp_major": (cc_x(d8s.ptr, 0, n, 1), st_x(d8s.ptr, 0, n, 1), lm_x(d8s.ptr, 0, n, 1), 1.0 * n * p + ldb * p, 97.0 * p + ldb * p, True),
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


def stats_dev(fisher):
    return lambda: _lib.check(K.pg_cc_stats_dev(ctx.handle, p, dcc.ptr, dcmh.ptr, fisher, dst.ptr), "pg_cc_stats_dev")


note("device blocks made")
for leg in legs.values():                  # warm-up: every launch shape once
    for fn in leg[:3]:
        fn()
legs["bed_S1"][0]()                        # the counts pg_cc_stats_dev is timed on
stats_dev(1)()
ctx.sync()
# the packed block through both routes gives the same counts
ref = dcc.download((p, 8), np.int64)
legs["f32_snp_major"][0]()
ctx.sync()
assert (dcc.download((p, 8), np.int64) == ref).all() and dhard.download((p,), np.uint8).all(), "packed float32 block: counts differ from the records'"
times = {k: {"cc": [], "stats": [], "lm": []} for k in legs}
t_stat = {0: [], 1: []}
names = list(legs)
for r in range(a.reps):
    for k in (names if r % 2 == 0 else names[::-1]):
        trio = list(zip(("cc", "stats", "lm"), legs[k][:3]))
        for which, fn in (trio if r % 2 == 0 else trio[::-1]):        # alternated: the order inside a trio flips too
            times[k][which].append(timed(fn))
    legs["bed_S1"][0]()
    for f in (0, 1):
        t_stat[f].append(timed(stats_dev(f)))
out = {"tool": "bench_case_control", "n": n, "p": p, "c": c, "t": t, "reps": a.reps, "kernel": {}}
ok = True
for k in names:
    ms, st_ms, lm_ms = (float(np.median(times[k][w])) for w in ("cc", "stats", "lm"))
    moved = legs[k][3] + legs[k][4]
    row = {"cc_ms": summary(times[k]["cc"]), "snp_stats_ms": summary(times[k]["stats"]), "lm_ms": summary(times[k]["lm"]), "bytes": int(moved),
           "achieved_TBps": round(moved / (ms * 1e-3) / 1e12, 3), "share_of_6.3": round(moved / (ms * 1e-3) / 6.3e12, 3),
           "cc_over_snp_stats": round(ms / st_ms, 3), "cc_over_lm": round(ms / lm_ms, 3)}
    if legs[k][5]:
        row["not_slower_than_lm"] = bool(ms <= lm_ms)
        ok = ok and ms <= lm_ms
    out["kernel"][k] = row
out["stats_dev"] = {"rows": p, "ms": summary(t_stat[0]), "ms_with_fisher": summary(t_stat[1])}
out["every_S1_leg_not_slower_than_lm"] = bool(ok)
for b in (d8s, d8m, dbed, dfs, dfm, res, swork, dcnt, dmom, drec, dhard, dcc, dcmh, dst):
    b.free()
ctx.sync()

note("kernel legs timed")

# ---- end to end: lmm.case_control against lmm.snp_stats (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    pe = min(a.e2e_p, p)
    Xh = _lib.pinned_empty((n, pe), np.float32)
    for s0 in range(0, pe, 8192):
        Xh[:, s0:s0 + 8192] = G8[s0:min(pe, s0 + 8192)].T
    pb = PackedBed(bed[:pe], n)
    del G8
    yh = y.astype(np.float64)
    for X in (Xh[:, :8192].copy(), PackedBed(bed[:8192], n)):       # warm-up of both paths (kernels, allocations)
        lmm.case_control(X, yh)
        lmm.snp_stats(X)
    out["e2e"] = {"p": pe}
    for tag, X in (("pinned_f32", Xh), ("packed_bed", pb)):
        e2e = {"cc": [], "stats": []}
        for r in range(a.e2e_reps):
            pair = (("cc", lambda: lmm.case_control(X, yh)), ("stats", lambda: lmm.snp_stats(X)))
            for name, fn in (pair if r % 2 == 0 else pair[::-1]):
                t0 = time.perf_counter()
                fn()
                e2e[name].append(time.perf_counter() - t0)
        out["e2e"][tag] = {"case_control_s": summary(e2e["cc"]), "snp_stats_s": summary(e2e["stats"]),
                           "ratio": round(float(np.median(e2e["cc"]) / np.median(e2e["stats"])), 3)}
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
