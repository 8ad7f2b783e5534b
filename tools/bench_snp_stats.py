"""SNP statistics (pg_snp_stats_x_dev / pg_snp_stats_bed_dev, pg_hwe_exact_dev, lmm.snp_stats) on one GPU.

At n = 10 000, p = 100 000 hard-call SNPs resident, alternating in one process:
  kernel:  device-event time of one statistics call on device-resident float32 sample-major, float32 SNP-major, int8 (both orders)
           and packed .bed blocks, each next to the linear-model scan (pg_lm_x_dev / pg_lm_bed_dev, c = 5, t = 1, p-values included)
           on the same block: the scan reads the same bytes and also runs the fp64 matrix pipe, so a QC pass slower than it is a
           defect (`not_slower_than_lm`; the tool exits 1 when a leg fails it).  For each leg the bytes it must move — the block read
           once and 64 p of outputs — over its time, as a share of 6.3 TB/s;
           the same for float32 dosage blocks (genotype plus noise: every SNP takes the second sweep), both orders;
           pg_hwe_exact_dev on the p rows of counts.
  e2e:     wall time of lmm.snp_stats against lmm.pygemma_lm from pinned float32 X and from a PackedBed.
Prints one JSON line (median, min, max of the repeats); --out also writes it to a file.
usage: bench_snp_stats.py [--reps R] [--e2e-reps R] [--e2e-p P] [--out path]"""
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


def note(msg):
    print(f"[bench_snp_stats] {msg}", file=sys.stderr, flush=True)


# ---- inputs: genotype codes, SNP-major int8 on the host; every other image of the block is made from it (as tools/bench_lm.py)
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

note("host genotypes made")
dW, dy = ctx.to_device(W), ctx.to_device(y)
d8s = ctx.to_device(G8)                                    # int8 SNP-major (p x n)
d8m = ctx.to_device(np.ascontiguousarray(G8.T))            # int8 sample-major (n x p)
dbed = ctx.to_device(bed)
dfs = ctx.alloc(p * ldx * 4)                               # float32 SNP-major (p x ldx)
dfm = ctx.alloc(n * p * 4)                                 # float32 sample-major (n x p)
_lib.check(L.pg_cast_i8_f32_dev(ctx.handle, p, n, d8s.ptr, 0, n, dfs.ptr, ldx), "pg_cast_i8_f32_dev")
_lib.check(L.pg_transpose_dev(ctx.handle, p, n, dfs.ptr, ldx, dfm.ptr, p), "pg_transpose_dev")
dds = ctx.alloc(p * ldx * 4)                               # float32 dosages SNP-major: the calls plus noise of sd 0.1
dos = np.zeros((8192, ldx), np.float32)
noise = (0.1 * rng.standard_normal((8192 + 64, n))).astype(np.float32)
for k, s0 in enumerate(range(0, p, 8192)):
    e0 = min(p, s0 + 8192)
    np.add(G8[s0:e0], noise[k % 64:k % 64 + e0 - s0], out=dos[:e0 - s0, :n])
    _lib.check(L.pg_memcpy_h2d(ctx.handle, dds.ptr + s0 * ldx * 4, dos.ctypes.data, (e0 - s0) * ldx * 4), "pg_memcpy_h2d")
del dos, noise
ddm = ctx.alloc(n * p * 4)                                 # ... and sample-major
_lib.check(L.pg_transpose_dev(ctx.handle, p, n, dds.ptr, ldx, ddm.ptr, p), "pg_transpose_dev")
work = ctx.alloc(L.pg_lm_work_bytes(n, c, t))
_lib.check(L.pg_lm_setup_dev(ctx.handle, n, c, t, dW.ptr, dy.ptr, n, work.ptr), "pg_lm_setup_dev")
res = ctx.alloc(32 * p)
r0 = res.ptr
lm_out = (r0 + 16 * p, r0 + 20 * p, r0 + 24 * p, r0, r0 + 8 * p)      # beta, se, tau | F, p
swork = ctx.alloc(L.pg_snp_stats_work_bytes(n, p))
dcnt, dmom, dhwe = ctx.alloc(32 * p), ctx.alloc(32 * p), ctx.alloc(8 * p)
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def lm_x(ptr, dtype, ldX, snp_major):
    return lambda: _lib.check(L.pg_lm_x_dev(ctx.handle, n, c, t, p, ptr, dtype, ldX, snp_major, work.ptr, *lm_out, p), "pg_lm_x_dev")


def st_x(ptr, dtype, ldX, snp_major):
    return lambda: _lib.check(L.pg_snp_stats_x_dev(ctx.handle, n, p, ptr, dtype, ldX, snp_major, swork.ptr, dcnt.ptr, dmom.ptr), "pg_snp_stats_x_dev")


# leg -> (statistics call, the linear-model call on the same block or None, bytes of the block)
legs = {
    "f32_sample_major": (st_x(dfm.ptr, 2, p, 0), lm_x(dfm.ptr, 2, p, 0), 4.0 * n * p),
    "f32_snp_major": (st_x(dfs.ptr, 2, ldx, 1), lm_x(dfs.ptr, 2, ldx, 1), 4.0 * n * p),
    "i8_sample_major": (st_x(d8m.ptr, 0, p, 0), lm_x(d8m.ptr, 0, p, 0), 1.0 * n * p),
    "i8_snp_major": (st_x(d8s.ptr, 0, n, 1), lm_x(d8s.ptr, 0, n, 1), 1.0 * n * p),
    "bed": (lambda: _lib.check(L.pg_snp_stats_bed_dev(ctx.handle, n, p, dbed.ptr, bpr, 0, swork.ptr, dcnt.ptr, dmom.ptr), "pg_snp_stats_bed_dev"),
            lambda: _lib.check(L.pg_lm_bed_dev(ctx.handle, n, c, t, p, dbed.ptr, bpr, 0, work.ptr, *lm_out, p), "pg_lm_bed_dev"), 1.0 * bpr * p),
    "f32_dosage_sample_major": (st_x(ddm.ptr, 2, p, 0), None, 4.0 * n * p),
    "f32_dosage_snp_major": (st_x(dds.ptr, 2, ldx, 1), None, 4.0 * n * p),
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


def hwe():
    _lib.check(L.pg_hwe_exact_dev(ctx.handle, n, p, dcnt.ptr, dhwe.ptr), "pg_hwe_exact_dev")


note("device blocks made")
for st_fn, lm_fn, _ in legs.values():      # warm-up: every launch shape once
    st_fn()
    if lm_fn:
        lm_fn()
legs["bed"][0]()                           # the counts pg_hwe_exact_dev is timed on: the hard calls
hwe()
ctx.sync()
times = {k: {"stats": [], "lm": []} for k in legs}
t_hwe = []
names = list(legs)
for r in range(a.reps):
    for k in (names if r % 2 == 0 else names[::-1]):
        st_fn, lm_fn, _ = legs[k]
        pair = [("stats", st_fn)] + ([("lm", lm_fn)] if lm_fn else [])
        for which, fn in (pair if r % 2 == 0 else pair[::-1]):       # alternated: the order inside a pair flips too
            times[k][which].append(timed(fn))
    legs["bed"][0]()
    t_hwe.append(timed(hwe))
out = {"tool": "bench_snp_stats", "n": n, "p": p, "c": c, "t": t, "reps": a.reps, "kernel": {}}
ok = True
for k in names:
    ms = float(np.median(times[k]["stats"]))
    moved = legs[k][2] + 64.0 * p
    row = {"stats_ms": summary(times[k]["stats"]), "bytes": int(moved), "achieved_TBps": round(moved / (ms * 1e-3) / 1e12, 3),
           "share_of_6.3": round(moved / (ms * 1e-3) / 6.3e12, 3), "hbm_roof_ms_at_6.3": round(moved / 6.3e12 * 1e3, 3)}
    if times[k]["lm"]:
        lm_ms = float(np.median(times[k]["lm"]))
        row.update({"lm_ms": summary(times[k]["lm"]), "stats_over_lm": round(ms / lm_ms, 3), "not_slower_than_lm": bool(ms <= lm_ms)})
        ok = ok and ms <= lm_ms
    out["kernel"][k] = row
out["hwe_exact"] = {"rows": p, "ms": summary(t_hwe)}
out["every_leg_not_slower_than_lm"] = bool(ok)
for b in (d8s, d8m, dbed, dfs, dfm, dds, ddm, res, swork, dcnt, dmom, dhwe):
    b.free()
ctx.sync()

note("kernel legs timed")

# ---- end to end: lmm.snp_stats against lmm.pygemma_lm (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    pe = min(a.e2e_p, p)
    Xh = _lib.pinned_empty((n, pe), np.float32)
    for s0 in range(0, pe, 8192):
        Xh[:, s0:s0 + 8192] = G8[s0:min(pe, s0 + 8192)].T
    pb = PackedBed(bed[:pe], n)
    del G8
    Yh = y.astype(np.float64)
    for X in (Xh[:, :8192].copy(), PackedBed(bed[:8192], n)):       # warm-up of both paths (kernels, allocations)
        lmm.snp_stats(X)
        lmm.pygemma_lm(Yh, X, W)
    out["e2e"] = {"p": pe}
    for tag, X in (("pinned_f32", Xh), ("packed_bed", pb)):
        e2e = {"stats": [], "lm": []}
        for r in range(a.e2e_reps):
            pair = (("stats", lambda: lmm.snp_stats(X)), ("lm", lambda: lmm.pygemma_lm(Yh, X, W)))
            for name, fn in (pair if r % 2 == 0 else pair[::-1]):
                t0 = time.perf_counter()
                fn()
                e2e[name].append(time.perf_counter() - t0)
        out["e2e"][tag] = {"stats_s": summary(e2e["stats"]), "lm_s": summary(e2e["lm"]),
                           "ratio": round(float(np.median(e2e["stats"]) / np.median(e2e["lm"])), 3)}
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
