"""LD scores (pg_ld_score_dev, lmm.ld_scores) on one GPU, next to the route without the fused kernel.

At n = 10 000, p = 100 000 hard-call SNPs (the shape of tools/bench_ld.py and profiles/ld_bench.json), in one process:
  kernel:  device-event time of pg_ld_score_dev over all p rows at window 256 and 2048, on the image without a missing call (one
           product per tile pair) and on the one with 2 % missing (nine products over the three planes), each next to pg_ld_band_dev on
           the same resident image: the same products, 16 bytes per SNP out instead of 4 w.  The two alternate, rep by rep.
  e2e:     wall time of lmm.ld_scores(bed, w, adjust=False) against ld_window(bed, w) and a NumPy fold of the band (float64 squares,
           row sums and a bincount per chunk of rows for the partners' side), the only route without the kernel; both times, their
           ratio (the two alternate, rep by rep), and the largest |difference| of the two l2 (what the fixed point and the float32 band allow: w 2^-32 + w 2^-23).
  limits:  the widest window whose (p, w) float32 band still fits the free device memory (resident) and the available host memory.
Every time is the median (with min and max) of --reps (7) repeats.  Prints one JSON line; --out also writes it to a file.
usage: bench_ld_scores.py [--n N] [--p P] [--reps R] [--e2e-reps R] [--windows W,W] [--out path]"""
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
ap.add_argument("--windows", default="256,2048")
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p = a.n, a.p
windows = [int(w) for w in a.windows.split(",")]
L = _lib.load()
ctx = _lib.Context(0)
free0, _total = ctx.mem_info()
bpr = (n + 3) // 4
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_ld_scores] {msg}", file=sys.stderr, flush=True)


def pack(G8, miss):
    """SNP-major int8 codes (p x n) -> .bed records, code 01 where `miss`."""
    code = np.zeros((G8.shape[0], 4 * bpr), np.uint8)
    code[:, :n] = np.where(miss, 1, G8 + (G8 > 0)) if miss is not None else G8 + (G8 > 0)      # 0 -> 00, 1 -> 10, 2 -> 11
    code = code.reshape(G8.shape[0], bpr, 4)
    return np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))


# ---- inputs: bench_ld's LD blocks of eight SNPs (a fresh draw, then neighbours with a tenth of the calls redrawn) as packed records
bed0, bed1 = np.empty((p, bpr), np.uint8), np.empty((p, bpr), np.uint8)
for s0 in range(0, p, 8192):
    e0 = min(p, s0 + 8192)
    thr = rng.uniform(0.05, 0.5, (e0 - s0, 1)).astype(np.float32)
    u = rng.random((2, e0 - s0, n), dtype=np.float32)
    blk = (u[0] < thr).astype(np.int8) + (u[1] < thr).astype(np.int8)
    redo = rng.random((e0 - s0, n), dtype=np.float32) < 0.1
    for j in range(1, e0 - s0):
        if j % 8:
            blk[j] = np.where(redo[j], blk[j], blk[j - 1])
    bed0[s0:e0] = pack(blk, None)
    bed1[s0:e0] = pack(blk, rng.random((e0 - s0, n), dtype=np.float32) < 0.02)
note("host genotypes made")

images = {}
for tag, bed in (("no_missing", bed0), ("2pct_missing", bed1)):
    dbed = ctx.to_device(bed)
    images[tag] = ctx.alloc(L.pg_ld_image_bytes(n, p))
    _lib.check(L.pg_ld_encode_bed_dev(ctx.handle, n, p, dbed.ptr, bpr, 0, images[tag].ptr, p, 0), "pg_ld_encode_bed_dev")
    ctx.sync()
    dbed.free()
evs = [C.c_void_p() for _ in range(2)]
for e in evs:
    _lib.check(L.pg_event_create(ctx.handle, C.byref(e)), "pg_event_create")


def timed(fn):
    L.pg_event_record(ctx.handle, evs[0])
    fn()
    L.pg_event_record(ctx.handle, evs[1])
    ms = C.c_float()
    _lib.check(L.pg_event_elapsed_ms(ctx.handle, evs[0], evs[1], C.byref(ms)), "pg_event_elapsed_ms")
    return ms.value


def spread(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


out = {"tool": "bench_ld_scores", "n": n, "p": p, "reps": a.reps, "kernel": {}, "e2e": {}}
dsum, dnp, dno = ctx.alloc(8 * p), ctx.alloc(4 * p), ctx.alloc(4 * p)
for buf in (dsum, dnp, dno):          # the sums are accumulated across the repeats: integers, far from their range
    _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, buf.nbytes), "pg_memset")
for w in windows:
    dband = ctx.alloc(4 * p * w)
    for tag, img in images.items():
        legs = {"band": lambda: _lib.check(L.pg_ld_band_dev(ctx.handle, n, img.ptr, p, 0, p, p, w, dband.ptr, w, None), "pg_ld_band_dev"),
                "score": lambda: _lib.check(L.pg_ld_score_dev(ctx.handle, n, img.ptr, p, 0, p, p, w, None, 1, dsum.ptr, dnp.ptr, dno.ptr),
                                            "pg_ld_score_dev")}
        ms = {name: [] for name in legs}
        for fn in legs.values():
            fn()
        ctx.sync()
        for r in range(a.reps):
            for name in (("band", "score") if r % 2 == 0 else ("score", "band")):
                ms[name].append(timed(legs[name]))
        pairs = sum(min(w, p - 1 - j) for j in range(p))
        band, score = spread(ms["band"]), spread(ms["score"])
        out["kernel"][f"w{w}_{tag}"] = {"band_ms": band, "score_ms": score, "score_over_band": round(score["median"] / band["median"], 3), "pairs": pairs,
                                        "score_Gpairs_per_s": round(pairs / (score["median"] * 1e-3) / 1e9, 3), "band_bytes_out": 4 * p * w,
                                        "score_bytes_out": 16 * p}
    dband.free()
for b in (dsum, dnp, dno, *images.values()):
    b.free()
ctx.sync()
note("kernel legs timed")


def fold(band):
    """l2 = 1 + the float64 squares of the band folded to both sides: row sums, and per chunk of rows a bincount over the partners."""
    pp, w = band.shape
    l2 = np.ones(pp)
    k = np.arange(1, w + 1)
    for s in range(0, pp, 8192):
        r2 = np.nan_to_num(band[s:s + 8192].astype(np.float64)) ** 2
        l2[s:s + len(r2)] += r2.sum(axis=1)
        partner = np.minimum(np.arange(s, s + len(r2))[:, None] + k[None, :], pp)      # past the last SNP: NaN in the band, 0 here
        l2 += np.bincount(partner.ravel(), weights=r2.ravel(), minlength=pp + 1)[:pp]
    return l2


# ---- end to end from packed records (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    X = PackedBed(bed0, n)
    small = PackedBed(bed0[:4096], n)
    lmm.ld_scores(small, 64)                                   # warm-up of both routes (kernels, allocations)
    fold(lmm.ld_window(small, 64))
    for w in windows:
        t = {"scores": [], "band_fold": [], "band_alone": []}
        gap = 0.0

        def scores_route():
            t0 = time.perf_counter()
            res["df"] = lmm.ld_scores(X, w, adjust=False)
            t["scores"].append(time.perf_counter() - t0)

        def band_route():
            t0 = time.perf_counter()
            band = lmm.ld_window(X, w)
            t["band_alone"].append(time.perf_counter() - t0)
            res["ref"] = fold(band)
            t["band_fold"].append(time.perf_counter() - t0)

        for r in range(a.e2e_reps):          # the two routes alternate: each follows the other's allocations as often as its own
            res = {}
            for route in ((scores_route, band_route) if r % 2 == 0 else (band_route, scores_route)):
                route()
            used = res["df"]["n_obs"].to_numpy() > 0
            gap = max(gap, float(np.abs(res["df"]["l2"].to_numpy()[used] - res["ref"][used]).max()))
        out["e2e"][f"w{w}"] = {"ld_scores_s": spread(t["scores"]), "ld_window_plus_fold_s": spread(t["band_fold"]), "ld_window_alone_s": spread(t["band_alone"]),
                               "ratio": round(float(np.median(t["band_fold"]) / np.median(t["scores"])), 2), "max_abs_l2_difference": gap,
                               "allowed_l2_difference": w * 2.0 ** -32 + w * 2.0 ** -23, "band_bytes": 4 * p * w}
        note(f"e2e w={w} timed")
    host_free = None
    if os.path.exists("/proc/meminfo"):
        with open("/proc/meminfo") as f:
            host_free = next((int(line.split()[1]) * 1024 for line in f if line.startswith("MemAvailable:")), None)
    out["band_route_limits"] = {"device_free_bytes": int(free0), "largest_resident_window": int(0.9 * free0 // (4 * p)),
                                "host_available_bytes": host_free, "largest_host_window": None if host_free is None else int(host_free // (4 * p)),
                                "note": "computed from the free memory, not run: a (p, w) float32 band on the device (ld_window keeps it resident below "
                                        "0.9 of the free memory, else it comes back batch by batch) and on the host; the fold needs its float64 chunks on top"}
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
