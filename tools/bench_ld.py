"""Linkage disequilibrium (pg_ld_encode_{bed,x}_dev, pg_ld_band_dev, pg_ld_block_dev, lmm.ld_window) on one GPU.

At n = 10 000, p = 100 000 hard-call SNPs (the bench workload), in one process:
  encode:  device-event time of one encode call on device-resident packed .bed records (without and with 2 % missing calls), int8 and
           float32 sample-major blocks; the bytes it must move (the block read once, three int8 planes written) over its time.
  band:    pg_ld_band_dev over all p rows at window 64 and 256, on the image without a missing call (one product per tile pair) and on
           the one with (nine products over the three planes); pairs per second, and the int8 operations the MFMA tiles that ran issued
           (2 x 256 x 256 x ldk each, counted on the host by the kernel's own rules) against the 2 620 TOP/s sustained figure of
           profiles/r03_mfma_sustained.txt.
  block:   an 8 192 x 8 192 dense block, both images.
  e2e:     wall time of lmm.ld_window(X, 256) next to lmm.snp_stats(X, hwe=False) on the same input in the same run — that pass reads
           the same bytes and is the stream's floor — from a PackedBed, pinned int8 and pinned float32.
Every time is the median of --reps (7) repeats, event-timed.  Prints one JSON line; --out also writes it to a file.
usage: bench_ld.py [--n N] [--p P] [--reps R] [--e2e-reps R] [--out path]"""
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
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--block", type=int, default=8192)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p = a.n, a.p
L = _lib.load()
ctx = _lib.Context(0)
bpr, ldk = (n + 3) // 4, (n + 127) // 128 * 128
T1, T3 = 252, 84
SUSTAINED = 2620e12
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_ld] {msg}", file=sys.stderr, flush=True)


def pack(G8, miss):
    """SNP-major int8 codes (p x n) -> .bed records, code 01 where `miss`."""
    code = np.zeros((G8.shape[0], 4 * bpr), np.uint8)
    code[:, :n] = np.where(miss, 1, G8 + (G8 > 0)) if miss is not None else G8 + (G8 > 0)      # 0 -> 00, 1 -> 10, 2 -> 11
    code = code.reshape(G8.shape[0], bpr, 4)
    return np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))


# ---- inputs: LD blocks of eight SNPs (a fresh draw, then neighbours with a tenth of the calls redrawn), SNP-major int8 on the host
G8 = np.empty((p, n), np.int8)
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
    G8[s0:e0] = blk
    bed0[s0:e0] = pack(blk, None)
    bed1[s0:e0] = pack(blk, rng.random((e0 - s0, n), dtype=np.float32) < 0.02)
note("host genotypes made")

dbed0, dbed1 = ctx.to_device(bed0), ctx.to_device(bed1)
d8m = ctx.to_device(np.ascontiguousarray(G8.T))            # int8 sample-major (n x p)
d8s = ctx.to_device(G8)
ldx = (n + 63) // 64 * 64
dfs = ctx.alloc(p * ldx * 4)
dfm = ctx.alloc(n * p * 4)                                 # float32 sample-major (n x p)
_lib.check(L.pg_cast_i8_f32_dev(ctx.handle, p, n, d8s.ptr, 0, n, dfs.ptr, ldx), "pg_cast_i8_f32_dev")
_lib.check(L.pg_transpose_dev(ctx.handle, p, n, dfs.ptr, ldx, dfm.ptr, p), "pg_transpose_dev")
ctx.sync()
dfs.free(); d8s.free()
img0, img1 = ctx.alloc(L.pg_ld_image_bytes(n, p)), ctx.alloc(L.pg_ld_image_bytes(n, p))
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


def median_of(fn):
    fn()
    ctx.sync()
    xs = np.asarray([timed(fn) for _ in range(a.reps)], np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


def enc_bed(d, img):
    return lambda: _lib.check(L.pg_ld_encode_bed_dev(ctx.handle, n, p, d.ptr, bpr, 0, img.ptr, p, 0), "pg_ld_encode_bed_dev")


def enc_x(d, dtype, img):
    return lambda: _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, p, d.ptr, dtype, p, 0, img.ptr, p, 0), "pg_ld_encode_x_dev")


out = {"tool": "bench_ld", "n": n, "p": p, "ldk": ldk, "reps": a.reps, "encode": {}, "band": {}, "block": {}}
for tag, fn, src_bytes in (("bed", enc_bed(dbed0, img0), bpr * p), ("bed_2pct_missing", enc_bed(dbed1, img1), bpr * p),
                           ("i8_sample_major", enc_x(d8m, 0, img0), n * p), ("f32_sample_major", enc_x(dfm, 2, img0), 4 * n * p)):
    ms = median_of(fn)
    moved = src_bytes + 3 * p * ldk
    out["encode"][tag] = {"ms": ms, "bytes": int(moved), "achieved_TBps": round(moved / (ms["median"] * 1e-3) / 1e12, 3)}
dfm.free(); d8m.free()
enc_bed(dbed0, img0)()
enc_bed(dbed1, img1)()
ctx.sync()
note("encode legs timed")


def band_tiles(w, three):
    """MFMA tiles pg_ld_band_dev runs over all p rows (the kernel's rules: a (sub-)tile pair runs when it meets the band and holds data)."""
    T, nsub, tiles = (T3, 3, 0) if three else (T1, 1, 0)
    for ta in range(-(-p // T1)):
        for tb in range(ta, ta + 1 + (T1 - 1 + w) // T1):
            for sub in range(nsub * nsub):
                as0, bs0 = ta * T1 + (sub // nsub) * T, tb * T1 + (sub % nsub) * T
                if as0 >= p:
                    continue
                as1 = min(as0 + T, p)
                if bs0 >= min(bs0 + T, as1 + w) or bs0 + T <= as0 + 1 or bs0 >= p:
                    continue
                tiles += 1
    return tiles


dband = ctx.alloc(4 * p * 256)
for w in (64, 256):
    for tag, img, three in (("no_missing", img0, False), ("2pct_missing", img1, True)):
        ms = median_of(lambda: _lib.check(L.pg_ld_band_dev(ctx.handle, n, img.ptr, p, 0, p, p, w, dband.ptr, w, None), "pg_ld_band_dev"))
        pairs = sum(min(w, p - 1 - j) for j in range(p))
        ops = band_tiles(w, three) * 2.0 * 256 * 256 * ldk
        sec = ms["median"] * 1e-3
        out["band"][f"w{w}_{tag}"] = {"ms": ms, "pairs": pairs, "Gpairs_per_s": round(pairs / sec / 1e9, 3), "mfma_tiles": band_tiles(w, three),
                                      "int8_TOPs": round(ops / sec / 1e12, 1), "share_of_sustained": round(ops / sec / SUSTAINED, 3)}
dband.free()
nb = min(a.block, p)
dblock = ctx.alloc(4 * nb * nb)
for tag, img, three in (("no_missing", img0, False), ("2pct_missing", img1, True)):
    ms = median_of(lambda: _lib.check(L.pg_ld_block_dev(ctx.handle, n, img.ptr, p, 0, nb, img.ptr, p, 0, nb, dblock.ptr, nb, None), "pg_ld_block_dev"))
    tiles = (-(-nb // T1)) ** 2 if not three else (-(-nb // T3)) ** 2
    ops, sec = tiles * 2.0 * 256 * 256 * ldk, ms["median"] * 1e-3
    out["block"][tag] = {"size": nb, "ms": ms, "Gpairs_per_s": round(nb * nb / sec / 1e9, 3), "mfma_tiles": tiles,
                         "int8_TOPs": round(ops / sec / 1e12, 1), "share_of_sustained": round(ops / sec / SUSTAINED, 3)}
out["planes_over_one_product_per_pair"] = {name: round(out[s][f"{k}2pct_missing"]["ms"]["median"] / out[s][f"{k}no_missing"]["ms"]["median"], 2)
                                           for name, s, k in (("w64", "band", "w64_"), ("w256", "band", "w256_"), ("block", "block", ""))}
for b in (dbed0, dbed1, img0, img1, dblock):
    b.free()
ctx.sync()
note("kernel legs timed")

# ---- end to end: lmm.ld_window against lmm.snp_stats(hwe=False) (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    out["e2e"] = {"window": 256}
    X8 = _lib.pinned_empty((n, p), np.int8)
    for s0 in range(0, p, 8192):
        X8[:, s0:s0 + 8192] = G8[s0:s0 + 8192].T
    del G8
    sources = [("packed_bed", lambda: PackedBed(bed0, n)), ("packed_bed_2pct_missing", lambda: PackedBed(bed1, n)), ("pinned_i8", lambda: X8)]

    def f32():
        Xf = _lib.pinned_empty((n, p), np.float32)
        np.copyto(Xf, X8)
        return Xf
    sources.append(("pinned_f32", f32))
    for tag, make in sources:
        X = make()
        small = PackedBed(X.data[:4096], n) if isinstance(X, PackedBed) else X[:, :4096].copy()
        lmm.ld_window(small, 256)                              # warm-up of both paths (kernels, allocations)
        lmm.snp_stats(small, hwe=False)
        e2e = {"ld": [], "stats": []}
        for r in range(a.e2e_reps):
            pair = (("ld", lambda: lmm.ld_window(X, 256)), ("stats", lambda: lmm.snp_stats(X, hwe=False)))
            for name, fn in (pair if r % 2 == 0 else pair[::-1]):
                t0 = time.perf_counter()
                fn()
                e2e[name].append(time.perf_counter() - t0)
        out["e2e"][tag] = {"ld_window_s": round(float(np.median(e2e["ld"])), 3), "snp_stats_s": round(float(np.median(e2e["stats"])), 3),
                           "ratio": round(float(np.median(e2e["ld"]) / np.median(e2e["stats"])), 2)}
        del X
        note(f"e2e {tag} timed")
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
