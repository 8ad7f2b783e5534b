"""The pairwise epistasis scan (pg_epi_split_dev, pg_epi_block_dev, lmm.epistasis) on one GPU, next to pg_ld_block_dev as the yardstick.

At n = 10 000 (half cases, half controls), in one process:
  split:   device-event time of pg_epi_split_dev over --block SNPs; the bytes it moves (two planes read, six written) over its time.
  block:   pg_epi_block_dev on a --block x --block dense window of one image against itself (every ordered pair, as pg_ld_block_dev
           computes them), cut at p = 1e-4, on the image without a missing call (one product per 128 x 256 tile pair) and on the one
           with 2 % missing (four products per tile pair): pairs per second, the int8 operations of the MFMA tiles that ran
           (2 x 256 x 256 x ldk each) against the 2 620 TOP/s sustained figure of profiles/r03_mfma_sustained.txt; the same window with
           upper = 1 (the pairs a < b only) and in case-only mode (one logarithm per pair instead of two: what the epilogue's fp64 costs).
  ld:      pg_ld_block_dev on the same panel and window in the same process, and the ratio of the two pair rates.
  e2e:     wall time of lmm.epistasis(X, y) on a packed .bed of --p SNPs (all pairs, p = 1e-4).
Every kernel time is the median of --reps (7) event-timed repeats.  Prints one JSON line; --out also writes it to a file.
usage: bench_epistasis.py [--n N] [--p P] [--block B] [--reps R] [--e2e-reps R] [--out path]"""
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
ap.add_argument("--p", type=int, default=20000)
ap.add_argument("--block", type=int, default=8192)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p = a.n, a.p
nb = min(a.block, p)
L = _lib.load()
ctx = _lib.Context(0)
bpr, ldk = (n + 3) // 4, (n + 127) // 128 * 128
SUSTAINED = 2620e12
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_epistasis] {msg}", file=sys.stderr, flush=True)


def pack(G8, miss):
    """SNP-major int8 codes (p x n) -> .bed records, code 01 where `miss`."""
    code = np.zeros((G8.shape[0], 4 * bpr), np.uint8)
    code[:, :n] = np.where(miss, 1, G8 + (G8 > 0)) if miss is not None else G8 + (G8 > 0)      # 0 -> 00, 1 -> 10, 2 -> 11
    code = code.reshape(G8.shape[0], bpr, 4)
    return np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))


# ---- inputs: LD blocks of eight SNPs as tools/bench_ld.py makes them, a random phenotype
bed0, bed1 = np.empty((p, bpr), np.uint8), np.empty((p, bpr), np.uint8)
for s0 in range(0, p, 4096):
    e0 = min(p, s0 + 4096)
    thr = rng.uniform(0.05, 0.5, (e0 - s0, 1)).astype(np.float32)
    u = rng.random((2, e0 - s0, n), dtype=np.float32)
    blk = (u[0] < thr).astype(np.int8) + (u[1] < thr).astype(np.int8)
    redo = rng.random((e0 - s0, n), dtype=np.float32) < 0.1
    for j in range(1, e0 - s0):
        if j % 8:
            blk[j] = np.where(redo[j], blk[j], blk[j - 1])
    bed0[s0:e0] = pack(blk, None)
    bed1[s0:e0] = pack(blk, rng.random((e0 - s0, n), dtype=np.float32) < 0.02)
y = (rng.random(n) < 0.5).astype(np.float64)
note("host genotypes made")

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


dgroup = ctx.to_device(y.astype(np.int8))
ld_bytes, epi_bytes = int(L.pg_ld_image_bytes(n, nb)), int(L.pg_epi_image_bytes(n, nb))
out = {"tool": "bench_epistasis", "n": n, "block": nb, "ldk": ldk, "reps": a.reps, "chi2_min": lmm._epi_chi2_min(1e-4, None), "split": {}, "block_pairs": {},
       "ld_block": {}}
ldims, images = [], []
for tag, bed in (("no_missing", bed0), ("2pct_missing", bed1)):
    dbed = ctx.to_device(bed[:nb])
    ldim, image = ctx.alloc(ld_bytes), ctx.alloc(epi_bytes)
    _lib.check(L.pg_ld_encode_bed_dev(ctx.handle, n, nb, dbed.ptr, bpr, 0, ldim.ptr, nb, 0), "pg_ld_encode_bed_dev")
    ms = median_of(lambda: _lib.check(L.pg_epi_split_dev(ctx.handle, n, ldim.ptr, nb, 0, nb, dgroup.ptr, image.ptr), "pg_epi_split_dev"))
    moved = 8 * nb * ldk
    out["split"][tag] = {"ms": ms, "bytes": int(moved), "achieved_TBps": round(moved / (ms["median"] * 1e-3) / 1e12, 3)}
    dbed.free()
    ldims.append(ldim); images.append(image)
note("split legs timed")

cap = 1 << 22
dcount, dhits = ctx.alloc(8), ctx.alloc(16 * cap)
dtot, dsig, dbest = ctx.alloc(4 * nb), ctx.alloc(4 * nb), ctx.alloc(8 * nb)
dr = ctx.alloc(4 * nb * nb)
for buf in (dtot, dsig, dbest):
    _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, buf.nbytes), "pg_memset")


def epi(image, mode, upper):
    def run():
        _lib.check(L.pg_memset(ctx.handle, dcount.ptr, 0, 8), "pg_memset")
        _lib.check(L.pg_epi_block_dev(ctx.handle, n, image.ptr, nb, 0, nb, 0, image.ptr, nb, 0, nb, 0, mode, upper, out["chi2_min"], dcount.ptr, dhits.ptr,
                                      cap, dtot.ptr, dsig.ptr, dbest.ptr, None), "pg_epi_block_dev")
    return run


for tag, image, ldim, products in (("no_missing", images[0], ldims[0], 1), ("2pct_missing", images[1], ldims[1], 4)):
    ms = median_of(lambda: _lib.check(L.pg_ld_block_dev(ctx.handle, n, ldim.ptr, nb, 0, nb, ldim.ptr, nb, 0, nb, dr.ptr, nb, None), "pg_ld_block_dev"))
    ld_rate = nb * nb / (ms["median"] * 1e-3) / 1e9
    out["ld_block"][tag] = {"ms": ms, "Gpairs_per_s": round(ld_rate, 3)}
    tiles = (-(-nb // 128)) * (-(-nb // 256)) * products
    ops = tiles * 2.0 * 256 * 256 * ldk
    leg = {}
    for name, mode, upper, pairs in (("dense", 0, 0, nb * nb), ("dense_case_only", 1, 0, nb * nb), ("upper", 0, 1, nb * (nb - 1) // 2)):
        ms = median_of(epi(image, mode, upper))
        ctx.sync()
        sec = ms["median"] * 1e-3
        leg[name] = {"ms": ms, "pairs": pairs, "Gpairs_per_s": round(pairs / sec / 1e9, 3), "hits": int(dcount.download((1,), np.uint64)[0])}
        if not upper:
            leg[name].update({"mfma_tiles": tiles, "int8_TOPs": round(ops / sec / 1e12, 1), "share_of_sustained": round(ops / sec / SUSTAINED, 3)})
    leg["pair_rate_over_ld"] = round(leg["dense"]["Gpairs_per_s"] / ld_rate, 3)
    out["block_pairs"][tag] = leg
    note(f"block legs on {tag} timed")
for b in ldims + images + [dcount, dhits, dtot, dsig, dbest, dr, dgroup]:
    b.free()
ctx.sync()

# ---- end to end: lmm.epistasis from a packed .bed (skipped with --e2e-reps 0)
if a.e2e_reps > 0:
    out["e2e"] = {"p": p, "pairs": p * (p - 1) // 2}
    lmm.epistasis(PackedBed(bed0[:2048], n), y)                    # warm-up (kernels, allocations)
    for tag, bed in (("packed_bed", bed0), ("packed_bed_2pct_missing", bed1)):
        secs, stats = [], {}
        for r in range(a.e2e_reps):
            t0 = time.perf_counter()
            res = lmm.epistasis(PackedBed(bed, n), y, stats=stats)
            secs.append(time.perf_counter() - t0)
        sec = float(np.median(secs))
        out["e2e"][tag] = {"seconds": round(sec, 3), "Gpairs_per_s": round(out["e2e"]["pairs"] / sec / 1e9, 3), "pairs_above_cut": len(res.pairs),
                           "blocks": stats["blocks"], "reruns": stats["reruns"]}
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
