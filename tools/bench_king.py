"""KING-robust relatedness (pg_king_bed_acc_dev, pg_king_finish_dev, lmm.king) on one GPU.

At n = 10 000 samples, p = 100 000 packed .bed records (the bench workload), without and with 2 % missing calls, in one process:
  batch:   device-event time of one pg_king_bed_acc_dev call on a device-resident batch of --pb (16 384) records, and, from the same
           calls repeated with PG_KING_TIMING=1 (the library's own events around its launches; pg_king_last_batch_ms), its two parts:
           encode (flags, the three int8 planes, per-sample counts, totals) and pair kernel.  The int8 operations of the GEMM tiles
           that ran (2 x 256 x 256 x ldk each: two products per pair of 256-sample tiles without a missing call, five with, four on
           the diagonal) over the pair kernel's time, against the int8 peak of the matrix pipe (5 POP/s dense: twice the BF16 rate)
           and the 2 620 TOP/s sustained figure of profiles/r03_mfma_sustained.txt.
  ld_tile: the yardstick: pg_ld_block_dev's one-product path (no missing call) on an LD image of K = --pb samples and 29 x 252 SNPs a
           side, 841 GEMM tiles of the same 256 x 256 x K shape on the same pipe, in the same run.  Both are reported as time per GEMM
           tile; the legs alternate, --repeats (3) times, each an event-timed median of --reps (7): the spread of the yardstick over
           the repeats is what a difference is read against.
  e2e:     wall time of lmm.king from pinned and from pageable records, and of lmm.kinship on the same pinned records, median of
           --e2e-reps (3).
Prints one JSON line; --out (default profiles/king_bench.json) also receives it.
usage: bench_king.py [--n N] [--p P] [--pb PB] [--reps R] [--repeats K] [--e2e-reps R] [--out path]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pygemma_amd import _lib, lmm  # noqa: E402
from pygemma_amd.bed import PackedBed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--p", type=int, default=100000)
ap.add_argument("--pb", type=int, default=16384)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--e2e-reps", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "king_bench.json"))
a = ap.parse_args()
n, p, pb = a.n, a.p, min(a.pb, a.p)
L = _lib.load()
ctx = _lib.Context(0)
bpr, ldk = (n + 3) // 4, (pb + 127) // 128 * 128
PEAK, SUSTAINED = 5000e12, 2620e12
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_king] {msg}", file=sys.stderr, flush=True)


def records(miss):
    """(p, ceil(n/4)) .bed records of independent SNPs, allele frequency 0.05 .. 0.5, `miss` of the calls code 01; pinned."""
    out = _lib.pinned_empty((p, bpr), np.uint8)
    for s0 in range(0, p, 8192):
        rows = min(p, s0 + 8192) - s0
        thr = rng.integers(13, 128, (rows, 1), dtype=np.uint8)
        u = rng.integers(0, 256, (2, rows, 4 * bpr), dtype=np.uint8)
        g = (u[0] < thr).astype(np.uint8) + (u[1] < thr).astype(np.uint8)
        code = g + (g > 0)                                               # 0 -> 00, 1 -> 10, 2 -> 11
        if miss > 0:
            code[rng.integers(0, 65536, code.shape, dtype=np.uint16) < int(miss * 65536)] = 1
        code[:, n:] = 0
        code = code.reshape(rows, bpr, 4)
        out[s0:s0 + rows] = code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)
    return out


beds = {"no_missing": records(0.0), "2pct_missing": records(0.02)}
note("host records made")
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
    return float(np.median([timed(fn) for _ in range(a.reps)]))


# ---- device legs: one batch of pb records, and the LD tile at the same K
dacc = ctx.alloc(L.pg_king_acc_bytes(n, pb))
_lib.check(L.pg_memset(ctx.handle, dacc.ptr, 0, L.pg_king_zero_bytes(n)), "pg_memset")
dbatch = {k: ctx.to_device(np.ascontiguousarray(v[:pb])) for k, v in beds.items()}
nt = -(-n // 256)
tiles = {"no_missing": 2 * nt * (nt + 1) // 2, "2pct_missing": 5 * nt * (nt + 1) // 2 - nt}
ld_side = 29 * 252
X8 = rng.integers(0, 3, (pb, ld_side), dtype=np.int8)                     # sample-major block of the LD image: pb "samples" = K
dX8 = ctx.to_device(X8)
img = ctx.alloc(L.pg_ld_image_bytes(pb, ld_side))
_lib.check(L.pg_ld_encode_x_dev(ctx.handle, pb, ld_side, dX8.ptr, 0, ld_side, 0, img.ptr, ld_side, 0), "pg_ld_encode_x_dev")
dr = ctx.alloc(4 * ld_side * ld_side)
ld_tiles = 29 * 29


def king_call(tag):
    return lambda: _lib.check(L.pg_king_bed_acc_dev(ctx.handle, n, pb, dbatch[tag].ptr, bpr, 0, dacc.ptr), "pg_king_bed_acc_dev")


def ld_call():
    _lib.check(L.pg_ld_block_dev(ctx.handle, pb, img.ptr, ld_side, 0, ld_side, img.ptr, ld_side, 0, ld_side, dr.ptr, ld_side, None), "pg_ld_block_dev")


def parts_of(fn):
    """Medians of the library's own (encode, pair kernel) milliseconds over --reps calls under PG_KING_TIMING=1."""
    os.environ["PG_KING_TIMING"] = "1"
    try:
        fn()
        xs = []
        for _ in range(a.reps):
            fn()
            enc, pair = C.c_float(), C.c_float()
            _lib.check(L.pg_king_last_batch_ms(C.byref(enc), C.byref(pair)), "pg_king_last_batch_ms")
            xs.append((enc.value, pair.value))
    finally:
        del os.environ["PG_KING_TIMING"]
    return tuple(float(v) for v in np.median(np.asarray(xs, np.float64), axis=0))


legs = {"ld_tile": [], "no_missing": [], "2pct_missing": [], "no_missing_encode": [], "2pct_missing_encode": [], "no_missing_pair": [],
        "2pct_missing_pair": []}
for _ in range(a.repeats):
    legs["ld_tile"].append(median_of(ld_call))
    for tag in beds:
        legs[tag].append(median_of(king_call(tag)))
        enc_ms, pair_ms = parts_of(king_call(tag))
        legs[tag + "_encode"].append(enc_ms)
        legs[tag + "_pair"].append(pair_ms)
ctx.sync()
note("device legs timed")


def spread(xs):
    return {"ms": [round(x, 3) for x in xs], "median": round(float(np.median(xs)), 3), "spread": round((max(xs) - min(xs)) / float(np.median(xs)), 4)}


out = {"tool": "bench_king", "n": n, "p": p, "pb": pb, "ldk": ldk, "reps": a.reps, "repeats": a.repeats, "int8_peak_TOPs": PEAK / 1e12,
       "int8_sustained_TOPs": SUSTAINED / 1e12, "batch": {}}
ld_ms = float(np.median(legs["ld_tile"]))
out["ld_tile"] = dict(spread(legs["ld_tile"]), K=ldk, tiles=ld_tiles, us_per_tile=round(1e3 * ld_ms / ld_tiles, 3),
                      int8_TOPs=round(ld_tiles * 2.0 * 256 * 256 * ldk / (ld_ms * 1e-3) / 1e12, 1))
for tag in beds:
    whole, enc, pair = legs[tag], legs[tag + "_encode"], legs[tag + "_pair"]
    pair_ms = float(np.median(pair))
    ops = tiles[tag] * 2.0 * 256 * 256 * ldk
    out["batch"][tag] = {"call": spread(whole), "encode": spread(enc), "pair": spread(pair), "gemm_tiles": tiles[tag],
                         "us_per_tile": round(1e3 * pair_ms / tiles[tag], 3),
                         "tile_time_over_ld_tile": round(pair_ms / tiles[tag] / (ld_ms / ld_tiles), 3),
                         "int8_TOPs": round(ops / (pair_ms * 1e-3) / 1e12, 1), "share_of_peak": round(ops / (pair_ms * 1e-3) / PEAK, 3),
                         "share_of_sustained": round(ops / (pair_ms * 1e-3) / SUSTAINED, 3),
                         "encode_bytes": int(pb * bpr + 3 * n * ldk),
                         "encode_TBps": round((pb * bpr + 3 * n * ldk) / (float(np.median(enc)) * 1e-3) / 1e12, 3),
                         "whole_stream_ms_estimate": round(float(np.median(whole)) * p / pb, 1)}
for b in list(dbatch.values()) + [dacc, dX8, img, dr]:
    b.free()

# ---- end to end
if a.e2e_reps > 0:
    out["e2e"] = {}
    small = PackedBed(np.ascontiguousarray(beds["2pct_missing"][:2048]), n)
    lmm.king(small)
    lmm.kinship(small)
    for tag, rec in beds.items():
        pageable = np.array(rec)
        runs = {"king_pinned_s": lambda: lmm.king(PackedBed(rec, n)), "king_pageable_s": lambda: lmm.king(PackedBed(pageable, n)),
                "kinship_pinned_s": lambda: lmm.kinship(PackedBed(rec, n))}
        ts = {k: [] for k in runs}
        for r in range(a.e2e_reps):
            for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
                t0 = time.perf_counter()
                runs[k]()
                ts[k].append(time.perf_counter() - t0)
        out["e2e"][tag] = {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in ts.items()}
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
