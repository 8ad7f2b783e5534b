"""Streamed kinship from a packed PLINK .bed (lmm.kinship(PackedBed), csrc/kinship.hip) on one GPU, n = 10 000, p = 100 000.

  e2e:    wall time of lmm.kinship(bed) — contexts, allocation, upload of the records, kernels, and the download of the
          400 MB K — for a PackedBed in pinned host memory (pinned_empty) and in pageable memory, at 0 % and 2 % missing calls;
          the same with PG_KINSHIP_FP32=1 (fp32 syrk); today's dense float32 path lmm.kinship(G) at p = 20 000.
  device: device-event time of the kernels alone (records resident on the device, default batch): accumulator reset, every
          pg_kinship_bed_acc_dev and pg_kinship_finish_dev — fp16 path and fp32 path.
  parts:  wall time of the pieces of the call outside the kernels: two contexts created and closed, the device allocations of the
          default batch, the upload of all records from pinned memory, the download of K into a new NumPy array.
--device-only runs only the device part (for rocprofv3 --kernel-trace --stats).
Effective rate = n^2 p / time (the lower-triangle convention of DESIGN's kinship row).  Prints one JSON line (median, min, max of
the repeats); --out also writes it to a file.
usage: bench_kinship_bed.py [--n N] [--p P] [--reps R] [--device-only] [--out path]"""
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
ap.add_argument("--p-dense", type=int, default=20000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p = a.n, a.p
bpr = (n + 3) // 4


def records(miss, seed, out):
    """random .bed records (allele frequency U(0.05, 0.5), hard calls, `miss` missing) packed into out (p, bpr)"""
    rng = np.random.default_rng(seed)
    for s in range(0, p, 4096):
        e = min(s + 4096, p)
        f = rng.uniform(0.05, 0.5, e - s).astype(np.float32)[:, None]
        u = rng.random((e - s, bpr * 4), dtype=np.float32)
        code = np.where(u < (1 - f) ** 2, 0, np.where(u < 1 - f * f, 2, 3)).astype(np.uint8)
        if miss:
            code[rng.random(code.shape, dtype=np.float32) < miss] = 1
        code[:, n:] = 0
        c = code.reshape(e - s, bpr, 4)
        out[s:e] = c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)
    return out


def stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1]}


def rate(st, pp):
    return {k.replace("_s", "_tf"): n * n * pp / v / 1e12 for k, v in st.items()}


def wall(fn, reps):
    fn()                                           # warm-up: code objects, first allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats(ts)


def set_fp32(on):
    if on:
        os.environ["PG_KINSHIP_FP32"] = "1"
    else:
        os.environ.pop("PG_KINSHIP_FP32", None)


res = {"n": n, "p": p, "reps": a.reps}
L = _lib.load()
for miss in (0.0, 0.02):
    tag = f"miss{int(miss * 100)}"
    pinned = records(miss, 1, lmm.pinned_empty((p, bpr), np.uint8))
    pageable = pinned.copy()
    bed_pin, bed_page = PackedBed(pinned, n), PackedBed(pageable, n)
    set_fp32(False)
    if not a.device_only:
        st = wall(lambda: lmm.kinship(bed_pin), a.reps)
        res[f"e2e_pinned_{tag}"] = {**st, **rate(st, p)}
        st = wall(lambda: lmm.kinship(bed_page), a.reps)
        res[f"e2e_pageable_{tag}"] = {**st, **rate(st, p)}
        set_fp32(True)
        st = wall(lambda: lmm.kinship(bed_pin), max(1, a.reps // 2))
        res[f"e2e_pinned_fp32_{tag}"] = {**st, **rate(st, p)}
        set_fp32(False)

    # device time of the kernels alone, records resident
    with _lib.Context(0) as ctx:
        pb = min(p, lmm._KIN_BATCH)
        dbed = ctx.to_device(pinned)
        dacc = ctx.alloc(L.pg_kinship_acc_bytes(n, pb))
        dK = ctx.alloc(4 * n * n)
        e0, e1 = C.c_void_p(), C.c_void_p()
        _lib.check(L.pg_event_create(ctx.handle, C.byref(e0)), "pg_event_create")
        _lib.check(L.pg_event_create(ctx.handle, C.byref(e1)), "pg_event_create")
        for fp32 in (False, True):
            set_fp32(fp32)
            ts = []
            for r in range(a.reps + 1):
                _lib.check(L.pg_event_record(ctx.handle, e0), "pg_event_record")
                _lib.check(L.pg_memset(ctx.handle, dacc.ptr, 0, 8 * n * n), "pg_memset")
                for s in range(0, p, pb):
                    w = min(pb, p - s)
                    _lib.check(L.pg_kinship_bed_acc_dev(ctx.handle, n, w, dbed.ptr + s * bpr, bpr, 0, 1, dacc.ptr), "pg_kinship_bed_acc_dev")
                _lib.check(L.pg_kinship_finish_dev(ctx.handle, n, p, dacc.ptr, dK.ptr), "pg_kinship_finish_dev")
                _lib.check(L.pg_event_record(ctx.handle, e1), "pg_event_record")
                ms = C.c_float()
                _lib.check(L.pg_event_elapsed_ms(ctx.handle, e0, e1, C.byref(ms)), "pg_event_elapsed_ms")
                if r:
                    ts.append(ms.value / 1e3)
            st = stats(ts)
            res[f"device_{'fp32' if fp32 else 'fp16'}_{tag}"] = {**st, **rate(st, p), "snp_batch": pb}
        set_fp32(False)
        L.pg_event_destroy(ctx.handle, e0)
        L.pg_event_destroy(ctx.handle, e1)
    if miss == 0.0 and not a.device_only:      # the pieces of lmm.kinship outside the kernels
        pb = min(p, lmm._KIN_BATCH)

        def contexts():
            with _lib.Context(0), _lib.Context(0):
                pass

        def allocs():
            with _lib.Context(0) as ctx:
                bufs = [ctx.alloc(L.pg_kinship_acc_bytes(n, pb)), ctx.alloc(4 * n * n), ctx.alloc(pb * bpr), ctx.alloc(pb * bpr)]
                ctx.sync()
                for b_ in bufs:
                    b_.free()

        with _lib.Context(0) as ctx:
            dbed = ctx.alloc(pinned.nbytes)
            dK = ctx.alloc(4 * n * n)

            def upload():
                _lib.check(L.pg_memcpy_h2d_async(ctx.handle, dbed.ptr, pinned.ctypes.data, pinned.nbytes), "pg_memcpy_h2d_async")
                ctx.sync()

            res["parts"] = {"two_contexts": wall(contexts, a.reps), "allocations": wall(allocs, a.reps),
                            "upload_all_records_pinned": wall(upload, a.reps),
                            "download_K": wall(lambda: dK.download((n, n), np.float32), a.reps)}
    del bed_pin, bed_page, pinned, pageable

if a.device_only:
    print(json.dumps(res))
    sys.exit(0)
# today's path: dense float32 (n, p_dense) uploaded whole, fp32 syrk
rng = np.random.default_rng(2)
G = rng.binomial(2, rng.uniform(0.05, 0.5, a.p_dense), size=(n, a.p_dense)).astype(np.float32)
st = wall(lambda: lmm.kinship(G), max(1, a.reps // 2))
res["e2e_dense_float32"] = {**st, **rate(st, a.p_dense), "p": a.p_dense}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
