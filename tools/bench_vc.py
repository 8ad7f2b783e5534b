"""Variance components for several kinship matrices (lmm.reml, csrc/vc.hip) on one GPU: n = 10 000, k = 3, c = 5 by default.

  phases:  device-event times of the entry points on device-resident operands — pg_vc_combine_dev, pg_potrf_dev (with its copy of the
           lower triangle into and out of the work matrix), pg_potri_dev, pg_sym_trdot_dev (one float32 K), pg_symv_dev (m = c + 1) —
           and of one whole pg_vc_eval_dev (wall time: it waits for its results).  potrf: n^3 / 3 flops; potri: 2 n^3 / 3 useful,
           4 n^3 / 3 executed (the level products and X'X run over the zero upper half of L^-1); both beside the fp64 rate of the rank-128
           update of the eigensolver (profiles/r04_syevd_summary.json: 35.8 TF/s).  trdot: the bytes of both lower triangles over its time,
           against 6.3 TB/s.
  fit:     lmm.reml end to end: iterations, evaluations, seconds, seconds per evaluation.
  cpu:     one evaluation of the NumPy truth (tests/_vc_truth.py) on the host's BLAS threads, and that time multiplied by the number of
           evaluations the fit took (an estimate of the same fit on the CPU, not a run of it); --cpu-n evaluates at a smaller n.
  bounds:  with --fractions <file written by tests/test_gpu_vc.py under PG_VC_FRACTIONS>, the largest fraction of each test bound used.
Prints one JSON line; --out also writes it to a file (profiles/vc_bench.json).
usage: bench_vc.py [--n N] [--k K] [--c C] [--reps R] [--cpu-n N] [--fractions path] [--out path]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pygemma_amd import _lib, lmm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10000)
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--c", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cpu-n", type=int, default=0, help="size of the CPU evaluation (0: n; -1: none)")
ap.add_argument("--fractions", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, k, c = a.n, a.k, a.c
L, V = _lib.load(), _lib.load_vc()
rng = np.random.default_rng(3)

# ---- inputs: k kinship matrices from independent genotype panels (float32, from lmm.kinship), y with a third of its variance in each of two
p = max(n, 64)
Ks = []
for i in range(k):
    f = rng.uniform(0.05, 0.5, p).astype(np.float32)
    G = (rng.random((n, p), dtype=np.float32) < f).astype(np.int8) + (rng.random((n, p), dtype=np.float32) < f).astype(np.int8)
    Ks.append(np.ascontiguousarray(lmm.kinship(G), np.float32))
del G
W = np.c_[np.ones(n), rng.standard_normal((n, c - 1))]
true = np.r_[np.linspace(1.0, 0.5, k) * (0.6 / k), 0.4]
y = W @ rng.standard_normal(c) + np.sqrt(true[k]) * rng.standard_normal(n)
for s, K in zip(true, Ks):      # g ~ N(0, s K) through K's own factor: K + 1e-3 I is positive definite
    y = y + np.sqrt(s) * (np.linalg.cholesky(K.astype(np.float64) + 1e-3 * np.eye(n)) @ rng.standard_normal(n))


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


out = {"tool": "bench_vc", "n": n, "k": k, "c": c, "reps": a.reps, "rank128_update_TFps": 35.8, "hbm_TBps": 6.3}

# ---- phases
with _lib.Context(0) as ctx:
    dK = [ctx.to_device(K) for K in Ks]
    ptrs, f64, ldk = (C.c_void_p * k)(*[b.ptr for b in dK]), (C.c_int * k)(*[0] * k), (C.c_int64 * k)(*[n] * k)
    sig = (C.c_double * (k + 1))(*true)
    dV, dI, dS = ctx.alloc(8 * n * n), ctx.alloc(8 * n * n), ctx.alloc(64)
    dX, dY = ctx.to_device(np.ascontiguousarray(np.c_[W, y])), ctx.alloc(8 * n * (c + 1))
    pwork, info = ctx.alloc(int(V.pg_potri_work_bytes(n))), ctx.alloc(8)
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

    legs = {
        "combine": lambda: _lib.check(V.pg_vc_combine_dev(ctx.handle, n, k, ptrs, f64, ldk, sig, dV.ptr, n), "pg_vc_combine_dev"),
        "potrf": lambda: _lib.check(V.pg_potrf_dev(ctx.handle, n, dV.ptr, n, info.ptr), "pg_potrf_dev"),
        "potri": lambda: _lib.check(V.pg_potri_dev(ctx.handle, n, dV.ptr, n, dI.ptr, n, pwork.ptr), "pg_potri_dev"),
        "trdot": lambda: _lib.check(V.pg_sym_trdot_dev(ctx.handle, n, dI.ptr, n, dK[0].ptr, 0, n, dS.ptr), "pg_sym_trdot_dev"),
        "symv": lambda: _lib.check(V.pg_symv_dev(ctx.handle, n, dI.ptr, 1, n, c + 1, dX.ptr, c + 1, dY.ptr, c + 1), "pg_symv_dev"),
    }
    times = {name: [] for name in legs}
    for r in range(a.reps + 1):                             # combine -> potrf -> potri keep their operands valid; the first round is the warm-up
        for name, fn in legs.items():
            t = timed(fn)
            if r:
                times[name].append(t)
    assert info.download((1,), np.int32)[0] == 0
    med = {name: float(np.median(v)) for name, v in times.items()}
    ph = {name: {"ms": summary(v)} for name, v in times.items()}
    ph["potrf"].update(flops=n ** 3 / 3, TFps=round(n ** 3 / 3 / (med["potrf"] * 1e-3) / 1e12, 2))
    ph["potri"].update(flops_useful=2 * n ** 3 / 3, flops_executed=4 * n ** 3 / 3, TFps_useful=round(2 * n ** 3 / 3 / (med["potri"] * 1e-3) / 1e12, 2),
                       TFps_executed=round(4 * n ** 3 / 3 / (med["potri"] * 1e-3) / 1e12, 2), zero_upper_half_multiplied=True)
    tb = (8 + 4) * n * (n + 1) / 2
    ph["trdot"].update(bytes=int(tb), TBps=round(tb / (med["trdot"] * 1e-3) / 1e12, 3), share_of_6_3=round(tb / (med["trdot"] * 1e-3) / 6.3e12, 3))
    sb = 8 * n * n
    ph["symv"].update(bytes=int(sb), TBps=round(sb / (med["symv"] * 1e-3) / 1e12, 3), note="every stored element of the lower triangle is read twice")
    work = ctx.alloc(int(V.pg_vc_work_bytes(n, k)))
    res, hinfo, ev_s = np.empty(int(V.pg_vc_out_len(k, c))), C.c_int(0), []
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        _lib.check(V.pg_vc_eval_dev(ctx.handle, n, k, c, ptrs, f64, ldk, sig, dX.ptr, work.ptr, res.ctypes.data, None, C.byref(hinfo)), "pg_vc_eval_dev")
        if r:
            ev_s.append((time.perf_counter() - t0) * 1e3)
    ph["eval"] = {"ms": summary(ev_s), "symv_calls": 1 + k + (k + 1 + 31) // 32, "trdot_calls": k}
    out["phases"] = ph
    for e in evs:
        L.pg_event_destroy(ctx.handle, e)

# ---- the fit
stats = {}
t0 = time.perf_counter()
fit = lmm.reml(y, W, Ks, stats=stats)
out["fit"] = {"seconds": round(time.perf_counter() - t0, 3), "iterations": fit.iters, "evaluations": stats["evaluations"], "converged": fit.converged,
              "seconds_per_evaluation": round(stats["seconds_eval"] / stats["evaluations"], 4), "sigma2": [round(float(v), 5) for v in fit.sigma2],
              "se": [round(float(v), 5) for v in fit.se], "sigma2_generating": [round(float(v), 5) for v in true]}

# ---- the NumPy truth, for context
if a.cpu_n >= 0:
    import _vc_truth as T
    m = a.cpu_n or n
    t0 = time.perf_counter()
    T.evaluate(y[:m], W[:m], [K[:m, :m] for K in Ks], fit.sigma2)
    sec = time.perf_counter() - t0
    out["cpu_truth"] = {"n": m, "threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count())), "seconds_per_evaluation": round(sec, 3),
                        "fit_seconds_estimated": round(sec * stats["evaluations"], 1), "estimated": True}
if a.fractions and os.path.exists(a.fractions):
    with open(a.fractions) as f:
        out["largest_fraction_of_test_bound"] = {key: float(f"{v:.3g}") for key, v in json.load(f).items()}
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
