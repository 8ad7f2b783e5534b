"""Permutation tests (pg_perm_block_dev, lmm.case_control_perm's kernel) on one GPU, next to the LD pair kernel.

At n = 10 000 and n = 1 000 samples, p = 65 536 fully called SNPs resident as an LD image and nperm = 4 096 labellings, alternating in
one process, device-event time of
  perm:    pg_perm_block_dev in reduce mode (n_ge and max_null) for both tests on both tile paths (PG_PERM_PLANES=0: one product per
           tile; 1: two products of 128 SNPs x {x, m});
  nostat:  the same calls through libpygemma_perm_nostat.so — csrc/perm.hip built with -DPG_PERM_BENCH_NOSTAT (make -C pygemma_amd/csrc
           bench_perm_nostat; not part of the package), in which the statistic of the epilogue is one conversion and everything else
           stays — when that library is there: the statistic's share of the kernel is 1 - nostat / perm;
  ld_band: pg_ld_band_dev (lmm.ld_window's pair kernel) on the same image with window = nperm: the yardstick, the same int8 tile with a
           float32 r per pair as its epilogue.
Rates are useful int8 operations (2 per multiply-add: 2 ldk p nperm for the permutation kernel, whichever path it takes; 2 ldk per
valid pair of the band) over the median time; the peak to hold them against is the int8 row of the matrix-core table, ~5 POP/s dense.
Prints one JSON line (median, min, max of the repeats); --out also writes it to a file.
usage: bench_case_control_perm.py [--n N[,N..]] [--p P] [--nperm B] [--reps R] [--out path]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygemma_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="10000,1000")
ap.add_argument("--p", type=int, default=65536)
ap.add_argument("--nperm", type=int, default=4096)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
p, B = a.p, a.nperm
L = _lib.load()
P = _lib.load_perm()
ctx = _lib.Context(0)
rng = np.random.default_rng(5)


def note(msg):
    print(f"[bench_case_control_perm] {msg}", file=sys.stderr, flush=True)


# the build with the statistic stubbed out, bound from the same header
NOSTAT = None
nostat_path = os.path.join(os.path.dirname(_lib.PERM_LIB_PATH), "libpygemma_perm_nostat.so")
if os.path.exists(nostat_path):
    NOSTAT = C.CDLL(nostat_path)
    with open(_lib.PERM_HEADER) as hdr:
        for fn, restype, argtypes in _lib.parse_header(hdr.read()):
            f = getattr(NOSTAT, fn)
            f.restype, f.argtypes = restype, argtypes
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


def summary(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": round(float(np.median(xs)), 3), "min": round(float(xs.min()), 3), "max": round(float(xs.max()), 3)}


def one_size(n):
    ldk = -(-n // 128) * 128
    # fully called hard calls, SNP-major int8; half the samples cases, 2 % out of the study
    G8 = rng.integers(0, 3, (p, n), dtype=np.int8)
    study = rng.random(n) >= 0.02
    ncase = int(study.sum()) // 2
    rows = np.zeros((2 + B, ldk), np.int8)
    rows[0, :n] = study
    members = np.flatnonzero(study)
    for b in range(1 + B):
        rows[1 + b, members[rng.permutation(members.size)[:ncase]]] = 1
    G8[:, ~study] = 0                                   # a fully called panel whose excluded samples count nowhere: every flag is 0
    dX = ctx.to_device(G8)
    image = ctx.alloc(L.pg_ld_image_bytes(n, p))
    _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, p, dX.ptr, 0, n, 1, image.ptr, p, 0), "pg_ld_encode_x_dev")
    ctx.sync()
    dX.free()
    del G8
    dlab, dlabc = ctx.alloc(P.pg_perm_label_bytes(n, 2 + B)).upload(rows), ctx.alloc(4 * (2 + B))
    _lib.check(P.pg_perm_label_counts_dev(ctx.handle, n, dlab.ptr, 2 + B, dlabc.ptr), "pg_perm_label_counts_dev")
    dtot, dobs, dnge, dmax = ctx.alloc(16 * p), ctx.alloc(8 * p), ctx.alloc(4 * p), ctx.alloc(8 * B)
    _lib.check(P.pg_perm_totals_dev(ctx.handle, n, image.ptr, p, 0, p, dlab.ptr, dtot.ptr), "pg_perm_totals_dev")
    dband = ctx.alloc(4 * p * B)
    ctx.sync()
    assert (dtot.download((p, 4), np.int32)[:, 3] == 0).all(), "the panel was meant to take the one-product path"
    note(f"n={n}: image, labels and totals on the device")

    def perm(lib, test, planes):
        def run():
            if planes:
                os.environ["PG_PERM_PLANES"] = "1"
            else:
                os.environ.pop("PG_PERM_PLANES", None)
            head = (ctx.handle, n, image.ptr, p, 0, p, dtot.ptr, dlab.ptr, dlabc.ptr)
            _lib.check(lib.pg_perm_block_dev(*head, 2, B, test, None, 0, dobs.ptr, dnge.ptr, dmax.ptr), "pg_perm_block_dev")
        return run

    def ld_band():
        _lib.check(L.pg_ld_band_dev(ctx.handle, n, image.ptr, p, 0, p, p, B, dband.ptr, B, None), "pg_ld_band_dev")

    head = (ctx.handle, n, image.ptr, p, 0, p, dtot.ptr, dlab.ptr, dlabc.ptr)
    legs = {"ld_band": ld_band}
    for test, tname in ((0, "allelic"), (1, "trend")):
        _lib.check(P.pg_perm_block_dev(*head, 1, 1, test, dobs.ptr, 1, None, None, None), "pg_perm_block_dev")      # obs: the last test's stays, both are timed on it
        for planes in (0, 1):
            legs[f"{tname}_planes{planes}"] = perm(P, test, planes)
            if NOSTAT is not None:
                legs[f"{tname}_planes{planes}_nostat"] = perm(NOSTAT, test, planes)
    # warm-up, and both tile paths give the same integers
    got = {}
    for k, fn in legs.items():
        for buf in (dnge, dmax):
            _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, buf.nbytes), "pg_memset")
        fn()
        ctx.sync()
        if k.startswith("trend") and not k.endswith("nostat"):
            got[k] = (dnge.download((p,), np.uint32), dmax.download((B,), np.uint64))
    assert (got["trend_planes0"][0] == got["trend_planes1"][0]).all() and (got["trend_planes0"][1] == got["trend_planes1"][1]).all()
    times = {k: [] for k in legs}
    names = list(legs)
    for r in range(a.reps):
        for k in (names if r % 2 == 0 else names[::-1]):       # alternated: the order flips every round
            times[k].append(timed(legs[k]))
    os.environ.pop("PG_PERM_PLANES", None)
    ops = 2.0 * ldk * p * B
    pairs = float(sum(min(B, p - 1 - j) for j in range(p)))
    out = {"ldk": ldk, "useful_int8_ops": ops, "ld_band": {"ms": summary(times["ld_band"]), "pairs": pairs,
                                                            "int8_POPs": round(2.0 * ldk * pairs / (np.median(times["ld_band"]) * 1e-3) / 1e15, 3)}}
    ld_rate = out["ld_band"]["int8_POPs"]
    for k in names[1:]:
        if k.endswith("nostat"):
            continue
        ms = float(np.median(times[k]))
        row = {"ms": summary(times[k]), "int8_POPs": round(ops / (ms * 1e-3) / 1e15, 3), "share_of_5_POPs": round(ops / (ms * 1e-3) / 5e15, 3)}
        row["rate_over_ld_band"] = round(row["int8_POPs"] / ld_rate, 3)
        if NOSTAT is not None:
            ns = float(np.median(times[k + "_nostat"]))
            row["nostat_ms"] = summary(times[k + "_nostat"])
            row["statistic_share"] = round(1.0 - ns / ms, 3)
        out[k] = row
    for b in (image, dlab, dlabc, dtot, dobs, dnge, dmax, dband):
        b.free()
    ctx.sync()
    return out


res = {"tool": "bench_case_control_perm", "p": p, "nperm": B, "reps": a.reps, "nostat_build": NOSTAT is not None, "sizes": {}}
for n in [int(v) for v in a.n.split(",")]:
    res["sizes"][f"n{n}"] = one_size(n)
    note(f"n={n} timed")
for e in evs:
    L.pg_event_destroy(ctx.handle, e)
ctx.close()
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
