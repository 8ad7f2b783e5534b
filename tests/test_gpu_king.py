"""GPU checks of the KING kernels (pg_king_{bed,x}_acc_dev, pg_king_finish_dev, pg_king_counts_dev, pg_sample_stats_{bed,x}_acc_dev) and
of lmm.king, ibs, sample_stats, unrelated and PackedBed.take_samples — run with -m gpu on an MI355X.

The truth is tests/_king_truth.py: NumPy int64 arithmetic.  The pair counts N, HH, IBS0, Hij, IBS1 and the five per-sample counts are
compared for EQUALITY, phi and ibs for BIT equality (NaN pattern included) with np.float32(np.float64(num) / np.float64(den)).  Shapes are
the smallest that cross every edge: n in {1, 2, 3, 63, 64, 65, 255, 256, 257, 515} (a single sample, the 16- and 64-sample edges, the
256-sample tile of the encode and of the pair kernel with its tails, two output tiles with a tail), SNPs per batch in {1, 15, 16, 17, 127,
128, 129, 300, 513} (the 16-SNP store group, the 128-SNP K-tile and the four K-tiles of an encode workgroup with their tails).  Every
case runs down both paths (PG_KING_PLANES unset and 1).  On every panel with p >= 17 fewer than 5 % of the pairs (those of a sample
without any call aside) may be NaN in phi, so that a kernel that returns NaN cannot pass; at p = 1 the counts carry the test."""
import functools
import os

import numpy as np
import pytest

import _king_truth as T

pytestmark = pytest.mark.gpu

DTYPES = {"int8": (np.int8, 0), "uint8": (np.uint8, 1), "float32": (np.float32, 2), "float64": (np.float64, 3)}
SOURCES = [("bed", "F"), ("bed_a1", "F")] + [(k, o) for k in DTYPES for o in ("C", "F")]
N_EDGES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 515]
PB_EDGES = [1, 15, 16, 17, 127, 128, 129, 300, 513]
MATS = ("N", "HH", "IBS0", "Hij", "IBS1")


def _cases():
    pairs = []
    for k, n in enumerate(N_EDGES):
        pairs += [(n, PB_EDGES[k % 9]), (n, PB_EDGES[(k + 4) % 9])]
    for k, p in enumerate(PB_EDGES):
        pairs += [(N_EDGES[(k + 2) % 10], p), (N_EDGES[(k + 6) % 10], p)]
    pairs = list(dict.fromkeys(pairs))
    return [(*SOURCES[i % len(SOURCES)], n, p) for i, (n, p) in enumerate(pairs)]


CASES = _cases()


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(params=["", "1"], ids=["auto", "planes"])
def planes(request):
    old = os.environ.get("PG_KING_PLANES")
    os.environ["PG_KING_PLANES"] = request.param
    yield request.param
    if old is None:
        del os.environ["PG_KING_PLANES"]
    else:
        os.environ["PG_KING_PLANES"] = old


@functools.lru_cache(maxsize=None)
def panel(n, p, seed, miss=0.07):
    G = T.king_panel(n, p, seed, miss=miss)
    G.setflags(write=False)
    return G


def for_kind(G, kind):
    """(what the source of this kind holds of the panel as a float64 matrix, the host array or records).  An 8-bit array has no missing
    code: its all-missing and dosage columns hold out-of-range values instead (both must come out all missing), and the sample without
    any call becomes a hom-0 sample."""
    if kind.startswith("bed"):
        V = T.bed_view(G)
        return (2.0 - V if kind == "bed_a1" else V), T.pack(V, count_a1=False)      # the same records read with count_a1 count the other allele
    if kind in ("float32", "float64"):
        return G, G.astype(DTYPES[kind][0])
    V = np.array(G)
    gone = np.isnan(V).all(axis=1)
    if gone.any() and (~gone).any():
        V[gone] = np.where(np.isnan(V[~gone]).all(axis=0), np.nan, 0.0)
    V = np.where(np.isfinite(V), V, -1 if kind == "int8" else 255)
    V = np.where(V == 0.5, 3, V)
    return V, V.astype(DTYPES[kind][0])


def upload_source(ctx, kind, H, order):
    """The host source on the device at a padded pitch whose pad bytes hold 0xff; returns (buffer, pitch in elements)."""
    if kind.startswith("bed"):
        ld = H.shape[1] + 5
        buf = np.full((H.shape[0], ld), 0xff, np.uint8)
        buf[:, :H.shape[1]] = H
        return ctx.to_device(buf), ld
    M = H.T if order == "F" else H                      # SNP-major: (p, n) rows
    ld = M.shape[1] + 3
    buf = np.full((M.shape[0], ld * M.itemsize), 0xff, np.uint8).view(M.dtype)
    buf[:, :M.shape[1]] = M
    return ctx.to_device(buf), ld


def run_abi(ctx, kind, order, H, n, batches):
    """The batches [(s, e)] of a source through the C ABI into one accumulator: scratch pre-filled with 0x7f, zeros only where the contract
    says zero.  Returns the dict of the five count matrices, `samples` (n, 5), phi and ibs."""
    from pygemma_amd import _lib
    L = _lib.load()
    pbmax = max(e - s for s, e in batches)
    nbytes, zero = int(L.pg_king_acc_bytes(n, pbmax)), int(L.pg_king_zero_bytes(n))
    assert 0 < zero < nbytes
    acc = ctx.alloc(nbytes)
    _lib.check(L.pg_memset(ctx.handle, acc.ptr, 0x7f, nbytes), "pg_memset")
    _lib.check(L.pg_memset(ctx.handle, acc.ptr, 0, zero), "pg_memset")
    ds = ctx.alloc(40 * n)
    _lib.check(L.pg_memset(ctx.handle, ds.ptr, 0, 40 * n), "pg_memset")
    for s, e in batches:
        pb = e - s
        if kind.startswith("bed"):
            dX, ld = upload_source(ctx, kind, H[s:e], order)
            a1 = int(kind == "bed_a1")
            _lib.check(L.pg_king_bed_acc_dev(ctx.handle, n, pb, dX.ptr, ld, a1, acc.ptr), "pg_king_bed_acc_dev")
            _lib.check(L.pg_sample_stats_bed_acc_dev(ctx.handle, n, pb, dX.ptr, ld, a1, ds.ptr), "pg_sample_stats_bed_acc_dev")
        else:
            dX, ld = upload_source(ctx, kind, np.ascontiguousarray(H[:, s:e]), order)
            code, f = DTYPES[kind][1], int(order == "F")
            _lib.check(L.pg_king_x_acc_dev(ctx.handle, n, pb, dX.ptr, code, ld, f, acc.ptr), "pg_king_x_acc_dev")
            _lib.check(L.pg_sample_stats_x_acc_dev(ctx.handle, n, pb, dX.ptr, code, ld, f, ds.ptr), "pg_sample_stats_x_acc_dev")
        ctx.sync()
        dX.free()
    guard = 64
    outs = [ctx.alloc(4 * n * n + guard) for _ in range(2)]
    dc, d5 = ctx.alloc(20 * n * n + guard), ctx.alloc(40 * n + guard)
    for b in outs + [dc, d5]:
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, b.nbytes), "pg_memset")
    for what, b in enumerate(outs):
        _lib.check(L.pg_king_finish_dev(ctx.handle, n, acc.ptr, what, b.ptr), "pg_king_finish_dev")
    _lib.check(L.pg_king_counts_dev(ctx.handle, n, acc.ptr, dc.ptr, d5.ptr), "pg_king_counts_dev")
    ctx.sync()
    for b, used in ((outs[0], 4 * n * n), (outs[1], 4 * n * n), (dc, 20 * n * n), (d5, 40 * n)):
        assert (b.download((guard,), np.uint8, offset=used) == 0x7f).all(), "bytes behind an output were written"
    mats = dc.download((5, n, n), np.int32)
    res = {k: mats[t] for t, k in enumerate(MATS)}
    res["samples"], res["stats_only"] = d5.download((n, 5), np.int64), ds.download((n, 5), np.int64)
    res["phi"], res["ibs"] = outs[0].download((n, n), np.float32), outs[1].download((n, n), np.float32)
    for b in outs + [dc, d5, ds, acc]:
        b.free()
    return res


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def compare(res, V, p):
    """Device counts, phi and ibs against the truth of the panel V (what the source holds)."""
    C = T.counts(V)
    for k in MATS:
        assert (res[k].astype(np.int64) == C[k]).all(), f"{k} differs from the integer truth"
    assert (res["N"] == res["N"].T).all() and (res["IBS0"] == res["IBS0"].T).all() and (res["IBS1"] == res["IBS1"].T).all()
    S = T.sample_counts(V)
    assert (res["samples"] == S).all(), "the per-sample counts of the pair stream differ from the truth"
    if "stats_only" in res:
        assert (res["stats_only"] == S).all(), "the per-sample counts of the count kernel alone differ from the truth"
    phi, ibs = T.phi_of(C), T.ibs_of(C)
    if p >= 17:
        live = np.diag(C["N"]) > 0
        nan = np.isnan(phi)[np.ix_(live, live)]
        assert nan.mean() < 0.05, f"{nan.mean():.0%} of the pairs are NaN: the panel cannot tell a kernel that returns NaN"
    assert (np.isnan(res["phi"]) == np.isnan(phi)).all() and (np.isnan(res["ibs"]) == np.isnan(ibs)).all(), "the NaN pattern differs"
    assert (bits(res["phi"]) == bits(phi)).all(), "phi is not the correctly rounded quotient of the counts"
    assert (bits(res["ibs"]) == bits(ibs)).all(), "ibs is not the correctly rounded value of the counts"
    assert (bits(res["phi"]) == bits(res["phi"].T)).all() and (bits(res["ibs"]) == bits(res["ibs"].T)).all()
    return C


@pytest.mark.parametrize("kind,order,n,p", CASES, ids=[f"{k}-{o}-n{n}-p{p}" for k, o, n, p in CASES])
def test_one_batch(ctx, planes, kind, order, n, p):
    V, H = for_kind(panel(n, p, n + p, 0.0 if kind.endswith("int8") else 0.07), kind)
    res = run_abi(ctx, kind, order, H, n, [(0, p)])
    compare(res, V, p)
    if n >= 16 and p >= 17:
        assert res["phi"][n - 1, 0] == 0.5 and res["phi"][0, n - 1] == 0.5          # the duplicate of sample 0


@pytest.mark.parametrize("kind,order", [("bed", "F"), ("float32", "C"), ("float64", "F"), ("int8", "C")])
def test_a_panel_without_missing_calls_takes_both_paths_to_the_same_integers(ctx, kind, order):
    n, p = 257, 300
    G = T.ld_panel(n, p, seed=5, miss=0.0, specials=False)
    V, H = for_kind(G, kind)
    out = []
    old = os.environ.get("PG_KING_PLANES")
    try:
        for env in ("", "1"):
            os.environ["PG_KING_PLANES"] = env
            out.append(run_abi(ctx, kind, order, H, n, [(0, p)]))
            C = compare(out[-1], V, p)
    finally:
        if old is None:
            del os.environ["PG_KING_PLANES"]
        else:
            os.environ["PG_KING_PLANES"] = old
    assert (C["N"] == p).all()
    for k in MATS:
        assert (out[0][k] == out[1][k]).all()
    assert (bits(out[0]["phi"]) == bits(out[1]["phi"])).all()


@pytest.mark.parametrize("kind,order", [("bed_a1", "F"), ("float32", "F"), ("uint8", "C")])
def test_the_path_switches_in_mid_stream(ctx, planes, kind, order):
    """The first batch has no missing call (two products, totals), the second has one (five products); a third is a tail of 44 SNPs."""
    n, p = 65, 300
    G = T.ld_panel(n, p, seed=9, miss=0.0, specials=False)
    if not kind.endswith("int8"):
        G[5, 200] = np.nan
    else:
        G[:, 200] = 3.0              # an 8-bit batch has no missing call: a SNP that is not hard-call in a batch that takes the totals
    V, H = for_kind(G, kind)
    res = run_abi(ctx, kind, order, H, n, [(0, 128), (128, 256), (256, 300)])
    C = compare(res, V, p)
    assert C["N"].max() == (p if not kind.endswith("int8") else p - 1)


def test_specials(ctx, planes):
    n, p = 65, 300
    G = panel(n, p, 77)
    res = run_abi(ctx, "float64", "C", np.array(G), n, [(0, p)])
    C = compare(res, G, p)
    phi = res["phi"]
    assert phi[n - 1, 0] == 0.5 and (np.diag(phi)[np.diag(C["HH"]) > 0] == 0.5).all()
    assert np.isnan(phi[n - 2]).all() and np.isnan(phi[:, n - 2]).all() and (res["N"][n - 2] == 0).all() and np.isnan(res["ibs"][n - 2]).all()
    assert np.isnan(phi[n - 3, n - 3]) and res["samples"][n - 3, 3] == 0
    # without the dosage column and the all-missing SNP: the same pair counts, one missing call less per column and sample
    cols = np.ones(p, bool)
    cols[[p - 8, p - 3]] = False
    G2 = np.ascontiguousarray(G[:, cols])
    res2 = run_abi(ctx, "float64", "C", G2, n, [(0, p - 2)])
    for k in MATS:
        assert (res[k] == res2[k]).all()
    assert (bits(phi) == bits(res2["phi"])).all()
    assert (res["samples"][:, 1] == res2["samples"][:, 1] + 2).all() and (res["samples"][:, [0, 2, 3, 4]] == res2["samples"][:, [0, 2, 3, 4]]).all()


def test_timing_changes_no_result(ctx, monkeypatch):
    """PG_KING_TIMING=1 brackets a batch with events: the same integers, and both parts of the last batch took time."""
    import ctypes as C
    from pygemma_amd import _lib
    n, p = 257, 300
    G = panel(n, p, 13)
    plain = run_abi(ctx, "float32", "C", G.astype(np.float32), n, [(0, 128), (128, 300)])
    monkeypatch.setenv("PG_KING_TIMING", "1")
    timed = run_abi(ctx, "float32", "C", G.astype(np.float32), n, [(0, 128), (128, 300)])
    enc, pair = C.c_float(), C.c_float()
    _lib.check(_lib.load().pg_king_last_batch_ms(C.byref(enc), C.byref(pair)), "pg_king_last_batch_ms")
    assert enc.value > 0 and pair.value > 0
    compare(timed, G, p)
    for k in MATS:
        assert (plain[k] == timed[k]).all()
    assert (bits(plain["phi"]) == bits(timed["phi"])).all()


def test_float64_is_classified_in_its_own_precision(ctx):
    n, p = 65, 20
    G = np.array(T.ld_panel(n, p, 7, miss=0.0, specials=False))
    G[3, 4] = 1.0 + 1e-12
    G[5, 9] = 1e300
    res = run_abi(ctx, "float64", "F", G, n, [(0, p)])
    C = compare(res, G, p)
    assert C["N"].max() == p - 2
    with np.errstate(over="ignore"):
        G32 = G.astype(np.float32)      # exactly 1, and +Inf: a missing call
    res = run_abi(ctx, "float32", "F", G32, n, [(0, p)])
    C = compare(res, G32.astype(np.float64), p)
    assert C["N"].max() == p and C["N"][5, 5] == p - 1


# ---- the public surface ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cohort():
    n, p = 64, 2000
    G = panel(n, p, 2)
    return n, p, G, T.counts(G)


def frame_counts(df):
    return df[["n_obs", "n_miss", "n0", "n1", "n2"]].to_numpy()


def test_batch_seams_do_not_show():
    from pygemma_amd import lmm
    n, p = 257, 300
    G = panel(n, p, 13)
    X = G.astype(np.float32)
    stats = {}
    runs = [lmm.king(X, counts=True, snp_batch=sb, stats=stats) for sb in (300, 128, 17)]
    assert stats["batches"] == 18 and stats["bytes_in"] == X.nbytes and stats["seconds"] > 0
    res = dict(runs[0][1], phi=runs[0][0], ibs=lmm.ibs(X, snp_batch=128))
    res["samples"] = frame_counts(res["samples"])
    res["IBS1"] = res["Hij"] + res["Hij"].T - 2 * res["HH"]
    compare(res, G, p)
    for phi, extra in runs[1:]:
        assert (bits(phi) == bits(runs[0][0])).all(), "phi depends on the batch boundaries"
        for k in ("N", "HH", "IBS0", "Hij"):
            assert extra[k].dtype == np.int32 and (extra[k] == runs[0][1][k]).all()
        assert (frame_counts(extra["samples"]) == res["samples"]).all()


def test_king_ibs_and_sample_stats_on_every_storage():
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    n, p, G, C = cohort()
    V = T.bed_view(G)
    CV = T.counts(V)
    bed = PackedBed(T.pack(V), n)
    pinned = lmm.pinned_empty((n, p), np.float32)
    pinned[:] = G
    pinned8 = lmm.pinned_empty((n, p), np.int8)
    X8 = for_kind(panel(n, p, 2, 0.0), "int8")           # an 8-bit array has no missing code: the panel without missing calls
    pinned8[:] = X8[1]
    sources = [(bed, V), (G.astype(np.float32), G), (np.asfortranarray(G), G), (pinned, G), (pinned8, X8[0]), (np.asfortranarray(X8[1]), X8[0])]
    for X, W in sources:
        Cw = T.counts(W)
        stats = {}
        phi = lmm.king(X, stats=stats)
        assert phi.shape == (n, n) and phi.dtype == np.float32 and sorted(stats) == ["batches", "bytes_in", "seconds"]
        assert (bits(phi) == bits(T.phi_of(Cw))).all()
        assert (bits(lmm.ibs(X, snp_batch=700)) == bits(T.ibs_of(Cw))).all()
        stats = {}
        st = lmm.sample_stats(X, samples=[f"id{i}" for i in range(n)], snp_batch=700, stats=stats)
        assert list(st.columns) == ["n_obs", "n_miss", "n0", "n1", "n2", "miss", "het", "samples"] and stats["batches"] == 3
        S = T.sample_counts(W)
        assert (frame_counts(st) == S).all() and st["n_obs"].dtype == np.int64
        assert (st["miss"].to_numpy() == S[:, 1] / float(p)).all()
        with np.errstate(invalid="ignore", divide="ignore"):
            het = S[:, 3] / S[:, 0].astype(np.float64)
        assert np.array_equal(st["het"].to_numpy(), het, equal_nan=True)
    # counting the other allele: the same phi, n0 and n2 swapped
    bed_a1 = PackedBed(T.pack(V), n, count_A1=True)
    phi, extra = lmm.king(bed_a1, counts=True)
    assert (bits(phi) == bits(T.phi_of(CV))).all()
    assert sorted(extra) == ["HH", "Hij", "IBS0", "N", "samples"]
    assert (frame_counts(extra["samples"]) == T.sample_counts(V, count_a1=True)).all()
    for k in ("N", "HH", "IBS0", "Hij"):
        assert extra[k].dtype == np.int32 and extra[k].shape == (n, n) and (extra[k] == CV[k]).all()
    assert not (extra["Hij"] == extra["Hij"].T).all()


def test_unrelated_subset_stays_packed_and_goes_into_kinship():
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    n, p, G, C = cohort()
    V = T.bed_view(G)
    bed = PackedBed(T.pack(V), n)
    phi = lmm.king(bed)
    keep = lmm.unrelated(phi, 0.177)
    assert (keep == T.unrelated(T.phi_of(T.counts(V)), 0.177)).all()
    assert not keep[n - 1] and keep[0], "the duplicate of sample 0 stays"
    assert (~keep[[1, 2, n - 4]]).sum() == 1 and (~keep).sum() == 2, "parent and child both stay, or more than they and the duplicate went"
    pairs = lmm.related_pairs(phi, 0.177)
    assert pairs.iloc[0].tolist() == [0, n - 1, 0.5] and len(pairs) == 3
    sub = bed.take_samples(keep)
    assert isinstance(sub, PackedBed) and sub.n == n - 2
    live = ~np.isnan(V[keep]).all(axis=0)                 # kinship's own contract for all-missing records is not at stake here
    sub = sub.take(live)
    K = lmm.kinship(sub)
    K2 = lmm.kinship(PackedBed(T.pack(V[keep][:, live]), n - 2))
    assert K.shape == (n - 2, n - 2) and (bits(K) == bits(K2)).all()
    assert len(lmm.related_pairs(lmm.king(sub), 0.177)) == 0
