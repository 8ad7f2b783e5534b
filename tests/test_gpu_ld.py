"""GPU checks of the LD kernels (pg_ld_encode_{bed,x}_dev, pg_ld_shift_dev, pg_ld_block_dev, pg_ld_band_dev) and of lmm.ld, ld_window,
ld_prune and clump — run with -m gpu on an MI355X.

The truth is tests/_ld_truth.py: NumPy integer arithmetic.  The six sums of every pair are compared for EQUALITY, the NaN pattern of r
for equality, pairs whose truth is exactly +-1 for equality, every other r within 2^-24 (half a float32 ulp at |r| <= 1 plus the three
fp64 roundings of the division, the product and the square root; the sums carry the exactness).  Shapes are the smallest that cross
every edge: n in {1, 3, 63, 64, 65, 129, 1030} (tails of the 16-sample store, of the 128-sample K-tile, more than one K-tile), SNP
counts in {1, 19, 86, 257, 300, 515} (across the 42-, 84- and 252-SNP tile edges, two tiles).  A panel with n >= 63 must hold fewer than
20 % NaN pairs (the truth helper gives 1-10 %), so that a kernel that returns NaN cannot pass; with n = 1 or 3 nearly every pair is
NaN by definition and the sums alone carry the test."""
import functools
import os

import numpy as np
import pandas as pd
import pytest

import _ld_truth as T

pytestmark = pytest.mark.gpu

DTYPES = {"int8": (np.int8, 0), "uint8": (np.uint8, 1), "float32": (np.float32, 2), "float64": (np.float64, 3)}
TOL = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def panel(n, p, seed, miss=0.07, specials=True):
    G = T.ld_panel(n, p, seed, miss=miss, specials=specials)
    G.setflags(write=False)
    return G


def for_kind(G, kind):
    """(what the source of this kind holds of the panel as a float64 matrix, the host array or records).  An 8-bit array has no missing
    code: its all-missing and dosage columns hold out-of-range values instead (both must come out all missing)."""
    if kind.startswith("bed"):
        V = T.bed_view(G)
        a1 = kind == "bed_a1"
        return (2.0 - V if a1 else V), T.pack(V, count_a1=False)      # the same records read with count_a1 count the other allele
    if kind in ("float32", "float64"):
        return G, G.astype(DTYPES[kind][0])
    oor = -1 if kind == "int8" else 255
    V = np.where(np.isfinite(G), G, oor)
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


def encode(ctx, kind, H, order, n, image, pe, at):
    from pygemma_amd import _lib
    L = _lib.load()
    dX, ld = upload_source(ctx, kind, H, order)
    pb = H.shape[0] if kind.startswith("bed") else H.shape[1]
    if kind.startswith("bed"):
        _lib.check(L.pg_ld_encode_bed_dev(ctx.handle, n, pb, dX.ptr, ld, int(kind == "bed_a1"), image.ptr, pe, at), "pg_ld_encode_bed_dev")
    else:
        _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, pb, dX.ptr, DTYPES[kind][1], ld, int(order == "F"), image.ptr, pe, at), "pg_ld_encode_x_dev")
    ctx.sync()
    dX.free()


def new_image(ctx, n, pe):
    from pygemma_amd import _lib
    L = _lib.load()
    nbytes = int(L.pg_ld_image_bytes(n, pe))
    assert nbytes > 0
    image = ctx.alloc(nbytes)
    _lib.check(L.pg_memset(ctx.handle, image.ptr, 0x7f, nbytes), "pg_memset")      # positions never encoded hold garbage
    return image


def windowed(ctx, rows, cols, ld, fn):
    """fn(r pointer, sums pointer) on the window [2, 2 + rows) x [0, cols) of (rows + 5)-row outputs of pitch ld > cols filled with 0x7f:
    every byte outside the window must come back as it was.  Returns (r (rows, cols) float32, sums (rows, cols, 6) int32)."""
    from pygemma_amd import _lib
    L = _lib.load()
    tot = rows + 5
    dr, ds = ctx.alloc(tot * ld * 4), ctx.alloc(tot * ld * 24)
    for b in (dr, ds):
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, b.nbytes), "pg_memset")
    fn(dr.ptr + 2 * ld * 4, ds.ptr + 2 * ld * 24)
    ctx.sync()
    r = dr.download((tot, ld), np.float32)
    s = ds.download((tot, ld, 6), np.int32)
    for full in (r, s):
        inside = np.zeros(full.shape, bool)
        inside[2:2 + rows, :cols] = True
        assert (full.view(np.uint8).reshape(full.shape + (-1,))[~inside] == 0x7f).all(), "bytes outside the window were written"
    dr.free(); ds.free()
    return np.ascontiguousarray(r[2:2 + rows, :cols]), np.ascontiguousarray(s[2:2 + rows, :cols])


def compare(r, s, S_true, n, counted=None):
    """Device r and sums against the truth sums of the same pairs.  `counted`: the pairs the NaN bound is taken over (all of them; a
    band's cells past the last SNP are NaN by definition and do not count)."""
    assert (s.astype(np.int64) == S_true).all(), "the six sums differ from the integer truth"
    R = T.r_of(S_true)
    nan = np.isnan(R)
    if n >= 63:
        assert (nan if counted is None else nan[counted]).mean() < 0.2, f"{nan.mean():.0%} of the pairs are NaN: the panel cannot tell a kernel that returns NaN"
    assert (np.isnan(r) == nan).all(), "the NaN pattern differs"
    one = ~nan & (np.abs(R) == 1)
    assert (r[one] == R[one]).all(), "a pair whose truth is exactly +-1 is not"
    err = np.abs(r[~nan].astype(np.float64) - R[~nan].astype(np.float64))
    assert err.size == 0 or err.max() <= TOL, f"|r - truth| = {err.max():.3g} > 2^-24"


def block(ctx, n, image, pe, a0, na, b0, nb):
    from pygemma_amd import _lib
    L = _lib.load()
    ldr = nb + 3
    return windowed(ctx, na, nb, ldr, lambda r, s: _lib.check(
        L.pg_ld_block_dev(ctx.handle, n, image.ptr, pe, a0, na, image.ptr, pe, b0, nb, r, ldr, s), "pg_ld_block_dev"))


CASES = [("bed", "F", 1030, 300), ("bed_a1", "F", 65, 257), ("bed", "F", 3, 19), ("bed", "F", 63, 86),
         ("int8", "C", 129, 257), ("int8", "F", 64, 86), ("uint8", "C", 63, 515), ("uint8", "F", 1, 19),
         ("float32", "C", 65, 300), ("float32", "F", 1030, 86), ("float32", "C", 3, 1), ("float32", "F", 129, 515),
         ("float64", "C", 1030, 257), ("float64", "F", 65, 19), ("float64", "C", 1, 300)]


@pytest.mark.parametrize("kind,order,n,p", CASES, ids=[f"{k}-{o}-n{n}-p{p}" for k, o, n, p in CASES])
def test_encode_and_block(ctx, kind, order, n, p):
    # five special columns out of 19 are 29 % NaN pairs on their own: the small panels go without them, so that every panel with
    # n >= 63 meets the 20 % bound (the copy, the flip and the not-hard-call columns are in every larger panel)
    V, H = for_kind(panel(n, p, n + p, 0.0 if kind.endswith("int8") else 0.07, specials=p >= 86), kind)
    at, pe = 3, p + 8
    image = new_image(ctx, n, pe)
    encode(ctx, kind, H, order, n, image, pe, at)
    off = min(2, p - 1)                                   # a0, b0, at and ldr are no multiples of a tile
    r, s = block(ctx, n, image, pe, at + off, p - off, at, p)
    compare(r, s, T.sums(V)[off:], n)
    if p >= 86 and n >= 63:
        assert r[p - 5 - off, 0] == 1.0 and r[p - 6 - off, 0] == -1.0      # the panel's copy and flip of SNP 0
    image.free()


@pytest.mark.parametrize("planes", ["", "1"])
def test_paths_give_the_same_integers(ctx, planes):
    """No missing call anywhere (one product per tile pair), one missing call in one SNP (its tile takes the three planes, the others one
    product), 7 % missing (three planes everywhere); with PG_LD_PLANES=1 the first panel takes the three planes as well."""
    n, p = 129, 300
    G0 = T.ld_panel(n, p, seed=5, miss=0.0, specials=False)
    G1 = G0.copy()
    G1[7, 260] = np.nan
    old = os.environ.get("PG_LD_PLANES")
    os.environ["PG_LD_PLANES"] = planes
    try:
        out = []
        for G in (G0, G1, panel(n, p, 11)):
            image = new_image(ctx, n, p)
            encode(ctx, "float32", G.astype(np.float32), "F", n, image, p, 0)
            r, s = block(ctx, n, image, p, 0, p, 0, p)
            compare(r, s, T.sums(G), n)
            out.append(r)
            image.free()
    finally:
        if old is None:
            del os.environ["PG_LD_PLANES"]
        else:
            os.environ["PG_LD_PLANES"] = old
    touched = np.zeros((p, p), bool)
    touched[260] = touched[:, 260] = True
    assert (out[0][~touched].view(np.uint32) == out[1][~touched].view(np.uint32)).all()


@pytest.mark.parametrize("miss", [0.07, 0.0], ids=["planes", "one-product"])
@pytest.mark.parametrize("w", [1, 7, 256, 600])
def test_band(ctx, w, miss):
    """The band mapping on both paths: with missing calls (three planes), and without any (one product per tile pair, N = n and the per-SNP
    totals at j0 > 0; no specials, their all-missing column would send its tile down the other path)."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = 65, 515
    G = panel(n, p, 21, miss, specials=miss > 0)
    pe, j0, have = p + 4, 5, p - 3                        # the image holds more SNPs than `have`: they must not be read as partners
    image = new_image(ctx, n, pe)
    encode(ctx, "float64", np.asarray(G), "C", n, image, pe, 0)
    rows, ldo = have - j0, w + 2
    r, s = windowed(ctx, rows, w, ldo, lambda rp, sp: _lib.check(
        L.pg_ld_band_dev(ctx.handle, n, image.ptr, pe, j0, rows, have, w, rp, ldo, sp), "pg_ld_band_dev"))
    S = T.band_of(T.sums(G[:, :have]), w, fill=0)[j0:]
    beyond = (np.arange(j0, have)[:, None] + 1 + np.arange(w)[None, :]) >= have
    compare(r, s, S, n, counted=~beyond)
    assert np.isnan(r[beyond]).all() and (s[beyond] == 0).all()
    if miss == 0:
        assert (s[~beyond][:, 0] == n).all()
    image.free()


def test_float64_is_classified_in_its_own_precision(ctx):
    """A double that only float32 rounding would turn into 1, and a finite double beyond float32's range, are values other than 0, 1, 2:
    their SNPs are all missing.  The same columns as float32 hold exactly 1 and +Inf (a missing call)."""
    n, p = 65, 20
    G = np.array(T.ld_panel(n, p, 7, miss=0.0, specials=False))
    G[3, 4] = 1.0 + 1e-12
    G[5, 9] = 1e300
    assert (T.sums(G)[4] == 0).all() and (T.sums(G)[9] == 0).all()
    with np.errstate(over="ignore"):
        G32 = G.astype(np.float32).astype(np.float64)      # 1e300 -> +Inf
    for kind, V in (("float64", G), ("float32", G32)):
        image = new_image(ctx, n, p)
        with np.errstate(over="ignore"):
            H = V.astype(DTYPES[kind][0])
        encode(ctx, kind, H, "F", n, image, p, 0)
        r, s = block(ctx, n, image, p, 0, p, 0, p)
        compare(r, s, T.sums(V), n)
        image.free()
    assert s[4, 4, 0] == n and s[9, 0, 0] == n - 1      # as float32: a hard call, and one missing call


def test_shift_is_overlap_safe(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = 129, 300
    G = panel(n, p, 31)
    image = new_image(ctx, n, p)
    encode(ctx, "float32", G.astype(np.float32), "C", n, image, p, 0)
    _lib.check(L.pg_ld_shift_dev(ctx.handle, n, image.ptr, p, 40, 260), "pg_ld_shift_dev")      # count > from: the runs overlap
    r, s = block(ctx, n, image, p, 0, 260, 1, 259)
    compare(r, s, T.sums(G[:, 40:])[:, 1:], n)
    image.free()


@functools.lru_cache(maxsize=None)
def window_case():
    n, p = 129, 515
    G = panel(n, p, 41)
    return n, p, G, T.r_of(T.sums(G))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("window", [7, 300])
def test_ld_window_does_not_depend_on_the_batches_or_the_storage(window):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    n, p, G, R = window_case()
    want = T.band_of(R, window)
    X = G.astype(np.float32)
    stats = {}
    bands = [lmm.ld_window(X, window, snp_batch=sb, stats=stats) for sb in (64, 130, 515)]
    assert stats["batches"] == 1 and stats["bytes_in"] == X.nbytes and stats["seconds"] > 0
    for b in bands:
        assert b.shape == (p, window) and b.dtype == np.float32
        assert (bits(b) == bits(bands[0])).all(), "the band depends on the batch boundaries"
    nan = np.isnan(want)
    assert (np.isnan(bands[0]) == nan).all()
    assert np.abs(bands[0][~nan].astype(np.float64) - want[~nan]).max() <= TOL
    one = ~nan & (np.abs(want) == 1)
    assert one.any() and (bands[0][one] == want[one]).all()
    # the dosage column is not hard-call: all missing, which is what the .bed file keeps of it
    bed = PackedBed(T.pack(T.bed_view(G)), n)
    for Xs in (bed, np.asfortranarray(G)):
        assert (bits(lmm.ld_window(Xs, window, snp_batch=130)) == bits(bands[0])).all()


def test_ld_window_comes_back_batch_by_batch_when_the_band_does_not_fit(monkeypatch):
    from pygemma_amd import _lib, lmm
    n, p, G, R = window_case()
    w, pb = 300, 64
    want = lmm.ld_window(G, w, snp_batch=pb)
    L = _lib.load()
    # room for the image, the slots and one batch of the band, not for the whole band
    need = 4 * (pb + w) * w + int(L.pg_ld_image_bytes(n, pb + w)) + 2 * pb * n * 8
    assert 0.9 * (need + 4096) < 4 * p * w + int(L.pg_ld_image_bytes(n, 128 + w))
    real = _lib.Context.mem_info
    monkeypatch.setattr(_lib.Context, "mem_info", lambda self: (need + 4096, real(self)[1]))
    got = lmm.ld_window(G, w, snp_batch=pb)
    assert (bits(got) == bits(want)).all()
    with pytest.raises(_lib.PgError, match="GiB of device memory"):
        lmm.ld_window(G, w, snp_batch=2 * pb)


def test_ld_that_does_not_fit_the_device_is_refused(monkeypatch):
    from pygemma_amd import _lib, lmm
    n, p, G, R = window_case()
    real = _lib.Context.mem_info
    monkeypatch.setattr(_lib.Context, "mem_info", lambda self: (4 * p * p, real(self)[1]))      # the r matrix alone
    with pytest.raises(_lib.PgError, match="ld: n=129, 515 x 515 SNPs.*GiB of device memory"):
        lmm.ld(G)


def test_ld_masks_indices_and_counts():
    from pygemma_amd import lmm
    n, p, G, R = window_case()
    S = T.sums(G)
    X = np.asfortranarray(G.astype(np.float32))
    ia = np.array([3, 500, 17, -1, 17])                   # any order, negative, repeated
    mb = np.zeros(p, bool)
    mb[100:400:3] = True
    r, s = lmm.ld(X, ia, mb, counts=True)
    rows = np.where(ia < 0, ia + p, ia)
    compare(r, s, S[np.ix_(rows, np.flatnonzero(mb))], n)
    r2 = lmm.ld(X, ia, np.flatnonzero(mb))
    assert (bits(r2) == bits(r)).all()
    sq = lmm.ld(X, mb)                                    # b=None: b = a
    assert sq.shape == (100, 100) and (bits(sq) == bits(lmm.ld(X, mb, mb))).all()
    full, sf = lmm.ld(X, counts=True)
    compare(full, sf, S, n)


def _clear_of(R, r2):
    with np.errstate(invalid="ignore"):
        d = np.abs(R.astype(np.float64) ** 2 - r2)
    return np.nanmin(d) > 1e-6


@pytest.mark.parametrize("window,r2", [(50, 0.5), (7, 0.2)])
def test_ld_prune_end_to_end(window, r2):
    from pygemma_amd import lmm
    n, p, G, R = window_case()
    assert _clear_of(R, r2), "an r^2 of the panel lies within 1e-6 of the threshold"
    keep = lmm.ld_prune(G, window, r2, snp_batch=130)
    want = T.prune(R, window, r2)
    assert keep.dtype == np.bool_ and (keep == want).all() and 0.1 * p < keep.sum() < 0.9 * p


def test_clump_finds_the_planted_loci():
    from pygemma_amd import lmm
    n, p, G, R = window_case()
    r2 = 0.5
    assert _clear_of(R, r2)
    rng = np.random.default_rng(3)
    pv = rng.uniform(0.05, 1, p)
    pv[rng.random(p) < 0.05] = np.nan
    lead = [60, 250, 430]
    for k, j in enumerate(lead):                          # a locus: the lead SNP and every SNP near it that is in LD with it
        near = [i for i in range(max(0, j - 20), min(p, j + 21)) if i != j and T.in_ld(R[min(i, j), max(i, j)], r2)]
        assert len(near) >= 2 and not np.isnan(R[j, j])
        pv[near] = rng.uniform(1e-6, 5e-3, len(near))
        pv[j] = 10.0 ** -(11 - k)
    df = pd.DataFrame({"p_wald": pv, "SNPs": [f"rs{j}" for j in range(p)]})
    want = T.clump(R, pv, 1e-8, 1e-2, r2, 40)
    assert [j for j, _ in want] == lead
    out = lmm.clump(df, G, p1=1e-8, p2=1e-2, r2=r2, window=40, snp_batch=64)
    assert list(out.columns) == ["index", "SNPs", "p", "n_members", "members"]
    assert out["index"].tolist() == lead and out["SNPs"].tolist() == [f"rs{j}" for j in lead] and (out["p"].to_numpy() == pv[lead]).all()
    for (j, mem), got, cnt in zip(want, out["members"], out["n_members"]):
        assert got.dtype == np.int64 and got.tolist() == mem and cnt == len(mem)
    chrom = np.repeat([1, 2], [250, p - 250])             # the second lead SNP is the first of its chromosome: it loses its left side
    want = T.clump(R, pv, 1e-8, 1e-2, r2, 40, chrom=chrom)
    out = lmm.clump(df, G, p1=1e-8, p2=1e-2, r2=r2, window=40, chrom=chrom)
    assert [(j, mem) for j, mem in want] == [(j, m.tolist()) for j, m in zip(out["index"], out["members"])]


def test_pruned_panel_goes_straight_into_kinship():
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    n, p, G, R = window_case()
    V = T.bed_view(G)
    keep_cols = ~np.isnan(V).all(axis=0)                  # kinship's own contract for all-missing records is not at stake here
    bed = PackedBed(T.pack(V[:, keep_cols]), n)
    keep = lmm.ld_prune(bed)
    assert keep.shape == (bed.p,) and 0 < keep.sum() < bed.p
    K = lmm.kinship(bed.take(keep))
    K2 = lmm.kinship(PackedBed(np.ascontiguousarray(bed.data[np.flatnonzero(keep)]), n))
    assert K.shape == (n, n) and (bits(K) == bits(K2)).all()
