"""GPU checks of the LD score kernel (pg_ld_score_dev) and of lmm.ld_scores — run with -m gpu on an MI355X.

The truth is tests/_ld_score_truth.py: the kernel's three (five) float64 operations on exact int64 terms, np.rint to fixed point at
2^-32, int64 sums.  Every operation is correctly rounded on both sides and the sums are integers, so `sum`, `npairs` and `nobs` are
compared for EQUALITY.  Shapes as in test_gpu_ld: n in {1, 3, 63, 65, 129, 1030}, p in {19, 86, 257, 300, 515}, windows across the 42-,
84- and 252-SNP edges.  For n >= 63 fewer than 20 % of the visited pairs may be undefined, so that a kernel that credits nothing cannot
pass; with n = 1 or 3 nearly every pair is undefined by definition and the equality alone carries the test."""
import functools
import os

import numpy as np
import pytest

import _ld_score_truth as ST
import _ld_truth as T

pytestmark = pytest.mark.gpu

GUARD = 4          # words before and after every output
EINVAL = -22


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def panel(n, p, seed, miss, specials):
    G = T.ld_panel(n, p, seed, miss=miss, specials=specials)
    G.setflags(write=False)
    return G, T.sums(G)


def new_image(ctx, G, pe):
    """The float64 panel encoded at positions [0, p) of an image for pe SNPs whose other positions hold garbage."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = G.shape
    nbytes = int(L.pg_ld_image_bytes(n, pe))
    assert nbytes > 0
    image = ctx.alloc(nbytes)
    _lib.check(L.pg_memset(ctx.handle, image.ptr, 0x7f, nbytes), "pg_memset")
    dX = ctx.to_device(np.ascontiguousarray(G))
    _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, p, dX.ptr, 3, p, 0, image.ptr, pe, 0), "pg_ld_encode_x_dev")
    ctx.sync()
    dX.free()
    return image


class Outputs:
    """sum, npairs and nobs of pe entries on the device, preset to a non-zero pattern, between guard words."""

    def __init__(self, ctx, pe):
        i = np.arange(pe + 2 * GUARD, dtype=np.int64)
        self.ctx, self.pe = ctx, pe
        self.host = [1000 + 7 * i, (3 + i).astype(np.int32), (-5 - i).astype(np.int32)]
        self.dev = [ctx.to_device(h) for h in self.host]

    def ptrs(self):
        return [d.ptr + GUARD * h.itemsize for d, h in zip(self.dev, self.host)]

    def read(self):
        """(what the call added to sum, to npairs; nobs as it is now, the preset nobs), the guard words checked."""
        now = [d.download(h.shape, h.dtype) for d, h in zip(self.dev, self.host)]
        for a, h in zip(now, self.host):
            assert (a[:GUARD] == h[:GUARD]).all() and (a[-GUARD:] == h[-GUARD:]).all(), "a guard word was written"
        inner = slice(GUARD, GUARD + self.pe)
        return now[0][inner] - self.host[0][inner], now[1][inner].astype(np.int64) - self.host[1][inner], now[2][inner], self.host[2][inner]

    def untouched(self):
        return all((d.download(h.shape, h.dtype) == h).all() for d, h in zip(self.dev, self.host))

    def free(self):
        for d in self.dev:
            d.free()


def score(ctx, n, image, pe, j0, rows, have, w, reach, adjust, out):
    from pygemma_amd import _lib
    L = _lib.load()
    dreach = None if reach is None else ctx.to_device(np.asarray(reach, np.int32))
    _lib.check(L.pg_ld_score_dev(ctx.handle, n, image.ptr, pe, j0, rows, have, w, None if reach is None else dreach.ptr, adjust, *out.ptrs()),
               "pg_ld_score_dev")
    ctx.sync()
    if dreach is not None:
        dreach.free()


# n, p, w, missing calls, adjust, a reach per row, PG_LD_PLANES
CASES = [(1030, 257, 100, 0.07, 1, False, ""), (1030, 257, 253, 0.0, 0, True, ""), (129, 515, 64, 0.07, 1, True, ""), (129, 515, 600, 0.0, 1, False, ""),
         (129, 515, 252, 0.0, 0, False, "1"), (129, 515, 251, 0.07, 0, False, ""), (65, 300, 300, 0.07, 0, False, ""), (65, 300, 84, 0.0, 1, True, "1"),
         (65, 300, 43, 0.07, 1, True, ""), (65, 300, 42, 0.0, 0, False, ""), (63, 86, 41, 0.07, 0, True, ""), (63, 86, 40, 0.0, 1, False, ""),
         (63, 86, 5, 0.07, 1, False, ""), (65, 257, 1, 0.0, 1, False, ""), (3, 19, 5, 0.07, 1, False, ""), (3, 19, 5, 0.07, 0, True, ""),
         (1, 19, 1, 0.0, 1, False, ""), (1, 19, 19, 0.07, 0, False, "")]


@pytest.mark.parametrize("n,p,w,miss,adjust,per_row,planes", CASES, ids=[f"n{c[0]}-p{c[1]}-w{c[2]}-miss{c[3]}-adj{c[4]}-reach{int(c[5])}-planes{c[6]}"
                                                                         for c in CASES])
def test_score_is_the_host_model(ctx, n, p, w, miss, adjust, per_row, planes):
    """j0 > 0 and have < p <= pe: the rows before j0 are not visited, the partners at or past `have` (encoded SNPs among them) add
    nothing.  The outputs hold a pattern: sum and npairs grow by the truth, nobs is overwritten for the rows alone."""
    G, S = panel(n, p, n + p, miss, miss > 0 and p >= 86)
    pe, j0, have = p + 4, 5, p - 3
    rows = have - j0
    reach = None
    if per_row:
        reach = np.random.default_rng(w).integers(0, w + 1, pe)
        reach[j0 + 1::9] = 0
    visit = ST.forward_mask(p, j0, rows, have, w, None if reach is None else reach[:p])
    tot, cnt, undefined = ST.credit(S, visit, adjust)
    assert visit.sum() > 0
    if n >= 63:
        assert undefined < 0.2, f"{undefined:.0%} of the visited pairs are undefined: the panel cannot tell a kernel that credits nothing"
    image, out = new_image(ctx, G, pe), Outputs(ctx, pe)
    old = os.environ.get("PG_LD_PLANES")
    os.environ["PG_LD_PLANES"] = planes
    try:
        score(ctx, n, image, pe, j0, rows, have, w, reach, adjust, out)
    finally:
        if old is None:
            del os.environ["PG_LD_PLANES"]
        else:
            os.environ["PG_LD_PLANES"] = old
    dsum, dcnt, nobs, nobs_before = out.read()
    pad = np.zeros(pe - p, np.int64)
    assert (dcnt == np.concatenate([cnt, pad])).all(), "npairs differs from the truth"
    assert (dsum == np.concatenate([tot, pad])).all(), "sum differs from the integer truth"
    is_row = (np.arange(pe) >= j0) & (np.arange(pe) < j0 + rows)
    assert (nobs[is_row] == ST.nobs(G)[j0:j0 + rows]).all(), "nobs differs from the truth"
    assert (nobs[~is_row] == nobs_before[~is_row]).all(), "nobs was written outside the rows"
    image.free(); out.free()


@pytest.mark.parametrize("miss", [0.0, 0.1], ids=["complete", "missing"])
def test_specials(ctx, miss):
    """A copy and a flip of a SNP are r^2 = 1 exactly: 2^32 a pair without the adjustment.  A monomorphic, an all-missing and a dosage
    column are nobody's partner."""
    n = 129
    rng = np.random.default_rng(3)
    x = rng.binomial(2, 0.3, n).astype(np.float64)
    x[rng.random(n) < miss] = np.nan
    y = rng.binomial(2, 0.4, n).astype(np.float64)
    G = np.stack([x, x, 2 - x, np.ones(n), np.full(n, np.nan), np.where(np.arange(n) % 2 == 0, 0.5, 1.0), y], axis=1)
    p = G.shape[1]
    image, out = new_image(ctx, G, p), Outputs(ctx, p)
    score(ctx, n, image, p, 0, p, p, 2, None, 0, out)              # w = 2: the first three columns meet each other, y nobody that counts
    dsum, dcnt, nobs, _ = out.read()
    called = int(np.isfinite(x).sum())
    assert dsum.tolist() == [2 << 32, 2 << 32, 2 << 32, 0, 0, 0, 0] and dcnt.tolist() == [2, 2, 2, 0, 0, 0, 0]
    assert nobs.tolist() == [called, called, called, 0, 0, 0, n]
    out.free()
    out = Outputs(ctx, p)
    score(ctx, n, image, p, 0, p, p, p, None, 0, out)              # every pair: the three dead columns still credit nobody
    dsum, dcnt, nobs, _ = out.read()
    tot, cnt, _ = ST.credit(T.sums(G), ST.forward_mask(p, 0, p, p, p), False)
    assert (dsum == tot).all() and (dcnt == cnt).all() and dcnt.tolist() == [3, 3, 3, 0, 0, 0, 3]
    assert (dsum[3:6] == 0).all() and (nobs[3:6] == 0).all()
    image.free(); out.free()


def test_refusals_leave_the_outputs_untouched(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = 65, 86
    G, _ = panel(n, p, 1, 0.07, True)
    image, out = new_image(ctx, G, p), Outputs(ctx, p)
    s, c, o = out.ptrs()
    good = dict(n=n, image=image.ptr, pe=p, j0=0, rows=p, have=p, w=5, sum=s, npairs=c, nobs=o)
    bad = {"NULL sum": dict(sum=None), "NULL npairs": dict(npairs=None), "NULL nobs": dict(nobs=None), "NULL image": dict(image=None),
           "w = 2^28": dict(w=1 << 28), "w = 0": dict(w=0), "w < 0": dict(w=-1), "sum off 8 bytes": dict(sum=s + 4), "image off 16 bytes": dict(image=image.ptr + 8),
           "rows beyond have": dict(j0=2, rows=p - 1), "have beyond pe": dict(have=p + 1, rows=1), "j0 < 0": dict(j0=-1), "rows < 0": dict(rows=-1),
           "n = 0": dict(n=0), "n = 2^28": dict(n=1 << 28), "pe = 0": dict(pe=0, have=0, rows=0)}
    for name, change in bad.items():
        a = dict(good, **change)
        rc = L.pg_ld_score_dev(ctx.handle, a["n"], a["image"], a["pe"], a["j0"], a["rows"], a["have"], a["w"], None, 1, a["sum"], a["npairs"], a["nobs"])
        assert rc == EINVAL and "pg_ld_score_dev" in L.pg_last_error().decode(), name
    assert L.pg_ld_score_dev(None, n, image.ptr, p, 0, p, p, 5, None, 1, s, c, o) == EINVAL
    ctx.sync()
    assert out.untouched()
    assert L.pg_ld_score_dev(ctx.handle, n, image.ptr, p, 3, 0, p, 5, None, 1, s, c, o) == 0       # no rows: nothing to do
    assert L.pg_ld_score_dev(ctx.handle, n, image.ptr, p, 0, p, p, (1 << 28) - 1, None, 1, s, c, o) == 0      # the widest window
    ctx.sync()
    dsum, dcnt, nobs, _ = out.read()
    tot, cnt, _ = ST.credit(T.sums(G), ST.forward_mask(p, 0, p, p, p), True)
    assert (dsum == tot).all() and (dcnt == cnt).all() and (nobs == ST.nobs(G)).all()
    image.free(); out.free()


# ---- lmm.ld_scores ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_case(miss):
    """(n, p, panel, sums).  Without missing calls the panel is one every source kind can hold (8-bit arrays have no missing code)."""
    n, p = 129, 515
    G = np.array(T.ld_panel(n, p, 41, miss=miss, specials=miss > 0))
    if miss == 0:
        G[:, 100] = 2.0                                  # a monomorphic column
    G.setflags(write=False)
    return n, p, G, T.sums(G)


def same_frames(a, b):
    return all((a[c].to_numpy().view(np.uint64) == b[c].to_numpy().view(np.uint64)).all() for c in ("l2", "n_pairs", "n_obs", "reach_fwd"))


@pytest.mark.parametrize("adjust", [True, False])
def test_ld_scores_is_the_host_model_whatever_the_batches(adjust):
    from pygemma_amd import lmm
    n, p, G, S = stream_case(0.07)
    X = G.astype(np.float32)
    names = [f"rs{j}" for j in range(p)]
    for window, batches in ((300, (64, 130, 600)), (7, (1, 130))):          # a window larger than the batch; the smallest batch
        tot, cnt, undefined = ST.credit(S, ST.window_mask(p, window), adjust)
        assert undefined < 0.2
        stats = {}
        frames = [lmm.ld_scores(X, window, adjust=adjust, snp_batch=sb, snps=names, stats=stats) for sb in batches]
        assert stats["batches"] == -(-p // batches[-1]) and stats["bytes_in"] == X.nbytes and stats["seconds"] > 0 and stats["w"] == window
        df = frames[0]
        assert list(df.columns) == ["l2", "n_pairs", "n_obs", "reach_fwd", "SNPs"] and list(df["SNPs"]) == names
        assert [str(df[c].dtype) for c in df.columns[:4]] == ["float64", "int64", "int64", "int64"]
        for other in frames[1:]:
            assert same_frames(df, other), "the scores depend on the batch boundaries"
        no = ST.nobs(G)
        assert (df["n_obs"] == no).all() and (df["n_pairs"] == cnt).all()
        assert (df["reach_fwd"] == np.minimum(window, p - 1 - np.arange(p))).all()
        want = ST.l2_of(tot, no)
        assert np.isnan(want).sum() == 3 and np.array_equal(df["l2"].to_numpy(), want, equal_nan=True)


def test_ld_scores_does_not_depend_on_the_storage():
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    window = 60
    n, p, G, _ = stream_case(0.07)                        # missing calls: packed records and floats
    V = T.bed_view(G)                                     # the dosage column is all missing in a .bed file, and for the kernel
    base = lmm.ld_scores(G.astype(np.float32), window, snp_batch=130)
    sources = [PackedBed(T.pack(V), n), PackedBed(T.pack(V, count_a1=True), n, count_A1=True), PackedBed(T.pack(V), n, count_A1=True),
               np.asfortranarray(G.astype(np.float32)), np.ascontiguousarray(G), np.asfortranarray(G)]
    for Xs in sources:                                     # counting the other allele flips the sign of r, not r^2
        assert same_frames(base, lmm.ld_scores(Xs, window, snp_batch=200))
    n, p, G, S = stream_case(0.0)                         # no missing call: every kind
    base = lmm.ld_scores(G, window)
    tot, cnt, _ = ST.credit(S, ST.window_mask(p, window), True)
    assert np.array_equal(base["l2"].to_numpy(), ST.l2_of(tot, ST.nobs(G)), equal_nan=True) and (base["n_pairs"] == cnt).all()
    for dtype in (np.int8, np.uint8, np.float32, np.float64):
        for order in "CF":
            assert same_frames(base, lmm.ld_scores(np.asarray(G.astype(dtype), order=order), window, snp_batch=130)), (dtype, order)
    assert same_frames(base, lmm.ld_scores(PackedBed(T.pack(G), n), window))


@pytest.mark.parametrize("window", [7, 300])
def test_unadjusted_scores_are_the_folded_band(window):
    """Against the route without the fused kernel: ld_window's float32 r, squared in float64 and folded to both sides.  Every pair is
    quantised once (half of 2^-32) and its r was rounded to float32 (r^2 off by up to 2 2^-25 |r| <= 2^-24); a SNP has 2 w pairs."""
    from pygemma_amd import lmm
    n, p, G, _ = stream_case(0.07)
    X = G.astype(np.float32)
    df = lmm.ld_scores(X, window, adjust=False)
    r2 = np.nan_to_num(lmm.ld_window(X, window).astype(np.float64) ** 2, nan=0.0)
    fold = 1.0 + r2.sum(axis=1)
    for k in range(min(window, p - 1)):
        fold[k + 1:] += r2[:p - 1 - k, k]
    tol = window * 2.0 ** -32 + window * 2.0 ** -23
    used = df["n_obs"].to_numpy() > 0
    assert used.sum() == p - 3 and np.isnan(df["l2"].to_numpy()[~used]).all()
    assert np.abs(df["l2"].to_numpy()[used] - fold[used]).max() <= tol
    assert df["l2"].to_numpy()[used].max() > 3                       # LD blocks: there is something to add up


def test_a_window_never_crosses_a_chromosome():
    from pygemma_amd import lmm
    n, p, G, _ = stream_case(0.07)
    X = G.astype(np.float32)
    cut = 200
    chrom = np.repeat(["1", "2"], [cut, p - cut])
    both = lmm.ld_scores(X, 50, chrom=chrom, snp_batch=130)
    parts = [lmm.ld_scores(X[:, :cut], 50), lmm.ld_scores(X[:, cut:], 50)]
    for col in ("l2", "n_pairs", "n_obs", "reach_fwd"):
        want = np.concatenate([part[col].to_numpy() for part in parts])
        assert (both[col].to_numpy().view(np.uint64) == want.view(np.uint64)).all(), col
    assert both["reach_fwd"][cut - 1] == 0 and not same_frames(both, lmm.ld_scores(X, 50))


@pytest.mark.parametrize("kind", [np.int64, np.float64])
def test_irregular_positions_with_ties(kind):
    from pygemma_amd import lmm
    n, p, G, S = stream_case(0.07)
    rng = np.random.default_rng(5)
    chrom = np.repeat([3, 4, 9], [150, 300, p - 450])
    step = rng.integers(0, 40, p)
    step[rng.random(p) < 0.3] = 0                         # ties
    pos = np.cumsum(step)
    for c in np.unique(chrom):
        pos[chrom == c] -= pos[chrom == c][0]             # positions restart on every chromosome
    pos = pos.astype(kind) if kind is np.int64 else pos / 8.0
    window = 300 if kind is np.int64 else 37.5
    visit = ST.window_mask(p, window, pos, chrom)
    tot, cnt, undefined = ST.credit(S, visit, True)
    assert undefined < 0.2 and visit.sum(axis=1).max() > 10 and visit.sum(axis=1).min() == 0
    df = lmm.ld_scores(G.astype(np.float32), window, pos=pos, chrom=chrom, snp_batch=64)
    assert (df["reach_fwd"] == visit.sum(axis=1)).all() and (df["n_pairs"] == cnt).all()
    assert np.array_equal(df["l2"].to_numpy(), ST.l2_of(tot, ST.nobs(G)), equal_nan=True)


def test_a_single_snp_and_an_empty_window():
    from pygemma_amd import lmm
    n, p, G, _ = stream_case(0.07)
    one = lmm.ld_scores(G[:, :1].astype(np.float32), 5)
    assert one["l2"].tolist() == [1.0] and one["n_pairs"].tolist() == [0] and one["n_obs"].tolist() == [int(ST.nobs(G)[0])]
    stats = {}
    apart = lmm.ld_scores(G[:, :40], 1, pos=np.arange(40) * 10, stats=stats)      # nobody within reach: the called samples still come back
    assert stats["w"] == 0 and (apart["n_pairs"] == 0).all() and (apart["n_obs"] == ST.nobs(G)[:40]).all() and (apart["l2"] == 1.0).all()
