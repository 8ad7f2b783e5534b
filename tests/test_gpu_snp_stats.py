"""GPU checks of the SNP statistics (pg_snp_stats_bed_dev, pg_snp_stats_x_dev, pg_hwe_exact_dev, lmm.snp_stats) — run with -m gpu on an
MI355X.

The truth is tests/_snp_stats_truth.py.  counts are compared for equality; the moments of a hard-call SNP for bit equality with the
integer formulas (one correctly rounded division each); the fp64 moments of any other SNP against NumPy's on the float32-rounded values
within the bounds of an fp64 sum of n terms plus the error of the mean carried into the squares,
  |mean - t| <= 4 n 2^-53 mean|x|,  |var - t| <= 8 n 2^-53 mean(x^2),  min and max exact;
the Hardy-Weinberg p-value within 8 N 2^-53 relative (at most 4 roundings per recurrence step and N/2 steps each way, plus two sums) on a
panel that the truth helper alone shows to have no term within 2^-20 of P(n1) other than exact ties."""
import functools

import numpy as np
import pytest

import _snp_stats_truth as T

pytestmark = pytest.mark.gpu

DTYPES = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
NS = [1, 3, 37, 257, 1030]          # tails of 4, 16 and 64 samples; more than one 256-sample chunk
PBS = {1: 2, 19: 0, 130: 0}         # block sizes and the panel column each starts at
U = 2.0 ** -53


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _call(ctx, pb, fn):
    """fn(counts, moments) on windows [3, 3 + pb) of (pb + 7)-row outputs filled with 0x7f: every byte outside the window must come
    back as it was.  Returns (counts (pb, 4) int64, moments (pb, 4) fp64)."""
    from pygemma_amd import _lib
    L = _lib.load()
    rows = pb + 7
    dc, dm = ctx.alloc(rows * 32), ctx.alloc(rows * 32)
    for b in (dc, dm):
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, rows * 32), "pg_memset")
    fn(dc.ptr + 3 * 32, dm.ptr + 3 * 32)
    ctx.sync()
    out = []
    for b, dt in ((dc, np.int64), (dm, np.float64)):
        full = b.download((rows, 4), dt)
        canary = np.concatenate([full[:3], full[3 + pb:]]).view(np.uint8)
        assert (canary == 0x7f).all(), "bytes outside the window [s, e) were written"
        out.append(np.ascontiguousarray(full[3:3 + pb]))
        b.free()
    return out


def run_bed(ctx, rec, n, ldb, count_a1):
    """pg_snp_stats_bed_dev on records copied into rows of pitch ldb whose pad bytes hold 0xff."""
    from pygemma_amd import _lib
    L = _lib.load()
    pb, bpr = rec.shape
    buf = np.full((pb, ldb), 0xff, np.uint8)
    buf[:, :bpr] = rec
    dX, work = ctx.to_device(buf), ctx.alloc(max(int(L.pg_snp_stats_work_bytes(n, pb)), 256))
    res = _call(ctx, pb, lambda c, m: _lib.check(L.pg_snp_stats_bed_dev(ctx.handle, n, pb, dX.ptr, ldb, count_a1, work.ptr, c, m), "pg_snp_stats_bed_dev"))
    dX.free(); work.free()
    return res


def aligned(width):
    """The extra pitch that puts a row of `width` elements of any dtype on a 16-byte pitch, with pad elements to spare."""
    return 16 + (-width) % 16


def run_x(ctx, X, snp_major, extra, shift=0):
    """pg_snp_stats_x_dev on the (n, p) host matrix X stored SNP-major (p x n) or sample-major (n x p) at a pitch `extra` elements
    larger than minimal, the block starting `shift` elements into its 256-byte aligned buffer; the pad holds NaN (0xff bytes for
    8-bit blocks).  The 16-byte (8-bit sample-major: 4-byte) loads run when base and pitch are on that many bytes."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, pb = X.shape
    A = np.ascontiguousarray(X.T) if snp_major else np.ascontiguousarray(X)
    rows, width = A.shape
    ldX = width + extra
    buf = np.full(shift + rows * ldX, np.nan, A.dtype) if A.dtype.kind == "f" else np.full(shift + rows * ldX, -1, np.int64).astype(A.dtype)
    buf[shift:].reshape(rows, ldX)[:, :width] = A
    base = shift * A.itemsize
    dX, work = ctx.to_device(buf), ctx.alloc(max(int(L.pg_snp_stats_work_bytes(n, pb)), 256))
    res = _call(ctx, pb, lambda c, m: _lib.check(L.pg_snp_stats_x_dev(ctx.handle, n, pb, dX.ptr + base, DTYPES[A.dtype], ldX, int(snp_major), work.ptr, c, m),
                                                 "pg_snp_stats_x_dev"))
    dX.free(); work.free()
    return res


def gate(counts, moments, tr, n, tag):
    """counts equal; hard-call and empty rows bit-equal to the truth; every other row inside the fp64 bounds, min and max exact."""
    assert (counts == tr["counts"]).all(), (tag, np.flatnonzero((counts != tr["counts"]).any(axis=1))[:5])
    t = tr["moments"]
    exact = tr["hard"] | (tr["counts"][:, 0] == n)
    same = (bits(moments) == bits(t)) | (np.isnan(moments) & np.isnan(t))
    assert same[exact].all(), (tag, "integer moments", np.flatnonzero(~same.all(axis=1) & exact)[:5])
    soft = ~exact
    if soft.any():
        em, ev = np.abs(moments[soft, 0] - t[soft, 0]), np.abs(moments[soft, 1] - t[soft, 1])
        bm, bv = 4 * n * U * tr["absx"][soft], 8 * n * U * tr["sqx"][soft]
        print(f"{tag}: {soft.sum()} fp64 rows, max mean err / bound {np.max(em / bm):.3f}, max var err / bound {np.max(ev / bv):.3f}")
        assert (em <= bm).all() and (ev <= bv).all(), (tag, np.max(em / bm), np.max(ev / bv))
        assert (moments[soft, 2:] == t[soft, 2:]).all(), (tag, "min / max")


@functools.lru_cache(maxsize=None)
def _calls(n, p=130, seed=0, miss=0.1):
    """(n, p) A2 dosages 0/1/2 with `miss` missing; column 0 all missing, column 1 monomorphic, column 2 fully called."""
    rng = np.random.default_rng(seed + 7 * n)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, p), (n, p)).astype(np.float64)
    G[rng.random((n, p)) < miss] = np.nan
    G[:, 0] = np.nan
    G[:, 1] = 2.0
    G[:, 2] = rng.integers(0, 3, n)
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _calls_truth(n, count_a1):
    G = _calls(n)
    return T.stats_truth(2 - G if count_a1 else G)


def _rows(tr, s, e):
    return {k: v[s:e] for k, v in tr.items()}


@pytest.mark.parametrize("n", NS)
def test_bed_blocks(ctx, n):
    G = _calls(n)
    bpr = (n + 3) // 4
    for pad_code in (1, 3):                                          # the pad calls of the last byte hold 'missing' and '11'
        rec = T.pack(G, pad_code)
        for pb, s in PBS.items():
            for ldb in (bpr, bpr + 3):                               # the second pitch is on no 4-byte boundary: byte loads
                for a1 in (0, 1):
                    counts, moments = run_bed(ctx, rec[s:s + pb], n, ldb, a1)
                    tr = _rows(_calls_truth(n, a1), s, s + pb)
                    assert tr["hard"].sum() + (tr["counts"][:, 0] == n).sum() == pb
                    gate(counts, moments, tr, n, f"bed n={n} pb={pb} ldb={ldb} a1={a1} pad={pad_code}")
    # a pitch on a 16-byte boundary takes the 16-byte loads
    counts, moments = run_bed(ctx, T.pack(G), n, (bpr + 15) // 16 * 16, 0)
    gate(counts, moments, _calls_truth(n, 0), n, f"bed n={n} 16-byte pitch")


@functools.lru_cache(maxsize=None)
def _array_panel(n, dtype):
    """(n, 130) in `dtype`: columns 0..39 plain hard calls (the same in every dtype), then the dtype's special values."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(5 + n)
    p = 130
    G = rng.binomial(2, rng.uniform(0.05, 0.5, p), (n, p))
    G[:, 1] = 2
    if dtype.kind == "f":
        X = G.astype(dtype)
        for j in range(40, 70):                                      # NaN, +Inf, -Inf as missing; -0.0 is a zero
            r = rng.random(n)
            X[r < 0.1, j] = np.nan
            X[(r >= 0.1) & (r < 0.15), j] = np.inf
            X[(r >= 0.15) & (r < 0.17), j] = -np.inf
            X[(r >= 0.17) & (X[:, j] == 0), j] = -0.0
        X[:, 40] = np.nan                                            # nothing observed
        X[:, 41] = np.inf
        for j in range(70, 100):                                     # dosages: genotype plus Gaussian noise, some missing
            X[:, j] = (G[:, j] + 0.1 * rng.standard_normal(n)).astype(np.float32)
            X[rng.random(n) < 0.05, j] = np.nan
        for j in range(100, 110):                                    # a large mean against a small spread
            X[:, j] = (1000.0 + rng.standard_normal(n)).astype(np.float32)
        if dtype == np.float64:                                      # not float32 numbers: rounded per element, 1 + 2^-30 is a 1
            X[:, 110:120] = np.where(G[:, 110:120] == 1, 1.0 + 2.0 ** -30, G[:, 110:120] * (1.0 + 2.0 ** -40))
    elif dtype == np.int8:
        X = G.astype(np.int8)
        X[:, 40:70] = rng.integers(-1, 4, (n, 30))                   # -1 and 3 are values, not codes
        X[:, 70:80] = rng.integers(-128, 128, (n, 10))
    else:
        X = G.astype(np.uint8)
        X[:, 40:70] = np.where(rng.random((n, 30)) < 0.1, 255, G[:, 40:70])     # 255 is a value: there is no missing code
        X[:, 70:80] = rng.integers(0, 256, (n, 10))
    X.flags.writeable = False
    return X


@functools.lru_cache(maxsize=None)
def _array_truth(n, dtype):
    return T.stats_truth(_array_panel(n, dtype))


@pytest.mark.parametrize("n", NS)
def test_array_blocks(ctx, n):
    plain = {}
    for dtype in (np.int8, np.uint8, np.float32, np.float64):
        X, tr = _array_panel(n, dtype), _array_truth(n, dtype)
        name = np.dtype(dtype).name
        if n >= 37 and np.dtype(dtype).kind != "f":
            assert not tr["hard"][40:70].any()                       # -1, 3 and 255 are values: those columns take the fp64 path
        if dtype == np.float64:
            assert (tr["counts"][:, 2] == (np.asarray(X) == 1.0 + 2.0 ** -30).sum(0))[110:120].all() and tr["hard"][110:120].all()
        for snp_major in (1, 0):
            for pb, s in PBS.items():
                # the minimal pitch; one on no 4-byte boundary (element loads); one on a 16-byte boundary for every dtype, where the
                # vector loads run: at n = 1030 a whole 1024-element step of an 8-bit SNP-major row, at pb = 130 full and partial lanes
                # of a sample-major row.  (A minimal pitch is aligned too where width x itemsize happens to be.)
                for extra in (0, 3, aligned(n if snp_major else pb)):
                    if pb == 130 or extra != 0:
                        counts, moments = run_x(ctx, X[:, s:s + pb], snp_major, extra)
                        gate(counts, moments, _rows(tr, s, s + pb), n, f"{name} n={n} pb={pb} snp_major={snp_major} ldX=+{extra}")
                        if pb == 130:
                            plain[(name, snp_major, extra)] = (counts[:40], moments[:40])
            # the aligned pitch from a base one element off: the same elements through element loads; and a sub-block of it
            ext = aligned(n if snp_major else 130)
            counts, moments = run_x(ctx, X, snp_major, ext, shift=1)
            gate(counts, moments, tr, n, f"{name} n={n} snp_major={snp_major} ldX=+{ext} base + 1")
            plain[(name, snp_major, "base + 1")] = (counts[:40], moments[:40])
            counts, moments = run_x(ctx, X[:, 5:123], snp_major, aligned(n if snp_major else 118), shift=16 if snp_major else 0)
            gate(counts, moments, _rows(tr, 5, 123), n, f"{name} n={n} snp_major={snp_major} columns 5..122 on an aligned pitch")
    # hard-call columns: the same bits from every dtype and layout
    ref_c, ref_m = plain[("float32", 1, 0)]
    assert len(plain) == 4 * 2 * 4
    for key, (c, m) in plain.items():
        assert (c == ref_c).all() and (bits(m) == bits(ref_m)).all(), key


def test_rows_do_not_depend_on_the_block(ctx):
    """The fp64 rows of a float32 block: the same bits whatever pb, the pitch and the position in the block, per layout."""
    n = 1030
    X = _array_panel(n, np.float32)
    for snp_major in (1, 0):
        _, full = run_x(ctx, X, snp_major, 0)
        for s, e, extra, shift in ((70, 110, 0, 0), (70, 110, 3, 0), (75, 76, 1, 0), (3, 130, 64, 0), (69, 108, 2, 0),
                                   (70, 110, aligned(n if snp_major else 40), 0), (70, 110, aligned(n if snp_major else 40), 3),
                                   (69, 108, aligned(n if snp_major else 39), 4)):
            _, sub = run_x(ctx, X[:, s:e], snp_major, extra, shift)
            assert ((bits(sub) == bits(full[s:e])) | (np.isnan(sub) & np.isnan(full[s:e]))).all(), (snp_major, s, e, extra, shift)


def test_abi_misuse_launches_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = 64, 4
    bufs = [ctx.alloc(1 << 16) for _ in range(5)]
    for b in bufs:
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, 1 << 16), "pg_memset")
    ctx.sync()
    X, work, cnt, mom, pv = [b.ptr for b in bufs]
    good = dict(n=n, pb=p, X=X, dtype=2, ldX=n, sm=1, ldb=16, work=work, cnt=cnt, mom=mom)

    def x(**kw):
        a = {**good, **kw}
        return L.pg_snp_stats_x_dev(ctx.handle, a["n"], a["pb"], a["X"], a["dtype"], a["ldX"], a["sm"], a["work"], a["cnt"], a["mom"])

    def bed(**kw):
        a = {**good, **kw}
        return L.pg_snp_stats_bed_dev(ctx.handle, a["n"], a["pb"], a["X"], a["ldb"], 0, a["work"], a["cnt"], a["mom"])

    for call in (x, bed):
        assert call(X=None) == -22 and call(work=None) == -22 and call(cnt=None) == -22 and call(mom=None) == -22
        assert call(n=0) == -22 and call(pb=-1) == -22 and call(n=1 << 30) == -22
        assert call(pb=(1 << 25) + 1, ldX=1 << 26) == -22                       # more SNPs than one launch is sure to hold
    assert x(ldX=n - 1) == -22 and x(sm=0, ldX=p - 1) == -22 and bed(ldb=15) == -22
    assert x(dtype=4) == -95 and x(dtype=-1) == -95
    assert x(n=1 << 20, pb=1 << 21, sm=0, ldX=1 << 21) == -22                    # 4096 chunks x 8192 column groups: 2^25 workgroups
    assert L.pg_hwe_exact_dev(ctx.handle, n, p, None, pv) == -22 and L.pg_hwe_exact_dev(ctx.handle, n, p, cnt, None) == -22
    assert L.pg_hwe_exact_dev(ctx.handle, 0, p, cnt, pv) == -22 and L.pg_hwe_exact_dev(ctx.handle, n, -1, cnt, pv) == -22
    assert x(pb=0) == 0 and bed(pb=0) == 0 and L.pg_hwe_exact_dev(ctx.handle, n, 0, cnt, pv) == 0      # nothing to do is no error
    ctx.sync()
    for b in bufs[1:]:
        assert (b.download((1 << 16,), np.uint8) == 0x7f).all()
    for b in bufs:
        b.free()


# ---- the exact Hardy-Weinberg test -------------------------------------------------------------------------------------------------

def _hwe(ctx, counts, n):
    from pygemma_amd import _lib
    L = _lib.load()
    counts = np.ascontiguousarray(counts, np.int64)
    p = counts.shape[0]
    dc, dp = ctx.to_device(counts), ctx.alloc(8 * (p + 2))
    _lib.check(L.pg_memset(ctx.handle, dp.ptr, 0x7f, 8 * (p + 2)), "pg_memset")
    _lib.check(L.pg_hwe_exact_dev(ctx.handle, n, p, dc.ptr, dp.ptr + 8), "pg_hwe_exact_dev")
    ctx.sync()
    full = dp.download((p + 2,), np.float64)
    assert (full[[0, -1]].view(np.uint8) == 0x7f).all()
    dc.free(); dp.free()
    return full[1:-1]


@functools.lru_cache(maxsize=None)
def _hwe_panel(n=1030, p=700, seed=1):
    """Genotypes at allele frequencies uniform in [0.01, 0.5]; per SNP a share of the heterozygotes is turned into homozygotes (p-values
    over many decades); 5 % missing.  Returns (G with NaN, counts (p, 4), reference p-values, gaps)."""
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, rng.uniform(0.01, 0.5, p), (n, p)).astype(np.float64)
    share = rng.uniform(0.0, 0.6, p) * (rng.random(p) < 0.7)
    flip = (G == 1) & (rng.random((n, p)) < share)
    G[flip] = 2.0 * (rng.random((n, p)) < 0.5)[flip]
    G[rng.random((n, p)) < 0.05] = np.nan
    counts = T.stats_truth(G)["counts"]
    ref = [T.hwe_reference(*row[1:]) for row in counts]
    G.flags.writeable = False
    return G, counts, np.array([r[0] for r in ref]), np.array([r[1] for r in ref])


def test_hwe_panel(ctx):
    n = 1030
    _, counts, ref, gaps = _hwe_panel()
    # from the truth alone: no term of any SNP within 2^-20 of P(n1) unless it is an exact tie, so no comparison hangs on a rounding
    assert gaps.min() > 2.0 ** -20, gaps.min()
    assert np.isfinite(ref).all() and (ref > 0).all()
    assert (ref < 1e-8).sum() >= 20 and (ref > 0.1).sum() >= 100 and np.log10(ref.max() / ref.min()) > 20      # many decades
    got = _hwe(ctx, counts, n)
    N = counts[:, 1:].sum(axis=1)
    err = np.abs(got - ref) / (8 * N * U * ref)
    print(f"hwe panel: smallest gap {gaps.min():.2e}, p from {ref.min():.2e} to {ref.max():.2e}, max |p - t| / bound {err.max():.3f}")
    assert (err <= 1).all(), (err.max(), int(err.argmax()))


def test_hwe_fixed_cases(ctx):
    n = 100
    rows = [(100, 0, 0, 0),        # N = 0
            (0, 100, 0, 0), (0, 0, 0, 100), (40, 0, 0, 60),       # monomorphic
            (0, 50, 0, 50), (10, 89, 0, 1),                       # no heterozygotes, both homozygotes present
            (0, 0, 100, 0), (60, 0, 40, 0),                       # all heterozygotes
            (0, 30, 40, 29), (1, 30, 40, 30), (0, 30, -1, 71),    # counts that do not add up to n, or negative: not hard-call
            (0, 25, 50, 25), (0, 1, 2, 97), (0, 97, 2, 1), (94, 1, 2, 3)]
    got = _hwe(ctx, np.array(rows), n)
    assert np.isnan(got[0]) and (got[1:4] == 1.0).all() and np.isnan(got[8:11]).all()
    for k in (4, 5, 6, 7, 11, 12, 13, 14):
        t, _ = T.hwe_reference(*rows[k][1:])
        assert abs(got[k] - t) <= 8 * sum(rows[k][1:]) * U * t, (rows[k], got[k], t)
        assert abs(t - T.hwe_rational(*rows[k][1:])) <= 8 * sum(rows[k][1:]) * U * t
    assert got[4] < 1e-25 and got[6] < 1e-25 and got[11] > 0.99 and got[14] == 1.0      # (1, 2, 3): every term is a tie of the mode


# ---- lmm.snp_stats -------------------------------------------------------------------------------------------------------------------

INT_COLS = ["n_obs", "n_miss", "n0", "n1", "n2"]
F64_COLS = ["miss", "mean", "var", "min", "max", "af", "maf", "hwe_p"]


def frame_bits(df):
    return {c: (df[c].to_numpy().view(np.uint64) if df[c].dtype == np.float64 else df[c].to_numpy()) for c in df.columns}


def same_frames(a, b):
    fa, fb = frame_bits(a), frame_bits(b)
    return list(fa) == list(fb) and all((fa[c] == fb[c]).all() for c in fa)


@functools.lru_cache(maxsize=None)
def _driver_panel():
    """n = 1030, p = 700 float32: the Hardy-Weinberg panel's calls (5 % NaN) with 60 dosage columns in the middle."""
    G = _hwe_panel()[0]
    X = G.astype(np.float32)
    rng = np.random.default_rng(2)
    X[:, 300:360] += (0.1 * rng.standard_normal((1030, 60))).astype(np.float32)
    X.flags.writeable = False
    return X


def test_driver_frame_and_batches():
    from pygemma import lmm
    X = _driver_panel()
    n, p = X.shape
    tr = T.stats_truth(X)
    snps = [f"rs{j}" for j in range(p)]
    st_ = {}
    ref = lmm.snp_stats(X, snps=snps, stats=st_)
    assert list(ref.columns) == INT_COLS + F64_COLS + ["SNPs"] and list(ref["SNPs"]) == snps and len(ref) == p
    assert all(ref[c].dtype == np.int64 for c in INT_COLS) and all(ref[c].dtype == np.float64 for c in F64_COLS)
    assert st_["batches"] == 1 and st_["bytes_in"] == 4 * n * p and st_["seconds"] > 0
    counts = ref[["n_miss", "n0", "n1", "n2"]].to_numpy()
    gate(counts, ref[["mean", "var", "min", "max"]].to_numpy(), tr, n, "lmm.snp_stats float32 C")
    assert (~tr["hard"]).sum() == 60
    assert (ref["n_obs"] == n - ref["n_miss"]).all() and (ref["miss"].to_numpy() == counts[:, 0] / n).all()
    af = ref["af"].to_numpy()
    inside = (ref["min"].to_numpy() >= 0) & (ref["max"].to_numpy() <= 2)
    assert (af[inside] == ref["mean"].to_numpy()[inside] / 2).all() and np.isnan(af[~inside]).all() and (~inside).sum() > 0
    assert (ref["maf"].to_numpy()[inside] == np.minimum(af, 1 - af)[inside]).all()
    hw = ref["hwe_p"].to_numpy()
    assert np.isnan(hw[~tr["hard"]]).all() and np.isfinite(hw[tr["hard"]]).all()
    href = _hwe_panel()[2]
    N = counts[:, 1:].sum(axis=1)
    assert (np.abs(hw - href)[tr["hard"]] <= (8 * N * U * href)[tr["hard"]]).all()
    # any batch size (129 columns: a pitch on no 16-byte boundary), a second run, hwe=False
    for sb in (128, 129, 700, None):
        st_ = {}
        assert same_frames(lmm.snp_stats(X, snps=snps, snp_batch=sb, stats=st_), ref), sb
        assert st_["batches"] == (1 if sb is None else -(-p // sb))
    no = lmm.snp_stats(X, hwe=False)
    assert list(no.columns) == INT_COLS + F64_COLS[:-1] and same_frames(no, ref[no.columns])
    # the filter and the mask's way back into a scan's input
    keep = lmm.snp_filter(ref)
    assert keep.dtype == np.bool_ and keep.shape == (p,) and 0 < keep.sum() < p
    assert (keep == ((ref["miss"] <= 0.05) & (ref["var"] > 0) & (ref["maf"] >= 0.01)).to_numpy()).all()


def test_driver_sources_agree(tmp_path):
    from pygemma import lmm
    from pygemma_amd.bed import PackedBed, write_bed
    X = _driver_panel()
    n, p = X.shape
    tr = T.stats_truth(X)
    hard = tr["hard"]
    ref = lmm.snp_stats(X)
    # Fortran order: SNP-major kernels.  Hard-call rows carry the same bits, the others meet the same truth
    f = lmm.snp_stats(np.asfortranarray(X), snp_batch=256)
    gate(f[["n_miss", "n0", "n1", "n2"]].to_numpy(), f[["mean", "var", "min", "max"]].to_numpy(), tr, n, "lmm.snp_stats float32 F")
    assert same_frames(f[hard], ref[hard])
    assert same_frames(lmm.snp_stats(np.asfortranarray(X)), f)
    # pinned against pageable, both orders
    Xp = lmm.pinned_empty((n, p), np.float32)
    Xp[:] = X
    assert same_frames(lmm.snp_stats(Xp, snp_batch=200), ref)
    Xq = lmm.pinned_empty((p, n), np.float32)
    Xq[:] = X.T
    assert same_frames(lmm.snp_stats(Xq.T, snp_batch=200), f)
    # the float64 image of the same matrix: rounded per element on the device
    assert same_frames(lmm.snp_stats(X.astype(np.float64), snp_batch=300), ref)
    # a .bed file of the calls against its own host decode passed as float32
    G = _hwe_panel()[0]
    write_bed(str(tmp_path / "qc"), G)
    for a1 in (False, True):
        bed = PackedBed.open(str(tmp_path / "qc"), count_A1=a1)
        st_ = {}
        b = lmm.snp_stats(bed, snps=bed.snps, snp_batch=128, stats=st_)
        assert st_["batches"] == 6 and st_["bytes_in"] == p * ((n + 3) // 4)
        d = lmm.snp_stats(bed.to_float(impute=False), snps=bed.snps)
        assert same_frames(b, d), a1
        assert same_frames(lmm.snp_stats(bed, snps=bed.snps), b)
        keep = lmm.snp_filter(b, hwe=1e-6)
        assert 0 < keep.sum() < p
        kept = bed.take(keep)
        assert same_frames(lmm.snp_stats(kept, snps=kept.snps), b[keep].reset_index(drop=True))
