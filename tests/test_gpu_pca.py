"""GPU checks of the principal components (pg_pca_{stat,proj,back}_{bed,x}_dev, lmm.pca, lmm.pca_project) — run with -m gpu on an MI355X.

The truth is tests/_pca_truth.py.  Every call writes into windows of pitch + 5 (stat: one window) inside buffers of 0x7f bytes; every
byte outside the windows must come back as it was.
Exact leg: hard calls with missing entries under a caller's stat with mu in {0, 0.5, 1} and isd in {0, 0.5, 1, 2}, against Q and T that
are integers in [-2^10, 2^10] over 2^10: every z is a multiple of 1/4 up to 4, every product a multiple of 2^-12 and every partial
sum below 2^13, so exact in fp64 in any order: proj and back must carry the bits of NumPy's product (with +0 for an empty sum).
Rounded leg: float dosages, 5 % missing, the device's own stat, normal Q and T, within
  |T - truth| <= (n + 8) 2^-53 sum_i |z||q|   and   |Y - truth| <= (pb + 8) 2^-53 sum_g |z||t|:
the bound of an fp64 sum of rounded products in any order, with eight to spare for the chunk additions (test_gpu_prs.py); the truth's
z follows the same two-rounding rule from the same stat, so its bits are the device's.
End to end: lmm.pca against the model run with the same arguments.  Device and BLAS each apply the operator Z Z'/p with a relative
error of about (n + p) 2^-53 of || |Z||Z|' || / p <= n; subspace iteration damps the errors of earlier passes by (lambda_{l+1} /
lambda_k)^2 ~ 0.01 per pass, so the last pass counts; 64 covers the two implementations, the QR and the l x l eigenproblem:
  eigenvalues within 64 (n + p) 2^-53 n, sign-fixed vectors within that over the model's gap lambda_k - lambda_{k+1}."""
import functools

import numpy as np
import pytest

import _pca_truth as T
import _prs_truth as P
import _snp_stats_truth as ST

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
DTYPES = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
# n: the 4-sample byte, the 16-sample run, the 64-sample chunk and the 256-sample group, more than one group; pb: the K-step of 4, the
# 128-SNP strip, both sides of a chunk edge, more than two chunks; l: one tile, a partial tile, a full one, two, four
COMBOS = [(1, 1, 1), (3, 3, 5), (37, 255, 16), (257, 256, 17), (1030, 257, 64), (1030, 600, 5), (1, 600, 17), (3, 257, 64), (37, 1, 5),
          (257, 3, 1), (1030, 255, 1), (37, 256, 64), (257, 600, 16)]
assert {c[0] for c in COMBOS} == {1, 3, 37, 257, 1030} and {c[1] for c in COMBOS} == {1, 3, 255, 256, 257, 600}
assert {c[2] for c in COMBOS} == {1, 5, 16, 17, 64}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ---- blocks on the device ------------------------------------------------------------------------------------------------------------

class Block:
    """A block on the device: .kind 'bed' or 'x', .src the arguments between (ctx, n, pb) and the entry's own."""

    def __init__(self, n, pb, kind, buf, src):
        self.n, self.pb, self.kind, self.buf, self.src = n, pb, kind, buf, src

    def call(self, ctx, stem, *tail):
        from pygemma_amd import _lib
        name = stem.format(self.kind)
        return getattr(_lib.load(), name)(ctx.handle, self.n, self.pb, *self.src, *tail), name

    def free(self):
        self.buf.free()


def bed_block(ctx, rec, n, ldb, count_a1):
    """Packed records in rows of pitch ldb whose pad bytes hold 0xff."""
    pb, bpr = rec.shape
    buf = np.full((pb, ldb), 0xff, np.uint8)
    buf[:, :bpr] = rec
    dX = ctx.to_device(buf)
    return Block(n, pb, "bed", dX, (dX.ptr, ldb, count_a1))


def x_block(ctx, X, snp_major, extra=0, shift=0):
    """The (n, pb) host matrix X stored SNP-major (pb x n) or sample-major (n x pb) at a pitch `extra` elements larger than minimal,
    `shift` elements into its buffer; the pad holds NaN (0xff bytes for 8-bit blocks)."""
    n, pb = X.shape
    A = np.ascontiguousarray(X.T) if snp_major else np.ascontiguousarray(X)
    rows, width = A.shape
    ldX = width + extra
    buf = np.full(shift + rows * ldX, np.nan, A.dtype) if A.dtype.kind == "f" else np.full(shift + rows * ldX, -1, np.int64).astype(A.dtype)
    buf[shift:].reshape(rows, ldX)[:, :width] = A
    dX = ctx.to_device(buf)
    return Block(n, pb, "x", dX, (dX.ptr + shift * A.itemsize, DTYPES[A.dtype], ldX, int(snp_major)))


class Guarded:
    """`rows` windows of `width` doubles at pitch width + 5, three doubles into a buffer of 0x7f bytes; the windows start as `fill`
    (None: 0x7f as well — the call has to write all of them)."""

    def __init__(self, ctx, rows, width, fill=None):
        self.rows, self.width, self.ld = rows, width, width + 5
        size = 3 + rows * self.ld + 4
        self.inside = np.zeros(size, bool)
        for k in range(rows):
            self.inside[3 + k * self.ld:3 + k * self.ld + width] = True
        host = np.full(size * 8, 0x7f, np.uint8)
        if fill is not None:
            host.view(np.float64)[self.inside] = fill
        self.buf = ctx.to_device(host)
        self.ptr = self.buf.ptr + 24

    def take(self):
        """The windows (rows, width) as float64; asserts the guard bytes and frees the buffer."""
        full = self.buf.download((self.inside.size,), np.uint64)
        self.buf.free()
        assert (full[~self.inside].view(np.uint8) == 0x7f).all(), "bytes outside the windows were written"
        return np.stack([full[3 + k * self.ld:3 + k * self.ld + self.width] for k in range(self.rows)]).view(np.float64)


def padded(ctx, A, extra=3):
    """The rows of A (rows, width) at pitch width + extra with NaN between them -> (device buffer, pitch)."""
    A = np.asarray(A, np.float64)
    buf = np.full((A.shape[0], A.shape[1] + extra), np.nan)
    buf[:, :A.shape[1]] = A
    return ctx.to_device(buf), A.shape[1] + extra


def work_area(ctx, n, pb, l):
    from pygemma_amd import _lib
    L = _lib.load()
    work = ctx.alloc(max(int(L.pg_pca_work_bytes(n, pb, l)), 256))
    _lib.check(L.pg_memset(ctx.handle, work.ptr, 0xff, work.nbytes), "pg_memset")
    return work


def run_stat(ctx, blk):
    from pygemma_amd import _lib
    out, work = Guarded(ctx, 1, 2 * blk.pb), work_area(ctx, blk.n, blk.pb, 1)
    _lib.check(*blk.call(ctx, "pg_pca_stat_{}_dev", work.ptr, out.ptr))
    ctx.sync()
    work.free()
    return out.take().reshape(blk.pb, 2)


def run_snp_stats(ctx, blk):
    """(counts (pb, 4) int64, moments (pb, 4)) of pg_snp_stats_*_dev on the same block."""
    from pygemma_amd import _lib
    L = _lib.load()
    work = ctx.alloc(max(int(L.pg_snp_stats_work_bytes(blk.n, blk.pb)), 256))
    dc, dm = ctx.alloc(32 * blk.pb), ctx.alloc(32 * blk.pb)
    _lib.check(*blk.call(ctx, "pg_snp_stats_{}_dev", work.ptr, dc.ptr, dm.ptr))
    ctx.sync()
    out = dc.download((blk.pb, 4), np.int64), dm.download((blk.pb, 4), np.float64)
    for b in (work, dc, dm):
        b.free()
    return out


def run_proj(ctx, blk, stat, Q):
    """T (l, pb) of the block under stat (pb, 2) and Q (l, n)."""
    from pygemma_amd import _lib
    l = Q.shape[0]
    dst, (dQ, ldq), out = ctx.to_device(np.ascontiguousarray(stat, np.float64)), padded(ctx, Q), Guarded(ctx, l, blk.pb)
    _lib.check(*blk.call(ctx, "pg_pca_proj_{}_dev", dst.ptr, l, dQ.ptr, ldq, out.ptr, out.ld))
    ctx.sync()
    dst.free(), dQ.free()
    return out.take()


def run_back(ctx, blocks, stat, Tm):
    """Y (l, n): the blocks' calls in order, block b on the stat rows and T columns of the SNPs after those of the blocks before it."""
    from pygemma_amd import _lib
    l, n = Tm.shape[0], blocks[0].n
    assert sum(b.pb for b in blocks) == Tm.shape[1] == stat.shape[0]
    dst, (dT, ldt), out = ctx.to_device(np.ascontiguousarray(stat, np.float64)), padded(ctx, Tm), Guarded(ctx, l, n, fill=0.0)
    s = 0
    for b in blocks:
        work = work_area(ctx, n, b.pb, l)
        _lib.check(*b.call(ctx, "pg_pca_back_{}_dev", dst.ptr + 16 * s, l, dT.ptr + 8 * s, ldt, work.ptr, out.ptr, out.ld))
        ctx.sync()
        work.free()
        s += b.pb
    dst.free(), dT.free()
    return out.take()


# ---- panels ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hard(n, pb, missing=0.08):
    """(n, pb) A2 dosages 0/1/2 with missing calls (NaN); where there is room SNP 0 is all missing, SNP 1 constant, SNP 2 misses one call."""
    rng = np.random.default_rng(100 * n + pb)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, pb), (n, pb)).astype(np.float64)
    G[rng.random((n, pb)) < missing] = np.nan
    if pb >= 3:
        if missing:
            G[:, 0] = np.nan
        G[:, 1] = 2.0
        G[:, 2] = rng.integers(0, 3, n)
        if missing:
            G[n // 2, 2] = np.nan
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _soft(n, pb):
    """(n, pb) float32 dosages (genotype plus noise) with 5 % missing, every fourth SNP left as hard calls; SNP 0 all missing, SNP 1
    constant, SNP 2 not hard-call."""
    rng = np.random.default_rng(7 + 100 * n + pb)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, pb), (n, pb)).astype(np.float64)
    X = (G + 0.1 * rng.standard_normal((n, pb))).astype(np.float32)
    X[:, ::4] = G[:, ::4]
    r = rng.random((n, pb))
    X[r < 0.04] = np.nan
    X[(r >= 0.04) & (r < 0.05)] = np.inf
    if pb >= 3:
        X[:, 0] = np.nan
        X[:, 1] = 0.75
        X[:, 2] = (G[:, 2] + 0.1 * rng.standard_normal(n)).astype(np.float32)
        X[n // 2, 2] = np.nan
    X.flags.writeable = False
    return X


@functools.lru_cache(maxsize=None)
def _panel(rows, l, exact, seed=0):
    """(l, rows) component-major Q or T."""
    rng = np.random.default_rng(3 + 10 * rows + l + seed)
    A = rng.integers(-2 ** 10, 2 ** 10 + 1, (l, rows)) / 1024.0 if exact else rng.standard_normal((l, rows))
    A.flags.writeable = False
    return A


@functools.lru_cache(maxsize=None)
def _exact_stat(pb):
    rng = np.random.default_rng(11 + pb)
    st = np.stack([rng.choice([0.0, 0.5, 1.0], pb), rng.choice([0.0, 0.5, 1.0, 2.0], pb)], axis=1)
    st.flags.writeable = False
    return st


def aligned(width):
    return 16 + (-width) % 16


def _sources(ctx, G, hard):
    """(tag, kind, block) of every storage of the panel G (NaN / Inf = missing): kind names the truth — packed records under either allele
    convention, 8-bit arrays (no missing code: a missing call is stored as 0) and float arrays."""
    n, pb = G.shape
    bpr = (n + 3) // 4
    if hard:
        rec = ST.pack(G, 1)                                           # the pad calls of the last byte hold 'missing'
        yield "bed a1=0", "bed0", bed_block(ctx, rec, n, bpr, 0)
        yield "bed a1=1 ldb+3", "bed1", bed_block(ctx, rec, n, bpr + 3, 1)
        yield "bed a1=0 16-byte pitch", "bed0", bed_block(ctx, ST.pack(G, 3), n, (bpr + 15) // 16 * 16, 0)
        I = np.where(np.isnan(G), 0, G)
        for dt in (np.int8, np.uint8):
            for sm in (1, 0):
                yield f"{np.dtype(dt).name} sm={sm} +3 base+1", "int", x_block(ctx, I.astype(dt), sm, 3, 1)
            yield f"{np.dtype(dt).name} sm=1 aligned", "int", x_block(ctx, I.astype(dt), 1, aligned(n), 0)
    for dt in (np.float32, np.float64):
        # float64 holds numbers that are not float32's: rounded per element they are the float32 panel again
        X = G.astype(dt) if dt == np.float32 else np.where(np.isfinite(G), G.astype(np.float64) * (1 + 2.0 ** -40), G)
        for sm in (1, 0):
            yield f"{np.dtype(dt).name} sm={sm} +3 base+1", "float", x_block(ctx, X, sm, 3, 1)
            yield f"{np.dtype(dt).name} sm={sm} aligned", "float", x_block(ctx, X, sm, aligned(n if sm else pb), 0)


def _truth_panel(G, kind):
    from pygemma_amd.bed import PackedBed
    if kind.startswith("bed"):
        return PackedBed(ST.pack(G), G.shape[0], count_A1=kind == "bed1")
    return np.where(np.isnan(G), 0, G).astype(np.int8) if kind == "int" else G.astype(np.float32)


# ---- stat ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,pb", [(1, 1), (3, 3), (37, 255), (257, 257), (1030, 600)])
def test_stat_is_the_rule_on_the_qc_pass(ctx, n, pb):
    seen = set()
    for G, hard in ((_hard(n, pb), True), (_soft(n, pb), False)):
        for tag, kind, blk in _sources(ctx, G, hard):
            counts, moments = run_snp_stats(ctx, blk)
            want = T.stat_rule(n, counts, moments)
            got = run_stat(ctx, blk)
            blk.free()
            assert (bits(got) == bits(want)).all(), (tag, np.argwhere(bits(got) != bits(want))[:5])
            assert np.isfinite(got).all()
            if pb >= 3 and kind != "int":
                assert (got[0] == 0).all()                                 # all missing: mu 0, isd 0
            if pb >= 3:
                assert got[1, 1] == 0 and got[1, 0] == (0.75 if not hard else (0.0 if kind == "bed1" else 2.0))     # constant
            if pb >= 3 and not hard and n >= 37:
                assert got[2, 1] > 0                                       # not hard-call
            # the model's stat: the same bits for hard calls (exact divisions).  Otherwise the QC pass's two-pass moments lie within
            # 4 n 2^-53 of mean |x| and mean x^2 of NumPy's (test_gpu_snp_stats.py); these dosages keep mean |x| / |mean| and
            # mean x^2 / var below 8, and 1 / sqrt halves the second
            model = T.stat(_truth_panel(G, kind) if hard else G)
            if hard:
                assert (bits(got) == bits(model)).all(), tag
            else:
                assert (np.abs(got - model) <= 32 * n * U * np.abs(model)).all(), tag
            seen.add(kind)
    assert seen == {"bed0", "bed1", "int", "float"}


# ---- the two products --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,pb,l", COMBOS)
def test_exact_leg(ctx, n, pb, l):
    G, st, Q, Tm = _hard(n, pb), _exact_stat(pb), _panel(n, l, True), _panel(pb, l, True, 1)
    seen = set()
    for tag, kind, blk in _sources(ctx, G, True):
        Z = T.z(_truth_panel(G, kind), st)
        assert (Z * 4 == np.round(Z * 4)).all() and np.abs(Z).max() <= 4
        want_t, want_y = (Z.T @ Q.T).T + 0.0, (Z @ Tm.T).T + 0.0
        got_t, got_y = run_proj(ctx, blk, st, Q), run_back(ctx, [blk], st, Tm)
        blk.free()
        assert (bits(got_t) == bits(want_t)).all(), (tag, "proj", np.argwhere(bits(got_t) != bits(want_t))[:5])
        assert (bits(got_y) == bits(want_y)).all(), (tag, "back", np.argwhere(bits(got_y) != bits(want_y))[:5])
        seen.add(kind)
    assert seen == {"bed0", "bed1", "int", "float"}


def _gate(got, want, bound, tag):
    err = np.abs(got - want)
    ratio = np.max(err / np.where(bound > 0, bound, 1.0))
    print(f"{tag}: max |got - truth| / bound {ratio:.3f}")
    assert (err <= bound).all(), (tag, ratio, np.argwhere(err > bound)[:5])


@pytest.mark.parametrize("n,pb,l", COMBOS)
def test_rounded_leg(ctx, n, pb, l):
    X, Q, Tm = _soft(n, pb), _panel(n, l, False), _panel(pb, l, False, 1)
    st, same_t, same_y = None, {}, {}
    for tag, _, blk in _sources(ctx, X, False):
        if st is None:
            st = run_stat(ctx, blk)            # the device's own; the layouts may differ in a two-pass mean, so all take the first
            Z = T.z(X, st)
            want_t, want_y = P.product(Z.T, Q.T).T, P.product(Z, Tm.T).T
            bound_t, bound_y = (n + 8) * U * (np.abs(Z).T @ np.abs(Q).T).T, (pb + 8) * U * (np.abs(Z) @ np.abs(Tm).T).T
        same_t[tag], same_y[tag] = run_proj(ctx, blk, st, Q), run_back(ctx, [blk], st, Tm)
        blk.free()
        _gate(same_t[tag], want_t, bound_t, f"n={n} pb={pb} l={l} proj {tag}")
        _gate(same_y[tag], want_y, bound_y, f"n={n} pb={pb} l={l} back {tag}")
    # a result does not depend on the storage, its pitch or its alignment
    ref = "float32 sm=1 +3 base+1"
    for tag in same_t:
        assert (bits(same_t[tag]) == bits(same_t[ref])).all() and (bits(same_y[tag]) == bits(same_y[ref])).all(), tag


@pytest.mark.parametrize("n,pb,l", [(37, 255, 16), (257, 600, 17), (1030, 257, 64)])
def test_every_storage_gives_the_same_bits(ctx, n, pb, l):
    """Hard calls without a missing one are the same values in all five storages: under rounded Q, T and stat the bits agree."""
    G, Q, Tm = _hard(n, pb, 0.0), _panel(n, l, False), _panel(pb, l, False, 1)
    assert not np.isnan(G).any()
    st = T.stat(G.astype(np.float32))
    ref, seen = None, set()
    for tag, kind, blk in _sources(ctx, G, True):
        if kind == "bed1":
            blk.free()
            continue                                   # the other allele's counts: other values
        got = run_proj(ctx, blk, st, Q), run_back(ctx, [blk], st, Tm)
        blk.free()
        ref = ref or got
        assert (bits(got[0]) == bits(ref[0])).all() and (bits(got[1]) == bits(ref[1])).all(), tag
        seen.add(tag.split()[0])
    assert seen == {"bed", "int8", "uint8", "float32", "float64"}


@pytest.mark.parametrize("n", [257, 1030])
def test_order_contract_and_slots(ctx, n):
    pb, l = 600, 5
    X, Q, Tm = _soft(n, pb), _panel(n, l, False), _panel(pb, l, False, 1)
    st = T.stat(X)
    Z = T.z(X, st)
    for sm in (1, 0):
        def split(cuts):
            edges = [0, *np.cumsum(cuts)]
            blocks = [x_block(ctx, X[:, a:b], sm) for a, b in zip(edges[:-1], edges[1:])]
            Y = run_back(ctx, blocks, st, Tm)
            for b in blocks:
                b.free()
            return Y
        one = split([600])
        # batches that are multiples of the chunk of 256: the same bits whatever their sizes; and a second run
        for cuts in ([256, 256, 88], [512, 88], [600]):
            assert (bits(split(cuts)) == bits(one)).all(), (sm, cuts)
        # another boundary may move the bits, not past the bound
        _gate(split([300, 300]), P.product(Z, Tm.T).T, (pb + 8) * U * (np.abs(Z) @ np.abs(Tm).T).T, f"n={n} 300 + 300 sm={sm}")
        # a row of proj is the same wherever its SNP sits: first or last of the block, in a block of its own, in another strip
        blk = x_block(ctx, X, sm)
        fwd = run_proj(ctx, blk, st, Q)
        blk.free()
        blk = x_block(ctx, np.ascontiguousarray(X[:, ::-1]), sm, 1, 1)
        rev = run_proj(ctx, blk, st[::-1], Q)
        blk.free()
        assert (bits(rev[:, ::-1]) == bits(fwd)).all(), sm
        blk = x_block(ctx, X[:, 599:], sm)
        assert (bits(run_proj(ctx, blk, st[599:], Q)[:, 0]) == bits(fwd[:, 599])).all(), sm
        blk.free()


def test_abi_misuse_launches_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, p, l = 64, 4, 2
    bufs = [ctx.alloc(1 << 16) for _ in range(6)]
    for b in bufs:
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, 1 << 16), "pg_memset")
    ctx.sync()
    X, st, Q, work, Tm, Y = [b.ptr for b in bufs]
    good = dict(n=n, pb=p, X=X, dtype=2, ldX=n, sm=1, ldb=16, st=st, l=l, Q=Q, ldq=n, T=Tm, ldt=p, work=work, Y=Y, ldy=n)

    def source(a, kind):
        return (a["X"], a["ldb"], 0) if kind == "bed" else (a["X"], a["dtype"], a["ldX"], a["sm"])

    def stat(kind, **kw):
        a = {**good, **kw}
        return getattr(L, f"pg_pca_stat_{kind}_dev")(ctx.handle, a["n"], a["pb"], *source(a, kind), a["work"], a["st"])

    def proj(kind, **kw):
        a = {**good, **kw}
        return getattr(L, f"pg_pca_proj_{kind}_dev")(ctx.handle, a["n"], a["pb"], *source(a, kind), a["st"], a["l"], a["Q"], a["ldq"], a["T"], a["ldt"])

    def back(kind, **kw):
        a = {**good, **kw}
        return getattr(L, f"pg_pca_back_{kind}_dev")(ctx.handle, a["n"], a["pb"], *source(a, kind), a["st"], a["l"], a["T"], a["ldt"], a["work"], a["Y"],
                                                     a["ldy"])

    shape = (dict(X=None), dict(st=None), dict(n=0), dict(n=1 << 30), dict(pb=-1),
             dict(pb=(1 << 25) + 1, ldX=1 << 26, ldt=1 << 26),
             dict(n=(1 << 30) - 1, pb=1 << 25, ldX=1 << 30, ldb=1 << 28, ldt=1 << 25, ldq=1 << 30, ldy=1 << 30))      # 2^39 workgroups
    for kind in ("x", "bed"):
        for call, stem, more in ((stat, "stat", (dict(work=None),)),
                                 (proj, "proj", (dict(Q=None), dict(T=None), dict(l=0), dict(ldq=n - 1), dict(ldt=p - 1))),
                                 (back, "back", (dict(T=None), dict(Y=None), dict(work=None), dict(l=0), dict(ldt=p - 1), dict(ldy=n - 1)))):
            name = f"pg_pca_{stem}_{kind}_dev".encode()
            for kw in shape + more:
                assert call(kind, **kw) == -22 and name in L.pg_last_error(), (name, kw)
            if stem != "stat":
                assert call(kind, l=65) == -95 and name in L.pg_last_error()
            assert call(kind, pb=0) == 0                                   # nothing to do is no error
            assert call(kind, ldb=15, ldX=n - 1) == -22 and name in L.pg_last_error()
        if kind == "x":
            for call in (stat, proj, back):
                assert call("x", sm=0, ldX=p - 1) == -22 and call("x", dtype=4) == -95 and call("x", dtype=-1) == -95
    ctx.sync()
    for b in bufs[1:]:
        assert (b.download((1 << 16,), np.uint8) == 0x7f).all()
    for b in bufs:
        b.free()


# ---- lmm.pca -------------------------------------------------------------------------------------------------------------------------

E2E = [(300, 2000), (257, 600)]
KW = dict(k=2, oversample=6, tol=0.0, iters=12)


@functools.lru_cache(maxsize=None)
def _e2e_panel(n, p):
    G = T.panel(n, p, seed=n + p)
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _e2e_model(n, p):
    return T.pca(_e2e_panel(n, p).astype(np.float32), **KW)


def _e2e_source(n, p, source):
    from pygemma_amd.bed import PackedBed
    G = _e2e_panel(n, p)
    return PackedBed(ST.pack(G), n) if source == "bed" else G.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _e2e_device(n, p, source, snp_batch=None):
    from pygemma import lmm
    st = {}
    res = lmm.pca(_e2e_source(n, p, source), samples=[f"id{i}" for i in range(n)], snps=[f"rs{g}" for g in range(p)], snp_batch=snp_batch,
                  stats=st, **KW)
    return res, st


def _e2e_bounds(n, p):
    m = _e2e_model(n, p)
    b_val = 64 * (n + p) * U * n
    return b_val, b_val / (m.ritz[KW["k"] - 1] - m.ritz[KW["k"]])


@pytest.mark.parametrize("source", ["bed", "float32"])
@pytest.mark.parametrize("n,p", E2E)
def test_driver_against_the_model(n, p, source):
    (res, st), m = _e2e_device(n, p, source), _e2e_model(n, p)
    k = KW["k"]
    assert list(res.pcs.columns) == list(res.loadings.columns) == ["PC1", "PC2"] and res.pcs.shape == (n, k) and res.loadings.shape == (p, k)
    assert list(res.pcs.index) == [f"id{i}" for i in range(n)] and list(res.loadings.index) == [f"rs{g}" for g in range(p)]
    assert set(st) >= {"resident", "passes", "converged", "batches", "bytes_in", "seconds", "seconds_orth"}
    assert st["resident"] is True and st["passes"] == 12 and st["converged"] is False and 0 <= st["seconds_orth"] <= st["seconds"]
    assert (bits(res.stat) == bits(m.stat)).all()                          # hard calls: exact divisions
    b_val, b_vec = _e2e_bounds(n, p)
    e_val, e_vec = np.max(np.abs(res.eigenvalues - m.eigenvalues)), np.max(np.abs(res.pcs.to_numpy() - m.pcs))
    print(f"n={n} p={p} {source}: eigenvalues {e_val:.2e} (bound {b_val:.2e}), vectors {e_vec:.2e} (bound {b_vec:.2e})")
    assert e_val <= b_val and e_vec <= b_vec
    p_used = int((m.stat[:, 1] > 0).sum())
    assert (res.explained == res.eigenvalues / (n * p_used / p)).all()
    # the loadings: Z L = pcs for a converged component
    lb = (p + 8) * U * (np.abs(m.Z) @ np.abs(res.loadings.to_numpy()))
    assert (np.abs(m.Z @ res.loadings.to_numpy() - res.pcs.to_numpy()) <= b_vec + lb).all()


@pytest.mark.parametrize("n,p", E2E)
def test_driver_against_the_kinship_route(n, p):
    res, m = _e2e_device(n, p, "bed")[0], _e2e_model(n, p)
    w, V = np.linalg.eigh(m.Z @ m.Z.T / p)
    w, V = w[::-1], V[:, ::-1][:, :2]
    assert (np.abs(res.eigenvalues - w[:2]) <= 1e-9 * w[:2]).all()
    A = res.pcs.to_numpy()
    sin = np.linalg.norm(A - V @ (V.T @ A), 2)                            # the largest principal angle between the two planes
    print(f"n={n} p={p}: sin of the largest principal angle {sin:.2e}")
    assert sin < 1e-6


@pytest.mark.parametrize("source", ["bed", "float32"])
def test_driver_resident_and_streamed_agree(source):
    n, p = 257, 600
    (res, st), (res2, st2) = _e2e_device(n, p, source), _e2e_device(n, p, source, 256)
    assert st["resident"] is True and st2["resident"] is False and st2["batches"] > st["batches"] and st2["bytes_in"] > st["bytes_in"]
    assert (bits(res.pcs.to_numpy()) == bits(res2.pcs.to_numpy())).all() and (bits(res.eigenvalues) == bits(res2.eigenvalues)).all()
    assert (bits(res.loadings.to_numpy()) == bits(res2.loadings.to_numpy())).all() and (bits(res.stat) == bits(res2.stat)).all()


@pytest.mark.parametrize("source", ["bed", "float32"])
def test_projection(source):
    from pygemma import lmm
    n, p = 257, 600
    res, m = _e2e_device(n, p, source)[0], _e2e_model(n, p)
    Lm = res.loadings.to_numpy()
    # the training panel: res.pcs again
    st = {}
    Pt = lmm.pca_project(_e2e_source(n, p, source), res, samples=list(res.pcs.index), stats=st)
    assert list(Pt.columns) == ["PC1", "PC2"] and list(Pt.index) == list(res.pcs.index) and st["resident"] is True
    lb = (p + 8) * U * (np.abs(m.Z) @ np.abs(Lm))
    assert (np.abs(Pt.to_numpy() - res.pcs.to_numpy()) <= _e2e_bounds(n, p)[1] + lb).all()
    # a held-out panel with missing calls under the training moments: a missing call is the training mean
    H = T.panel(45, p, seed=99)
    from pygemma_amd.bed import PackedBed
    Xn = PackedBed(ST.pack(H), 45) if source == "bed" else H.astype(np.float32)
    Zn = T.z(H.astype(np.float32), res.stat)
    want = P.product(Zn, Lm)
    for sb in (None, 256):
        got = lmm.pca_project(Xn, res, snp_batch=sb)
        assert got.shape == (45, 2)
        assert (np.abs(got.to_numpy() - want) <= (p + 8) * U * (np.abs(Zn) @ np.abs(Lm))).all(), sb
        if sb is None:
            first = got
    assert (bits(got.to_numpy()) == bits(first.to_numpy())).all()


def test_no_usable_snp_is_an_error():
    from pygemma import lmm
    with pytest.raises(RuntimeError):
        lmm.pca(np.ones((20, 8), np.float32), k=2, oversample=2)
