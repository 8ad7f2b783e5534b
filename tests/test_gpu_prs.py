"""GPU checks of the polygenic scores (pg_prs_bed_acc_dev, pg_prs_x_acc_dev, lmm.prs) — run with -m gpu on an MI355X.

The truth is tests/_prs_truth.py.  Every call writes into t rows of pitch n + 5 inside a buffer of 0x7f bytes: the windows start at zero
and every byte outside them must come back as it was.
Exact leg: hard calls against weights that are integers in [-2^20, 2^20] over 2^10 (a third of them zero), missing calls skipped: every
product and every partial sum is an integer multiple of 2^-10 below 2^32, so exact in fp64 in any order, and score must carry the bits of
NumPy's fp64 product (with +0 for an empty sum: the accumulators start at +0); called must equal the integer product.
Rounded leg: float dosages, normal weights over six decades, 5 % missing, with and without imputation, within
  |score - truth| <= (pb + 8) 2^-53 sum_g |x_gi||w_gk|  +  4 n 2^-53 |mu_g||w_gk| per imputed entry of a SNP that is not hard-call:
the first term is the bound of an fp64 sum of pb rounded products in any order (pb - 1 additions and one rounding per product, each
2^-53 relative to the partial sums, which sum |x||w| bounds) with eight to spare for the chunk additions; the second is the distance
test_gpu_snp_stats.py allows between the device's two-pass mean and NumPy's."""
import functools

import numpy as np
import pandas as pd
import pytest

import _prs_truth as T
import _snp_stats_truth as ST

pytestmark = pytest.mark.gpu

DTYPES = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
# n: the 4-sample byte, the 16-sample tile, the 256-sample group, more than one group; pb: the K-step of 4, both sides of a chunk edge,
# more than two chunks; t: one tile, a partial tile, a full one, two, four
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

def bed_block(ctx, rec, n, ldb, count_a1):
    """Packed records in rows of pitch ldb whose pad bytes hold 0xff -> call(t, Wt, ldw, impute, work, score, called, lds)."""
    from pygemma_amd import _lib
    L = _lib.load()
    pb, bpr = rec.shape
    buf = np.full((pb, ldb), 0xff, np.uint8)
    buf[:, :bpr] = rec
    dX = ctx.to_device(buf)

    def call(t, Wt, ldw, impute, work, score, called, lds):
        return L.pg_prs_bed_acc_dev(ctx.handle, n, pb, dX.ptr, ldb, count_a1, t, Wt, ldw, impute, work, score, called, lds)
    call.pb, call.n, call.free, call.name = pb, n, dX.free, "pg_prs_bed_acc_dev"
    return call


def x_block(ctx, X, snp_major, extra=0, shift=0):
    """The (n, pb) host matrix X stored SNP-major (pb x n) or sample-major (n x pb) at a pitch `extra` elements larger than minimal,
    `shift` elements into its buffer; the pad holds NaN (0xff bytes for 8-bit blocks)."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, pb = X.shape
    A = np.ascontiguousarray(X.T) if snp_major else np.ascontiguousarray(X)
    rows, width = A.shape
    ldX = width + extra
    buf = np.full(shift + rows * ldX, np.nan, A.dtype) if A.dtype.kind == "f" else np.full(shift + rows * ldX, -1, np.int64).astype(A.dtype)
    buf[shift:].reshape(rows, ldX)[:, :width] = A
    dX, base, code = ctx.to_device(buf), shift * A.itemsize, DTYPES[A.dtype]

    def call(t, Wt, ldw, impute, work, score, called, lds):
        return L.pg_prs_x_acc_dev(ctx.handle, n, pb, dX.ptr + base, code, ldX, int(snp_major), t, Wt, ldw, impute, work, score, called, lds)
    call.pb, call.n, call.free, call.name = pb, n, dX.free, "pg_prs_x_acc_dev"
    return call


def run(ctx, blocks, W, impute, counts=True, keep=False):
    """The blocks' calls in order, block b on the weights of the SNPs after those of the blocks before it, into guarded outputs.
    Returns (score (t, n) fp64, called (t, n) int64 or None).  The blocks are freed unless `keep`."""
    from pygemma_amd import _lib
    L = _lib.load()
    W = np.asarray(W, np.float64)
    P, t = W.shape
    n = blocks[0].n
    assert sum(b.pb for b in blocks) == P
    ldw, lds = P + 3, n + 5
    Wt = np.full((t, ldw), np.nan)
    Wt[:, :P] = W.T
    dW = ctx.to_device(Wt)
    size = 3 + t * lds + 4
    inside = np.zeros(size, bool)
    for k in range(t):
        inside[3 + k * lds:3 + k * lds + n] = True
    outs = []
    for _ in range(2 if counts else 1):
        host = np.full(size * 8, 0x7f, np.uint8)
        host.view(np.uint64)[inside] = 0
        outs.append(ctx.to_device(host))
    s = 0
    for b in blocks:
        work = ctx.alloc(max(int(L.pg_prs_work_bytes(n, b.pb, t)), 256))
        _lib.check(L.pg_memset(ctx.handle, work.ptr, 0xff, work.nbytes), "pg_memset")
        _lib.check(b(t, dW.ptr + 8 * s, ldw, impute, work.ptr, outs[0].ptr + 24, outs[1].ptr + 24 if counts else None, lds), b.name)
        ctx.sync()
        work.free()
        s += b.pb
    res = []
    for o, dt in zip(outs, (np.float64, np.int64)):
        full = o.download((size,), np.uint64)
        assert (full[~inside].view(np.uint8) == 0x7f).all(), "bytes outside the windows [k lds, k lds + n) were written"
        res.append(np.stack([full[3 + k * lds:3 + k * lds + n] for k in range(t)]).view(dt))
        o.free()
    dW.free()
    if not keep:
        for b in blocks:
            b.free()
    return res[0], (res[1] if counts else None)


# ---- panels ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hard(n, pb):
    """(n, pb) A2 dosages 0/1/2 with 8 % missing (NaN); where there is room SNP 0 is all missing, SNP 1 constant, SNP 2 misses one call."""
    rng = np.random.default_rng(100 * n + pb)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, pb), (n, pb)).astype(np.float64)
    G[rng.random((n, pb)) < 0.08] = np.nan
    if pb >= 3:
        G[:, 0] = np.nan
        G[:, 1] = 2.0
        G[:, 2] = rng.integers(0, 3, n)
        G[n // 2, 2] = np.nan
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _soft(n, pb):
    """(n, pb) float32 dosages (genotype plus noise) with 5 % missing, every fourth SNP left as hard calls; the same three special SNPs."""
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
def _weights(pb, t, exact):
    rng = np.random.default_rng(3 + 10 * pb + t)
    if exact:
        W = rng.integers(-2 ** 20, 2 ** 20 + 1, (pb, t)) / 1024.0
        W[rng.random((pb, t)) < 1 / 3] = 0.0
    else:
        W = rng.standard_normal((pb, t)) * 10.0 ** rng.uniform(-3, 3, (pb, t))
        W[rng.random((pb, t)) < 0.1] = 0.0
    W.flags.writeable = False
    return W


def aligned(width):
    return 16 + (-width) % 16


def _sources(ctx, G, exact):
    """(tag, kind, block) of every storage of the panel G (NaN / Inf = missing): kind names the truth — packed records under either allele
    convention, 8-bit arrays (no missing code: a missing call is stored as 0) and float arrays."""
    n, pb = G.shape
    bpr = (n + 3) // 4
    if exact:
        rec = ST.pack(G, 1)                                           # the pad calls of the last byte hold 'missing'
        yield "bed a1=0", "bed0", bed_block(ctx, rec, n, bpr, 0)
        yield "bed a1=1 ldb+3", "bed1", bed_block(ctx, rec, n, bpr + 3, 1)
        yield "bed a1=0 16-byte pitch", "bed0", bed_block(ctx, ST.pack(G, 3), n, (bpr + 15) // 16 * 16, 0)
        I = np.where(np.isnan(G), 0, G)
        for dt in (np.int8, np.uint8):
            for sm in (1, 0):
                yield f"{np.dtype(dt).name} sm={sm} +3 base+1", "int", x_block(ctx, I.astype(dt), sm, 3, 1)
            yield f"{np.dtype(dt).name} sm=0 aligned", "int", x_block(ctx, I.astype(dt), 0, aligned(pb), 0)
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


@pytest.mark.parametrize("n,pb,t", COMBOS)
def test_exact_leg(ctx, n, pb, t):
    G, W = _hard(n, pb), _weights(pb, t, True)
    truth = {}
    for tag, kind, block in _sources(ctx, G, True):
        # missing calls are skipped, or there are none to impute (8-bit)
        for impute in ((0, 1) if kind == "int" else (0,)):
            if kind not in truth:
                tr = T.scores(_truth_panel(G, kind), W, 0)
                assert (tr["score"] == (tr["x"] @ W).T).all()          # exact: the wide product and NumPy's agree
                truth[kind] = tr
            tr = truth[kind]
            score, called = run(ctx, [block], W, impute, keep=impute == 0 and kind == "int")
            assert (bits(score) == bits(tr["score"] + 0.0)).all(), (tag, impute, np.argwhere(bits(score) != bits(tr["score"] + 0.0))[:5])
            assert (called == tr["called"]).all(), (tag, impute, np.argwhere(called != tr["called"])[:5])
    assert set(truth) == {"bed0", "bed1", "int", "float"}


def _rounded_gate(score, called, tr, n, pb, tag):
    err, b = np.abs(score - tr["score"]), T.bound(tr, n, pb)
    ratio = np.max(err / np.where(b > 0, b, 1.0))
    print(f"{tag}: max |score - truth| / bound {ratio:.3f}")
    assert (err <= b).all(), (tag, ratio, np.argwhere(err > b)[:5])
    if called is not None:
        assert (called == tr["called"]).all(), (tag, np.argwhere(called != tr["called"])[:5])
    return ratio


@pytest.mark.parametrize("n,pb,t", COMBOS)
def test_rounded_leg(ctx, n, pb, t):
    from pygemma_amd.bed import PackedBed
    X, W = _soft(n, pb), _weights(pb, t, False)
    for impute in (0, 1):
        tr = T.scores(X, W, impute)
        if impute and pb >= 255 and n >= 37:
            assert (tr["soft"] > 0).any()
        same = {}
        for tag, _, block in _sources(ctx, X, False):
            score, called = run(ctx, [block], W, impute)
            _rounded_gate(score, called, tr, n, pb, f"n={n} pb={pb} t={t} impute={impute} {tag}")
            same[tag] = score
        # a result does not depend on pitch, alignment or dtype; the layouts share the chunk order, so they agree too unless a mean differs
        ref = same["float32 sm=1 +3 base+1"]
        for tag, score in same.items():
            if "sm=1" in tag or impute == 0:
                assert (bits(score) == bits(ref)).all(), tag
        assert (bits(same["float32 sm=0 aligned"]) == bits(same["float64 sm=0 +3 base+1"])).all()
    # packed records and 8-bit arrays under rounded weights: imputed means that are no dyadic numbers
    G = _hard(n, pb)
    for a1 in (0, 1):
        tr = T.scores(PackedBed(ST.pack(G), n, count_A1=bool(a1)), W, 1)
        score, called = run(ctx, [bed_block(ctx, ST.pack(G, 1), n, (n + 3) // 4 + 1, a1)], W, 1)
        _rounded_gate(score, called, tr, n, pb, f"n={n} pb={pb} t={t} bed a1={a1} imputed")
        assert (tr["soft"] == 0).all()
    I = np.where(np.isnan(G), 3, G).astype(np.uint8)
    score, called = run(ctx, [x_block(ctx, I, 0, 1, 0)], W, 1, counts=False)
    _rounded_gate(score, called, T.scores(I, W, 1), n, pb, f"n={n} pb={pb} t={t} uint8")


def _split(ctx, X, W, cuts, impute, sm):
    edges = [0, *np.cumsum(cuts)]
    return run(ctx, [x_block(ctx, X[:, a:b], sm, 0, 0) for a, b in zip(edges[:-1], edges[1:])], W, impute)


@pytest.mark.parametrize("n", [257, 1030])
def test_order_contract_and_repeat(ctx, n):
    pb, t = 600, 5
    X, W = _soft(n, pb), _weights(pb, t, False)
    for sm in (1, 0):
        for impute in (0, 1):
            one = _split(ctx, X, W, [600], impute, sm)
            # batches that are multiples of the chunk of 256: the same bits whatever their sizes; and a second run
            for cuts in ([256, 256, 88], [512, 88], [600]):
                got = _split(ctx, X, W, cuts, impute, sm)
                assert (bits(got[0]) == bits(one[0])).all() and (got[1] == one[1]).all(), (sm, impute, cuts)
            # another boundary may move the bits (chunks of 256 from each block's first SNP, and the batch's own means), not past the
            # bound; the truth imputes with the means of the whole panel, the batches with their own — the same SNPs, so the same means
            got = _split(ctx, X, W, [300, 300], impute, sm)
            _rounded_gate(got[0], got[1], T.scores(X, W, impute), n, pb, f"n={n} 300 + 300 sm={sm} impute={impute}")


def test_abi_misuse_launches_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, p, t = 64, 4, 2
    bufs = [ctx.alloc(1 << 16) for _ in range(5)]
    for b in bufs:
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, 1 << 16), "pg_memset")
    ctx.sync()
    X, Wt, work, sc, cn = [b.ptr for b in bufs]
    good = dict(n=n, pb=p, X=X, dtype=2, ldX=n, sm=1, ldb=16, t=t, Wt=Wt, ldw=p, work=work, sc=sc, cn=cn, lds=n)

    def x(**kw):
        a = {**good, **kw}
        return L.pg_prs_x_acc_dev(ctx.handle, a["n"], a["pb"], a["X"], a["dtype"], a["ldX"], a["sm"], a["t"], a["Wt"], a["ldw"], 1, a["work"], a["sc"],
                                  a["cn"], a["lds"])

    def bed(**kw):
        a = {**good, **kw}
        return L.pg_prs_bed_acc_dev(ctx.handle, a["n"], a["pb"], a["X"], a["ldb"], 0, a["t"], a["Wt"], a["ldw"], 1, a["work"], a["sc"], a["cn"], a["lds"])

    for call, name in ((x, b"pg_prs_x_acc_dev"), (bed, b"pg_prs_bed_acc_dev")):
        for kw in (dict(X=None), dict(Wt=None), dict(work=None), dict(sc=None), dict(n=0), dict(n=1 << 30), dict(pb=-1),
                   dict(pb=(1 << 25) + 1, ldX=1 << 26, ldw=1 << 26), dict(t=0), dict(ldw=p - 1), dict(lds=n - 1),
                   dict(n=(1 << 30) - 1, pb=1 << 25, ldX=1 << 30, ldb=1 << 28, ldw=1 << 25, lds=1 << 30)):      # 2^39 workgroups
            assert call(**kw) == -22 and name in L.pg_last_error(), kw
        assert call(t=65) == -95 and name in L.pg_last_error()
        assert call(pb=0) == 0 and call(pb=0, cn=None) == 0                       # nothing to do is no error
    assert x(ldX=n - 1) == -22 and x(sm=0, ldX=p - 1) == -22 and bed(ldb=15) == -22
    assert x(dtype=4) == -95 and x(dtype=-1) == -95
    ctx.sync()
    for b in bufs[2:]:
        assert (b.download((1 << 16,), np.uint8) == 0x7f).all()
    for b in bufs:
        b.free()


# ---- lmm.prs -------------------------------------------------------------------------------------------------------------------------

def frame_bits(df):
    return df.to_numpy().view(np.uint64) if (df.dtypes == np.float64).all() else df.to_numpy()


@functools.lru_cache(maxsize=None)
def _driver_panel():
    n, p = 257, 1500
    G = _hard(n, p)
    rng = np.random.default_rng(9)
    X = G.astype(np.float32)
    X[:, 100:160] += (0.1 * rng.standard_normal((n, 60))).astype(np.float32)
    X.flags.writeable = False
    return G, X


def _driver_sources():
    from pygemma_amd.bed import PackedBed
    G, X = _driver_panel()
    n = G.shape[0]
    return {"bed": (PackedBed(ST.pack(G), n), lambda ctx: bed_block(ctx, ST.pack(G), n, (n + 3) // 4, 0)),
            "float32 C": (np.array(X), lambda ctx: x_block(ctx, X, 0)),
            "int8 F": (np.asfortranarray(np.where(np.isnan(G), 0, G).astype(np.int8)), lambda ctx: x_block(ctx, np.where(np.isnan(G), 0, G).astype(np.int8), 1))}


@pytest.mark.parametrize("source", ["bed", "float32 C", "int8 F"])
def test_driver_against_the_abi(ctx, source):
    from pygemma import lmm
    src, block = _driver_sources()[source]
    n, p = src.shape
    W = _weights(p, 3, False)
    for missing, impute in (("mean", 1), ("skip", 0)):
        score, called = run(ctx, [block(ctx)], W, impute)
        st_ = {}
        names = [f"id{i}" for i in range(n)]
        S, Cn = lmm.prs(src, pd.DataFrame(np.array(W), columns=["a", "b", "c"]), missing=missing, counts=True, samples=names, stats=st_)
        assert list(S.columns) == list(Cn.columns) == ["a", "b", "c"] and list(S.index) == list(Cn.index) == names
        assert (S.dtypes == np.float64).all() and (Cn.dtypes == np.int64).all() and S.shape == Cn.shape == (n, 3)
        assert (frame_bits(S) == bits(score.T)).all() and (Cn.to_numpy() == called.T).all()
        assert set(st_) >= {"batches", "bytes_in", "seconds", "snps_used"} and st_["batches"] == 1 and st_["snps_used"] == p
        # the batch size is rounded up to the chunk: the same bits from any
        for sb in (256, 300, None):
            st_ = {}
            S2 = lmm.prs(src, W, missing=missing, snp_batch=sb, stats=st_)
            assert list(S2.columns) == [0, 1, 2] and list(S2.index) == list(range(n))
            assert (frame_bits(S2) == frame_bits(S)).all(), (missing, sb)
            assert st_["batches"] == {256: 6, 300: 3, None: 1}[sb]


def test_driver_drops_unweighted_snps(monkeypatch):
    from pygemma import lmm
    import pygemma_amd.lmm as impl
    for source, (src, _) in _driver_sources().items():
        if source == "float32 C":                                      # the exact leg: hard calls
            src = _driver_panel()[0].astype(np.float32)
        n, p = src.shape
        W = np.array(_weights(p, 3, True))
        W[np.random.default_rng(1).random(p) < 0.9] = 0.0
        used = int((W != 0).any(axis=1).sum())
        assert 0 < used <= p // 2
        st_ = {}
        S, Cn = lmm.prs(src, W, missing="skip", counts=True, stats=st_)
        assert st_["snps_used"] == used
        with monkeypatch.context() as m:
            m.setattr(impl, "_PRS_DROP", 2.0)
            st_ = {}
            S0, Cn0 = lmm.prs(src, W, missing="skip", counts=True, stats=st_)
            assert st_["snps_used"] == p
        assert (frame_bits(S) == frame_bits(S0)).all() and (Cn.to_numpy() == Cn0.to_numpy()).all(), source
        tr = T.scores(src, W, 0)
        assert (frame_bits(S) == bits((tr["score"] + 0.0).T)).all() and (Cn.to_numpy() == tr["called"].T).all()


def test_driver_column_groups():
    from pygemma import lmm
    src = _driver_sources()["bed"][0]
    n, p = src.shape
    W = _weights(p, 70, False)
    S, Cn = lmm.prs(src, W, counts=True, snp_batch=512)
    assert S.shape == Cn.shape == (n, 70) and list(S.columns) == list(range(70))
    for a, b in ((0, 64), (64, 70)):
        Sg, Cg = lmm.prs(src, W[:, a:b], counts=True, snp_batch=512)
        assert (frame_bits(Sg) == frame_bits(S.iloc[:, a:b])).all() and (Cg.to_numpy() == Cn.iloc[:, a:b].to_numpy()).all()
    tr = T.scores(src, W, 1)
    _rounded_gate(S.to_numpy().T, Cn.to_numpy().T, tr, n, p, "lmm.prs t=70")
