"""GPU checks of the case/control tests (pg_cc_setup_dev, pg_cc_pack_x_dev, pg_cc_count_dev, pg_cc_stats_dev, lmm.case_control) — run with
-m gpu on an MI355X.

The truth is tests/_case_control_truth.py.  Counts are compared for equality, for every source kind; packed records byte for byte with
the host's own packing.  With u = 2^-53: the chi2 columns, or and af_* lie within 16 u relative of the exact-rational truth (the stated
operation order has at most 8 roundings for a 2 x 2 or trend statistic, 7 for the three-term genotypic sum and 11 for the same sum
over its six cells; the gate is twice the larger count, with 16 for 22), cmh_v and or_mh within (16 + S + 8) u, cmh_u within
(S + 3) u sum |term_k| absolute; chi2_cmh is bit-equal to cmh_u * cmh_u / cmh_v evaluated in NumPy on the device's own two columns; the
NaN / inf patterns equal the truth's; and every fp64 column is bit-equal to the NumPy replay of the documented operation order.
p_fisher lies within 8 M u relative (M recurrence steps, the smallest margin of the table) on panels that the truth helper alone shows
to have no non-tie term within 2^-20 of P(obs)."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import _case_control_truth as T

pytestmark = pytest.mark.gpu

DTYPES = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}
NS = [1, 3, 17, 63, 64, 65, 257, 1030]     # tails of a byte, of a 16-call word and of a 64-call lane load; past the 1024 calls of a step
U = 2.0 ** -53
EINVAL, ENOTSUP = -22, -95
COLS = ("af_case", "af_ctrl", "or", "chi2_allelic", "chi2_trend", "chi2_geno", "chi2_dom", "chi2_rec", "p_fisher", "chi2_cmh", "or_mh")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _call(ctx, specs, fn):
    """fn(*window pointers) on windows of larger buffers filled with 0x7f: specs is [(rows, bytes per row, dtype)], a window starts three
    rows into a buffer of rows + 7.  Every byte outside the windows must come back as it was.  Returns the windows as (rows, -1) arrays."""
    from pygemma_amd import _lib
    L = _lib.load()
    K = _lib.load_cc()
    bufs = []
    for rows, rb, _ in specs:
        b = ctx.alloc((rows + 7) * rb)
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, (rows + 7) * rb), "pg_memset")
        bufs.append(b)
    fn(*[b.ptr + 3 * rb for b, (_, rb, _) in zip(bufs, specs)])
    ctx.sync()
    out = []
    for b, (rows, rb, dt) in zip(bufs, specs):
        full = b.download((rows + 7, rb), np.uint8)
        assert (full[:3] == 0x7f).all() and (full[3 + rows:] == 0x7f).all(), "bytes outside the window were written"
        out.append(np.ascontiguousarray(full[3:3 + rows]).view(dt))
        b.free()
    return out


def pitches(bpr):
    """Record pitches on 16 bytes, on 4 bytes (and not on 16) and odd, each with its base offset into a 256-byte aligned buffer."""
    p16 = (bpr + 15) // 16 * 16 + 16
    p4 = (bpr + 3) // 4 * 4 + 4
    p4 += 4 if p4 % 16 == 0 else 0
    return {"16": (p16, 0), "4": (p4, 4), "odd": ((bpr | 1) + 2, 1)}


@functools.lru_cache(maxsize=None)
def _calls(n, p=130, seed=0, miss=0.1):
    """(n, p) dosages 0/1/2 with `miss` missing; column 0 all missing, column 1 monomorphic, column 2 fully called."""
    rng = np.random.default_rng(seed + 7 * n)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, p), (n, p)).astype(np.float64)
    G[rng.random((n, p)) < miss] = np.nan
    G[:, 0] = np.nan
    G[:, 1] = 2.0
    G[:, 2] = rng.integers(0, 3, n)
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _groups(n, S, kind):
    """(status int8, stratum int32 or None).  mixed: cases, controls and -1 at random, strata at random with some excluded (-1, and one
    label >= S); single: one case, the rest controls; degenerate: stratum 1 without a control, the last stratum of one sample."""
    rng = np.random.default_rng(1000 * S + n + len(kind))
    status = rng.choice(np.array([-1, 0, 1, 1], np.int8), n)
    stratum = None
    if S > 1 or kind == "degenerate":
        stratum = rng.integers(0, S, n).astype(np.int32)
        stratum[rng.random(n) < 0.1] = -1
        if n > 5:
            stratum[5] = S                                              # outside 0..S-1: in no group
    if kind == "single":
        status[:] = 0
        status[n // 2] = 1
    if kind == "degenerate" and S > 1:
        status[stratum == 1] = 1
        stratum[stratum == S - 1] = 0
        stratum[0] = S - 1
    for a in (status, stratum):
        if a is not None:
            a.flags.writeable = False
    return status, stratum


def run_count(ctx, rec, n, S, status, stratum, count_a1, pitch="16", hard=None, stat=False, fisher=1):
    """pg_cc_setup_dev and pg_cc_count_dev (then pg_cc_stats_dev) on records copied into rows whose pad bytes hold 0xff."""
    from pygemma_amd import _lib
    L = _lib.load()
    K = _lib.load_cc()
    pb, bpr = rec.shape
    ldb, shift = pitches(bpr)[pitch]
    buf = np.full(shift + pb * ldb, 0xff, np.uint8)
    buf[shift:].reshape(pb, ldb)[:, :bpr] = rec
    dX, dst = ctx.to_device(buf), ctx.to_device(np.ascontiguousarray(status, np.int8))
    dk = None if stratum is None else ctx.to_device(np.ascontiguousarray(stratum, np.int32))
    dh = None if hard is None else ctx.to_device(np.ascontiguousarray(hard, np.uint8))
    wb = int(K.pg_cc_work_bytes(n, S))
    assert wb == 256 + 2 * S * (((n + 15) // 16 + 3) // 4 * 4) * 4
    work = ctx.alloc(wb)
    _lib.check(K.pg_cc_setup_dev(ctx.handle, n, S, dst.ptr, None if dk is None else dk.ptr, work.ptr), "pg_cc_setup_dev")

    def fn(c, m, s=None):
        _lib.check(K.pg_cc_count_dev(ctx.handle, n, pb, dX.ptr + shift, ldb, count_a1, S, work.ptr, None if dh is None else dh.ptr, c, m), "pg_cc_count_dev")
        if s is not None:
            _lib.check(K.pg_cc_stats_dev(ctx.handle, pb, c, m, fisher, s), "pg_cc_stats_dev")
    res = _call(ctx, [(pb, 64, np.int64), (pb, 32, np.float64)] + ([(pb, 88, np.float64)] if stat else []), fn)
    for b in (dX, dst, dk, dh, work):
        if b is not None:
            b.free()
    return res


CONFIGS = [(1, 130, "16", 0, "mixed"), (1, 19, "odd", 1, "single"), (2, 130, "4", 0, "mixed"), (4, 19, "16", 0, "mixed"), (5, 19, "16", 1, "degenerate"),
           (16, 130, "odd", 0, "degenerate"), (16, 1, "4", 1, "mixed")]


@pytest.mark.parametrize("n", NS)
def test_count_blocks(ctx, n):
    """Counts equal the boolean-mask truth and the CMH sums the replay of their order, bit for bit: every load path, both allele
    conventions, pad calls of the last byte that hold 11, partly empty workgroups, every compiled stratum bucket."""
    G = _calls(n)
    for S, pb, pitch, a1, kind in CONFIGS:
        status, stratum = _groups(n, S, kind)
        s0 = 0 if pb == 130 else 2
        rec = T.pack(G[:, s0:s0 + pb], pad_code=3)
        counts, cmh = run_count(ctx, rec, n, S, status, stratum, a1, pitch)
        tab = T.tables((2 - G if a1 else G)[:, s0:s0 + pb], status, stratum, S)
        tag = (n, S, pb, pitch, a1, kind)
        assert (counts == tab.sum(axis=1)).all(), (tag, np.flatnonzero((counts != tab.sum(axis=1)).any(axis=1))[:5])
        assert same_bits(cmh, T.replay_cmh(tab)).all(), tag


def run_pack(ctx, X, snp_major, extra, shift, pitch):
    """pg_cc_pack_x_dev on the (n, p) host matrix X stored SNP-major (p x n) or sample-major (n x p) at a pitch `extra` elements larger than
    minimal, the block `shift` elements into its buffer, the pad holding NaN (0xff bytes for 8-bit blocks).  Returns (records (pb,
    ceil(n/4)), hard): the records are a window of a 0x7f buffer, and the bytes of a row beyond ceil(n/4) must stay 0x7f."""
    from pygemma_amd import _lib
    L = _lib.load()
    K = _lib.load_cc()
    n, pb = X.shape
    A = np.ascontiguousarray(X.T) if snp_major else np.ascontiguousarray(X)
    rows, width = A.shape
    ldX = width + extra
    buf = np.full(shift + rows * ldX, np.nan, A.dtype) if A.dtype.kind == "f" else np.full(shift + rows * ldX, -1, np.int64).astype(A.dtype)
    buf[shift:].reshape(rows, ldX)[:, :width] = A
    dX = ctx.to_device(buf)
    bpr = (n + 3) // 4
    ldb, off = pitches(bpr)[pitch]
    rec, hard = _call(ctx, [(pb + 1, ldb, np.uint8), (pb, 1, np.uint8)], lambda r, h: _lib.check(
        K.pg_cc_pack_x_dev(ctx.handle, n, pb, dX.ptr + shift * A.itemsize, DTYPES[A.dtype], ldX, int(snp_major), r + off, ldb, h), "pg_cc_pack_x_dev"))
    dX.free()
    flat = rec.reshape(-1)[off:off + pb * ldb].reshape(pb, ldb)
    assert (rec.reshape(-1)[:off] == 0x7f).all() and (rec.reshape(-1)[off + pb * ldb:] == 0x7f).all() and (flat[:, bpr:] == 0x7f).all(), "pad bytes were written"
    return np.ascontiguousarray(flat[:, :bpr]), hard[:, 0]


@pytest.mark.parametrize("n", NS)
def test_pack_blocks(ctx, n):
    """Records byte-equal to the host's packing and the hard flags equal to the truth: four dtypes, both layouts, vector and scalar loads
    and stores; a SNP with one 0.5, one with a NaN (still hard-call), an all-missing one; then the counts from the device's own records."""
    G = _calls(n).copy()
    if n > 1:
        G[1, 3] = np.nan
    soft = G.copy()
    soft[n // 2, 4] = 0.5                                               # an observed value that is no call
    soft[0, 6] = 1e300 if n > 2 else soft[0, 6]                         # finite in float64, a value; +inf in float32, missing
    Gi = np.where(np.isnan(G), 0, G)                                    # 8-bit blocks have no missing code
    Gi[n // 2, 4] = 3
    status, stratum = _groups(n, 5, "mixed")
    with np.errstate(over="ignore"):
        soft32 = soft.astype(np.float32)
    kinds = [(soft32, True, "16"), (soft32, False, "4"), (soft, True, "odd"), (soft, False, "16"),
             (Gi.astype(np.int8), True, "4"), (Gi.astype(np.int8), False, "odd"), (Gi.astype(np.uint8), True, "16"), (Gi.astype(np.uint8), False, "16")]
    for k, (X, snp_major, pitch) in enumerate(kinds):
        width = n if snp_major else X.shape[1]
        for extra, shift in ((16 + (-width) % 16, 0), (1, 1)):
            rec, hard = run_pack(ctx, X, snp_major, extra, shift, pitch)
            Xd = X.astype(np.float64)
            if X.dtype == np.float32:
                Xd[~np.isfinite(X)] = np.nan
            want_hard = T.hard_calls(Xd)
            tag = (n, X.dtype, snp_major, pitch, extra)
            assert (hard == want_hard).all(), (tag, np.flatnonzero(hard != want_hard))
            assert (rec[want_hard] == T.pack(Xd)[want_hard]).all(), tag
        if k < 4:
            counts, _ = run_count(ctx, rec, n, 5, status, stratum, 0, "16", hard=hard)
            assert (counts == T.tables(Xd, status, stratum, 5).sum(axis=1)).all(), tag
            assert not want_hard[4] and (counts[4] == 0).all()


def _stat_panel(n, p, S, seed):
    """Genotypes with an association in some columns, groups of kind degenerate, and the tables' truth."""
    rng = np.random.default_rng(seed)
    status, stratum = _groups(n, S, "degenerate" if S > 1 else "mixed")
    G = rng.binomial(2, rng.uniform(0.05, 0.6, p), (n, p)).astype(np.float64)
    lift = (status == 1)[:, None] & (rng.random((n, p)) < 0.3) & (np.arange(p) % 3 == 0)[None, :]
    G = np.minimum(G + lift, 2.0)
    G[rng.random((n, p)) < 0.05] = np.nan
    if p > 4:
        G[:, 0] = np.nan
        G[:, 1] = 2.0
        if n < 300:                                                     # (at n = 1030 its exact p, 1e-600, is no double)
            G[:, 2] = np.where(status == 1, 2.0, 0.0)                   # complete separation: b c = 0 < a d
        G[:, 3] = np.where(G[:, 3] == 2, 1.0, G[:, 3])                  # an unseen genotype
    tab = T.tables(G, status, stratum, S)
    return G, status, stratum, tab


PANELS = [(257, 130, 5, 11), (1030, 19, 16, 12), (65, 130, 1, 13), (64, 130, 2, 14)]


@pytest.mark.parametrize("n,p,S,seed", PANELS)
def test_statistics(ctx, n, p, S, seed):
    G, status, stratum, tab = _stat_panel(n, p, S, seed)
    tr = T.truth(tab)
    counts, cmh, stat = run_count(ctx, T.pack(G), n, S, status, stratum, 0, "16", stat=True)
    assert (counts == tr["counts"]).all()
    got = dict(zip(COLS, stat.T), cmh_u=cmh[:, 0], cmh_v=cmh[:, 1])
    tag = (n, p, S)
    for k in COLS + ("cmh_u", "cmh_v"):
        assert (np.isnan(got[k]) == np.isnan(tr[k])).all() and (np.isinf(got[k]) == np.isinf(tr[k])).all(), (tag, k, "NaN / inf pattern")
    live = ~np.isnan(tr["af_case"])
    assert live.sum() >= p - 3
    with np.errstate(invalid="ignore"):
        for k in T.STAT + ("cmh_v", "or_mh"):
            m = np.isfinite(tr[k])
            bound = (16 + (S + 8 if k in ("cmh_v", "or_mh") else 0)) * U
            err = np.abs(got[k][m] - tr[k][m]) / np.where(tr[k][m] == 0, 1.0, np.abs(tr[k][m]))
            print(f"{tag} {k}: {m.sum()} rows, max err / bound {err.max() / bound if m.any() else 0:.3f}")
            assert (err <= bound).all(), (tag, k, err.max() / U)
        eu = np.abs(got["cmh_u"][live] - tr["cmh_u"][live])
        bu = (S + 3) * U * tr["cmh_abs"][live]
        assert (eu <= bu).all(), (tag, "cmh_u")
        want = np.where(got["cmh_v"] == 0, np.nan, got["cmh_u"] * got["cmh_u"] / got["cmh_v"])
    assert same_bits(got["chi2_cmh"], want).all(), (tag, "chi2_cmh is not cmh_u * cmh_u / cmh_v")
    # Fisher: the panel holds no near-tie (seed chosen on the CPU), so the tail is the same set of terms as the exact one
    assert (tr["fisher_gap"][live] > 2.0 ** -20).all(), "choose another seed: a non-tie term lies within 2^-20 of P(obs)"
    M = np.maximum(tr["fisher_steps"][live], 1)
    ef = np.abs(got["p_fisher"][live] - tr["p_fisher"][live]) / tr["p_fisher"][live]
    print(f"{tag} p_fisher: max err / bound {np.max(ef / (8 * M * U)):.3f}, p from {tr['p_fisher'][live].min():.3g}")
    assert (ef <= 8 * M * U).all(), (tag, "p_fisher")
    # and every column is the documented operation order, bit for bit
    rp = T.replay(tab)
    for j, k in enumerate(COLS):
        assert same_bits(got[k], rp[:, j]).all(), (tag, k, "replay")
    # without the exact test the column is NaN and nothing else moves
    _, _, st0 = run_count(ctx, T.pack(G), n, S, status, stratum, 0, "4", stat=True, fisher=0)
    assert np.isnan(st0[:, 8]).all() and same_bits(np.delete(st0, 8, axis=1), np.delete(stat, 8, axis=1)).all()


def test_stats_rows_by_hand(ctx):
    """pg_cc_stats_dev on counts written by hand: an exact Fisher tie (a = d, b = c), no called case, a zero cell, b c = 0 < a d, a
    monomorphic SNP, a count outside its range; cmh NULL."""
    from pygemma_amd import _lib
    L = _lib.load()
    K = _lib.load_cc()
    rows = np.array([[2, 0, 5, 0, 5, 0, 2, 0], [0, 0, 0, 4, 3, 2, 1, 0], [5, 0, 0, 0, 3, 2, 0, 0], [0, 0, 4, 0, 3, 0, 0, 0], [4, 0, 0, 0, 3, 0, 0, 0],
                     [3, 1, 2, 0, 4, 4, 1, 1], [-1, 1, 2, 0, 4, 4, 1, 1]], np.int64)
    dc = ctx.to_device(rows)
    stat, = _call(ctx, [(len(rows), 88, np.float64)], lambda s: _lib.check(K.pg_cc_stats_dev(ctx.handle, len(rows), dc.ptr, None, 1, s), "pg_cc_stats_dev"))
    dc.free()
    good = rows[:6]
    tr = T.truth(good[:, None, :])
    assert T.allelic(rows[0]) == (10, 4, 4, 10)
    pf = T.fisher(10, 4, 4, 10)[0]
    assert abs(stat[0, 8] - float(pf)) <= 8 * 14 * U * float(pf) and stat[0, 8] < 1.0
    assert np.isnan(stat[1]).all() and np.isnan(stat[6]).all()
    assert stat[2, 2] == 0.0 and stat[3, 2] == math.inf and np.isnan(stat[4, 2]) and np.isnan(stat[4, 3]) and stat[4, 8] == 1.0
    assert np.isnan(stat[:, 9:]).all()
    rp = T.replay(good[:, None, :])
    assert same_bits(stat[:6, :9], rp[:, :9]).all()
    for j, k in enumerate(T.STAT):
        m = np.isfinite(tr[k])
        assert (np.isnan(stat[:6, j]) == np.isnan(tr[k])).all() and (np.abs(stat[:6, j][m] - tr[k][m]) <= 16 * U * np.abs(tr[k][m])).all(), k


def test_misuse_is_refused_and_writes_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    K = _lib.load_cc()
    n, pb, bpr = 37, 5, 10
    h = ctx.handle
    dX, dst = ctx.to_device(np.zeros((pb, 16), np.uint8)), ctx.to_device(np.ones(n, np.int8))
    dF = ctx.to_device(np.zeros((pb, n), np.float32))
    work = ctx.alloc(int(K.pg_cc_work_bytes(n, 16)))
    assert K.pg_cc_work_bytes(0, 1) == 0 and K.pg_cc_work_bytes(1 << 30, 1) == 0 and K.pg_cc_work_bytes(n, 0) == 0 and K.pg_cc_work_bytes(n, 17) == 0
    bufs = [ctx.alloc(4096) for _ in range(4)]
    for b in bufs + [work]:
        _lib.check(L.pg_memset(h, b.ptr, 0x7f, b.nbytes), "pg_memset")
    c, m, s, r = (b.ptr for b in bufs)
    calls = [
        (K.pg_cc_setup_dev(h, n, 1, None, None, work.ptr), EINVAL), (K.pg_cc_setup_dev(h, n, 1, dst.ptr, None, None), EINVAL),
        (K.pg_cc_setup_dev(None, n, 1, dst.ptr, None, work.ptr), EINVAL), (K.pg_cc_setup_dev(h, 0, 1, dst.ptr, None, work.ptr), EINVAL),
        (K.pg_cc_setup_dev(h, 1 << 30, 1, dst.ptr, None, work.ptr), EINVAL), (K.pg_cc_setup_dev(h, n, 0, dst.ptr, None, work.ptr), ENOTSUP),
        (K.pg_cc_setup_dev(h, n, 17, dst.ptr, None, work.ptr), ENOTSUP), (K.pg_cc_setup_dev(h, n, 1, dst.ptr, None, work.ptr + 4), EINVAL),
        (K.pg_cc_count_dev(h, n, pb, None, 16, 0, 1, work.ptr, None, c, m), EINVAL), (K.pg_cc_count_dev(h, n, pb, dX.ptr, 16, 0, 1, None, None, c, m), EINVAL),
        (K.pg_cc_count_dev(h, n, pb, dX.ptr, 16, 0, 1, work.ptr, None, None, m), EINVAL), (K.pg_cc_count_dev(h, n, pb, dX.ptr, 16, 0, 1, work.ptr, None, c, None), EINVAL),
        (K.pg_cc_count_dev(h, n, pb, dX.ptr, bpr - 1, 0, 1, work.ptr, None, c, m), EINVAL), (K.pg_cc_count_dev(h, n, -1, dX.ptr, 16, 0, 1, work.ptr, None, c, m), EINVAL),
        (K.pg_cc_count_dev(h, n, (1 << 25) + 1, dX.ptr, 16, 0, 1, work.ptr, None, c, m), EINVAL),
        (K.pg_cc_count_dev(h, n, pb, dX.ptr, 16, 0, 0, work.ptr, None, c, m), ENOTSUP), (K.pg_cc_count_dev(h, n, pb, dX.ptr, 16, 0, 17, work.ptr, None, c, m), ENOTSUP),
        (K.pg_cc_count_dev(h, n, 0, dX.ptr, 16, 0, 1, work.ptr, None, c, m), 0),
        (K.pg_cc_pack_x_dev(h, n, pb, None, 2, n, 1, r, 16, s), EINVAL), (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, 2, n, 1, None, 16, s), EINVAL),
        (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, 2, n, 1, r, 16, None), EINVAL), (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, 2, n - 1, 1, r, 16, s), EINVAL),
        (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, 2, pb - 1, 0, r, 16, s), EINVAL), (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, 2, n, 1, r, bpr - 1, s), EINVAL),
        (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, 4, n, 1, r, 16, s), ENOTSUP), (K.pg_cc_pack_x_dev(h, n, pb, dF.ptr, -1, n, 1, r, 16, s), ENOTSUP),
        (K.pg_cc_pack_x_dev(h, n, 0, dF.ptr, 2, n, 1, r, 16, s), 0),
        (K.pg_cc_stats_dev(h, pb, None, None, 1, s), EINVAL), (K.pg_cc_stats_dev(h, pb, c, None, 1, None), EINVAL), (K.pg_cc_stats_dev(h, -1, c, None, 1, s), EINVAL),
        (K.pg_cc_stats_dev(h, 1 << 31, c, None, 1, s), EINVAL), (K.pg_cc_stats_dev(h, 0, c, None, 1, s), 0),
    ]
    ctx.sync()
    for k, (rc, want) in enumerate(calls):
        assert rc == want, (k, rc, want)
    for b in bufs + [work]:
        assert (b.download((b.nbytes,), np.uint8) == 0x7f).all(), "a refused call or a no-op wrote"
    for b in bufs + [work, dX, dst, dF]:
        b.free()


# ---- lmm.case_control end to end -------------------------------------------------------------------------------------------------------
N2, P2 = 257, 300


@functools.lru_cache(maxsize=None)
def _cohort():
    rng = np.random.default_rng(21)
    G = rng.binomial(2, rng.uniform(0.1, 0.5, P2), (N2, P2)).astype(np.float64)
    G[:, 7] = rng.binomial(2, 0.4, N2)
    y = (G[:, 7] + rng.normal(0, 0.4, N2) > 0.9).astype(np.float64)     # SNP 7 is causal
    y[rng.random(N2) < 0.05] = np.nan
    full = G.copy()
    G[rng.random(G.shape) < 0.05] = np.nan
    G[:, 7] = full[:, 7]
    strata = rng.integers(0, 4, N2) * 10 - 10                          # labels -10 (excluded), 0, 10, 20
    return G, full, y, strata


def assert_same_frame(a, b, tag):
    assert list(a.columns) == list(b.columns), tag
    for col in a.columns:
        x, z = a[col].to_numpy(), b[col].to_numpy()
        if x.dtype.kind == "f":
            assert same_bits(x, z).all(), (tag, col, np.flatnonzero(~same_bits(x, z))[:5])
        else:
            assert x.dtype == z.dtype and (x == z).all(), (tag, col)


def test_case_control_sources_batches_and_columns(ctx):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    G, full, y, strata = _cohort()
    bed = PackedBed(T.pack(G), N2)
    st = {}
    ref = lmm.case_control(bed, y, strata=strata, stats=st)
    assert st["batches"] == 1 and st["bytes_in"] == P2 * 65 and st["seconds"] > 0
    z = ref["chi2_trend"].to_numpy()
    assert st["lambda_gc"] == float(np.median(z[~np.isnan(z)]) / 0.4549364)
    assert list(ref.columns) == list(lmm._CC_COLS) and ref["case0"].dtype == np.int64 and ref["hard"].dtype == np.bool_ and ref["hard"].all()
    # the truth, through the wrapper's own mapping of y and the labels
    status = np.where(y == 1, 1, np.where(y == 0, 0, -1))
    code = np.where(strata < 0, -1, strata // 10)
    tab = T.tables(G, status, code, 3)
    assert (ref[list(lmm._CC_COUNTS)].to_numpy() == tab.sum(axis=1)).all()
    rp = T.replay(tab)
    for j, k in enumerate(COLS):
        assert same_bits(ref[k].to_numpy(), rp[:, j]).all(), k
    assert same_bits(ref[["cmh_u", "cmh_v"]].to_numpy(), T.replay_cmh(tab)[:, :2]).all()
    # every source gives the same frame
    Xf = bed.to_float(impute=False)
    assert np.isnan(Xf).any()
    for tag, X in (("float32 C", Xf), ("float32 F", np.asfortranarray(Xf)), ("float64", Xf.astype(np.float64)), ("float64 F", np.asfortranarray(Xf.astype(np.float64)))):
        assert_same_frame(lmm.case_control(X, y, strata=strata), ref, tag)
    flip = PackedBed(T.pack(G), N2, count_A1=True)
    assert_same_frame(lmm.case_control(flip, y, strata=strata), lmm.case_control(flip.to_float(impute=False), y, strata=strata), "count_A1")
    assert (lmm.case_control(flip, y)["case0"].to_numpy() == lmm.case_control(bed, y)["case2"].to_numpy()).all()
    whole = lmm.case_control(PackedBed(T.pack(full), N2), y, strata=strata)
    for tag, X in (("int8 C", full.astype(np.int8)), ("int8 F", np.asfortranarray(full.astype(np.int8))), ("uint8 C", full.astype(np.uint8))):
        assert_same_frame(lmm.case_control(X, y, strata=strata), whole, tag)
    # batches
    st2 = {}
    assert_same_frame(lmm.case_control(bed, y, strata=strata, snp_batch=128, stats=st2), ref, "snp_batch=128, records")
    assert st2["batches"] == 3
    assert_same_frame(lmm.case_control(Xf, y, strata=strata, snp_batch=128), ref, "snp_batch=128, float32")
    # a dosage makes its SNP no hard call: counts 0, statistics NaN, the other rows as they were
    Xs = Xf.copy()
    Xs[3, 5] = 0.5
    soft = lmm.case_control(Xs, y, strata=strata, snps=[f"rs{j}" for j in range(P2)])
    assert list(soft.columns)[-1] == "SNPs" and soft["SNPs"][5] == "rs5"
    assert not soft["hard"][5] and (soft.loc[5, list(lmm._CC_COUNTS)] == 0).all() and soft.loc[5, list(COLS) + ["p_trend", "cmh_u"]].isna().all()
    keep = np.arange(P2) != 5
    assert_same_frame(soft.drop(columns="SNPs")[keep].reset_index(drop=True), ref[keep].reset_index(drop=True), "beside a soft SNP")
    # p-values: the wrapper's own expressions on the returned chi2
    for name in ("allelic", "trend", "dom", "rec", "cmh"):
        assert same_bits(ref["p_" + name].to_numpy(), lmm._cc_p1(ref["chi2_" + name].to_numpy())).all(), name
    assert same_bits(ref["p_geno"].to_numpy(), lmm._cc_p2(ref["chi2_geno"].to_numpy())).all()
    assert ref["p_trend"].idxmin() == 7 and ref["p_trend"][7] < 1e-12
    # no strata against a single stratum; no exact test
    plain, one = lmm.case_control(bed, y), lmm.case_control(bed, y, strata=np.zeros(N2, np.int64))
    assert list(plain.columns) == [c for c in lmm._CC_COLS if c not in lmm._CC_CMH]
    assert_same_frame(plain, one[list(plain.columns)], "strata=None")
    nof = lmm.case_control(bed, y, fisher=False)
    assert_same_frame(nof, plain.drop(columns="p_fisher"), "fisher=False")
    # one stratum: chi2_cmh = chi2_allelic (T - 1) / T, T the alleles of the table
    alleles = 2 * one[["case0", "case1", "case2", "ctrl0", "ctrl1", "ctrl2"]].to_numpy().sum(axis=1)
    for g in range(P2):
        a, c = one["chi2_allelic"][g], one["chi2_cmh"][g]
        assert np.isnan(a) == np.isnan(c)
        if not np.isnan(a):
            want = Fraction(a) * Fraction(int(alleles[g]) - 1, int(alleles[g]))
            assert abs(Fraction(c) - want) <= Fraction(16 * U) * want, (g, a, c)
