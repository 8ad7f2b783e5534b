"""GPU checks of the permutation tests (pg_perm_label_counts_dev, pg_perm_totals_dev, pg_perm_block_dev, lmm.case_control_perm) — run
with -m gpu on an MI355X.

The truth is tests/_perm_truth.py.  Totals, counts and maxima are compared for equality (integers and bit patterns).  With u = 2^-53,
every statistic is bit-equal to the NumPy replay of the documented operation order, NaN pattern included, and lies within 16 u relative
of the exact rational value (the stated order has at most 8 roundings; the gate is case_control's: 15.5 u against the exact value
rounded once).  Both tile paths (PG_PERM_PLANES) give the same bits, and every byte around an output window stays as it was."""
import functools
import math
import os

import numpy as np
import pytest

import _case_control_truth as CT
import _perm_truth as T

pytestmark = pytest.mark.gpu

NS = [1, 3, 127, 128, 129, 257, 1030]                 # the K-tile edges
# (a0, na, nb): na over the SNP edges of both tile paths, nb over the labelling tile's; a0 + na <= 520, a0 = 256 starts in the tile that
# holds missing calls of the mixed panel
WINDOWS = [(0, 1, 257), (0, 127, 256), (3, 128, 255), (0, 129, 1), (0, 256, 257), (0, 257, 256), (3, 257, 1), (256, 257, 255), (259, 256, 257),
           (263, 257, 257)]
KINDS = ("full", "miss", "mix")
P, NB = 520, 257
EINVAL, ENOTSUP = -22, -95


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def planes_env():
    def set_planes(on):
        if on:
            os.environ["PG_PERM_PLANES"] = "1"
        else:
            os.environ.pop("PG_PERM_PLANES", None)
    yield set_planes
    os.environ.pop("PG_PERM_PLANES", None)


def _windows(ctx, specs, fn):
    """fn(*window pointers) on windows of larger buffers filled with 0x7f: specs is [(rows, bytes per row used, bytes of row pitch,
    dtype)]; a window starts three rows into a buffer of rows + 7.  Every byte outside the windows — the rows around and the pad of
    every row — must come back as it was.  Returns the windows as (rows, -1) arrays."""
    from pygemma_amd import _lib
    L = _lib.load()
    bufs = []
    for rows, used, pitch, _ in specs:
        b = ctx.alloc((rows + 7) * pitch)
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, (rows + 7) * pitch), "pg_memset")
        bufs.append(b)
    fn(*[b.ptr + 3 * pitch for b, (_, _, pitch, _) in zip(bufs, specs)])
    ctx.sync()
    out = []
    for b, (rows, used, pitch, dt) in zip(bufs, specs):
        full = b.download((rows + 7, pitch), np.uint8)
        assert (full[:3] == 0x7f).all() and (full[3 + rows:] == 0x7f).all() and (full[3:3 + rows, used:] == 0x7f).all(), "bytes outside the window were written"
        out.append(np.ascontiguousarray(full[3:3 + rows, :used]).view(dt))
        b.free()
    return out


@functools.lru_cache(maxsize=None)
def _panel(n, kind, p=P, seed=0):
    """(n, p) dosages.  full: every call present; miss: 10 % missing; mix: columns [256, 512) 10 % missing, the rest present.  Every
    panel then gets, in its last tile (columns 512 ..), an all-missing column, a monomorphic one and one that is not hard-call."""
    rng = np.random.default_rng(seed + 11 * n + len(kind))
    G = rng.binomial(2, rng.uniform(0.05, 0.6, p), (n, p)).astype(np.float64)
    hole = rng.random((n, p)) < 0.1
    if kind == "mix":
        hole[:, :256] = False
        hole[:, 512:] = False
    if kind != "full":
        G[hole] = np.nan
    G[:, p - 6] = np.nan
    G[:, p - 5] = 2.0
    G[n // 2, p - 4] = 0.5
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _labels(n, nb=NB, seed=0):
    """(study (n,) bool with excluded samples, labellings (nb, n) int8 <= study): random subsets of every size, row 0 empty, row 1 all
    of the study."""
    rng = np.random.default_rng(seed + 13 * n)
    study = rng.random(n) < 0.85
    study[0] = True
    lab = (rng.random((nb, n)) < rng.uniform(0.1, 0.9, (nb, 1))) & study[None, :]
    lab[0] = False
    if nb > 1:
        lab[1] = study
    lab = lab.astype(np.int8)
    for a in (study, lab):
        a.flags.writeable = False
    return study, lab


@functools.lru_cache(maxsize=None)
def _truth(n, kind, test):
    G = _panel(n, kind)
    study, lab = _labels(n)
    tot = T.totals(G, study)
    a, R = T.sums(G, lab)
    out = tot, T.replay(test, tot[:, 0], tot[:, 1], tot[:, 2], a, R), T.exact(test, tot[:, 0], tot[:, 1], tot[:, 2], a, R)
    for v in out:
        v.flags.writeable = False
    return out


def _rows(n, *parts):
    """int8 label rows at the device's pitch: zero past sample n."""
    ldk = -(-n // 128) * 128
    parts = [np.atleast_2d(np.asarray(q)) for q in parts]
    out = np.zeros((sum(q.shape[0] for q in parts), ldk), np.int8)
    out[:, :n] = np.concatenate(parts)
    return out


class Dev:
    """A panel encoded into an LD image, its totals, and label rows (row 0: the study flags) with their counts, all on the device."""

    def __init__(self, ctx, G, study, lab):
        from pygemma_amd import _lib
        self.ctx, self.L, self.P = ctx, _lib.load(), _lib.load_perm()
        L, Pm = self.L, self.P
        self.n, self.p = G.shape
        n, p = G.shape
        rows = _rows(n, study, lab)
        self.nrows = rows.shape[0]
        assert int(Pm.pg_perm_label_bytes(n, self.nrows)) >= rows.nbytes
        self.bufs = []
        dX = self.hold(ctx.to_device(np.ascontiguousarray(G.T)))
        self.image = self.hold(ctx.alloc(L.pg_ld_image_bytes(n, p)))
        _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, p, dX.ptr, 3, n, 1, self.image.ptr, p, 0), "pg_ld_encode_x_dev")
        self.lab = self.hold(ctx.alloc(Pm.pg_perm_label_bytes(n, self.nrows)).upload(rows))
        self.labc = self.hold(ctx.alloc(4 * self.nrows))
        _lib.check(Pm.pg_perm_label_counts_dev(ctx.handle, n, self.lab.ptr, self.nrows, self.labc.ptr), "pg_perm_label_counts_dev")
        self.tot = self.hold(ctx.alloc(16 * p))
        _lib.check(Pm.pg_perm_totals_dev(ctx.handle, n, self.image.ptr, p, 0, p, self.lab.ptr, self.tot.ptr), "pg_perm_totals_dev")
        ctx.sync()
        assert (self.labc.download((self.nrows,), np.int32) == rows.sum(axis=1)).all()

    def hold(self, b):
        self.bufs.append(b)
        return b

    def close(self):
        for b in self.bufs:
            b.free()

    def block(self, a0, na, b0, nb, test, dense=None, ldo=0, obs=None, n_ge=None, max_null=None):
        """labellings [b0, b0 + nb) counted from the first labelling (device row 1 + b0)"""
        from pygemma_amd import _lib
        _lib.check(self.P.pg_perm_block_dev(self.ctx.handle, self.n, self.image.ptr, self.p, a0, na, self.tot.ptr + 16 * a0, self.lab.ptr, self.labc.ptr,
                                            1 + b0, nb, test, dense, ldo, obs, n_ge, max_null), "pg_perm_block_dev")

    def dense(self, a0, na, b0, nb, test):
        ldo = nb + 3
        return _windows(self.ctx, [(na, 8 * nb, 8 * ldo, np.float64)], lambda d: self.block(a0, na, b0, nb, test, dense=d, ldo=ldo))[0]


@pytest.mark.parametrize("n", NS)
def test_totals_and_dense_blocks(ctx, planes_env, n):
    """pg_perm_totals_dev equals the boolean-mask truth inside a guarded window; the dense statistics of every window, both tests and
    both tile paths are bit-equal to the replay and within the gate of the exact values."""
    from pygemma_amd import _lib
    study, lab = _labels(n)
    for kind in KINDS:
        G = _panel(n, kind)
        dev = Dev(ctx, G, study, lab)
        tot = T.totals(G, study)
        for frm, count in ((0, P), (5, 1), (250, 263)):
            got = _windows(ctx, [(count, 16, 16, np.int32)], lambda t: _lib.check(
                dev.P.pg_perm_totals_dev(ctx.handle, n, dev.image.ptr, P, frm, count, dev.lab.ptr, t), "pg_perm_totals_dev"))[0]
            assert (got == tot[frm:frm + count]).all(), (n, kind, frm, np.flatnonzero((got != tot[frm:frm + count]).any(axis=1))[:5])
        if n > 2:
            assert tot[P - 6, 3] == 1 and tot[P - 5, 3] == 0 and tot[P - 4, 3] == 3 and (tot[:256, 3] == 0).all() == (kind != "miss")
        for test in (T.ALLELIC, T.TREND):
            _, rp, ex = _truth(n, kind, test)
            for a0, na, nb in WINDOWS:
                b0 = NB - nb if nb < 255 else 0
                want, exact = rp[a0:a0 + na, b0:b0 + nb], ex[a0:a0 + na, b0:b0 + nb]
                planes_env(False)
                got = dev.dense(a0, na, b0, nb, test)
                tag = (n, kind, test, a0, na, nb)
                assert T.same_bits(got, want).all(), (tag, np.argwhere(~T.same_bits(got, want))[:5])
                assert T.within(got, exact).all(), tag
                planes_env(True)
                assert T.same_bits(dev.dense(a0, na, b0, nb, test), got).all(), tag
            planes_env(False)
            if n > 100:
                assert not np.isnan(rp[:500]).all() and np.isnan(rp[P - 6:P - 3]).all()
        dev.close()


@functools.lru_cache(maxsize=None)
def _tie_case(n=257, p=300, nb=513):
    """A panel with missing calls in its second tile only, excluded samples, and labellings with planted exact ties: labelling 7 is the
    observed status, labelling 8 its complement within the study, labelling 9 a copy of labelling 3."""
    rng = np.random.default_rng(77)
    G = _panel(n, "mix", p=p, seed=5).copy()
    G[:, 256:][rng.random((n, p - 256)) < 0.1] = np.nan
    G[:, p - 6] = np.nan
    study, lab = _labels(n, nb=nb, seed=3)
    lab = lab.copy()
    observed = (study & (rng.random(n) < 0.45)).astype(np.int8)
    lab[7] = observed
    lab[8] = study & ~observed.astype(bool)
    lab[9] = lab[3]
    return G, study, observed, lab


@pytest.mark.parametrize("test", [T.ALLELIC, T.TREND])
def test_reduce_mode_equals_the_dense_output(ctx, planes_env, test):
    """(na, nb) = (300, 513): n_ge and max_null equal the values computed from the dense output of the same kernel — integers and bit
    patterns — ties count as >=, the sum over calls split at non-tile boundaries equals one call, on both tile paths."""
    from pygemma_amd import _lib
    G, study, observed, lab = _tie_case()
    n, p = G.shape
    nb = lab.shape[0]
    dev = Dev(ctx, G, study, np.concatenate([lab, observed[None, :]]))      # labelling nb: the observed status
    L = dev.L
    tot = T.totals(G, study)
    a, R = T.sums(G, lab)
    dense = dev.dense(0, p, 0, nb, test)
    assert T.same_bits(dense, T.replay(test, tot[:, 0], tot[:, 1], tot[:, 2], a, R)).all()
    obs = dev.dense(0, p, nb, 1, test)[:, 0]
    assert T.same_bits(obs, dense[:, 7]).all() and T.same_bits(obs, dense[:, 8]).all() and T.same_bits(dense[:, 3], dense[:, 9]).all()
    want_ge, want_max = T.reduce(dense, obs)
    defined = ~np.isnan(obs)
    assert defined.sum() > 250 and (want_ge[defined] >= 2).all() and (want_ge[~defined] == 0).all()
    dobs = dev.hold(ctx.to_device(obs))

    def run(splits_a, splits_b):
        def fn(g, m):
            for buf, nbytes in ((g, 4 * p), (m, 8 * nb)):
                _lib.check(L.pg_memset(ctx.handle, buf, 0, nbytes), "pg_memset")
            for a0, a1 in splits_a:
                for b0, b1 in splits_b:
                    dev.block(a0, a1 - a0, b0, b1 - b0, test, obs=dobs.ptr + 8 * a0, n_ge=g + 4 * a0, max_null=m + 8 * b0)
        ge, mx = _windows(ctx, [(1, 4 * p, 4 * p + 16, np.uint32), (1, 8 * nb, 8 * nb + 16, np.uint64)], fn)
        return ge[0], mx[0]

    for on in (False, True):
        planes_env(on)
        for splits_a, splits_b in (([(0, p)], [(0, nb)]), ([(0, 130), (130, p)], [(0, nb)]), ([(0, p)], [(0, 200), (200, nb)]),
                                   ([(0, 1), (1, 257), (257, p)], [(0, 255), (255, 256), (256, nb)])):
            ge, mx = run(splits_a, splits_b)
            assert (ge == want_ge).all(), (on, splits_a, splits_b)
            assert (mx == T.bits(want_max)).all(), (on, splits_a, splits_b)
    dev.close()


def test_refused_calls(ctx):
    from pygemma_amd import _lib
    G, study, observed, lab = _tie_case()
    n, p = G.shape
    dev = Dev(ctx, G[:, :40].copy(), study, lab[:5])
    P_, h = dev.P, ctx.handle
    out = ctx.alloc(8 * 40 * 5)
    ok = (h, n, dev.image.ptr, 40, 0, 40, dev.tot.ptr, dev.lab.ptr, dev.labc.ptr, 1, 5, 0, out.ptr, 5, None, None, None)

    def call(**kw):
        names = ("ctx", "n", "image", "pe", "a0", "na", "totals", "labels", "labc", "b0", "nb", "test", "dense", "ldo", "obs", "n_ge", "max_null")
        args = dict(zip(names, ok))
        args.update(kw)
        return P_.pg_perm_block_dev(*[args[k] for k in names])
    assert call() == 0
    assert call(na=0) == 0 and call(nb=0) == 0
    assert call(test=2) == ENOTSUP
    for kw in (dict(image=None), dict(totals=None), dict(labels=None), dict(labc=None), dict(n=0), dict(n=1 << 28), dict(a0=1), dict(na=-1), dict(nb=-1),
               dict(ldo=4), dict(n_ge=out.ptr), dict(image=dev.image.ptr + 8), dict(dense=out.ptr + 4), dict(totals=dev.tot.ptr + 4)):
        assert call(**kw) == EINVAL, kw
    assert b"pg_perm_block_dev" in dev.L.pg_last_error()
    assert P_.pg_perm_totals_dev(h, n, dev.image.ptr, 40, 0, 41, dev.lab.ptr, dev.tot.ptr) == EINVAL
    assert P_.pg_perm_totals_dev(h, n, dev.image.ptr, 40, 0, 0, dev.lab.ptr, dev.tot.ptr) == 0
    assert P_.pg_perm_label_counts_dev(h, n, None, 1, dev.labc.ptr) == EINVAL and P_.pg_perm_label_counts_dev(h, n, dev.lab.ptr, 0, dev.labc.ptr) == 0
    ctx.sync()
    out.free()
    dev.close()


# ---- lmm.case_control_perm ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lmm_case(missing):
    """n = 257, p = 300, nperm = 513: genotypes (with or without missing calls), a status with excluded samples, strata."""
    n, p = 257, 300
    rng = np.random.default_rng(21 + missing)
    G = rng.binomial(2, rng.uniform(0.05, 0.6, p), (n, p)).astype(np.float64)
    y = rng.choice([0.0, 1.0, 1.0, np.nan], n, p=[0.45, 0.25, 0.2, 0.1])
    G = np.minimum(G + ((y == 1)[:, None] & (rng.random((n, p)) < 0.4) & (np.arange(p) % 50 == 0)[None, :]), 2.0)      # some signal
    if missing:
        G[rng.random((n, p)) < 0.05] = np.nan
        G[:, 0] = np.nan
        G[n // 2, 2] = 0.5
    G[:, 1] = 2.0
    strata = rng.integers(0, 3, n).astype(np.float64)
    strata[rng.random(n) < 0.05] = np.nan
    for a in (G, y, strata):
        a.flags.writeable = False
    return G, y, strata


def _expect(G, y, strata, lab, test):
    from pygemma_amd import lmm
    n = G.shape[0]
    group = lmm._epi_group(y, n, False)
    strat, _ = lmm._cc_strata(strata, n)
    study = lmm._perm_study(group, strat)
    tot = T.totals(G, study)
    rows = np.concatenate([(study & (group == 1))[None, :].astype(np.int8), lab])
    a, R = T.sums(G, rows)
    st = T.replay(test, tot[:, 0], tot[:, 1], tot[:, 2], a, R)
    obs = st[:, 0]
    n_ge, mx = T.reduce(st[:, 1:], obs)
    B = lab.shape[0]
    emp1 = np.where(np.isnan(obs), np.nan, (n_ge + 1.0) / (B + 1.0))
    return obs, n_ge, mx, emp1, T.emp2(mx, obs), T.hard_calls(G)


def _check(res, want, nperm):
    obs, n_ge, mx, emp1, emp2, hard = want
    df = res.snps
    assert list(df.columns)[:6] == ["hard", "chi2", "p", "n_ge", "emp1", "emp2"] and res.nperm == nperm
    assert (df["hard"].to_numpy() == hard).all()
    assert T.same_bits(df["chi2"].to_numpy(), obs).all()
    assert (df["n_ge"].to_numpy() == n_ge).all()
    assert (T.bits(res.max_null) == T.bits(mx)).all()
    assert T.same_bits(df["emp1"].to_numpy(), emp1).all() and T.same_bits(df["emp2"].to_numpy(), emp2).all()
    assert (np.isnan(df["p"].to_numpy()) == np.isnan(obs)).all()


@pytest.mark.parametrize("test", ["allelic", "trend"])
def test_case_control_perm_against_the_truth_and_case_control(test):
    """chi2 bit-equal to lmm.case_control's column; n_ge, max_null, emp1, emp2 equal to the truth for explicit labels (with planted
    ties) and for a seed, with and without strata; independent of snp_batch."""
    from pygemma_amd import lmm
    G, y, strata = _lmm_case(True)
    n, p = G.shape
    tcode = T.ALLELIC if test == "allelic" else T.TREND
    group = lmm._epi_group(y, n, False)
    cc = lmm.case_control(G, y, fisher=False)
    # explicit labels: the generator's, then the observed status, its complement and a copy planted
    lab = lmm._perm_labels(group, None, 1, 513, 4).copy()
    lab[10] = group == 1
    lab[11] = group == 0
    lab[12] = lab[5]
    st = {}
    res = lmm.case_control_perm(G, y, test=test, labels=lab, snps=[f"rs{j}" for j in range(p)], stats=st)
    _check(res, _expect(G, y, None, lab, tcode), 513)
    assert T.same_bits(res.snps["chi2"].to_numpy(), cc["chi2_" + test].to_numpy()).all()
    assert list(res.snps["SNPs"][:2]) == ["rs0", "rs1"] and st["batches"] == 1 and st["bytes_in"] == G.nbytes and st["seconds"] > 0
    assert (res.snps["n_ge"].to_numpy()[~np.isnan(res.snps["chi2"].to_numpy())] >= 2).all()
    thr = res.threshold(0.05)
    assert thr == np.sort(res.max_null)[math.ceil(0.95 * 514) - 1]
    assert ((res.snps["emp2"] <= 0.05) == (res.snps["chi2"] > thr)).all()
    # a seed: the labels are _perm_labels's; snp_batch 130 against 300
    want = _expect(G, y, None, lmm._perm_labels(group, None, 1, 513, 9), tcode)
    for sb in (130, 300):
        _check(lmm.case_control_perm(G, y, test=test, nperm=513, seed=9, snp_batch=sb), want, 513)
    # strata: the shuffles stay within the strata, a sample without a stratum leaves the study
    strat, S = lmm._cc_strata(strata, n)
    slab = lmm._perm_labels(group, strat, S, 64, 2)
    res = lmm.case_control_perm(G, y, test=test, nperm=64, seed=2, strata=strata)
    _check(res, _expect(G, y, strata, slab, tcode), 64)
    assert T.same_bits(res.snps["chi2"].to_numpy(), lmm.case_control(G, y, strata=strata, fisher=False)["chi2_" + test].to_numpy()).all()


@pytest.mark.parametrize("test", ["allelic", "trend"])
def test_case_control_perm_is_independent_of_the_source_kind(test):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    G, y, _ = _lmm_case(False)
    n, p = G.shape
    group = lmm._epi_group(y, n, False)
    tcode = T.ALLELIC if test == "allelic" else T.TREND
    want = _expect(G, y, None, lmm._perm_labels(group, None, 1, 513, 1), tcode)
    for X in (PackedBed(CT.pack(G), n), G.astype(np.int8), np.asfortranarray(G.astype(np.float32))):
        _check(lmm.case_control_perm(X, y, test=test, nperm=513, seed=1, snp_batch=130), want, 513)
    # with missing calls: records against a float32 Fortran-order array
    G, y, _ = _lmm_case(True)
    G = G.copy()
    G[G == 0.5] = np.nan                                                   # a .bed record holds hard calls only
    want = _expect(G, y, None, lmm._perm_labels(lmm._epi_group(y, n, False), None, 1, 513, 1), tcode)
    for X in (PackedBed(CT.pack(G), n), np.asfortranarray(G.astype(np.float32))):
        _check(lmm.case_control_perm(X, y, test=test, nperm=513, seed=1), want, 513)
