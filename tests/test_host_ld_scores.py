"""CPU checks of the LD score feature: the public surface, every refusal of lmm.ld_scores before the device, the truth helper's fixed
point against a float64 sum, the C ABI's argument checks, and lmm.ldsc against the exact line and against a plain independent
implementation (np.linalg.lstsq on sqrt(w)-scaled rows, a Python loop that deletes each block and refits)."""
import inspect

import numpy as np
import pytest

import _ld_score_truth as ST
import _ld_truth as T


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


X0 = np.random.default_rng(0).integers(0, 3, (20, 6)).astype(np.float32)


def test_public_names_signatures_and_defaults():
    import pygemma.lmm as ref_style
    from pygemma_amd import lmm
    for name in ("ld_scores", "ldsc", "LdscResult"):
        assert name in lmm.__all__ and getattr(ref_style, name) is getattr(lmm, name)
    assert str(inspect.signature(lmm.ld_scores)) == ("(X, window, *, pos=None, chrom=None, adjust=True, snps=None, snp_batch=None, device=0, "
                                                     "verbose=0, stats=None)")
    assert str(inspect.signature(lmm.ldsc)) == "(chi2, l2, n, *, m=None, blocks=200, intercept=None)"
    assert lmm.LdscResult._fields == ("h2", "h2_se", "intercept", "intercept_se", "mean_chi2", "lambda_gc", "ratio", "m", "n_used")


BAD_X = {"X 1-D": X0[:, 0], "X 3-D": X0[:, :, None], "X int32": X0.astype(np.int32), "X float16": X0.astype(np.float16), "no SNPs": X0[:, :0],
         "no samples": X0[:0]}


@pytest.mark.parametrize("bad", sorted(BAD_X))
def test_bad_genotypes_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.ld_scores(BAD_X[bad], 3)


BAD_KW = {
    "window 0": dict(window=0), "window float": dict(window=3.0), "window bool": dict(window=True), "window negative": dict(window=-2),
    "window below one with pos": dict(window=0.5, pos=np.arange(6)), "window string with pos": dict(window="1", pos=np.arange(6)),
    "snp_batch 0": dict(window=3, snp_batch=0), "snp_batch float": dict(window=3, snp_batch=64.0), "snp_batch bool": dict(window=3, snp_batch=True),
    "snps short": dict(window=3, snps=list("abcde")), "chrom short": dict(window=3, chrom=[1] * 5), "chrom 2-D": dict(window=3, chrom=np.ones((6, 1))),
    "pos long": dict(window=3, pos=np.arange(7)), "pos decreasing": dict(window=3, pos=[0, 10, 20, 15, 30, 40]),
    "pos strings": dict(window=3, pos=list("abcdef")), "pos nan": dict(window=3, pos=[0, 1, 2, np.nan, 4, 5]),
    "pos beyond int64": dict(window=3, pos=np.array([0, 1, 2, 3, 4, 2 ** 63], np.uint64)),
    "pos restarts inside a chromosome": dict(window=3, chrom=[1, 1, 1, 1, 2, 2], pos=[5, 6, 7, 1, 2, 3]),
}


@pytest.mark.parametrize("bad", sorted(BAD_KW))
def test_bad_arguments_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    _no_device(monkeypatch)
    kw = dict(BAD_KW[bad])
    window = kw.pop("window")
    for X in (X0, PackedBed(T.pack(X0.astype(np.float64)), 20)):
        with pytest.raises(ValueError):
            lmm.ld_scores(X, window, **kw)


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    _lib.load()
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(_lib.PgError):
        lmm.ld_scores(X0, 3)
    with pytest.raises(_lib.PgError):
        lmm.ld_scores(X0, 2.5, pos=np.arange(6.0), chrom=[1, 1, 1, 2, 2, 2])


def test_score_entry_point_refuses_a_null_context_by_name():
    from pygemma_amd import _lib
    L = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert L.pg_ld_score_dev(None, 8, p, 4, 0, 2, 4, 3, None, 1, p, p, p) == -22          # PG_EINVAL
    assert "pg_ld_score_dev" in L.pg_last_error().decode()
    assert not buf.any()


@pytest.mark.parametrize("n,p,w", [(63, 86, 40), (129, 515, 64)])
@pytest.mark.parametrize("adjust", [False, True])
def test_truth_fixed_point_is_the_float_sum_within_its_quantisation(n, p, w, adjust):
    """Every pair is rounded to 2^-32 once (half a unit at most) and a SNP has at most 2 w pairs: |fixed - float64| <= w 2^-32, the
    float64 sum's own rounding (2 w terms of at most 1: below 2 w^2 2^-53) far inside that."""
    S = T.sums(T.ld_panel(n, p, seed=n + p))
    visit = ST.forward_mask(p, 0, p, p, w)
    tot, cnt, undefined = ST.credit(S, visit, adjust)
    ref = ST.credit_float(S, visit, adjust)
    assert undefined < 0.2 and cnt.max() > w
    assert np.abs(tot / ST.ONE - ref).max() <= w * 2.0 ** -32
    if not adjust:
        assert tot.min() >= 0 and (tot <= cnt * 2 ** 32).all()


def test_truth_specials():
    n, p = 65, 40
    G = T.ld_panel(n, p, seed=9)
    S = T.sums(G)
    ok, q = ST.pair_q(S, False)
    assert q[0, p - 5] == 2 ** 32 and q[0, p - 6] == 2 ** 32          # the copy and the flip of column 0
    for col in (p - 2, p - 3, p - 8):                                  # monomorphic, all missing, dosage
        assert not ok[col].any() and not ok[:, col].any() and ST.nobs(G)[col] == 0
    assert (ST.nobs(G)[:p - 8] > 0).all()


# ---- ldsc -----------------------------------------------------------------------------------------------------------------------------------
def _synthetic(seed, p=3000, noise=True):
    rng = np.random.default_rng(seed)
    l2 = 1.0 + rng.gamma(2.0, 20.0, p)
    l2[rng.random(p) < 0.02] = 0.6                     # below one: the weights take max(l2, 1)
    n = rng.integers(40000, 60000, p).astype(np.float64)
    h2, a = 0.37, 1.08
    mean = a + n * h2 * l2 / p
    chi2 = mean * rng.chisquare(1, p) if noise else mean
    return chi2, l2, n, h2, a


def _reference_ldsc(chi2, l2, n, M, blocks, intercept):
    """The issue's estimator in the plainest form: lstsq on sqrt(w)-scaled rows, refit without each block in a Python loop."""
    x = n * l2 / M
    lw = np.maximum(l2, 1.0)

    def fit(rows, wt):
        sw = np.sqrt(wt[rows])
        if intercept is None:
            A = np.stack([x[rows], np.ones(len(rows))], axis=1) * sw[:, None]
            return np.linalg.lstsq(A, chi2[rows] * sw, rcond=None)[0]
        A = (x[rows] * sw)[:, None]
        return np.array([np.linalg.lstsq(A, (chi2[rows] - intercept) * sw, rcond=None)[0][0], intercept])

    every = np.arange(len(chi2))
    a = 1.0 if intercept is None else intercept
    h2 = min(max(M * (chi2.mean() - a) / (n * l2).mean(), 0.0), 1.0)
    for _ in range(2):
        wt = 1.0 / (lw * 2.0 * (a + n * h2 * lw / M) ** 2)
        h2, a = fit(every, wt)
    parts = np.array_split(every, blocks)
    dele = np.array([fit(np.setdiff1d(every, part), wt) for part in parts])
    pseudo = blocks * np.array([h2, a]) - (blocks - 1) * dele
    se = np.sqrt(pseudo.var(axis=0, ddof=1) / blocks)
    return h2, a, se[0], se[1]


def _close(got, want, rel=1e-9):
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("intercept", [None, 1.08])
def test_ldsc_returns_the_exact_line(intercept):
    from pygemma_amd import lmm
    chi2, l2, n, h2, a = _synthetic(1, noise=False)
    res = lmm.ldsc(chi2, l2, n, blocks=50, intercept=intercept)
    assert _close(res.h2, h2) and _close(res.intercept, a)
    assert res.h2_se <= 1e-9 * h2 and res.m == len(chi2) and res.n_used == len(chi2)
    assert np.isnan(res.intercept_se) if intercept is not None else res.intercept_se <= 1e-9
    res = lmm.ldsc(chi2, l2, n, m=2 * len(chi2), blocks=2)        # M scales the slope
    assert _close(res.h2, 2 * h2) and _close(res.intercept, a) and res.m == 2 * len(chi2)


@pytest.mark.parametrize("intercept,blocks,scalar_n", [(None, 200, False), (None, 7, True), (1.0, 200, False), (1.2, 13, False)])
def test_ldsc_is_the_plain_implementation(intercept, blocks, scalar_n):
    from pygemma_amd import lmm
    chi2, l2, n, _h2, _a = _synthetic(2)
    if scalar_n:
        n = np.full(len(chi2), 50000.0)
    res = lmm.ldsc(chi2, l2, 50000 if scalar_n else n, blocks=blocks, intercept=intercept)
    h2, a, h2_se, a_se = _reference_ldsc(chi2, l2, n, float(len(chi2)), blocks, intercept)
    assert _close(res.h2, h2) and _close(res.intercept, a) and _close(res.h2_se, h2_se)
    if intercept is None:
        assert _close(res.intercept_se, a_se) and res.intercept_se > 0
        if not scalar_n:          # the model the data were drawn from: the truth lies within a few standard errors
            assert abs(res.h2 - 0.37) < 4 * res.h2_se and abs(res.intercept - 1.08) < 4 * res.intercept_se
    else:
        assert res.intercept == intercept and np.isnan(res.intercept_se)
    assert res.h2_se > 0
    assert res.mean_chi2 == chi2.mean() and res.lambda_gc == np.median(chi2) / 0.454936423119572
    assert _close(res.ratio, (res.intercept - 1) / (chi2.mean() - 1))


def test_ldsc_drops_rows_that_are_not_finite():
    from pygemma_amd import lmm
    chi2, l2, n, _h2, _a = _synthetic(3, p=800)
    clean = lmm.ldsc(chi2, l2, n, blocks=20, m=800)
    pad = lambda v, bad: np.concatenate([v[:100], [bad, 1.0, 1.0], v[100:], [1.0]])
    c2, e2, n2 = pad(chi2, np.nan), pad(l2, 1.0), pad(n, 5e4)
    e2[101], n2[102], c2[-1] = np.nan, np.inf, np.inf
    res = lmm.ldsc(c2, e2, n2, blocks=20, m=800)
    assert res.n_used == 800 and res == clean
    assert lmm.ldsc(c2, e2, n2, blocks=20).m == 800            # M defaults to the SNPs used
    frame = lmm.ldsc(list(chi2), l2.astype(np.float32).astype(np.float64), n, blocks=20)     # any 1-D sequence will do
    assert frame.n_used == 800


@pytest.mark.parametrize("bad", ["blocks 1", "blocks beyond the SNPs", "blocks float", "blocks bool", "l2 short", "n short", "chi2 2-D", "m zero"])
def test_ldsc_refusals(bad):
    from pygemma_amd import lmm
    chi2, l2, n, _h2, _a = _synthetic(4, p=50)
    chi2[3] = np.nan                                            # 49 usable SNPs
    assert lmm.ldsc(chi2, l2, n, blocks=49).n_used == 49        # one SNP a block is the most
    kw = dict(blocks=10)
    if bad == "blocks 1":
        kw["blocks"] = 1
    elif bad == "blocks beyond the SNPs":
        kw["blocks"] = 50
    elif bad == "blocks float":
        kw["blocks"] = 10.0
    elif bad == "blocks bool":
        kw["blocks"] = True
    elif bad == "l2 short":
        l2 = l2[:-1]
    elif bad == "n short":
        n = n[:-1]
    elif bad == "chi2 2-D":
        chi2, l2 = chi2[:, None], l2[:, None]
    elif bad == "m zero":
        kw["m"] = 0
    with pytest.raises(ValueError):
        lmm.ldsc(chi2, l2, n, **kw)


# ---- the forward reach ----------------------------------------------------------------------------------------------------------------------
def _two_pointers(coord, run, window):
    """The plain loop, in Python integers: no difference can wrap."""
    coord, m = [int(c) for c in coord], len(coord)
    reach, hi = [0] * m, 0
    for c in range(m):
        hi = max(hi, c)
        while hi + 1 < m and run[hi + 1] == run[c] and coord[hi + 1] - coord[c] <= window:
            hi += 1
        reach[c] = hi - c
    return reach


def test_reach_of_negative_coordinates_is_the_loops():
    from pygemma_amd import lmm
    assert lmm._clump_reach(np.array([-5, -3, 100]), np.zeros(3, np.int64), 3).tolist() == [1, 0, 0]


@pytest.mark.parametrize("where", ["negative", "zero-crossing", "positive", "near int64 max", "near int64 min"])
@pytest.mark.parametrize("window", [1, 7, 50, 2.5, 1e30])
def test_integer_reach_is_the_two_pointer_loop(where, window):
    from pygemma_amd import lmm
    rng = np.random.default_rng(len(where) + int(min(window, 99)))
    top, low = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    for trial in range(40):
        m = int(rng.integers(1, 80))
        run = np.cumsum(rng.random(m) < 0.08)                       # several chromosome runs
        step = rng.integers(0, 9, m)
        step[rng.random(m) < 0.3] = 0                               # ties
        pos = np.cumsum(step)
        for r in np.unique(run):
            pos[run == r] -= pos[run == r][0]                       # positions restart on every run
        span = int(pos.max())
        offset = {"negative": -1000 - span, "zero-crossing": -(span // 2), "positive": 3, "near int64 max": top - span - int(rng.integers(0, 3)),
                  "near int64 min": low + int(rng.integers(0, 3))}[where]
        pos = pos + offset
        want = _two_pointers(pos, run, window)
        assert lmm._clump_reach(pos, run, window).tolist() == want, (where, window, pos, run)
        if where == "positive" and pos.max() < 256:
            assert lmm._clump_reach(pos.astype(np.uint8), run, window).tolist() == want
