"""CPU checks of the polygenic scores' boundary (lmm.prs, lmm.prs_weights, pg_prs_*): names and signatures, the entries' refusals without
a device, the inputs refused before any device work, the all-zero-weights shortcut, prs_weights on a hand-made frame and the truth helper
of _prs_truth.py against exact rational arithmetic."""
import ctypes as C
import inspect
import os
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import _prs_truth as T
import _snp_stats_truth as ST

SYMS = ("pg_prs_work_bytes", "pg_prs_bed_acc_dev", "pg_prs_x_acc_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_public_names_and_signatures():
    from pygemma import lmm
    import pygemma_amd.lmm as impl
    sig = inspect.signature(lmm.prs)
    assert list(sig.parameters) == ["X", "weights", "missing", "counts", "samples", "device", "snp_batch", "verbose", "stats"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == {
        "missing": "mean", "counts": False, "samples": None, "device": 0, "snp_batch": None, "verbose": 0, "stats": None}
    assert [v.kind for v in sig.parameters.values()] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 2 + [inspect.Parameter.KEYWORD_ONLY] * 7
    sig = inspect.signature(lmm.prs_weights)
    assert list(sig.parameters) == ["df", "loci", "thresholds", "col", "beta"]
    assert [v.default for v in sig.parameters.values()][1:] == [None, (5e-8, 1e-5, 1e-3, 1e-2, 0.05, 1.0), "p_wald", "beta"]
    assert "prs" in impl.__all__ and "prs_weights" in impl.__all__


def test_entries_exported_and_refuse_without_a_device():
    _lib, L = _lib_loaded()
    for sym in SYMS:
        assert hasattr(L, sym) and sym in _lib.SYMBOLS
    wb = L.pg_prs_work_bytes
    assert wb(0, 4, 1) == 0 and wb(16, -1, 1) == 0 and wb(16, 4, 0) == 0 and wb(16, 4, 65) == 0 and wb(16, (1 << 25) + 1, 1) == 0
    assert wb(1 << 30, 4, 1) == 0 and wb((1 << 30) - 1, 1 << 25, 1) == 0           # 2^22 sample groups x 2^17 chunks: no one launch
    assert wb(1, 0, 1) > 0 and wb(16, 1 << 25, 1) > 0 and wb(16, 4, 64) > 0 and wb((1 << 30) - 1, 4, 1) > 0
    # the chunk partials of the split-K schedule: 12 bytes per (chunk, column, sample)
    assert wb(1030, 600, 5) >= 3 * 5 * 1030 * 12
    buf = (C.c_double * 64)()
    vp = C.cast(buf, C.c_void_p)
    assert L.pg_prs_bed_acc_dev(None, 16, 4, vp, 4, 0, 1, vp, 4, 1, vp, vp, vp, 16) == -22 and b"pg_prs_bed_acc_dev" in L.pg_last_error()
    assert L.pg_prs_x_acc_dev(None, 16, 4, vp, 2, 16, 1, 1, vp, 4, 1, vp, vp, vp, 16) == -22 and b"pg_prs_x_acc_dev" in L.pg_last_error()


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


BAD = ["weight NaN", "weight Inf", "X 1-D", "X 3-D", "X int32", "X float16", "no SNPs", "no samples", "weights short", "weights long",
       "weights 3-D", "no columns", "samples short", "samples long", "snp_batch 0", "snp_batch float", "snp_batch bool", "snp_batch negative",
       "missing other", "missing None"]


@pytest.mark.parametrize("bad", BAD)
def test_bad_inputs_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, (20, 5)).astype(np.float32)
    w = rng.standard_normal((5, 2))
    kw = {}
    if bad == "weight NaN":
        w[3, 1] = np.nan
    elif bad == "weight Inf":
        w[0, 0] = -np.inf
    elif bad == "X 1-D":
        X = X[:, 0]
    elif bad == "X 3-D":
        X = X[:, :, None]
    elif bad == "X int32":
        X = X.astype(np.int32)
    elif bad == "X float16":
        X = X.astype(np.float16)
    elif bad == "no SNPs":
        X, w = X[:, :0], w[:0]
    elif bad == "no samples":
        X = X[:0]
    elif bad == "weights short":
        w = w[:4]
    elif bad == "weights long":
        w = np.concatenate([w, w])
    elif bad == "weights 3-D":
        w = w[:, :, None]
    elif bad == "no columns":
        w = w[:, :0]
    elif bad == "samples short":
        kw["samples"] = list(range(19))
    elif bad == "samples long":
        kw["samples"] = list(range(21))
    elif bad.startswith("missing"):
        kw["missing"] = {"missing other": "median", "missing None": None}[bad]
    else:
        kw["snp_batch"] = {"snp_batch 0": 0, "snp_batch float": 256.0, "snp_batch bool": True, "snp_batch negative": -256}[bad]
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.prs(X, w, **kw)


def test_all_zero_weights_touch_no_device(monkeypatch):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    _no_device(monkeypatch)
    G = np.random.default_rng(1).integers(0, 3, (20, 5)).astype(np.float64)
    names = [f"id{i}" for i in range(20)]
    for X in (G.astype(np.float32), np.asfortranarray(G.astype(np.int8)), PackedBed(ST.pack(G), 20)):
        st = {}
        S = lmm.prs(X, np.zeros(5), stats=st)
        assert S.shape == (20, 1) and list(S.columns) == [0] and S[0].dtype == np.float64 and (S.to_numpy() == 0).all()
        assert st["batches"] == 0 and st["bytes_in"] == 0 and st["snps_used"] == 0 and st["seconds"] >= 0
        w = pd.DataFrame(np.zeros((5, 3)), columns=["a", "b", "c"])
        S, Cn = lmm.prs(X, w, counts=True, samples=names, missing="skip")
        for f, dt in ((S, np.float64), (Cn, np.int64)):
            assert f.shape == (20, 3) and list(f.columns) == ["a", "b", "c"] and list(f.index) == names
            assert all(f[c].dtype == dt for c in f.columns) and (f.to_numpy() == 0).all()
        assert list(lmm.prs(X, pd.Series(np.zeros(5))).columns) == [0]


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    from pygemma_amd.bed import PackedBed
    _lib_loaded()
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    G = np.random.default_rng(0).integers(0, 3, (20, 5)).astype(np.float64)
    for X in (G.astype(np.float32), G.astype(np.int8), PackedBed(ST.pack(G), 20)):
        with pytest.raises(_lib.PgError):
            lmm.prs(X, np.ones(5))


def test_prs_weights_on_a_hand_made_frame():
    from pygemma_amd import lmm
    nan = np.nan
    df = pd.DataFrame({"beta":   [0.5, -0.25, 1.5, nan, 2.0, -3.0, 0.125, 4.0],
                       "p_wald": [1e-9, 1e-5, 1e-4, 1e-9, nan, 0.05, 1.0, 5e-8]})
    w = lmm.prs_weights(df)
    assert w.shape == (8, 6) and list(w.columns) == [5e-8, 1e-5, 1e-3, 1e-2, 0.05, 1.0] and all(w[c].dtype == np.float64 for c in w.columns)
    # p == threshold counts; a NaN p or a NaN beta never does
    assert w[5e-8].tolist() == [0.5, 0, 0, 0, 0, 0, 0, 4.0]
    assert w[1e-5].tolist() == [0.5, -0.25, 0, 0, 0, 0, 0, 4.0]
    assert w[1e-3].tolist() == w[1e-2].tolist() == [0.5, -0.25, 1.5, 0, 0, 0, 0, 4.0]
    assert w[0.05].tolist() == [0.5, -0.25, 1.5, 0, 0, -3.0, 0, 4.0]
    assert w[1.0].tolist() == [0.5, -0.25, 1.5, 0, 0, -3.0, 0.125, 4.0]
    assert not np.isnan(w.to_numpy()).any()
    # with the loci of a clump frame only the index SNPs keep their weight
    loci = pd.DataFrame({"index": np.array([7, 1, 3, 5], np.int64), "p": [5e-8, 1e-5, 1e-9, 0.05]})
    wl = lmm.prs_weights(df, loci, thresholds=[1e-5, 1.0])
    assert list(wl.columns) == [1e-5, 1.0]
    assert wl[1e-5].tolist() == [0, -0.25, 0, 0, 0, 0, 0, 4.0] and wl[1.0].tolist() == [0, -0.25, 0, 0, 0, -3.0, 0, 4.0]
    assert (lmm.prs_weights(df, loci.iloc[:0]).to_numpy() == 0).all()
    # other columns
    alt = df.rename(columns={"beta": "b", "p_wald": "p_score"})
    assert (lmm.prs_weights(alt, col="p_score", beta="b").to_numpy() == w.to_numpy()).all()
    for kw in (dict(col="p_lrt"), dict(beta="b"), dict(thresholds=(0.1, 1.5)), dict(thresholds=(-0.1,)), dict(thresholds=(nan,)),
               dict(loci=pd.DataFrame({"index": [8]})), dict(loci=pd.DataFrame({"index": [-1]})), dict(loci=pd.DataFrame({"idx": [1]}))):
        with pytest.raises(ValueError):
            lmm.prs_weights(df, **kw)


def test_truth_helper_against_exact_rationals():
    """7 samples x 9 SNPs x 2 columns of float32 dosages with missing calls, an all-missing SNP and two hard-call SNPs, against Fractions."""
    rng = np.random.default_rng(4)
    n, p, t = 7, 9, 2
    X = (rng.integers(0, 3, (n, p)) + rng.standard_normal((n, p)) * 0.1).astype(np.float32)
    X[:, 2] = rng.integers(0, 3, n)
    X[:, 5] = [0, 1, 2, 2, 1, 0, 1]
    X[rng.random((n, p)) < 0.2] = np.nan
    X[:, 4] = np.nan
    X[3, 5] = np.nan
    X[1, 0] = np.inf
    W = rng.standard_normal((p, t)) * 10.0 ** rng.uniform(-3, 3, (p, t))
    W[6] = 0.0
    W[1, 0] = 0.0
    V, miss = T.decode(X)
    assert (miss == ~np.isfinite(X)).all() and (V[~miss] == X[~miss]).all() and (V[miss] == 0).all()
    mu, hard = T.means(V, miss)
    assert np.isnan(mu[4]) and hard[2] and hard[5] and not hard[4] and not hard[0]
    for g in (2, 5):                                                  # a hard-call SNP's mean is one exact division
        assert (~miss[:, g]).sum() > 0 and mu[g] == int(V[:, g].sum()) / int((~miss[:, g]).sum())
    for impute in (0, 1):
        tr = T.scores(X, W, impute)
        assert tr["score"].shape == (t, n) and tr["called"].shape == (t, n) and tr["called"].dtype == np.int64
        exact = np.zeros((t, n))
        cnt = np.zeros((t, n), np.int64)
        for i in range(n):
            for k in range(t):
                acc = Fraction(0)
                for g in range(p):
                    if not miss[i, g]:
                        acc += Fraction(float(X[i, g])) * Fraction(W[g, k])
                        cnt[k, i] += W[g, k] != 0
                    elif impute and not np.isnan(mu[g]):
                        acc += Fraction(mu[g]) * Fraction(W[g, k])
                exact[k, i] = float(acc)
        assert (tr["called"] == cnt).all()
        # the wide product: p roundings at 2^-64 and a second rounding to fp64
        assert (np.abs(tr["score"] - exact) <= 2.0 ** -52 * np.abs(exact) + p * 2.0 ** -63 * tr["mag"]).all()
        # the fsum leg rounds once: the exact value's own bits
        assert (T.product(tr["x"], W, wide=False).T == exact).all()
        b = T.bound(tr, n, p)
        assert (b >= (p + 8) * 2.0 ** -53 * tr["mag"]).all() and ((b > (p + 8) * 2.0 ** -53 * tr["mag"]) == (tr["soft"] > 0)).all()
        assert (tr["soft"] > 0).any() == bool(impute)
    # packed records decode like their float image, under both allele conventions
    from pygemma_amd.bed import PackedBed
    G = rng.integers(0, 3, (n, p)).astype(np.float64)
    G[rng.random((n, p)) < 0.2] = np.nan
    for a1 in (False, True):
        V, miss = T.decode(PackedBed(ST.pack(G), n, count_A1=a1))
        assert (miss == np.isnan(G)).all() and (V[~miss] == (2 - G if a1 else G)[~miss]).all()
    for dt in (np.int8, np.uint8):
        A = rng.integers(0, 120, (n, p)).astype(dt)
        V, miss = T.decode(A)
        assert not miss.any() and (V == A).all()
