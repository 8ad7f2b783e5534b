"""CPU checks of the principal components' boundary (lmm.pca, lmm.pca_project, pg_pca_*): the NumPy model of _pca_truth.py against an
exact eigendecomposition, `explained` against the trace, names and signatures, the entries' refusals without a device and the inputs
refused before any device work."""
import ctypes as C
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest

import _pca_truth as T
import _snp_stats_truth as ST

SYMS = ("pg_pca_work_bytes", "pg_pca_stat_bed_dev", "pg_pca_stat_x_dev", "pg_pca_proj_bed_dev", "pg_pca_proj_x_dev", "pg_pca_back_bed_dev",
        "pg_pca_back_x_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


# panels whose relative gap (lambda_2 - lambda_3) / lambda_1 is 0.83 - 0.86: fourteen passes converge to rounding
@pytest.mark.parametrize("n,p", [(300, 2000), (1030, 1500), (257, 600)])
def test_model_against_exact_eigendecomposition(n, p):
    G = T.panel(n, p, seed=n + p)
    res = T.pca(G.astype(np.float32), k=2, oversample=6, tol=0.0, iters=14)
    assert res.passes == 14 and not res.converged
    w, U = np.linalg.eigh(res.Z @ res.Z.T / p)
    w, U = w[::-1], T.fix_signs(U[:, ::-1][:, :2])
    gap = (w[1] - w[2]) / w[0]
    e_val, e_vec = np.max(np.abs(res.eigenvalues - w[:2])) / w[0], np.max(np.abs(res.pcs - U))
    print(f"n={n} p={p}: gap {gap:.3f}, eigenvalue error {e_val:.2e} of lambda_1, vector error {e_vec:.2e}")
    assert gap > 0.6
    assert e_val <= 1e-12 and e_vec <= 1e-10
    # the loadings reproduce a converged component, and projecting the training panel is that product
    assert np.max(np.abs(res.Z @ res.loadings - res.pcs)) <= 1e-10
    assert (T.project(G.astype(np.float32), res) == res.Z @ res.loadings).all()


def test_value_rule_and_stat():
    G = T.panel(37, 50, seed=1)
    G[:, 0] = np.nan                                  # all missing
    G[:, 1] = 2.0                                     # constant
    X = G.astype(np.float32)
    X[:, 2] = (G[:, 2] + 0.25).astype(np.float32)     # not hard-call
    X[3, 2] = np.inf
    st = T.stat(X)
    assert st.shape == (50, 2) and (st[0] == 0).all() and st[1, 0] == 2.0 and st[1, 1] == 0.0 and st[2, 1] > 0
    Z = T.z(X, st)
    assert (Z[:, :2] == 0).all() and Z[3, 2] == 0 and (Z[np.isnan(G)] == 0).all()
    for g in range(2, 50):
        obs = np.isfinite(X[:, g])
        x = X[obs, g].astype(np.float64)
        n_obs = int(obs.sum())
        # population sd over all n samples after mean imputation
        sd = np.sqrt(((x - x.mean()) ** 2).sum() / 37)
        assert abs(st[g, 0] - x.mean()) <= 1e-14
        if sd == 0:                                                    # constant among its called samples: contributes zeros
            assert st[g, 1] == 0 and (Z[:, g] == 0).all()
            continue
        assert abs(st[g, 1] * sd - 1) <= 1e-13
        assert (Z[obs, g] == (x - st[g, 0]) * st[g, 1]).all()
        assert abs((Z[:, g] ** 2).sum() - 37) <= 1e-11                 # every usable SNP has sum_i z^2 = n
        assert n_obs > 0
    # packed records decode like their float image
    from pygemma_amd.bed import PackedBed
    H = T.panel(37, 20, seed=2)
    assert (T.stat(PackedBed(ST.pack(H), 37)) == T.stat(H.astype(np.float32))).all()


def test_explained_sums_to_the_trace():
    n, p = 40, 300
    G = T.panel(n, p, seed=5)
    G[:, 7] = 1.0                                     # unusable SNPs still count in p
    G[:, 9] = np.nan
    res = T.pca(G.astype(np.float32), k=n, oversample=0, iters=3, tol=0.0, loadings=False)
    p_used = int((res.stat[:, 1] > 0).sum())
    assert p - 10 <= p_used <= p - 2                  # a rare allele may leave another SNP constant among 40 samples
    trace = np.trace(res.Z @ res.Z.T) / p
    assert abs(trace - n * p_used / p) <= 1e-12 * trace
    # the whole space: the Ritz values are all the eigenvalues, and explained sums to one
    assert abs(res.explained.sum() - 1) <= 1e-12
    assert np.allclose(res.explained * n * p_used / p, res.eigenvalues, rtol=1e-15, atol=0)


def test_public_names_and_signatures():
    from pygemma import lmm
    import pygemma_amd.lmm as impl
    sig = inspect.signature(lmm.pca)
    assert list(sig.parameters) == ["X", "k", "oversample", "iters", "tol", "seed", "loadings", "samples", "snps", "device", "snp_batch",
                                    "verbose", "stats"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == {
        "k": 10, "oversample": 10, "iters": 12, "tol": 1e-10, "seed": 0, "loadings": True, "samples": None, "snps": None, "device": 0,
        "snp_batch": None, "verbose": 0, "stats": None}
    assert [v.kind for v in sig.parameters.values()] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 2 + [inspect.Parameter.KEYWORD_ONLY] * 11
    sig = inspect.signature(lmm.pca_project)
    assert list(sig.parameters) == ["X_new", "res", "samples", "device", "snp_batch", "verbose", "stats"]
    assert [v.kind for v in sig.parameters.values()] == [inspect.Parameter.POSITIONAL_OR_KEYWORD] * 2 + [inspect.Parameter.KEYWORD_ONLY] * 5
    assert "pca" in impl.__all__ and "pca_project" in impl.__all__
    assert impl.PcaResult._fields == ("pcs", "eigenvalues", "explained", "loadings", "stat")


def test_header_declares_and_load_binds_the_entries():
    _lib, L = _lib_loaded()
    with open(_lib.HEADER) as f:
        text = f.read()
    decl = {name: args for name, _, args in _lib.parse_header(text)}
    for sym in SYMS:
        assert sym in decl and sym in _lib.SYMBOLS and hasattr(L, sym)
        assert getattr(L, sym).argtypes == decl[sym]
    assert [len(decl[s]) for s in SYMS] == [3, 8, 9, 12, 13, 13, 14]
    assert "#define PG_PCA_CHUNK 256" in text and "#define PG_PCA_MAX_L 64" in text
    wb = L.pg_pca_work_bytes
    assert wb.restype is C.c_size_t
    assert wb(0, 4, 1) == 0 and wb(16, -1, 1) == 0 and wb(16, 4, 0) == 0 and wb(16, 4, 65) == 0 and wb(16, (1 << 25) + 1, 1) == 0
    assert wb(1 << 30, 4, 1) == 0 and wb((1 << 30) - 1, 1 << 25, 1) == 0           # 2^22 sample groups x 2^17 chunks: no one launch
    assert wb(1, 0, 1) > 0 and wb(16, 1 << 25, 1) > 0 and wb(16, 4, 64) > 0 and wb((1 << 30) - 1, 4, 1) > 0
    assert wb(1030, 600, 5) >= 3 * 5 * 1030 * 8 and wb(1030, 600, 64) > wb(1030, 600, 5)
    buf = (C.c_double * 64)()
    vp = C.cast(buf, C.c_void_p)
    calls = {"pg_pca_stat_bed_dev": (None, 16, 4, vp, 4, 0, vp, vp), "pg_pca_stat_x_dev": (None, 16, 4, vp, 2, 16, 1, vp, vp),
             "pg_pca_proj_bed_dev": (None, 16, 4, vp, 4, 0, vp, 1, vp, 16, vp, 4), "pg_pca_proj_x_dev": (None, 16, 4, vp, 2, 16, 1, vp, 1, vp, 16, vp, 4),
             "pg_pca_back_bed_dev": (None, 16, 4, vp, 4, 0, vp, 1, vp, 4, vp, vp, 16),
             "pg_pca_back_x_dev": (None, 16, 4, vp, 2, 16, 1, vp, 1, vp, 4, vp, vp, 16)}
    for name, args in calls.items():
        assert getattr(L, name)(*args) == -22 and name.encode() in L.pg_last_error()


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


BAD = ["k 0", "k float", "k + oversample 65", "k > n", "k > p", "oversample negative", "iters 0", "tol negative", "tol NaN", "X 1-D", "X 3-D",
       "X int32", "X float16", "no SNPs", "no samples", "samples short", "samples long", "snps short", "snps long", "snp_batch 0",
       "snp_batch float", "snp_batch bool", "snp_batch negative"]


@pytest.mark.parametrize("bad", BAD)
def test_bad_inputs_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, (20, 5)).astype(np.float32)
    kw = dict(k=2)
    if bad == "k 0":
        kw["k"] = 0
    elif bad == "k float":
        kw["k"] = 2.0
    elif bad == "k + oversample 65":
        X, kw = rng.integers(0, 3, (80, 90)).astype(np.float32), dict(k=33, oversample=32)
    elif bad == "k > n":
        X, kw = rng.integers(0, 3, (4, 30)).astype(np.float32), dict(k=5, oversample=0)
    elif bad == "k > p":
        kw = dict(k=6, oversample=0)
    elif bad == "oversample negative":
        kw["oversample"] = -1
    elif bad == "iters 0":
        kw["iters"] = 0
    elif bad == "tol negative":
        kw["tol"] = -1e-12
    elif bad == "tol NaN":
        kw["tol"] = float("nan")
    elif bad == "X 1-D":
        X = X[:, 0]
    elif bad == "X 3-D":
        X = X[:, :, None]
    elif bad == "X int32":
        X = X.astype(np.int32)
    elif bad == "X float16":
        X = X.astype(np.float16)
    elif bad == "no SNPs":
        X = X[:, :0]
    elif bad == "no samples":
        X = X[:0]
    elif bad.startswith("samples"):
        kw["samples"] = list(range(19 if bad.endswith("short") else 21))
    elif bad.startswith("snps"):
        kw["snps"] = list(range(4 if bad.endswith("short") else 6))
    else:
        kw["snp_batch"] = {"snp_batch 0": 0, "snp_batch float": 256.0, "snp_batch bool": True, "snp_batch negative": -256}[bad]
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.pca(X, **kw)


@pytest.mark.parametrize("bad", ["no loadings", "other SNP count", "X 1-D", "X int32", "samples short", "snp_batch 0", "empty"])
def test_bad_projections_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, (20, 5)).astype(np.float32)
    res = lmm.PcaResult(None, np.ones(2), np.ones(2) / 2, pd.DataFrame(rng.standard_normal((5, 2)), columns=["PC1", "PC2"]), np.ones((5, 2)))
    kw = {}
    if bad == "no loadings":
        res = res._replace(loadings=None)
    elif bad == "other SNP count":
        X = X[:, :4]
    elif bad == "X 1-D":
        X = X[:, 0]
    elif bad == "X int32":
        X = X.astype(np.int32)
    elif bad == "samples short":
        kw["samples"] = list(range(19))
    elif bad == "snp_batch 0":
        kw["snp_batch"] = 0
    else:
        X = X[:0]
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.pca_project(X, res, **kw)
    if bad == "no loadings":
        with pytest.raises(ValueError):
            lmm.pca_project(X, SimpleNamespace(pcs=None), **kw)
