"""CPU checks of the linear-model scan's boundary (lmm.pygemma_lm, ops.lm, pg_lm_*): the public signature, the C ABI declaration and
export, the inputs refused before any device work, the loud failure without a GPU, and the contract's formulas (an fp64 replica of
what csrc/lm.hip computes) against the per-SNP OLS algebra of the reference's experiments/1000G/run_lin_reg.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pg_lm_work_bytes", "pg_lm_setup_dev", "pg_lm_x_dev", "pg_lm_bed_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_pygemma_lm_is_public_with_its_signature():
    from pygemma import lmm
    assert callable(lmm.pygemma_lm)
    sig = inspect.signature(lmm.pygemma_lm)
    assert list(sig.parameters) == ["Y", "X", "W", "snps", "verbose", "device", "snp_batch", "stats"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"snps": None, "verbose": 0, "device": 0, "snp_batch": None, "stats": None}
    import pygemma_amd.lmm as impl
    assert "pygemma_lm" in impl.__all__
    from pygemma_amd import ops
    assert list(inspect.signature(ops.lm).parameters) == ["W", "Y", "X", "ctx"]


def test_lm_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    _lib, L = _lib_loaded()
    for sym in SYMS:
        assert hasattr(L, sym) and sym in _lib.SYMBOLS
    assert L.pg_lm_work_bytes(203, 3, 1) >= 8 * 203 * 16
    assert L.pg_lm_work_bytes(203, 30, 35) == 0                      # c + t > 64: refused by the entries


def test_lm_entries_refuse_a_null_context_without_touching_a_device():
    _lib, L = _lib_loaded()
    buf = (C.c_float * 64)()
    vp = C.cast(buf, C.c_void_p)
    rc = L.pg_lm_setup_dev(None, 16, 2, 1, vp, vp, 16, vp)
    assert rc == -22 and b"pg_lm_setup_dev" in L.pg_last_error()
    rc = L.pg_lm_x_dev(None, 16, 2, 1, 4, vp, 2, 16, 1, vp, vp, vp, vp, vp, None, 4)
    assert rc == -22 and b"pg_lm_x_dev" in L.pg_last_error()
    rc = L.pg_lm_bed_dev(None, 16, 2, 1, 4, vp, 4, 0, vp, vp, vp, vp, vp, None, 4)
    assert rc == -22 and b"pg_lm_bed_dev" in L.pg_last_error()


def _inputs(n=20, p=5, c=2, t=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, t)), rng.standard_normal((n, p)).astype(np.float32), np.ones((n, c), np.float32)


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


@pytest.mark.parametrize("bad", ["Y rows", "W rows", "X 1-D", "X 3-D", "c = 0", "c > 30", "W 1-D", "c + t > 64", "n - c - 1 <= 0",
                                 "snp_batch 0", "snp_batch float", "snp_batch bool", "Y 3-D"])
def test_bad_inputs_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    Y, X, W = _inputs()
    kw = {}
    if bad == "Y rows":
        Y = Y[:-1]
    elif bad == "W rows":
        W = W[:-1]
    elif bad == "X 1-D":
        X = X[:, 0]
    elif bad == "X 3-D":
        X = X[:, :, None]
    elif bad == "c = 0":
        W = W[:, :0]
    elif bad == "c > 30":
        Y, X, W = _inputs(n=64, c=31)
    elif bad == "W 1-D":
        W = W[:, 0]
    elif bad == "c + t > 64":
        Y, X, W = _inputs(n=128, c=30, t=35)
    elif bad == "n - c - 1 <= 0":
        W = np.ones((20, 19), np.float32)
    elif bad == "snp_batch 0":
        kw["snp_batch"] = 0
    elif bad == "snp_batch float":
        kw["snp_batch"] = 64.0
    elif bad == "snp_batch bool":
        kw["snp_batch"] = True
    else:
        Y = Y[:, :, None]
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.pygemma_lm(Y, X, W, **kw)


@pytest.mark.parametrize("kw", [{"nproc": 2}, {"checkpoint": "ckpt"}, {"Z": None}, {"K": None}])
def test_out_of_scope_options_are_not_accepted(kw):
    from pygemma_amd import lmm
    Y, X, W = _inputs()
    with pytest.raises(TypeError):
        lmm.pygemma_lm(Y, X, W, **kw)


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    _lib_loaded()
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    Y, X, W = _inputs()
    with pytest.raises(_lib.PgError):
        lmm.pygemma_lm(Y, X, W)


def contract_replica(W, Y, X):
    """The arithmetic csrc/lm.hip is specified to do, in fp64 NumPy: Cholesky of W'W, Q = W L^-T, Y~ = Y - Q Q'Y, then per SNP
    sxx = x'x - |Q'x|^2, sxy = x'y~, rss = syy - sxy^2/sxx.  W (n,c), Y (n,t), X (n,p) -> (t,p) columns."""
    W, Y, X = (np.asarray(a, np.float64) for a in (W, Y, X))
    n, c = W.shape
    df = n - c - 1
    Lc = np.linalg.cholesky(W.T @ W)
    Q = np.linalg.solve(Lc, W.T).T
    Yt = Y - Q @ (Q.T @ Y)
    syy = np.einsum("ik,ik->k", Yt, Yt)
    xx = np.einsum("ip,ip->p", X, X)
    z = Q.T @ X
    sxx = xx - np.einsum("jp,jp->p", z, z)
    sxy = Yt.T @ X                                              # (t, p)
    rss = syy[:, None] - sxy ** 2 / sxx[None, :]
    return {"beta": sxy / sxx, "se_beta": np.sqrt(rss / (df * sxx)), "tau": df / rss, "F_wald": df * sxy ** 2 / (sxx * rss)}


def test_contract_formulas_are_the_reference_ols_algebra():
    # run_lin_reg.py's run_gwas, restated: H = W (W'W)^-1 W', X and y residualised, sigma^2 = rss / (n - c - 1)
    n, p, c = 203, 40, 3
    rng = np.random.default_rng(12)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32).astype(np.float64)
    X = rng.binomial(2, rng.uniform(0.1, 0.5, p), (n, p)).astype(np.float64)
    y = (X[:, :3] @ np.array([0.5, -0.3, 0.2]) + rng.standard_normal(n)).astype(np.float32).astype(np.float64)
    H = W @ np.linalg.inv(W.T @ W) @ W.T
    yr, Xr = y - H @ y, X - H @ X
    rep = contract_replica(W, y[:, None], X)
    for g in range(p):
        x = Xr[:, g]
        beta = (x @ yr) / (x @ x)
        resid = y - x * beta - H @ y
        var = (1.0 / (X[:, g] @ X[:, g] - X[:, g] @ H @ X[:, g])) * (resid @ resid) / (n - c - 1)
        se = np.sqrt(var)
        F = (beta / se) ** 2
        assert abs(rep["beta"][0, g] - beta) <= 1e-10 * abs(beta), g
        assert abs(rep["se_beta"][0, g] - se) <= 1e-10 * se, g
        assert abs(rep["F_wald"][0, g] - F) <= 1e-10 * F, g
        assert abs(rep["tau"][0, g] - (n - c - 1) / (resid @ resid)) <= 1e-10 * rep["tau"][0, g], g


def _y_forms(n=20, t=3, seed=1):
    """The phenotype arguments lmm._pheno_columns takes, as (Y, labels, float64 (n, t') matrix of its columns): those of
    test_host_multi_pheno.py."""
    import pandas as pd
    Y = np.random.default_rng(seed).standard_normal((n, t)) * 1e3 + 1 / 3        # not float32 numbers: the cast rounds
    return {"(n,)": (Y[:, 0], [0], Y[:, :1]), "(n, 1)": (Y[:, :1], [0], Y[:, :1]), "(n, t)": (Y, [0, 1, 2], Y),
            "(n, t) F": (np.asfortranarray(Y), [0, 1, 2], Y), "float32": (Y.astype(np.float32), [0, 1, 2], Y.astype(np.float32)),
            "frame": (pd.DataFrame(Y, columns=["bmi", "ldl", "hdl"]), ["bmi", "ldl", "hdl"], Y)}


@pytest.mark.parametrize("form", ["(n,)", "(n, 1)", "(n, t)", "(n, t) F", "float32", "frame"])
def test_every_phenotype_form_reaches_the_scan_as_float32_rows(form, monkeypatch):
    """pygemma_lm takes the phenotype forms pygemma_multi takes (one lmm._pheno_columns): the scan gets their (t, n) float32 image."""
    from pygemma_amd import lmm
    _, X, W = _inputs()
    Y, labels, cols = _y_forms()[form]
    t, seen = len(labels), {}

    def stream(X_, W_, Yt, *a):
        seen["Y"] = Yt
        return {col: np.arange(t * 5, dtype=np.float64).reshape(t, 5) for col in lmm._LM_COLS}

    monkeypatch.setattr(lmm, "_lm_stream", stream)
    res = lmm.pygemma_lm(Y, X, W, snps=list("abcde"))
    assert seen["Y"].dtype == np.float32 and seen["Y"].shape == cols.T.shape and seen["Y"].flags.c_contiguous
    assert (seen["Y"] == cols.T.astype(np.float32)).all()
    frames = {labels[0]: res} if t == 1 else res
    assert list(frames) == labels
    for k, lab in enumerate(labels):
        assert list(frames[lab].columns) == list(lmm._LM_COLS) + ["SNPs"] and list(frames[lab]["SNPs"]) == list("abcde")
        assert (frames[lab]["beta"].to_numpy() == np.arange(5 * k, 5 * k + 5)).all()


@pytest.mark.parametrize("bad", ["no columns", "3-D", "empty frame"])
def test_bad_phenotype_matrix_is_refused_before_the_device(bad, monkeypatch):
    import pandas as pd
    from pygemma_amd import lmm
    Y, X, W = _inputs()
    Y = {"no columns": Y[:, :0], "3-D": Y[:, :, None], "empty frame": pd.DataFrame(index=range(20))}[bad]
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.pygemma_lm(Y, X, W)
