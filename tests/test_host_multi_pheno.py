"""CPU checks of the multi-phenotype scan's boundary (lmm.pygemma_multi, pg_assoc_pheno_dev): the public signature, the C ABI
declaration and export, the inputs refused before any device work, and the loud failure without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_pygemma_multi_is_public_with_its_signature():
    from pygemma import lmm
    assert callable(lmm.pygemma_multi)
    sig = inspect.signature(lmm.pygemma_multi)
    assert list(sig.parameters) == ["Y", "X", "W", "K", "Z", "snps", "verbose", "disable_checks", "grid", "eigen", "nproc",
                                    "eigenpairs", "stats"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"Z": None, "snps": None, "verbose": 0, "disable_checks": True, "grid": False, "eigen": True, "nproc": 1,
                        "eigenpairs": None, "stats": None}
    import pygemma_amd.lmm as impl
    assert "pygemma_multi" in impl.__all__


def test_pheno_entry_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in ("pg_assoc_pheno_dev", "pg_assoc_pheno_warm"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    _lib, L = _lib_loaded()
    for sym in ("pg_assoc_pheno_dev", "pg_assoc_pheno_warm"):
        assert hasattr(L, sym) and sym in _lib.SYMBOLS


def test_pheno_entry_refuses_a_null_context_without_touching_a_device():
    _lib, L = _lib_loaded()
    buf = (C.c_float * 64)()
    vp = C.cast(buf, C.c_void_p)
    rc = L.pg_assoc_pheno_dev(None, 16, 2, 4, 3, vp, vp, vp, 16, vp, 16, 0, vp, vp, vp, vp, vp, vp, None)
    assert rc == -22 and b"pg_assoc_pheno_dev" in L.pg_last_error()
    assert L.pg_assoc_pheno_warm(None, 16, 2, 3, 4) == -22


def _inputs(n=20, p=5, c=2, t=3, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, t)), rng.standard_normal((n, p)).astype(np.float32), np.ones((n, c), np.float32),
            np.abs(rng.standard_normal(n)).astype(np.float32))


@pytest.mark.parametrize("bad", ["rows", "empty", "3d"])
def test_bad_phenotype_matrix_is_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import _lib, lmm
    Y, X, W, d = _inputs()
    Y = {"rows": Y[:-1], "empty": Y[:, :0], "3d": Y[:, :, None]}[bad]
    # any device or library work would go through the pipeline: it must not be reached
    monkeypatch.setattr(lmm, "_scan", lambda *a, **k: pytest.fail("reached the pipeline"))
    with pytest.raises(ValueError):
        lmm.pygemma_multi(Y, X, W, d, eigen=False)


@pytest.mark.parametrize("kw", [{"lrt": True}, {"checkpoint": "ckpt"}, {"de": True}])
def test_out_of_scope_options_are_not_accepted(kw):
    from pygemma_amd import lmm
    Y, X, W, d = _inputs()
    with pytest.raises(TypeError):
        lmm.pygemma_multi(Y, X, W, d, eigen=False, **kw)


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    Y, X, W, d = _inputs()
    with pytest.raises(_lib.PgError):
        lmm.pygemma_multi(Y, X, W, d, eigen=False)


def _y_forms(n=20, t=3, seed=1):
    """The phenotype arguments lmm._pheno_columns takes, as (Y, labels, float64 (n, t') matrix of its columns)."""
    import pandas as pd
    Y = np.random.default_rng(seed).standard_normal((n, t)) * 1e3 + 1 / 3        # not float32 numbers: the cast rounds
    return {"(n,)": (Y[:, 0], [0], Y[:, :1]), "(n, 1)": (Y[:, :1], [0], Y[:, :1]), "(n, t)": (Y, [0, 1, 2], Y),
            "(n, t) F": (np.asfortranarray(Y), [0, 1, 2], Y), "float32": (Y.astype(np.float32), [0, 1, 2], Y.astype(np.float32)),
            "frame": (pd.DataFrame(Y, columns=["bmi", "ldl", "hdl"]), ["bmi", "ldl", "hdl"], Y)}


@pytest.mark.parametrize("form", ["(n,)", "(n, 1)", "(n, t)", "(n, t) F", "float32", "frame"])
def test_every_phenotype_form_reaches_the_pipeline_as_float32_columns(form, monkeypatch):
    from pygemma_amd import lmm
    _, X, W, d = _inputs()
    Y, labels, cols = _y_forms()[form]
    seen = {}

    def scan(Y32, *a, npheno, **k):
        seen["Y"] = Y32
        return {col: np.arange(npheno * 5, dtype=np.float64).reshape(npheno, 5) for col in lmm._COLS}

    monkeypatch.setattr(lmm, "_scan", scan)
    res = lmm.pygemma_multi(Y, X, W, d, eigen=False, snps=list("abcde"))
    assert seen["Y"].dtype == np.float32 and seen["Y"].shape == cols.shape and seen["Y"].flags.c_contiguous
    assert (seen["Y"] == cols.astype(np.float32)).all()
    assert isinstance(res, dict) and list(res) == labels
    for k, lab in enumerate(labels):
        assert list(res[lab].columns) == list(lmm._COLS) + ["SNPs"] and list(res[lab]["SNPs"]) == list("abcde")
        assert (res[lab]["beta"].to_numpy() == np.arange(5 * k, 5 * k + 5)).all()


def test_pheno_columns_casts_per_column_and_refuses_what_is_no_phenotype_matrix():
    import pandas as pd
    from pygemma_amd import lmm
    for form, (Y, labels, cols) in _y_forms().items():
        got_labels, got = lmm._pheno_columns(Y)
        assert got_labels == labels and len(got) == cols.shape[1], form
        for k, col in enumerate(got):
            assert col.dtype == np.float32 and col.ndim == 1 and (col == cols[:, k].astype(np.float32)).all(), (form, k)
    for bad in (np.zeros((20, 0)), np.zeros((20, 2, 1)), np.float64(1.0), pd.DataFrame(index=range(20))):
        with pytest.raises(ValueError):
            lmm._pheno_columns(bad)
