"""CPU checks of the score test's boundary (lmm.pygemma_score, pg_score_null_dev, pg_score_dev): the public signature, the C ABI
declaration and export, the inputs refused before any device work, and the loud failure without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pg_score_null_dev", "pg_score_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_pygemma_score_is_public_with_its_signature():
    from pygemma import lmm
    assert callable(lmm.pygemma_score)
    sig = inspect.signature(lmm.pygemma_score)
    assert list(sig.parameters) == ["Y", "X", "W", "K", "Z", "snps", "verbose", "disable_checks", "eigen", "nproc", "eigenpairs", "stats"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"Z": None, "snps": None, "verbose": 0, "disable_checks": True, "eigen": True, "nproc": 1, "eigenpairs": None,
                        "stats": None}
    import pygemma_amd.lmm as impl
    assert "pygemma_score" in impl.__all__
    from pygemma_amd import ops
    assert list(inspect.signature(ops.score).parameters) == ["d", "Wr", "yr", "Xr", "lam0", "ctx"]


def test_score_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    _lib, L = _lib_loaded()
    for sym in SYMS:
        assert hasattr(L, sym) and sym in _lib.SYMBOLS


def test_score_entries_refuse_a_null_context_without_touching_a_device():
    _lib, L = _lib_loaded()
    buf = (C.c_float * 64)()
    vp = C.cast(buf, C.c_void_p)
    rc = L.pg_score_dev(None, 16, 2, 4, vp, vp, vp, 1.0, vp, 16, vp, vp, vp, vp, vp, None)
    assert rc == -22 and b"pg_score_dev" in L.pg_last_error()
    rc = L.pg_score_null_dev(None, 16, 2, vp, vp, vp, vp)
    assert rc == -22 and b"pg_score_null_dev" in L.pg_last_error()


def _inputs(n=20, p=5, c=2, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 1)), rng.standard_normal((n, p)).astype(np.float32), np.ones((n, c), np.float32),
            np.abs(rng.standard_normal(n)).astype(np.float32))


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


@pytest.mark.parametrize("bad", ["Y rows", "W rows", "c > 30", "n - c - 1 <= 0"])
def test_bad_inputs_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    Y, X, W, d = _inputs()
    if bad == "Y rows":
        Y = Y[:-1]
    elif bad == "W rows":
        W = W[:-1]
    elif bad == "c > 30":
        Y, X, W, d = _inputs(n=64, c=31)
    else:
        W = np.ones((20, 19), np.float32)
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.pygemma_score(Y, X, W, d, eigen=False)


def test_packed_bed_with_eigen_false_is_refused(monkeypatch):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    n, p = 20, 5
    Y, _X, W, d = _inputs(n, p)
    bed = PackedBed(np.zeros((p, (n + 3) // 4), np.uint8), n)
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.pygemma_score(Y, bed, W, d, eigen=False)


@pytest.mark.parametrize("kw", [{"lrt": True}, {"checkpoint": "ckpt"}, {"grid": True}, {"de": True}])
def test_out_of_scope_options_are_not_accepted(kw):
    from pygemma_amd import lmm
    Y, X, W, d = _inputs()
    with pytest.raises(TypeError):
        lmm.pygemma_score(Y, X, W, d, eigen=False, **kw)


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    Y, X, W, d = _inputs()
    with pytest.raises(_lib.PgError):
        lmm.pygemma_score(Y, X, W, d, eigen=False)
