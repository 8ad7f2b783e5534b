"""CPU checks of the interaction scan's boundary (lmm.pygemma_gxe, ops.gxe, pg_assoc_gxe_dev, pg_assoc_gxe_warm, pg_gxe_scale_u_dev):
the public signature, the C ABI declaration and export, the inputs refused before any device work, and the loud failure without
a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pg_assoc_gxe_dev", "pg_assoc_gxe_warm", "pg_gxe_scale_u_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_pygemma_gxe_is_public_with_its_signature():
    from pygemma import lmm
    assert callable(lmm.pygemma_gxe)
    sig = inspect.signature(lmm.pygemma_gxe)
    assert list(sig.parameters) == ["Y", "X", "W", "K", "E", "Z", "snps", "verbose", "disable_checks", "eigen", "nproc", "eigenpairs",
                                    "checkpoint", "stats"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"Z": None, "snps": None, "verbose": 0, "disable_checks": True, "eigen": True, "nproc": 1, "eigenpairs": None,
                        "checkpoint": None, "stats": None}
    import pygemma_amd.lmm as impl
    assert "pygemma_gxe" in impl.__all__
    from pygemma_amd import ops
    sig = inspect.signature(ops.gxe)
    assert list(sig.parameters) == ["d", "Wr", "yr", "Xr", "XEr", "ctx", "want_p", "return_stats"]


def test_gxe_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    _lib, L = _lib_loaded()
    for sym in SYMS:
        assert hasattr(L, sym) and sym in _lib.SYMBOLS


def test_gxe_entries_refuse_a_null_context_without_touching_a_device():
    _lib, L = _lib_loaded()
    buf = (C.c_float * 64)()
    vp = C.cast(buf, C.c_void_p)
    rc = L.pg_assoc_gxe_dev(None, 16, 2, 4, vp, vp, vp, vp, 16, vp, 16, vp, vp, vp, vp, vp, None, None)
    assert rc == -22 and b"pg_assoc_gxe_dev" in L.pg_last_error()
    rc = L.pg_assoc_gxe_warm(None, 16, 2)
    assert rc == -22 and b"pg_assoc_gxe_warm" in L.pg_last_error()
    rc = L.pg_gxe_scale_u_dev(None, 16, vp, 16, vp, vp)
    assert rc == -22 and b"pg_gxe_scale_u_dev" in L.pg_last_error()


def _inputs(n=20, p=5, c=2, seed=0):
    rng = np.random.default_rng(seed)
    W = np.c_[np.ones(n), rng.standard_normal((n, c - 1))].astype(np.float32)
    K = rng.standard_normal((n, n))
    K = (K @ K.T / n).astype(np.float32)
    return (rng.standard_normal((n, 1)), rng.integers(0, 3, (n, p)).astype(np.float32), W, K,
            rng.standard_normal(n).astype(np.float32))


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


@pytest.mark.parametrize("bad", ["E shape (n, 2)", "E rows", "E NaN", "E inf", "e in span(W)", "W 0 columns", "W 29 columns",
                                 "n - c - 3 <= 0", "eigen=False"])
def test_bad_inputs_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    Y, X, W, K, E = _inputs()
    kw = {}
    if bad == "E shape (n, 2)":
        E = np.c_[E, E]
    elif bad == "E rows":
        E = E[:-1]
    elif bad == "E NaN":
        E = E.copy(); E[3] = np.nan
    elif bad == "E inf":
        E = E.copy(); E[0] = np.inf
    elif bad == "e in span(W)":
        E = 2.0 * W[:, 1] - 0.5 * W[:, 0]
    elif bad == "W 0 columns":
        W = np.ones((20, 0), np.float32)
    elif bad == "W 29 columns":
        Y, X, W, K, E = _inputs(n=64, c=29)
    elif bad == "n - c - 3 <= 0":
        W = np.c_[np.ones(20), np.random.default_rng(1).standard_normal((20, 16))].astype(np.float32)   # c = 17: n - c - 3 = 0
    else:
        kw["eigen"] = False
    _no_device(monkeypatch)
    with pytest.raises(ValueError) as ex:
        lmm.pygemma_gxe(Y, X, W, K, E, **kw)
    if bad == "eigen=False":
        assert "ops.gxe" in str(ex.value)


def test_largest_accepted_shapes_pass_the_checks(monkeypatch):
    """W with 28 columns and n - c - 3 = 1 are accepted (the refusals stop exactly at the limits): the call gets as far as the
    device."""
    from pygemma_amd import _lib, lmm
    rng = np.random.default_rng(2)
    for n, c in ((64, 28), (20, 16)):
        Y, X, W, K, E = _inputs(n=n, c=c)
        W = np.c_[np.ones(n), rng.standard_normal((n, c - 1))].astype(np.float32)
        reached = []

        def stop(*a, **k):
            reached.append(True)
            raise _lib.PgError("stop")
        monkeypatch.setattr(_lib, "device_count", stop)
        monkeypatch.setattr(_lib, "Context", stop)
        with pytest.raises(_lib.PgError):
            lmm.pygemma_gxe(Y, X, W, K, E)
        assert reached


def _reaches_the_device(monkeypatch, Y, X, W, K, E):
    from pygemma_amd import _lib, lmm
    reached = []

    def stop(*a, **k):
        reached.append(True)
        raise _lib.PgError("stop")
    monkeypatch.setattr(_lib, "device_count", stop)
    monkeypatch.setattr(_lib, "Context", stop)
    with pytest.raises(_lib.PgError):
        lmm.pygemma_gxe(Y, X, W, K, E)
    return bool(reached)


@pytest.mark.parametrize("n,mean,sd", [(10000, 130.0, 15.0),     # systolic blood pressure
                                       (40000, 50.0, 10.0),      # age
                                       (2000, 1960.0, 10.0),     # birth year
                                       (2000, 2000.0, 0.5)])
def test_uncentred_environment_beside_an_intercept_is_accepted(n, mean, sd, monkeypatch):
    """The span check is scale-invariant: an environment with a large mean and a small spread, beside an intercept, is not in W's
    span at any n (lmm.pygemma takes the same column in W)."""
    rng = np.random.default_rng(n)
    E = (mean + sd * rng.standard_normal(n)).astype(np.float32)
    W = np.ones((n, 1), np.float32)
    X = rng.integers(0, 3, (n, 4)).astype(np.float32)
    Y = rng.standard_normal((n, 1))
    K = np.zeros((1, 1), np.float32)         # never looked at: the stub stops the call at the device
    assert _reaches_the_device(monkeypatch, Y, X, W, K, E)
    W2 = np.c_[np.ones(n), rng.standard_normal(n) * 1e3 + 5e4].astype(np.float32)
    assert _reaches_the_device(monkeypatch, Y, X, W2, K, E)


@pytest.mark.parametrize("case", ["float32 combination", "constant", "scaled intercept", "copy of a column"])
def test_environment_in_the_span_of_W_is_refused(case, monkeypatch):
    from pygemma_amd import lmm
    n = 10000
    rng = np.random.default_rng(3)
    W = np.c_[np.ones(n), 130 + 15 * rng.standard_normal(n), rng.standard_normal(n)].astype(np.float32)
    E = {"float32 combination": W[:, 1] * np.float32(0.25) - W[:, 2] * np.float32(3.5) + np.float32(7.0),
         "constant": np.full(n, 5.0, np.float32),
         "scaled intercept": np.full(n, 1e-20, np.float32),
         "copy of a column": W[:, 1].copy()}[case]
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="span"):
        lmm.pygemma_gxe(rng.standard_normal((n, 1)), np.zeros((n, 2), np.float32), W, np.zeros((1, 1), np.float32), E)


@pytest.mark.parametrize("kw", [{"lrt": True}, {"grid": True}, {"de": True}])
def test_out_of_scope_options_are_not_accepted(kw):
    from pygemma_amd import lmm
    Y, X, W, K, E = _inputs()
    with pytest.raises(TypeError):
        lmm.pygemma_gxe(Y, X, W, K, E, **kw)


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    Y, X, W, K, E = _inputs()
    with pytest.raises(_lib.PgError):
        lmm.pygemma_gxe(Y, X, W, K, E)
