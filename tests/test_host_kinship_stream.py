"""CPU checks of the streamed kinship's boundary (lmm.kinship with a PackedBed or snp_batch, pg_kinship_*_acc_dev): the public
signature, the C ABI declaration and export, the inputs refused before any device use, and the loud failure without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pg_kinship_acc_bytes", "pg_kinship_bed_acc_dev", "pg_kinship_x_acc_dev", "pg_kinship_finish_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_kinship_signature_and_defaults():
    from pygemma_amd import lmm
    sig = inspect.signature(lmm.kinship)
    assert list(sig.parameters) == ["G", "standardize", "device", "snp_batch"]
    assert sig.parameters["snp_batch"].kind is inspect.Parameter.KEYWORD_ONLY
    defaults = {k: v.default for k, v in sig.parameters.items()}
    assert defaults == {"G": inspect.Parameter.empty, "standardize": True, "device": 0, "snp_batch": None}


def test_kinship_stream_entries_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
    _lib, L = _lib_loaded()
    for sym in SYMS:
        assert hasattr(L, sym) and sym in _lib.SYMBOLS


def test_kinship_stream_entries_refuse_misuse_without_touching_a_device():
    _lib, L = _lib_loaded()
    buf = (C.c_double * 64)()
    vp = C.cast(buf, C.c_void_p)
    assert L.pg_kinship_acc_bytes(0, 10) == 0 and L.pg_kinship_acc_bytes(10, 0) == 0
    assert L.pg_kinship_acc_bytes(10, 1) >= 8 * 10 * 10
    rc = L.pg_kinship_bed_acc_dev(None, 16, 4, vp, 4, 0, 1, vp)
    assert rc == -22 and b"pg_kinship_bed_acc_dev" in L.pg_last_error()
    rc = L.pg_kinship_x_acc_dev(None, 16, 4, vp, 0, 4, 0, 1, vp)
    assert rc == -22 and b"pg_kinship_x_acc_dev" in L.pg_last_error()
    rc = L.pg_kinship_finish_dev(None, 16, 4, vp, vp)
    assert rc == -22 and b"pg_kinship_finish_dev" in L.pg_last_error()


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


def _bed(n=20, p=5):
    from pygemma_amd.bed import PackedBed
    return PackedBed(np.zeros((p, (n + 3) // 4), np.uint8), n)


@pytest.mark.parametrize("bad", [0, -3, 2.5, True, "8"])
def test_bad_snp_batch_is_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.kinship(_bed(), snp_batch=bad)
    with pytest.raises(ValueError):
        lmm.kinship(np.zeros((20, 5), np.int8), snp_batch=bad)


@pytest.mark.parametrize("G", [np.zeros(20, np.int8), np.zeros((2, 20, 5), np.float32), np.zeros((0, 5), np.float32),
                               np.zeros((20, 0), np.uint8), np.zeros((20, 5), np.int16), np.zeros((20, 5), np.float16),
                               np.zeros((20, 5), bool), np.zeros((20, 5), np.complex64)])
def test_bad_arrays_are_refused_before_the_device(G, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.kinship(G, snp_batch=4)


def test_empty_packed_bed_is_refused_before_the_device(monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.kinship(_bed(n=0, p=5))
    with pytest.raises(ValueError):
        lmm.kinship(_bed(n=8, p=0))


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(_lib.PgError):
        lmm.kinship(_bed())
    with pytest.raises(_lib.PgError):
        lmm.kinship(np.zeros((20, 5), np.int8), snp_batch=2)
