"""CPU checks of the SNP statistics' boundary (lmm.snp_stats, lmm.snp_filter, PackedBed.take, pg_snp_stats_*, pg_hwe_exact_dev): the
Hardy-Weinberg reference of _snp_stats_truth.py against exact rational arithmetic, the filter on a hand-made frame, take() against the
host decode, the inputs refused before any device work and the loud failure without a GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import _snp_stats_truth as T

SYMS = ("pg_snp_stats_work_bytes", "pg_snp_stats_bed_dev", "pg_snp_stats_x_dev", "pg_hwe_exact_dev")


def _lib_loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_public_names_and_signatures():
    from pygemma import lmm
    import pygemma_amd.lmm as impl
    sig = inspect.signature(lmm.snp_stats)
    assert list(sig.parameters) == ["X", "snps", "hwe", "device", "snp_batch", "verbose", "stats"]
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == {
        "snps": None, "hwe": True, "device": 0, "snp_batch": None, "verbose": 0, "stats": None}
    sig = inspect.signature(lmm.snp_filter)
    assert list(sig.parameters) == ["st", "maf", "miss", "hwe"]
    assert [v.default for v in sig.parameters.values()][1:] == [0.01, 0.05, 0.0]           # GEMMA's defaults
    assert "snp_stats" in impl.__all__ and "snp_filter" in impl.__all__


def test_entries_exported_and_refuse_without_a_device():
    _lib, L = _lib_loaded()
    for sym in SYMS:
        assert hasattr(L, sym) and sym in _lib.SYMBOLS
    assert L.pg_snp_stats_work_bytes(1030, 130) >= 130 * 5 * 40
    assert L.pg_snp_stats_work_bytes(0, 4) == 0 and L.pg_snp_stats_work_bytes(16, -1) == 0
    assert L.pg_snp_stats_work_bytes(16, 1 << 25) > 0 and L.pg_snp_stats_work_bytes(16, (1 << 25) + 1) == 0
    buf = (C.c_double * 64)()
    vp = C.cast(buf, C.c_void_p)
    assert L.pg_snp_stats_bed_dev(None, 16, 4, vp, 4, 0, vp, vp, vp) == -22 and b"pg_snp_stats_bed_dev" in L.pg_last_error()
    assert L.pg_snp_stats_x_dev(None, 16, 4, vp, 2, 16, 1, vp, vp, vp) == -22 and b"pg_snp_stats_x_dev" in L.pg_last_error()
    assert L.pg_hwe_exact_dev(None, 16, 4, vp, vp) == -22 and b"pg_hwe_exact_dev" in L.pg_last_error()


def test_hwe_reference_against_exact_rationals():
    rng = np.random.default_rng(11)
    worst = 0.0
    triples = [(0, 5, 0), (3, 0, 4), (1, 0, 0), (0, 1, 0), (7, 7, 7), (40, 40, 40), (0, 120, 0), (60, 0, 60), (1, 1, 1), (2, 0, 1)]
    while len(triples) < 300:
        N = int(rng.integers(1, 121))
        a = int(rng.integers(0, N + 1))
        b = int(rng.integers(0, N - a + 1))
        triples.append((a, b, N - a - b))
    for n0, n1, n2 in triples:
        p, _ = T.hwe_reference(n0, n1, n2)
        if 2 * min(n0, n2) + n1 == 0:
            assert p == 1.0
            continue
        t = T.hwe_rational(n0, n1, n2)
        assert 0 < p <= 1
        worst = max(worst, abs(p - t) / t)
        assert abs(p - t) <= 8 * (n0 + n1 + n2) * 2.0 ** -53 * t, (n0, n1, n2, p, t)
    print(f"hwe reference against exact rationals: worst relative error {worst:.2e}")
    assert np.isnan(T.hwe_reference(0, 0, 0)[0])
    assert T.hwe_reference(5, 0, 0)[0] == 1.0 and T.hwe_reference(0, 0, 9)[0] == 1.0
    # a symmetric table has exact ties that different arms of the recurrence reach: they are ties, not gaps
    for tie in ((1, 2, 3), (3, 2, 1), (0, 4, 2)):                                # P(2) = P(4) exactly at N = 6, nr = 4
        p, gap = T.hwe_reference(*tie)
        assert p == T.hwe_rational(*tie) == 1.0 and gap > 0.5, (tie, p, gap)


def test_integer_moments_are_single_divisions():
    assert T.int_moments(4, 2, 1) == (4 / 4, (4 * 6 - 16) / 16)
    st = T.stats_truth(np.array([[0, 1.5, np.nan], [2, 0.5, np.nan], [1, np.inf, np.nan], [np.nan, -0.0, np.nan]]))
    assert st["counts"].tolist() == [[1, 1, 1, 1], [1, 1, 0, 0], [4, 0, 0, 0]]
    assert st["hard"].tolist() == [True, False, False]
    assert st["moments"][0].tolist() == [1.0, 2 / 3, 0.0, 2.0]
    assert np.isnan(st["moments"][2]).all()


def test_snp_filter_on_a_hand_made_frame():
    import pandas as pd
    from pygemma_amd import lmm
    nan = np.nan
    st = pd.DataFrame({
        "miss":  [0.05, 0.0500001, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0],
        "var":   [0.3,  0.3,       0.0, 0.3, 0.3, 0.3, 0.3, 0.3, nan],
        "maf":   [0.2,  0.2,       0.0, 0.01, 0.0099, nan, 0.2, 0.2, nan],
        "hwe_p": [0.5,  0.5,       1.0, 0.5, 0.5, nan, 1e-4, nan, nan]})
    # miss at the threshold stays; above it goes; var == 0 goes; maf at the threshold stays; below goes; NaN maf goes; all-missing goes
    assert lmm.snp_filter(st).tolist() == [True, False, False, True, False, False, True, True, False]
    assert lmm.snp_filter(st, maf=0).tolist() == [True, False, False, True, True, True, True, True, False]
    assert lmm.snp_filter(st, hwe=1e-4).tolist() == [True, False, False, True, False, False, True, True, False]       # equality keeps
    assert lmm.snp_filter(st, hwe=1e-3).tolist() == [True, False, False, True, False, False, False, True, False]     # NaN hwe_p: no test
    assert lmm.snp_filter(st, maf=0, miss=1.0, hwe=0.6).tolist() == [False, False, False, False, False, True, False, True, False]
    assert lmm.snp_filter(st.drop(columns="hwe_p")).tolist() == lmm.snp_filter(st).tolist()
    with pytest.raises(ValueError):
        lmm.snp_filter(st.drop(columns="hwe_p"), hwe=0.01)
    assert lmm.snp_filter(st).dtype == np.bool_


def test_packed_bed_take(tmp_path):
    from pygemma_amd.bed import PackedBed, write_bed
    rng = np.random.default_rng(3)
    n, p = 37, 19
    G = rng.integers(0, 3, (n, p)).astype(np.float64)
    G[rng.random((n, p)) < 0.1] = np.nan
    write_bed(str(tmp_path / "t"), G)
    for bed in (PackedBed.open(str(tmp_path / "t")), PackedBed.open(str(tmp_path / "t"), count_A1=True),         # file-backed memmaps
                PackedBed(T.pack(G), n)):
        full = bed.to_float(impute=False)
        mask = rng.random(p) < 0.5
        for idx in (mask, np.flatnonzero(mask), rng.permutation(p), np.array([5, 5, 0, 18]), [3, 1, 2], np.array([-1, 0]), np.zeros(p, bool),
                    np.array([], np.int64)):
            sub = bed.take(idx)
            cols = np.asarray(idx) if len(idx) else np.array([], np.int64)
            if full[:, cols].shape[1] == 0:                                      # an empty selection: nothing to decode
                assert sub.shape == (n, 0) and sub.data.shape == (0, (n + 3) // 4) and not sub.snps
                continue
            np.testing.assert_array_equal(sub.to_float(impute=False), full[:, cols])
            assert sub.n == n and sub.count_A1 == bed.count_A1 and sub.shape == (n, full[:, cols].shape[1])
            assert not isinstance(sub.data, np.memmap) and sub.data.flags.c_contiguous
            if bed.snps is None:
                assert sub.snps is None
            else:
                assert sub.snps == list(np.asarray(bed.snps)[cols])
        for bad in (np.ones(p + 1, bool), np.ones((p, 1), bool), [p], [-p - 1], np.array([0.0, 1.0]), np.zeros((2, 2), np.int64)):
            with pytest.raises(ValueError):
                bed.take(bad)


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


@pytest.mark.parametrize("bad", ["X 1-D", "X 3-D", "X int32", "X float16", "no SNPs", "no samples", "snps short", "snps long", "snp_batch 0",
                                 "snp_batch float", "snp_batch bool", "snp_batch negative"])
def test_bad_inputs_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    X = np.random.default_rng(0).integers(0, 3, (20, 5)).astype(np.float32)
    kw = {}
    if bad == "X 1-D":
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
    elif bad == "snps short":
        kw["snps"] = list("abcd")
    elif bad == "snps long":
        kw["snps"] = list("abcdef")
    else:
        kw["snp_batch"] = {"snp_batch 0": 0, "snp_batch float": 64.0, "snp_batch bool": True, "snp_batch negative": -4}[bad]
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        lmm.snp_stats(X, **kw)


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    from pygemma_amd.bed import PackedBed
    _lib_loaded()
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    G = np.random.default_rng(0).integers(0, 3, (20, 5)).astype(np.float64)
    for X in (G.astype(np.float32), G.astype(np.int8), PackedBed(T.pack(G), 20)):
        with pytest.raises(_lib.PgError):
            lmm.snp_stats(X)
