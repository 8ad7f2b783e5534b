"""CPU-only checks of the permutation tests: the label generator (lmm._perm_labels), emp2 and threshold on hand-made maxima, the truth
helper (tests/_perm_truth.py) against the case/control truth and its own exact values, every refusal of lmm.case_control_perm — which
must come before any device work — and the ABI of libpygemma_perm.so against include/pygemma_perm.h."""
import math

import numpy as np
import pytest

import _case_control_truth as CT
import _perm_truth as T


def _groups(n, seed=0):
    rng = np.random.default_rng(seed)
    group = rng.choice(np.array([-1, 0, 0, 1, 1], np.int8), n)
    strat = rng.integers(0, 3, n).astype(np.int32)
    strat[rng.random(n) < 0.1] = -1
    return group, strat


def test_perm_labels_keep_the_case_counts_and_the_study():
    from pygemma_amd import lmm
    n = 200
    group, strat = _groups(n)
    for st, S in ((None, 1), (strat, 3)):
        study = lmm._perm_study(group, st)
        lab = lmm._perm_labels(group, st, S, 40, seed=5)
        assert lab.shape == (40, n) and lab.dtype == np.int8 and set(np.unique(lab)) <= {0, 1}
        assert not lab[:, ~study].any()                                    # never an excluded sample
        for k in range(S):
            members = study & ((st == k) if st is not None else True)
            assert (lab[:, members].sum(axis=1) == ((group == 1) & members).sum()).all()
        assert len({row.tobytes() for row in lab}) > 30                    # they are shuffles
        assert (lab == lmm._perm_labels(group, st, S, 40, seed=5)).all()   # reproducible per seed
        assert (lab != lmm._perm_labels(group, st, S, 40, seed=6)).any()
        assert (lab[:7] == lmm._perm_labels(group, st, S, 7, seed=5)).all()      # row b does not change with nperm
    # a stratum-free sample is out of the study even when it has a status
    assert not lmm._perm_study(group, strat)[strat < 0].any() and lmm._perm_study(group, None)[(strat < 0) & (group >= 0)].all()


def test_emp2_and_threshold_on_hand_made_maxima():
    from pygemma_amd import lmm
    mx = np.array([1.0, 3.0, 3.0, 5.0, 0.0, 2.0, 3.0, 8.0, 4.0])          # nperm = 9; three tied at 3
    chi2 = np.array([3.0, 3.0000000000000004, 9.0, 0.0, np.nan, 8.0, 2.9999999999999996])
    want = np.array([(6 + 1) / 10, (3 + 1) / 10, (0 + 1) / 10, (9 + 1) / 10, np.nan, (1 + 1) / 10, (6 + 1) / 10])
    got = lmm._perm_emp2(mx, chi2)
    assert T.same_bits(got, want).all() and T.same_bits(got, T.emp2(mx, chi2)).all()
    res = lmm.PermResult(None, mx, "allelic")
    assert res.nperm == 9
    # rank ceil((1 - alpha) 10) of the sorted maxima 0 1 2 3 3 3 4 5 8
    assert res.threshold(0.5) == 3.0 and res.threshold(0.7) == 2.0 and res.threshold(0.2) == 5.0 and res.threshold(0.1) == 8.0
    assert res.threshold(0.4) == 3.0 and res.threshold(0.3) == 4.0         # inside and past the tie
    assert res.threshold(0.05) == math.inf                                 # rank 10 of 9
    assert lmm.PermResult(None, np.arange(19.0), "trend").threshold(0.05) == 18.0      # (1 - 0.05) * 20 is rank 19, not 20
    # a SNP above the threshold has emp2 <= alpha
    assert lmm._perm_emp2(mx, [np.nextafter(res.threshold(0.2), np.inf)])[0] <= 0.2
    for bad in (0, 1, -0.1, True, "a"):
        with pytest.raises(ValueError, match="alpha"):
            res.threshold(bad)


def _panel(n, p, seed):
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, rng.uniform(0.05, 0.6, p), (n, p)).astype(np.float64)
    G[rng.random((n, p)) < 0.08] = np.nan
    G[:, 0] = np.nan
    G[:, 1] = 2.0
    G[n // 2, 2] = 0.5
    return G


def test_truth_with_the_observed_labels_is_the_case_control_truth():
    """The sums of the observed status reproduce case_control's tables; the replay is bit-equal to case_control's replay, and within
    the 16 u gate of the exact values; the complement of a labelling has the same bits."""
    from pygemma_amd import lmm
    n, p = 150, 40
    G = _panel(n, p, 1)
    group, strat = _groups(n, 2)
    study = lmm._perm_study(group, strat)
    tot = T.totals(G, study)
    lab = np.stack([study & (group == 1), study & (group == 0)] + list(lmm._perm_labels(group, strat, 3, 30, 0)))
    a, R = T.sums(G, lab)
    tab = CT.tables(G, np.where(study, group, -1)).sum(axis=1)
    assert (tot[:, 1] == tab[:, [0, 1, 2, 4, 5, 6]].sum(axis=1)).all() and (R[:, 0] == tab[:, :3].sum(axis=1)).all()
    assert (a[:, 0] == tab[:, 1] + 2 * tab[:, 2]).all() and (tot[:, 2] == tab[:, [1, 5]].sum(axis=1) + 4 * tab[:, [2, 6]].sum(axis=1)).all()
    assert tot[0, 3] == 1 and tot[2, 3] == 3 and tot[1, 3] == 0 and tot[0, 1] == 0 and tot[2, 1] == 0
    cc = CT.replay(CT.tables(G, np.where(study, group, -1)))
    for test, col in ((T.ALLELIC, 3), (T.TREND, 4)):
        rp = T.replay(test, tot[:, 0], tot[:, 1], tot[:, 2], a, R)
        assert T.same_bits(rp[:, 0], cc[:, col]).all()
        assert T.same_bits(rp[:, 0], rp[:, 1]).all()                        # the complement: an exact tie
        ex = T.exact(test, tot[:, 0], tot[:, 1], tot[:, 2], a, R)
        assert T.within(rp, ex).all() and np.isnan(rp[:3]).all() and not np.isnan(rp[3:]).all()
        j, b = 5, 7
        fr = T.exact_fraction(test, *tot[j, :3], a[j, b], R[j, b])
        assert fr is not None and float(fr) == ex[j, b]
    n_ge, mx = T.reduce(rp, rp[:, 0])
    assert (n_ge[:3] == 0).all() and (n_ge[3:][~np.isnan(rp[3:, 0])] >= 2).all() and (mx >= 0).all()


def test_refusals_come_before_any_device_work(monkeypatch):
    from pygemma_amd import _lib, lmm
    from pygemma_amd.bed import PackedBed

    def no_device(*a, **k):
        raise AssertionError("a refused call reached the device")
    for name in ("load", "load_perm", "Context", "device_count"):
        monkeypatch.setattr(_lib, name, no_device)
    n, p = 12, 5
    X = np.zeros((n, p), np.int8)
    y = np.array([0, 1] * 6, np.float64)
    y[3] = np.nan
    bed = PackedBed(np.zeros((p, 3), np.uint8), n)
    good = np.zeros((4, n), np.int8)
    good[:, 1] = 1
    touched = good.copy()
    touched[2, 3] = 1                                                      # sample 3 has no status
    nostrat = np.zeros(n, np.int64)
    nostrat[5] = -1
    touched5 = good.copy()
    touched5[0, 5] = 1
    bad = [
        (dict(X=np.zeros(n, np.int8)), "2-D"),
        (dict(X=np.zeros((n, p), np.int32)), "int8, uint8, float32 or float64"),
        (dict(X=np.zeros((n, 0), np.int8)), "at least one sample"),
        (dict(y=y[:-1]), "shape mismatch"),
        (dict(y=np.where(y == 1, 2.0, y)), "0 .control., 1 .case. or NaN"),
        (dict(y=np.zeros(n)), "no case"),
        (dict(y=np.ones(n)), "no control"),
        (dict(strata=np.zeros(n - 1, np.int64)), "shape mismatch"),
        (dict(strata=np.arange(n) + 0.5), "integer labels"),
        (dict(snps=["rs1"]), "SNP names"),
        (dict(snp_batch=0), "snp_batch"),
        (dict(nperm=0), "nperm"),
        (dict(nperm=2.5), "nperm"),
        (dict(nperm=True), "nperm"),
        (dict(seed=-1), "seed"),
        (dict(test="geno"), "test must be one of"),
        (dict(test=0), "test must be one of"),
        (dict(labels=np.zeros((4, n - 1), np.int8)), "labels has shape"),
        (dict(labels=np.zeros(n, np.int8)), "labels has shape"),
        (dict(labels=np.zeros((0, n), np.int8)), "labels has shape"),
        (dict(labels=good * 2), "0 and 1"),
        (dict(labels=touched), "out of the study"),
        (dict(labels=touched5, strata=nostrat), "out of the study"),
    ]
    for kw, msg in bad:
        for src in (X, bed):
            args = dict(X=src, y=y)
            args.update(kw)
            with pytest.raises(ValueError, match=msg):
                lmm.case_control_perm(args.pop("X"), args.pop("y"), **args)
    # valid calls get as far as the device
    for kw in (dict(nperm=3), dict(labels=good), dict(labels=touched5), dict(nperm=2, strata=nostrat, test="trend")):
        with pytest.raises(AssertionError, match="reached the device"):
            lmm.case_control_perm(X, y, **kw)
    from pygemma import lmm as drop_in
    assert drop_in.case_control_perm is lmm.case_control_perm and "case_control_perm" in lmm.__all__ and "PermResult" in lmm.__all__


def test_perm_library_exports_what_its_header_declares_and_nothing_else():
    """libpygemma_perm.so against include/pygemma_perm.h, as tests/test_host_abi.py holds the main library to its header; the main
    and the case/control library carry none of the unit's entry points."""
    import ctypes as C
    import re
    import subprocess
    from pygemma_amd import _lib
    P = _lib.load_perm()
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.PERM_HEADER).read(), flags=re.S)
    decl = re.findall(r"\b(pgx?_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert [name for name, _ in decl] == _lib.PERM_SYMBOLS == ["pg_perm_label_bytes", "pg_perm_label_counts_dev", "pg_perm_totals_dev", "pg_perm_block_dev"]
    for name, params in decl:
        assert len(getattr(P, name).argtypes) == params.count(",") + 1, name

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(("pg_", "pgx_"))}
    assert exported(_lib.PERM_LIB_PATH) == set(_lib.PERM_SYMBOLS)
    assert not exported(_lib.LIB_PATH) & set(_lib.PERM_SYMBOLS) and not exported(_lib.CC_LIB_PATH) & set(_lib.PERM_SYMBOLS)
    vp, i64, i32, f64 = C.c_void_p, C.c_int64, C.c_int, C.c_double
    assert P.pg_perm_label_bytes.restype is C.c_size_t and P.pg_perm_label_bytes.argtypes == [i64, i64]
    assert P.pg_perm_totals_dev.argtypes == [vp, i64, vp, i64, i64, i64, vp, vp]
    assert P.pg_perm_block_dev.argtypes == [vp, i64, vp, i64, i64, i64, vp, vp, vp, i64, i64, i32, vp, i64, vp, vp, vp]
    assert P.pg_perm_label_bytes(129, 3) == 3 * 256 and P.pg_perm_label_bytes(1, 1) == 256 and P.pg_perm_label_bytes(300, 5) == 2048      # 5 rows of 384, up to 256
    assert P.pg_perm_label_bytes(0, 1) == 0 and P.pg_perm_label_bytes(1 << 28, 1) == 0 and P.pg_perm_label_bytes(5, 0) == 0
