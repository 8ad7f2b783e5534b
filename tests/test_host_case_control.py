"""CPU-only checks of the case/control tests: the truth helper (tests/_case_control_truth.py) against SciPy and against textbook forms in
exact rationals, the degenerate strata of the Cochran-Mantel-Haenszel sums, the replay of the device's operation order against the exact
values, and every refusal of lmm.case_control — which must come before any device work, so they pass without a GPU."""
import math
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import _case_control_truth as T

U = 2.0 ** -53


def _random_tables(seed, count, hi):
    rng = np.random.default_rng(seed)
    return [tuple(int(v) for v in rng.integers(1, hi, 4)) for _ in range(count)]


def test_chi2_and_fisher_against_scipy():
    """About 50 random small tables: chi2 within 1e-12 relative of chi2_contingency(correction=False), Fisher within 1e-9 of
    fisher_exact (SciPy's own summation is the looser side)."""
    from scipy import stats as sps
    for a, b, c, d in _random_tables(1, 50, 60):
        want = sps.chi2_contingency([[a, b], [c, d]], correction=False)[0]
        assert abs(float(T.chi2_2x2(a, b, c, d)) - want) <= 1e-12 * want, (a, b, c, d)
        pf = float(T.fisher(a, b, c, d)[0])
        assert abs(pf - sps.fisher_exact([[a, b], [c, d]])[1]) <= 1e-9 * pf, (a, b, c, d)
        assert abs(T.replay_fisher(a, b, c, d) - pf) <= 8 * min(a + b, c + d, a + c, b + d) * U * pf, (a, b, c, d)


def test_geno_against_scipy_and_trend_against_its_textbook_form():
    from scipy import stats as sps
    rng = np.random.default_rng(2)
    for _ in range(50):
        t = np.zeros(8, np.int64)
        t[[0, 1, 2, 4, 5, 6]] = rng.integers(1, 80, 6)
        want = sps.chi2_contingency([t[:3], t[4:7]], correction=False)[0]
        assert abs(float(T.geno(t)) - want) <= 1e-12 * want, t
        assert T.trend(t) == T.trend_textbook(t), t                   # equal as rationals
    assert T.trend(np.array([3, 0, 0, 0, 5, 0, 0, 0])) is None       # one genotype only: no variance
    assert T.geno(np.array([3, 2, 0, 0, 5, 1, 0, 0])) is None        # an unseen genotype


def test_cmh_degenerate_strata_and_the_one_stratum_identity():
    full = [4, 6, 3, 1, 5, 2, 7, 0]
    no_ctrl = [2, 1, 1, 0, 0, 0, 0, 3]            # controls all missing: no called control
    single = [0, 1, 0, 0, 0, 0, 0, 0]             # a stratum of one sample
    empty = [0] * 8
    u, v, sad, sbc, absu, used = T.cmh(np.array([full, no_ctrl, single, empty]))
    assert used == 1
    assert (u, v, sad, sbc) == T.cmh(np.array([full]))[:4]
    # one stratum: chi2_cmh = chi2_allelic (T - 1) / T
    a, b, c, d = T.allelic(full)
    tot = a + b + c + d
    assert u * u / v == T.chi2_2x2(a, b, c, d) * Fraction(tot - 1, tot)
    # every stratum without both groups: v = 0, no statistic
    no_case = [0, 0, 0, 2, 3, 1, 0, 0]
    tab = np.array([[no_ctrl, no_case, single]])
    tr = T.truth(tab)
    assert not np.isnan(tr["chi2_allelic"][0]) and tr["cmh_u"][0] == 0 and tr["cmh_v"][0] == 0 and np.isnan(tr["chi2_cmh"][0]) and np.isnan(tr["or_mh"][0])


def test_truth_rules_for_empty_groups_and_zero_cells():
    tab = np.array([[[0, 0, 0, 4, 3, 2, 1, 0]],           # no called case: every statistic NaN, the counts stay
                    [[5, 0, 0, 0, 3, 2, 0, 0]],           # cases carry no counted allele: a = 0 -> or = 0
                    [[0, 0, 4, 0, 3, 0, 0, 0]],           # b = 0 and c = 0 -> b c = 0 < a d: +inf
                    [[4, 0, 0, 0, 3, 0, 0, 0]]])          # monomorphic: a column margin is 0, a d = b c = 0
    tr = T.truth(tab)
    assert all(np.isnan(tr[k][0]) for k in T.STAT + ("p_fisher", "cmh_u", "cmh_v", "chi2_cmh", "or_mh"))
    assert (tr["counts"][0] == tab[0, 0]).all()
    assert tr["or"][1] == 0.0 and tr["or"][2] == math.inf and np.isnan(tr["or"][3])
    assert np.isnan(tr["chi2_allelic"][3]) and np.isnan(tr["chi2_trend"][3]) and tr["p_fisher"][3] == 1.0
    rp = T.replay(tab)
    assert np.isnan(rp[0]).all() and rp[1, 2] == 0.0 and rp[2, 2] == math.inf and np.isnan(rp[3, 2]) and rp[3, 8] == 1.0


def test_replay_of_the_device_order_is_within_the_rounding_bounds_of_the_truth():
    """At most 8 roundings for a 2 x 2 or trend statistic and 7 for the three-term genotypic sum: the gate of the GPU test, 16 x 2^-53."""
    rng = np.random.default_rng(3)
    G = rng.binomial(2, rng.uniform(0.05, 0.6, 200), (300, 200)).astype(np.float64)
    G[rng.random(G.shape) < 0.05] = np.nan
    status = rng.integers(-1, 2, 300)
    stratum = rng.integers(0, 5, 300)
    tab = T.tables(G, status, stratum, 5)
    tr, rp = T.truth(tab), T.replay(tab)
    for j, k in enumerate(T.STAT):
        ok = np.isnan(tr[k]) == np.isnan(rp[:, j])
        with np.errstate(invalid="ignore"):
            ok &= np.isnan(tr[k]) | (np.abs(rp[:, j] - tr[k]) <= 16 * U * np.abs(tr[k]))
        assert ok.all(), k
    cm = T.replay_cmh(tab)
    assert (np.abs(cm[:, 0] - tr["cmh_u"]) <= (5 + 3) * U * tr["cmh_abs"]).all()
    assert (np.abs(cm[:, 1] - tr["cmh_v"]) <= (16 + 5 + 8) * U * tr["cmh_v"]).all()


def test_pack_matches_write_bed(tmp_path):
    from pygemma_amd.bed import write_bed
    rng = np.random.default_rng(4)
    G = rng.integers(0, 3, (37, 11)).astype(np.float64)
    G[rng.random(G.shape) < 0.1] = np.nan
    assert (T.pack(G) == write_bed(str(tmp_path / "t"), G)).all()


def test_strata_labels():
    from pygemma_amd import lmm
    code, S = lmm._cc_strata(np.array([7, -3, 2, 7, 100, 2]), 6)
    assert S == 3 and code.dtype == np.int32 and code.tolist() == [1, -1, 0, 1, 2, 0]
    code, S = lmm._cc_strata(np.array([1.0, np.nan, 0.0]), 3)
    assert S == 2 and code.tolist() == [1, -1, 0]
    code, S = lmm._cc_strata(pd.Categorical(["b", "a", None, "b"]), 4)
    assert S == 2 and code.tolist() == [1, 0, -1, 1]
    code, S = lmm._cc_strata(pd.Series(["x", "y", "x"], dtype="category"), 3)
    assert S == 2 and code.tolist() == [0, 1, 0]
    assert lmm._cc_strata(None, 5) == (None, 1)


def test_p_value_expressions():
    from pygemma_amd import lmm
    chi2 = np.array([0.0, 0.4549364, 3.841458820694124, 50.0, np.nan])
    p1, p2 = lmm._cc_p1(chi2), lmm._cc_p2(chi2)
    assert p1[0] == 1.0 and abs(p1[1] - 0.5) < 1e-7 and abs(p1[2] - 0.05) < 1e-12 and np.isnan(p1[4])
    assert [abs(p1[k] - math.erfc(math.sqrt(chi2[k] / 2))) <= 4 * U * p1[k] for k in range(4)] == [True] * 4
    assert p2[0] == 1.0 and p2[3] == math.exp(-25.0) and np.isnan(p2[4])


def test_refusals_come_before_any_device_work(monkeypatch):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed

    def no_device():
        raise AssertionError("a refused call reached the device")
    monkeypatch.setattr(lmm, "_gpus", no_device)
    n, p = 12, 5
    X = np.zeros((n, p), np.int8)
    y = np.array([0, 1] * 6, np.float64)
    bed = PackedBed(np.zeros((p, 3), np.uint8), n)
    bad = [
        (dict(X=np.zeros(n, np.int8)), "2-D"),
        (dict(X=np.zeros((n, p), np.int32)), "int8, uint8, float32 or float64"),
        (dict(X=np.zeros((0, p), np.int8), y=np.zeros(0)), "at least one sample"),
        (dict(X=np.zeros((n, 0), np.int8)), "at least one sample"),
        (dict(y=y[:-1]), "shape mismatch"),
        (dict(y=np.zeros((n, 2))), "shape mismatch"),
        (dict(y=np.where(y == 1, 2.0, y)), "0 .control., 1 .case. or NaN"),
        (dict(y=np.array(["a"] * n)), "dtype"),
        (dict(y=np.zeros(n)), "no case"),
        (dict(y=np.ones(n)), "no control"),
        (dict(strata=np.zeros(n - 1, np.int64)), "shape mismatch"),
        (dict(strata=np.arange(n) + 0.5), "integer labels"),
        (dict(strata=np.array(["a"] * n)), "integer labels"),
        (dict(strata=np.arange(17).repeat(2)[:n + 22], X=np.zeros((34, p), np.int8), y=np.array([0, 1] * 17)), "at most 16 strata"),
        (dict(strata=np.full(n, -1)), "no sample"),
        (dict(snps=["rs1"]), "SNP names"),
        (dict(snp_batch=0), "snp_batch"),
        (dict(snp_batch=2.5), "snp_batch"),
        (dict(snp_batch=True), "snp_batch"),
    ]
    for kw, msg in bad:
        for src in (X, bed):
            args = dict(X=src, y=y)
            args.update(kw)
            with pytest.raises(ValueError, match=msg):
                lmm.case_control(args.pop("X"), args.pop("y"), **args)
    # a valid call gets as far as the device
    with pytest.raises(AssertionError, match="reached the device"):
        lmm.case_control(X, y, strata=np.arange(n) % 16)
    from pygemma import lmm as drop_in
    assert drop_in.case_control is lmm.case_control


def test_cc_library_exports_what_its_header_declares_and_nothing_else():
    """libpygemma_cc.so against include/pygemma_cc.h, as tests/test_host_abi.py holds the main library to its header; the main
    library carries none of the unit's entry points."""
    import ctypes as C
    import re
    import subprocess
    from pygemma_amd import _lib
    K = _lib.load_cc()
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.CC_HEADER).read(), flags=re.S)
    decl = re.findall(r"\b(pgx?_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert [name for name, _ in decl] == _lib.CC_SYMBOLS == ["pg_cc_work_bytes", "pg_cc_setup_dev", "pg_cc_pack_x_dev", "pg_cc_count_dev", "pg_cc_stats_dev"]
    for name, params in decl:
        assert len(getattr(K, name).argtypes) == params.count(",") + 1, name

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(("pg_", "pgx_"))}
    assert exported(_lib.CC_LIB_PATH) == set(_lib.CC_SYMBOLS)
    assert not exported(_lib.LIB_PATH) & set(_lib.CC_SYMBOLS)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    assert K.pg_cc_work_bytes.restype is C.c_size_t and K.pg_cc_work_bytes.argtypes == [i64, i32]
    assert K.pg_cc_count_dev.argtypes == [vp, i64, i64, vp, i64, i32, i32, vp, vp, vp, vp]
    assert K.pg_cc_pack_x_dev.argtypes == [vp, i64, i64, vp, i32, i64, i32, vp, i64, vp]
    assert K.pg_cc_work_bytes(37, 2) == 256 + 2 * 2 * 4 * 4 and K.pg_cc_work_bytes(0, 1) == 0 and K.pg_cc_work_bytes(37, 17) == 0
