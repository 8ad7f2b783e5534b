"""CPU-only checks of the epistasis scan's definition (tests/_epi_truth.py against a brute-force genotype table), of the host side of
lmm.epistasis (the p <-> chi2 cut, every refusal before device work) and of the new entry points' declarations."""
import math

import numpy as np
import pytest

import _epi_truth as E
import _ld_truth as T


def test_cells_are_the_folded_genotype_table():
    n, p = 40, 12
    G = T.ld_panel(n, p, 7, miss=0.15)
    g = E.group_vector(n, 3)
    assert (g == 1).sum() > 5 and (g == 0).sum() > 5 and (g == -1).sum() > 0
    S = E.sums(G, g)
    for k, val in enumerate((1, 0)):
        A, B, C, D = E.cells(S[..., 4 * k:4 * k + 4])
        brute = E.brute_cells(G, G, g, val)
        assert (np.stack([A, B, C, D], axis=-1) == brute).all()
        assert (brute.sum(axis=-1) == 4 * S[..., 4 * k]).all()          # four allele pairs per jointly called sample
    # two images: rows from one panel, columns from another
    G2 = T.ld_panel(n, 7, 9, miss=0.1, specials=False)
    S2 = E.sums(G, g, G2)
    assert (np.stack(E.cells(S2[..., :4]), axis=-1) == E.brute_cells(G, G2, g, 1)).all()


def test_z_is_bit_symmetric():
    n, p = 200, 30
    G = T.ld_panel(n, p, 11, miss=0.05)
    g = E.group_vector(n, 5)
    for case_only in (False, True):
        ok, z = E.z_of(E.sums(G, g), case_only)
        assert ok.sum() > 0.7 * p * p and (ok == ok.T).all()
        assert (z.view(np.uint64) == z.T.copy().view(np.uint64)).all()


def hand_pair(xa, xb, g, case_only=False):
    G = np.stack([np.asarray(xa, np.float64), np.asarray(xb, np.float64)], axis=1)
    S = E.sums(G, np.asarray(g))[0, 1]
    ok, z = E.z_of(S, case_only)
    return S, bool(ok), float(z)


def test_zero_cell_and_undefined_rules_on_hand_made_columns():
    g = [1] * 6 + [0] * 6
    xa = [0, 0, 1, 1, 2, 2] * 2
    xb = [0, 1, 0, 1, 2, 2] * 2
    S, ok, z = hand_pair(xa, xb, g)
    assert S.tolist() == [6, 6, 6, 9] * 2 and ok and z == 0.0          # the same table in both groups
    A, B, C, D = (int(c) for c in E.cells(S[:4]))
    assert (A, B, C, D) == (9, 3, 3, 9)
    okg, L, v = E.terms(S[:4])                                            # no zero cell: t = 2 cell
    assert okg and L == math.log((18.0 * 18.0) / (6.0 * 6.0)) and v == (2 / 18.0 + 2 / 18.0) + (2 / 6.0 + 2 / 6.0)
    # a zero cell: b is 0 wherever a is 0 and 2 wherever a is 2, no heterozygote -> B = C = 0; half a count goes to every cell
    S, ok, z = hand_pair([0, 0, 2, 2, 0, 2] * 2, [0, 0, 2, 2, 0, 2] * 2, g, case_only=True)
    A, B, C, D = (int(c) for c in E.cells(S[:4]))
    assert (A, B, C, D) == (12, 0, 0, 12) and ok
    assert z == math.log((25.0 * 25.0) / (1.0 * 1.0)) / math.sqrt((2 / 25.0 + 2 / 25.0) + (2 / 1.0 + 2 / 1.0))
    # monomorphic a (all 0): C + D = 0 -> undefined; all 2: A + B = 0
    assert not hand_pair([0] * 12, xb, g)[1] and not hand_pair([2] * 12, xb, g)[1]
    # all-missing and dosage columns are nobody's partner
    assert not hand_pair([np.nan] * 12, xb, g)[1]
    S, ok, _ = hand_pair([0.5, 1, 1, 0, 2, 1] * 2, xb, g)
    assert not ok and (S == 0).all()
    # an empty group: case/control undefined, case-only defined
    assert not hand_pair(xa, xb, [1] * 12)[1] and hand_pair(xa, xb, [1] * 12, case_only=True)[1]
    # monomorphic among the controls only: the pair is undefined for case/control, defined case-only
    xa2 = xa[:6] + [0] * 6
    assert not hand_pair(xa2, xb, g)[1] and hand_pair(xa2, xb, g, case_only=True)[1]
    # samples outside both groups do not count
    S, _, _ = hand_pair(xa, xb, [1] * 6 + [-1] * 6)
    assert S.tolist() == [6, 6, 6, 9, 0, 0, 0, 0]


def test_p_and_chi2_cut():
    from pygemma_amd import lmm
    for p in (0.5, 0.05, 1e-4, 5e-8, 1e-30):
        c = lmm._epi_chi2_min(p, None)
        z = math.sqrt(c)
        assert math.erfc(z / math.sqrt(2)) >= p > math.erfc(z * (1 + 1e-12) / math.sqrt(2))
    assert abs(lmm._epi_chi2_min(0.05, None) - 3.841458820694124) < 1e-9
    assert lmm._epi_chi2_min(1.0, None) == 0.0
    assert lmm._epi_chi2_min(lmm._EPI_P, 3.84) == 3.84 and lmm._epi_chi2_min(lmm._EPI_P, 0) == 0.0
    assert E.p_of(np.array([0.0]))[0] == 1.0


def test_refusals_fire_without_a_device(monkeypatch):
    from pygemma_amd import _lib, lmm

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "Context", no_device)
    n, p = 20, 6
    X = T.ld_panel(n, p, 1, specials=False).astype(np.float32)
    y = (np.arange(n) % 2).astype(np.float64)
    bad = [dict(y=y[:-1]), dict(y=np.where(np.arange(n) == 3, 2.0, y)), dict(y=np.where(np.arange(n) == 3, 0.5, y)), dict(y=np.zeros(n)),
           dict(y=np.full(n, np.nan)), dict(y=np.ones(n)), dict(y=np.array(["a"] * n)), dict(a=np.zeros(p, bool)), dict(b=[]), dict(a=[p]),
           dict(p=0.01, chi2=3.0), dict(p=1e-4, chi2=3.0), dict(p=0.0), dict(p=1.5), dict(p=-0.1), dict(p=float("nan")), dict(chi2=-1.0),
           dict(chi2=float("inf")), dict(snp_batch=0), dict(X=X[:, :0]), dict(X=X.ravel())]
    for kw in bad:
        args = dict(X=X, y=y)
        args.update(kw)
        with pytest.raises(ValueError):
            lmm.epistasis(args.pop("X"), args.pop("y"), **args)
    # all cases is fine for a case-only scan: it gets as far as the device
    with pytest.raises(AssertionError, match="device work"):
        lmm.epistasis(X, np.ones(n), case_only=True)
    with pytest.raises(AssertionError, match="device work"):
        lmm.epistasis(X, y.astype(bool), chi2=3.84)
    assert "epistasis" in lmm.__all__


def test_entry_points_are_declared_and_exported():
    from pygemma_amd import _lib
    L = _lib.load()
    for sym in ("pg_epi_image_bytes", "pg_epi_split_dev", "pg_epi_block_dev"):
        assert hasattr(L, sym) and sym in _lib.SYMBOLS
    assert L.pg_epi_image_bytes(0, 5) == 0 and L.pg_epi_image_bytes(5, 0) == 0 and L.pg_epi_image_bytes(1 << 28, 5) == 0
    assert L.pg_epi_image_bytes(129, 3) >= 6 * 3 * 256 + 3 * 20 and L.pg_epi_image_bytes(129, 3) % 16 == 0
