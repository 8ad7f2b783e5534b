"""The truth the epistasis tests compare against: NumPy integer arithmetic and fp64, written independently of pygemma_amd from the
definition in DESIGN §4.16.  Shared by test_host_epistasis.py and test_gpu_epistasis.py, not collected.

A panel is a float64 (n, p) matrix with NaN for a missing call (_ld_truth); a group vector holds 1 (case), 0 (control), anything else
(in neither).  For a pair (a, b) and a group the four sums N, Sa, Sb, Sab over the group's samples give the allele table
A = 4N - 2Sa - 2Sb + Sab, B = 2Sb - Sab, C = 2Sa - Sab, D = Sab."""
import math

import numpy as np

import _ld_truth as T


def group_vector(n, seed, out=0.1, cases=0.5):
    """A random int8 group vector with about `out` of the samples in neither group."""
    rng = np.random.default_rng(seed)
    g = (rng.random(n) < cases).astype(np.int8)
    g[rng.random(n) < out] = -1
    return g


def sums(GA, group, GB=None):
    """The eight sums of every pair (a of GA, b of GB) as an int64 (pa, pb, 8) array: N, Sa, Sb, Sab of the cases, then of the controls."""
    ma, xa, _ = T.planes(GA)
    mb, xb, _ = (ma, xa, None) if GB is None else T.planes(GB)
    group = np.asarray(group)
    out = []
    for val in (1, 0):
        k = (group == val).astype(np.int64)[:, None]
        out += [(ma * k).T @ mb, (xa * k).T @ mb, (ma * k).T @ xb, (xa * k).T @ xb]
    return np.stack(out, axis=-1)


def cells(S4):
    """The allele table (A, B, C, D) of an array (..., 4) of sums N, Sa, Sb, Sab."""
    S4 = np.asarray(S4, np.int64)
    N, Sa, Sb, Sab = (S4[..., t] for t in range(4))
    return 4 * N - 2 * Sa - 2 * Sb + Sab, 2 * Sb - Sab, 2 * Sa - Sab, Sab


def terms(S4):
    """(defined, L, v) of one group; L and v are 0 where the group is not defined."""
    A, B, C, D = cells(S4)
    ok = (A + B > 0) & (C + D > 0) & (A + C > 0) & (B + D > 0)
    z = ((A == 0) | (B == 0) | (C == 0) | (D == 0)).astype(np.int64)
    tA, tB, tC, tD = (np.where(ok, 2 * c + z, 1).astype(np.float64) for c in (A, B, C, D))
    L = np.log((tA * tD) / (tB * tC))
    v = (2.0 / tA + 2.0 / tD) + (2.0 / tB + 2.0 / tC)
    return ok, np.where(ok, L, 0.0), np.where(ok, v, 0.0)


def z_of(S8, case_only=False):
    """(defined, z) of an array (..., 8) of sums; z is NaN where the pair is not defined."""
    S8 = np.asarray(S8, np.int64)
    ok1, L1, v1 = terms(S8[..., :4])
    if case_only:
        ok, num, den = ok1, L1, v1
    else:
        ok0, L0, v0 = terms(S8[..., 4:])
        ok, num, den = ok1 & ok0, L1 - L0, v1 + v0
    z = num / np.sqrt(np.where(ok, den, 1.0))
    return ok, np.where(ok, z, np.nan)


def p_of(z):
    return np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in np.asarray(z, np.float64).ravel().tolist()]).reshape(np.shape(z))


def summary(ok, z, visit, chi2_min, ga, gb, size):
    """Hits and per-SNP summary of the visited pairs.  ok, z, visit: (pa, pb); ga, gb: the global index of every row and column SNP.
    Returns (hits as a sorted list of (a, b, z), n_tot, n_sig, best) with best the uint64 (float32 bits of chi2) << 32 | ~partner."""
    ok = ok & visit
    chi2 = np.where(ok, z * z, 0.0)
    hit = ok & (chi2 >= chi2_min)
    n_tot, n_sig, best = np.zeros(size, np.int64), np.zeros(size, np.int64), np.zeros(size, np.uint64)
    np.add.at(n_tot, ga, ok.sum(axis=1)); np.add.at(n_tot, gb, ok.sum(axis=0))
    np.add.at(n_sig, ga, hit.sum(axis=1)); np.add.at(n_sig, gb, hit.sum(axis=0))
    bits = chi2.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)
    inv = lambda g: (~np.asarray(g, np.int64)).astype(np.uint32).astype(np.uint64)
    ka = np.where(ok, bits | inv(gb)[None, :], 0).astype(np.uint64)          # what the row SNP sees of its partners
    kb = np.where(ok, bits | inv(ga)[:, None], 0).astype(np.uint64)
    np.maximum.at(best, ga, ka.max(axis=1, initial=0)); np.maximum.at(best, gb, kb.max(axis=0, initial=0))
    ia, ib = np.nonzero(hit)
    hits = sorted(zip(np.asarray(ga)[ia].tolist(), np.asarray(gb)[ib].tolist(), z[ia, ib].tolist()))
    return hits, n_tot, n_sig, best


def near_cut(ok, z, visit, chi2_min, eps=1e-9):
    """How many visited, defined pairs have chi2 within eps of the cut."""
    return int((ok & visit & (np.abs(np.where(ok, z * z, np.inf) - chi2_min) <= eps)).sum())


def brute_cells(GA, GB, group, val):
    """The allele table of every pair by the 3 x 3 genotype table of the samples of group `val` called at both SNPs, folded to alleles:
    a sample with genotypes (i, j) holds (2 - i)(2 - j), (2 - i) j, i (2 - j), i j allele pairs.  Plain loops."""
    n, pa = GA.shape
    out = np.zeros((pa, GB.shape[1], 4), np.int64)
    hard = lambda col: all((not np.isfinite(v)) or v in (0.0, 1.0, 2.0) for v in col)
    for a in range(pa):
        for b in range(GB.shape[1]):
            if not (hard(GA[:, a]) and hard(GB[:, b])):
                continue
            tab = np.zeros((3, 3), np.int64)
            for s in range(n):
                if group[s] == val and np.isfinite(GA[s, a]) and np.isfinite(GB[s, b]):
                    tab[int(GA[s, a]), int(GB[s, b])] += 1
            for i in range(3):
                for j in range(3):
                    out[a, b] += tab[i, j] * np.array([(2 - i) * (2 - j), (2 - i) * j, i * (2 - j), i * j])
    return out
