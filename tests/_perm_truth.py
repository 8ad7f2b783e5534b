"""The truth of the permutation tests (lmm.case_control_perm, csrc/perm.hip): the sums by boolean masks, the two statistics in Python
integers (one correctly rounded division at the end: int / int in Python rounds once) and as fractions.Fraction, a replay of the
device's documented operation order in NumPy fp64 for the bit-level checks, and the two reductions.  Pure NumPy / Python: imported by
the host and the GPU tests."""
from fractions import Fraction

import numpy as np

ALLELIC, TREND = 0, 1
U = 2.0 ** -53


def hard_calls(G):
    G = np.asarray(G, np.float64)
    return ((G == 0) | (G == 1) | (G == 2) | ~np.isfinite(G)).all(axis=0)


def planes(G):
    """x, m (n, p) int64 of dosages G: a missing call (NaN, inf) has x = m = 0, a SNP that is not hard-call is all missing."""
    G = np.asarray(G, np.float64)
    m = np.isfinite(G) & hard_calls(G)[None, :]
    return np.where(m, G, 0).astype(np.int64), m.astype(np.int64)


def totals(G, study):
    """(p, 4) int64 {At, Nc, Q, flag} over the study samples; flag bit 0: a study sample is uncalled, bit 1: not hard-call."""
    x, m = planes(G)
    s = np.asarray(study).astype(np.int64)
    At, Nc, Q = s @ x, s @ m, s @ (x * x)
    flag = (Nc != s.sum()).astype(np.int64) | (2 * (~hard_calls(G)).astype(np.int64))
    return np.stack([At, Nc, Q, flag], axis=1)


def sums(G, labels):
    """a, R (p, nb) int64 of the labellings (nb, n)."""
    x, m = planes(G)
    lab = np.asarray(labels).astype(np.int64)
    return (lab @ x).T.copy(), (lab @ m).T.copy()


def _parts(test, At, Nc, Q, a, R):
    """(num, den, defined) of the statistic as exact integers (object arrays of Python ints), broadcast over (p, nb)."""
    At, Nc, Q = (np.asarray(v, np.int64).astype(object)[:, None] for v in (At, Nc, Q))
    a, R = np.asarray(a, np.int64).astype(object), np.asarray(R, np.int64).astype(object)
    ok = (R > 0) & (R < Nc)
    if test == ALLELIC:
        b, c = 2 * R - a, At - a
        d = 2 * (Nc - R) - c
        r1, r2, c1, c2 = a + b, c + d, a + c, b + d
        num, den = (r1 + r2) * (a * d - b * c) ** 2, r1 * r2 * c1 * c2
    else:
        num, den = Nc * (Nc * a - R * At) ** 2, R * (Nc - R) * (Nc * Q - At * At)
    ok = ok & (den != 0)
    return num, den, ok.astype(bool)


def exact(test, At, Nc, Q, a, R):
    """The statistic, each value the exact rational rounded once to fp64; NaN where it is not defined."""
    num, den, ok = _parts(test, At, Nc, Q, a, R)
    out = np.full(ok.shape, np.nan)
    out[ok] = [int(u) / int(v) for u, v in zip(num[ok], den[ok])]
    return out


def exact_fraction(test, At, Nc, Q, a, R):
    """One (SNP, labelling) as a Fraction; None when not defined."""
    num, den, ok = _parts(test, [At], [Nc], [Q], [[a]], [[R]])
    return Fraction(int(num[0, 0]), int(den[0, 0])) if ok[0, 0] else None


def replay(test, At, Nc, Q, a, R):
    """The device's operation order in NumPy fp64: int64 arithmetic, one conversion of every exact integer, one rounding per * and /."""
    At, Nc, Q = (np.asarray(v, np.int64)[:, None] for v in (At, Nc, Q))
    a, R = np.asarray(a, np.int64), np.asarray(R, np.int64)
    f = lambda v: np.asarray(v, np.int64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if test == ALLELIC:
            b, c = 2 * R - a, At - a
            d = 2 * (Nc - R) - c
            r1, r2, c1, c2 = a + b, c + d, a + c, b + d
            D = f(a * d - b * c)
            v = (f(r1 + r2) * (D * D)) / (f(r1 * r2) * f(c1 * c2))
            bad = (r1 == 0) | (r2 == 0) | (c1 == 0) | (c2 == 0)
        else:
            Uf, Vi = f(Nc * a - R * At), Nc * Q - At * At
            v = (f(Nc) * (Uf * Uf)) / (f(R * (Nc - R)) * f(Vi))
            bad = Vi == 0
    return np.where(bad | (R <= 0) | (R >= Nc), np.nan, v)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def within(v, truth, ulps=15.5):
    """Same NaN pattern, and |v - truth| <= ulps u |truth|.  `truth` is the exact value rounded once (1/2 u), so 15.5 u here is inside
    the 16 u gate against the exact value."""
    v, truth = np.asarray(v, np.float64), np.asarray(truth, np.float64)
    with np.errstate(invalid="ignore"):
        return (np.isnan(v) == np.isnan(truth)) & (np.isnan(truth) | (np.abs(v - truth) <= ulps * U * np.abs(truth)))


def reduce(dense, obs):
    """(n_ge (p,) int64, max_null (nb,) fp64) of a (p, nb) block of statistics against obs (p,): NaN never counts, the maximum skips NaN
    and is 0 where nothing is defined."""
    with np.errstate(invalid="ignore"):
        n_ge = (dense >= np.asarray(obs)[:, None]).sum(axis=1).astype(np.int64)
    mx = np.where(np.isnan(dense), 0.0, dense).max(axis=0) if dense.shape[0] else np.zeros(dense.shape[1])
    return n_ge, mx


def emp2(max_null, chi2):
    """(#{b: max_null[b] >= chi2} + 1) / (nperm + 1) by the definition, one SNP at a time; NaN where chi2 is."""
    mx = np.asarray(max_null, np.float64)
    return np.array([np.nan if np.isnan(c) else (int((mx >= c).sum()) + 1) / (mx.size + 1) for c in np.asarray(chi2, np.float64)])
