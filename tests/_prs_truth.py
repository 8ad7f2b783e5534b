"""NumPy / pure-Python truth for the polygenic scores (csrc/prs.hip): shared by test_host_prs.py and test_gpu_prs.py, not collected
itself.

Values follow include/pygemma_hip.h: an element is rounded to float32 first, non-finite (and .bed code 01) is missing; a missing call
is 0, or with impute the mean of its SNP as _snp_stats_truth.stats_truth defines it (one exact division for a hard-call SNP, NumPy's
fp64 mean of the observed values otherwise), and every call of an all-missing SNP is 0.  Scores are the product in np.longdouble where
that has 63 mantissa bits or more, math.fsum per element elsewhere; counts an integer product."""
import math

import numpy as np

import _snp_stats_truth as ST

WIDE = np.finfo(np.longdouble).nmant >= 63


def decode(X):
    """(values (n, p) fp64 with 0 where missing, missing (n, p) bool) of a PackedBed or an int8, uint8, float32 or float64 array."""
    if hasattr(X, "to_float"):
        V = X.to_float(impute=False).astype(np.float64)
    else:
        with np.errstate(over="ignore"):
            V = np.asarray(X).astype(np.float32).astype(np.float64)
    miss = ~np.isfinite(V)
    return np.where(miss, 0.0, V), miss


def means(V, miss):
    """(mu (p,) fp64, NaN for an all-missing SNP; hard (p,) bool) of decoded values: the `mean` column and the hard-call rule of snp_stats."""
    st = ST.stats_truth(np.where(miss, np.nan, V))
    return st["moments"][:, 0].copy(), st["hard"].copy()


def filled(V, miss, impute):
    """The (n, p) fp64 matrix the score multiplies: missing calls 0, or with impute their SNP's mean (0 for an all-missing SNP)."""
    if not impute:
        return V.copy()
    mu = means(V, miss)[0]
    return np.where(miss, np.where(np.isnan(mu), 0.0, mu)[None, :], V)


def _two_prod(a, b):
    """a * b as an unevaluated sum of two floats (Dekker's product on Veltkamp splits): exact short of overflow."""
    p = a * b
    c = 134217729.0 * a
    ah = c - (c - a)
    al = a - ah
    c = 134217729.0 * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def product(A, B, wide=None):
    """A @ B of fp64 matrices to well below an fp64 ulp: np.longdouble where it is wider than fp64 (`wide`, by default WIDE), else
    math.fsum per element over the exact two-float products: one rounding."""
    if WIDE if wide is None else wide:
        return (A.astype(np.longdouble) @ B.astype(np.longdouble)).astype(np.float64)
    out = np.empty((A.shape[0], B.shape[1]))
    for i in range(A.shape[0]):
        for k in range(B.shape[1]):
            terms = []
            for a, b in zip(A[i].tolist(), B[:, k].tolist()):
                terms += _two_prod(a, b)
            out[i, k] = math.fsum(terms)
    return out


def scores(X, W, impute):
    """Truth of one call on the whole of X: dict with score (t, n) fp64, called (t, n) int64, mag (t, n) = sum_g |x_gi||w_gk|, and for
    the bound of the imputed entries soft (t, n) = sum over imputed entries of SNPs that are not hard-call of |mu_g||w_gk|."""
    W = np.asarray(W, np.float64)
    V, miss = decode(X)
    x = filled(V, miss, impute)
    mu, hard = means(V, miss)
    out = {"score": product(x, W).T, "called": ((W != 0).T.astype(np.int64) @ (~miss).T.astype(np.int64)),
           "mag": (np.abs(x) @ np.abs(W)).T}
    soft_mu = np.where(hard | np.isnan(mu), 0.0, np.abs(mu))
    out["soft"] = ((miss * soft_mu[None, :]) @ np.abs(W)).T if impute else np.zeros_like(out["mag"])
    out["x"] = x
    return out


def bound(tr, n, pb):
    """|score - truth| allowed: (pb + 8) 2^-53 sum_g |x_gi||w_gk|, the bound of an fp64 sum of pb products in any order with room for the
    chunk additions, plus 4 n 2^-53 |mu_g||w_gk| for every imputed entry of a SNP whose mean is a rounded fp64 sum (test_gpu_snp_stats.py)."""
    u = 2.0 ** -53
    return (pb + 8) * u * tr["mag"] + 4 * n * u * tr["soft"]
