"""NumPy fp64 model of the principal components (csrc/pca.hip, lmm.pca): shared by test_host_pca.py and test_gpu_pca.py, not collected
itself.

Values follow include/pygemma_hip.h: an element is rounded to float32 first, non-finite (and .bed code 01) is missing; stat holds
{mu_g, isd_g} with mu_g the mean _snp_stats_truth.stats_truth defines (0 without a called sample), v = var_g (n_obs / n) and
isd_g = 1 / sqrt(v) where v > 0, else 0; z_gi = fl(fl(x_gi - mu_g) isd_g), two roundings, 0 for a missing call.  proj and back are
plain products; the driver is lmm.pca's, with the same orth (Householder QR, diagonal of R positive) and the same sign rule."""
from types import SimpleNamespace

import numpy as np

import _prs_truth as P
import _snp_stats_truth as ST

decode = P.decode


def stat_rule(n, counts, moments):
    """stat (p, 2) from the (p, 4) counts {n_miss, ...} and moments {mean, var, ...} of a QC pass over n samples."""
    n_obs = n - np.asarray(counts)[:, 0].astype(np.int64)
    mean, var = np.asarray(moments)[:, 0], np.asarray(moments)[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        v = var * (n_obs.astype(np.float64) / np.float64(n))
        isd = np.where(v > 0, 1.0 / np.sqrt(np.where(v > 0, v, 1.0)), 0.0)
    return np.ascontiguousarray(np.stack([np.where(n_obs > 0, mean, 0.0), isd], axis=1))


def stat(X):
    """stat (p, 2) of a PackedBed or an array, from the QC truth."""
    V, miss = decode(X)
    st = ST.stats_truth(np.where(miss, np.nan, V))
    return stat_rule(V.shape[0], st["counts"], st["moments"])


def z(X, st):
    """The (n, p) standardised matrix: (x - mu) and the product with isd rounded separately, 0 where the call is missing."""
    V, miss = decode(X)
    d = V - st[None, :, 0]
    return np.where(miss, 0.0, d * st[None, :, 1])


def proj(Z, Q):
    """T (p, l) = Z'Q."""
    return Z.T @ Q


def back(Z, T):
    """Y (n, l) = Z T."""
    return Z @ T


def orth(A):
    """Householder QR of A (n, l) with the diagonal of R made positive: the orthonormal factor."""
    Q, R = np.linalg.qr(A)
    s = np.where(np.diagonal(R) < 0, -1.0, 1.0)
    return Q * s[None, :]


def fix_signs(U):
    """Every column's entry of largest magnitude made positive."""
    U = np.array(U)
    for j in range(U.shape[1]):
        if U[np.argmax(np.abs(U[:, j])), j] < 0:
            U[:, j] = -U[:, j]
    return U


def pca(X, k=10, oversample=10, iters=12, tol=1e-10, seed=0, loadings=True):
    """lmm.pca's driver on the host: namespace with pcs (n, k), eigenvalues (k,), explained (k,), loadings (p, k) or None, stat (p, 2),
    ritz (all l Ritz values of the last pass, descending), passes, converged and Z."""
    st = stat(X)
    Z = z(X, st)
    n, p = Z.shape
    l = min(k + oversample, 64, n)
    Q = orth(np.random.default_rng(seed).standard_normal((n, l)))
    prev, converged = None, False
    for it in range(iters):
        Y = back(Z, proj(Z, Q)) / p
        B = Q.T @ Y
        w, V = np.linalg.eigh((B + B.T) / 2)
        w, V = w[::-1], V[:, ::-1]
        passes = it + 1
        if prev is not None and np.max(np.abs(w[:k] - prev[:k])) < tol * abs(w[0]):
            converged = True
            break
        prev = w
        if it + 1 < iters:
            Q = orth(Y)
    pcs = fix_signs(Q @ V[:, :k])
    lam = w[:k].copy()
    p_used = int((st[:, 1] > 0).sum())
    L = proj(Z, pcs) / (p * lam)[None, :] if loadings else None
    return SimpleNamespace(pcs=pcs, eigenvalues=lam, explained=lam / (n * p_used / p), loadings=L, stat=st, ritz=w, passes=passes,
                           converged=converged, Z=Z)


def project(X_new, res):
    """lmm.pca_project's values: Z_new L with the training panel's stat."""
    return back(z(X_new, res.stat), res.loadings)


def panel(n, p, seed=0, fst=0.1, missing=0.02):
    """(n, p) hard calls 0/1/2 as float64 with NaN for a missing call: three Balding-Nichols populations of n // 3 (+ remainder) samples,
    ancestral frequencies U(0.1, 0.9), population frequencies Beta(f (1 - F) / F, (1 - f)(1 - F) / F)."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.1, 0.9, p)
    a = (1 - fst) / fst
    pop = np.arange(n) * 3 // n
    freq = rng.beta(f * a, (1 - f) * a, (3, p))
    G = rng.binomial(2, freq[pop]).astype(np.float64)
    G[rng.random((n, p)) < missing] = np.nan
    return G
