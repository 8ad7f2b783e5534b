"""The truth the LD score tests compare against, on top of _ld_truth: NumPy int64 and float64, written independently of pygemma_amd.

A pair's value is the kernel's by definition (include/pygemma_hip.h, pg_ld_score_dev): from the exact int64 ca, cb, cab of its six
sums, in float64 with one rounding per operation,
    r2 = min((cab cab) / (ca cb), 1);   with adjust  r2 = r2 - (1 - r2) / (N - 2);   q = rint(r2 2^32)
for a pair with ca > 0, cb > 0 (and N > 2 with adjust).  int64 -> float64, multiply, divide, subtract and round-to-nearest-even are
correctly rounded on the host and on the device, and the per-SNP sums are integers: the tests compare for EQUALITY."""
import numpy as np

import _ld_truth as T

ONE = 2.0 ** 32


def pair_terms(S, adjust):
    """(defined, r2) of an array (..., 6) of sums: the boolean mask of the pairs that count and their float64 r2 (0 elsewhere)."""
    S = np.asarray(S, np.int64)
    N, Sa, Sb, Saa, Sbb, Sab = (S[..., t] for t in range(6))
    ca, cb, cab = N * Saa - Sa * Sa, N * Sbb - Sb * Sb, N * Sab - Sa * Sb
    ok = (ca > 0) & (cb > 0)
    if adjust:
        ok &= N > 2
    num = cab.astype(np.float64) * cab.astype(np.float64)
    den = np.where(ok, ca, 1).astype(np.float64) * np.where(ok, cb, 1).astype(np.float64)
    r2 = np.minimum(num / den, 1.0)
    if adjust:
        r2 = r2 - (1.0 - r2) / np.where(ok, N - 2, 1).astype(np.float64)
    return ok, np.where(ok, r2, 0.0)


def pair_q(S, adjust):
    """(defined, q): q = rint(r2 2^32) as int64, 0 where the pair is undefined."""
    ok, r2 = pair_terms(S, adjust)
    return ok, np.rint(r2 * ONE).astype(np.int64)


def forward_mask(p, j0, rows, have, w, reach=None):
    """visit[j, i]: row j in [j0, j0 + rows) meets partner i = j + 1 + k, 0 <= k < min(w, reach[j]), i < have."""
    j, i = np.arange(p)[:, None], np.arange(p)[None, :]
    lim = np.full(p, w, np.int64) if reach is None else np.minimum(w, np.asarray(reach, np.int64))
    k = i - j - 1
    return (j >= j0) & (j < j0 + rows) & (k >= 0) & (k < lim[:, None]) & (i < have)


def credit(S, visit, adjust):
    """(sum int64 (p,), npairs int64 (p,), share of the visited pairs that are undefined): every visited defined pair (j, i) adds its q
    to both j and i."""
    ok, q = pair_q(S, adjust)
    take = visit & ok
    qt = np.where(take, q, 0)
    tot = qt.sum(axis=1) + qt.sum(axis=0)
    cnt = take.sum(axis=1) + take.sum(axis=0)
    return tot, cnt.astype(np.int64), 1.0 - take.sum() / max(1, visit.sum())


def credit_float(S, visit, adjust):
    """The same sum without the fixed point: float64 r2 added in float64."""
    ok, r2 = pair_terms(S, adjust)
    rt = np.where(visit & ok, r2, 0.0)
    return rt.sum(axis=1) + rt.sum(axis=0)


def nobs(G):
    """Called samples of every SNP whose own variance term is positive, else 0 (monomorphic, all missing, not hard-call)."""
    m, x, x2 = T.planes(G)
    nm, s1, s2 = m.sum(axis=0), x.sum(axis=0), x2.sum(axis=0)
    return np.where(nm * s2 - s1 * s1 > 0, nm, 0).astype(np.int64)


def window_mask(p, window, pos=None, chrom=None):
    """visit[j, i] for i > j by the definition of the window: |i - j| <= window, or |pos_i - pos_j| <= window, on one chromosome."""
    coord = np.arange(p, dtype=np.float64) if pos is None else np.asarray(pos, np.float64)
    near = np.abs(coord[:, None] - coord[None, :]) <= window
    if chrom is not None:
        chrom = np.asarray(chrom)
        near &= chrom[:, None] == chrom[None, :]
    return near & (np.arange(p)[None, :] > np.arange(p)[:, None])


def l2_of(tot, no):
    return np.where(no > 0, 1.0 + tot / ONE, np.nan)
