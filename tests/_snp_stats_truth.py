"""NumPy / pure-Python truth for the SNP statistics (csrc/snp_stats.hip): shared by test_host_snp_stats.py and test_gpu_snp_stats.py,
not collected itself.

counts and moments follow the definitions of include/pygemma_hip.h: an element is rounded to float32 first, non-finite is missing, a
hard-call SNP takes mean and var from Python integers (one correctly rounded division each), any other SNP NumPy's fp64 mean / var of
the float32-rounded observed values.  The Hardy-Weinberg reference is the recurrence as the header defines it, in Python floats."""
import math
from fractions import Fraction

import numpy as np


def pack(G, pad_code=0):
    """(n, p) dosages (0/1/2 of the A2 allele, NaN = missing) -> (p, ceil(n/4)) packed .bed records; the pad calls after sample n - 1
    hold the 2-bit code `pad_code`."""
    G = np.asarray(G, np.float64)
    n, p = G.shape
    code = np.full(G.shape, 1, np.uint8)
    code[G == 0] = 0; code[G == 1] = 2; code[G == 2] = 3
    c = np.concatenate([code.T, np.full((p, (-n) % 4), pad_code, np.uint8)], axis=1).reshape(p, -1, 4)
    return np.ascontiguousarray((c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8))


def int_moments(n_obs, n1, n2):
    """(mean, var) of a hard-call SNP from Python ints: each one correctly rounded division of exact integers."""
    n_obs, n1, n2 = int(n_obs), int(n1), int(n2)
    S1, S2 = n1 + 2 * n2, n1 + 4 * n2
    return S1 / n_obs, (n_obs * S2 - S1 * S1) / (n_obs * n_obs)


def stats_truth(X):
    """X (n, p), any real dtype, NaN / Inf = missing.  Returns dict: counts (p, 4) int64 {n_miss, n0, n1, n2}; moments (p, 4) fp64
    {mean, var, min, max}; hard (p,) bool; absx, sqx (p,): mean |x| and mean x^2 of the observed values (the scale of the bounds)."""
    X = np.asarray(X)
    with np.errstate(over="ignore"):
        Xf = X.astype(np.float32).astype(np.float64)
    n, p = Xf.shape
    fin = np.isfinite(Xf)
    counts = np.stack([(~fin).sum(0), (fin & (Xf == 0)).sum(0), (fin & (Xf == 1)).sum(0), (fin & (Xf == 2)).sum(0)], axis=1).astype(np.int64)
    moments = np.full((p, 4), np.nan)
    hard = np.zeros(p, bool)
    absx, sqx = np.zeros(p), np.zeros(p)
    for j in range(p):
        nm, n0, n1, n2 = (int(v) for v in counts[j])
        n_obs = n - nm
        if n_obs == 0:
            continue
        x = Xf[fin[:, j], j]
        absx[j], sqx[j] = np.abs(x).mean(), (x * x).mean()
        if n0 + n1 + n2 == n_obs:
            hard[j] = True
            mean, var = int_moments(n_obs, n1, n2)
            moments[j] = (mean, var, 0.0 if n0 else (1.0 if n1 else 2.0), 2.0 if n2 else (1.0 if n1 else 0.0))
        else:
            moments[j] = (x.mean(), x.var(), x.min(), x.max())
    return {"counts": counts, "moments": moments, "hard": hard, "absx": absx, "sqx": sqx}


def _hwe_setup(n0, n1, n2):
    N = n0 + n1 + n2
    nr = 2 * min(n0, n2) + n1
    nc = 2 * N - nr
    mid = nr * nc // (2 * N)
    if (mid ^ nr) & 1:
        mid += 1
    return N, nr, mid


def hwe_terms(n0, n1, n2):
    """The unnormalised P(h) of the recurrence, in sweep order (mode, downward, upward): ([h], [P(h)])."""
    N, nr, mid = _hwe_setup(n0, n1, n2)
    hs, Ps = [mid], [1.0]
    P, a = 1.0, (nr - mid) // 2
    b = N - mid - a
    h = mid
    while h >= 2:
        P = P * (float(h) * float(h - 1)) / (4.0 * float(a + 1) * float(b + 1))
        hs.append(h - 2); Ps.append(P)
        a += 1; b += 1; h -= 2
    P, a = 1.0, (nr - mid) // 2
    b = N - mid - a
    h = mid
    while h <= nr - 2:
        P = P * (4.0 * float(a) * float(b)) / (float(h + 2) * float(h + 1))
        hs.append(h + 2); Ps.append(P)
        a -= 1; b -= 1; h += 2
    return hs, Ps


def _weight(N, nr, h):
    """The exact probability of h heterozygotes, up to the factor that does not depend on h."""
    a = (nr - h) // 2
    return Fraction(2 ** h, math.factorial(h) * math.factorial(a) * math.factorial(N - h - a))


def hwe_reference(n0, n1, n2):
    """(p, gap): the two-sided exact test by the recurrence, p = sum{P(h) <= P(n1)(1 + 2^-30)} / sum P(h) capped at 1 (NaN for N = 0,
    1.0 for a monomorphic SNP), and the smallest |P(h) / P(n1) - 1| over the terms h != n1 that are not exact (rational) ties of P(n1);
    inf when there is none."""
    n0, n1, n2 = int(n0), int(n1), int(n2)
    N = n0 + n1 + n2
    if N == 0:
        return float("nan"), float("inf")
    if 2 * min(n0, n2) + n1 == 0:
        return 1.0, float("inf")
    hs, Ps = hwe_terms(n0, n1, n2)
    Pobs = Ps[hs.index(n1)]
    thr = Pobs * (1.0 + 2.0 ** -30)
    total = tail = 0.0
    for P in Ps:
        total += P
    for P in Ps:
        if P <= thr:
            tail += P
    gap = float("inf")
    if Pobs > 0:
        nr = 2 * min(n0, n2) + n1
        for h, P in zip(hs, Ps):
            if h == n1:
                continue
            g = abs(P / Pobs - 1.0)
            if g < gap and not (g <= 2.0 ** -20 and _weight(N, nr, h) == _weight(N, nr, n1)):
                gap = g
    return min(1.0, tail / total), gap


def hwe_rational(n0, n1, n2):
    """The same p-value in exact rational arithmetic (ties are exact ties), rounded once at the end."""
    n0, n1, n2 = int(n0), int(n1), int(n2)
    N = n0 + n1 + n2
    nr = 2 * min(n0, n2) + n1
    w = {h: _weight(N, nr, h) for h in range(nr % 2, nr + 1, 2)}
    return float(sum(v for v in w.values() if v <= w[n1]) / sum(w.values()))
