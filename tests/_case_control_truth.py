"""The truth of the case/control tests (lmm.case_control, csrc/case_control.hip): counts with boolean masks, every statistic in Python
integers and fractions.Fraction up to the last division (float(Fraction) rounds once, correctly), and a replay of the device's
documented operation order in NumPy fp64 for the bit-level checks.  Pure NumPy / Python: imported by the host and the GPU tests."""
import math
from fractions import Fraction

import numpy as np

NAN = float("nan")
STAT = ("af_case", "af_ctrl", "or", "chi2_allelic", "chi2_trend", "chi2_geno", "chi2_dom", "chi2_rec")


def pack(G, pad_code=0):
    """(n, p) dosages of the counted allele (0, 1, 2; anything else: missing) -> (p, ceil(n/4)) .bed records, 0 -> 00, 1 -> 10, 2 -> 11,
    missing -> 01, the pad calls of the last byte holding pad_code."""
    G = np.asarray(G, np.float64)
    n, p = G.shape
    code = np.full(G.shape, 1, np.uint8)
    code[G == 0] = 0; code[G == 1] = 2; code[G == 2] = 3
    c = np.concatenate([code.T, np.full((p, (-n) % 4), pad_code, np.uint8)], axis=1).reshape(p, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def hard_calls(G):
    """Per SNP: every observed (finite) value is exactly 0, 1 or 2.  An all-missing SNP is hard-call."""
    G = np.asarray(G, np.float64)
    return ((G == 0) | (G == 1) | (G == 2) | ~np.isfinite(G)).all(axis=0)


def tables(G, status, stratum=None, S=1):
    """(p, S, 8) int64 {case0, case1, case2, case_miss, ctrl0, ctrl1, ctrl2, ctrl_miss} per stratum, by boolean masks.  status: 1 case,
    0 control, anything else neither; stratum: 0..S-1, anything else excluded (None: everyone in stratum 0).  A SNP that is not
    hard-call has every count 0."""
    G = np.asarray(G, np.float64)
    n, p = G.shape
    status = np.asarray(status)
    stratum = np.zeros(n, np.int64) if stratum is None else np.asarray(stratum)
    out = np.zeros((p, S, 8), np.int64)
    miss = ~np.isfinite(G)
    for k in range(S):
        for col, st in ((0, 1), (4, 0)):
            m = (status == st) & (stratum == k)
            for v in range(3):
                out[:, k, col + v] = ((G == v) & m[:, None]).sum(axis=0)
            out[:, k, col + 3] = (miss & m[:, None]).sum(axis=0)
    out[~hard_calls(G)] = 0
    return out


def allelic(t):
    """The allelic 2 x 2 table (a, b, c, d) of one row of 8 counts, as Python ints."""
    r0, r1, r2, _, s0, s1, s2, _ = (int(v) for v in t)
    R, Sp = r0 + r1 + r2, s0 + s1 + s2
    a, c = r1 + 2 * r2, s1 + 2 * s2
    return a, 2 * R - a, c, 2 * Sp - c


def chi2_2x2(a, b, c, d):
    """T (a d - b c)^2 / (r1 r2 c1 c2) as a Fraction; None when a margin is 0."""
    r1, r2, c1, c2 = a + b, c + d, a + c, b + d
    if 0 in (r1, r2, c1, c2):
        return None
    return Fraction((r1 + r2) * (a * d - b * c) ** 2, r1 * r2 * c1 * c2)


def trend(t):
    """Cochran-Armitage, weights 0, 1, 2: N (N A_case - R A_tot)^2 / (R S' (N (n1 + 4 n2) - A_tot^2)); None when the divisor is 0."""
    r0, r1, r2, _, s0, s1, s2, _ = (int(v) for v in t)
    R, Sp = r0 + r1 + r2, s0 + s1 + s2
    N, n1, n2 = R + Sp, r1 + s1, r2 + s2
    A, At = r1 + 2 * r2, n1 + 2 * n2
    den = R * Sp * (N * (n1 + 4 * n2) - At * At)
    return Fraction(N * (N * A - R * At) ** 2, den) if den else None


def trend_textbook(t):
    """The same test as statistic^2 / variance: T = sum w_i (r_i S' - s_i R), Var = R S' / N (sum w_i^2 n_i (N - n_i) - 2 sum_{i<j} w_i
    w_j n_i n_j) (Agresti, Categorical Data Analysis, 5.3.5)."""
    r, s, w = [int(v) for v in t[:3]], [int(v) for v in t[4:7]], (0, 1, 2)
    R, Sp = sum(r), sum(s)
    N, nn = R + Sp, [r[i] + s[i] for i in range(3)]
    T = sum(w[i] * (r[i] * Sp - s[i] * R) for i in range(3))
    var = Fraction(R * Sp, N) * (sum(w[i] ** 2 * nn[i] * (N - nn[i]) for i in range(3))
                                 - 2 * sum(w[i] * w[j] * nn[i] * nn[j] for i in range(3) for j in range(i + 1, 3)))
    return Fraction(T * T) / var if var else None


def geno(t):
    """The 2 x 3 chi2 as the sum of its six cells (O - E)^2 / E; None when a genotype is unseen."""
    r, s = [int(v) for v in t[:3]], [int(v) for v in t[4:7]]
    R, Sp = sum(r), sum(s)
    N, nn = R + Sp, [r[i] + s[i] for i in range(3)]
    if 0 in nn:
        return None
    tot = Fraction(0)
    for obs, G in ((r, R), (s, Sp)):
        for i in range(3):
            E = Fraction(G * nn[i], N)
            tot += (obs[i] - E) ** 2 / E
    return tot


def cmh(strata_tables):
    """The exact CMH sums over the (S, 8) tables of one SNP: (u, v, sum a d / T, sum b c / T, sum |u_k|, strata that contribute)."""
    u = v = sad = sbc = absu = Fraction(0)
    used = 0
    for t in strata_tables:
        a, b, c, d = allelic(t)
        r1, r2, c1, c2 = a + b, c + d, a + c, b + d
        T = r1 + r2
        if r1 == 0 or r2 == 0:
            continue
        used += 1
        term = a - Fraction(r1 * c1, T)
        u += term; absu += abs(term)
        v += Fraction(r1 * r2 * c1 * c2, T * T * (T - 1))
        sad += Fraction(a * d, T); sbc += Fraction(b * c, T)
    return u, v, sad, sbc, absu, used


def fisher(a, b, c, d):
    """The two-sided Fisher exact test of a 2 x 2 table in exact rationals: (p as a Fraction, the smallest relative gap |P(x) - P(obs)| /
    P(obs) over the terms that are no exact tie — inf without one —, the number of recurrence steps = the smallest margin)."""
    r1, c1, T = a + b, a + c, a + b + c + d
    lo, hi = max(0, r1 + c1 - T), min(r1, c1)
    w = [math.comb(c1, x) * math.comb(T - c1, r1 - x) for x in range(lo, hi + 1)]
    obs = w[a - lo]
    gap = min([Fraction(abs(v - obs), obs) for v in w if v != obs], default=math.inf)
    return Fraction(sum(v for v in w if v <= obs), sum(w)), gap, hi - lo


def _f(x):
    return NAN if x is None else float(x)


def truth(tab):
    """Every statistic of a (p, S, 8) table array, exact up to the last rounding: a dict of (p,) arrays — the pooled counts, STAT,
    p_fisher, fisher_gap, fisher_steps, cmh_u, cmh_v, chi2_cmh, or_mh, cmh_abs (sum |u_k|) — with the NaN rules of lmm.case_control."""
    p = tab.shape[0]
    pooled = tab.sum(axis=1)
    out = {k: np.full(p, NAN) for k in STAT + ("p_fisher", "cmh_u", "cmh_v", "chi2_cmh", "or_mh", "cmh_abs")}
    out["fisher_gap"], out["fisher_steps"] = np.full(p, math.inf), np.zeros(p, np.int64)
    out["counts"] = pooled
    for g in range(p):
        t = pooled[g]
        r0, r1, r2, _, s0, s1, s2, _ = (int(v) for v in t)
        R, Sp = r0 + r1 + r2, s0 + s1 + s2
        if R == 0 or Sp == 0:
            continue
        a, b, c, d = allelic(t)
        out["af_case"][g], out["af_ctrl"][g] = float(Fraction(a, 2 * R)), float(Fraction(c, 2 * Sp))
        out["or"][g] = float(Fraction(a * d, b * c)) if b * c else (math.inf if a * d else NAN)
        out["chi2_allelic"][g] = _f(chi2_2x2(a, b, c, d))
        out["chi2_trend"][g] = _f(trend(t))
        out["chi2_geno"][g] = _f(geno(t))
        out["chi2_dom"][g] = _f(chi2_2x2(r1 + r2, r0, s1 + s2, s0))
        out["chi2_rec"][g] = _f(chi2_2x2(r2, r0 + r1, s2, s0 + s1))
        pf, gap, steps = fisher(a, b, c, d)
        out["p_fisher"][g], out["fisher_gap"][g], out["fisher_steps"][g] = float(pf), float(gap), steps
        u, v, sad, sbc, absu, _ = cmh(tab[g])
        out["cmh_u"][g], out["cmh_v"][g], out["cmh_abs"][g] = float(u), float(v), float(absu)
        out["chi2_cmh"][g] = float(u * u / v) if v else NAN
        out["or_mh"][g] = float(sad / sbc) if sbc else NAN
    return out


# ---- the device's operation order in NumPy fp64 (csrc/case_control.hip, header comment) ------------------------------------------------
def _d(x):
    return np.asarray(x, np.int64).astype(np.float64)              # one conversion, round to nearest even


def _replay_2x2(a, b, c, d):
    r1, r2, c1, c2 = a + b, c + d, a + c, b + d
    D = _d(a * d - b * c)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (_d(r1 + r2) * (D * D)) / (_d(r1 * r2) * _d(c1 * c2))
    return np.where((r1 == 0) | (r2 == 0) | (c1 == 0) | (c2 == 0), NAN, x)


def replay_cmh(tab):
    """(p, 4) fp64 {u, v, sum a d / T, sum b c / T} as pg_cc_count_dev adds them: strata in order, one conversion and one division per
    term; NaN rows without a called case or control."""
    p, S, _ = tab.shape
    acc = np.zeros((p, 4))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(S):
            t = tab[:, k].astype(np.int64)
            R, Sp = t[:, :3].sum(axis=1), t[:, 4:7].sum(axis=1)
            a, c = t[:, 1] + 2 * t[:, 2], t[:, 5] + 2 * t[:, 6]
            b, d = 2 * R - a, 2 * Sp - c
            m1, m2, k1, k2 = a + b, c + d, a + c, b + d
            T = m1 + m2
            use = (R > 0) & (Sp > 0)
            terms = [_d(a * T - m1 * k1) / _d(T), (_d(m1 * m2) * _d(k1 * k2)) / (_d(T * T) * _d(T - 1)), _d(a * d) / _d(T), _d(b * c) / _d(T)]
            for j, term in enumerate(terms):
                acc[:, j] = acc[:, j] + np.where(use, term, 0.0)
    pooled = tab.sum(axis=1)
    acc[(pooled[:, :3].sum(axis=1) == 0) | (pooled[:, 4:7].sum(axis=1) == 0)] = NAN
    return acc


def replay_fisher(a, b, c, d):
    """One table through the two sweeps of cc_fisher, in Python floats (IEEE fp64)."""
    r1, c1, T = a + b, a + c, a + b + c + d
    lo, hi, off = max(0, r1 + c1 - T), min(r1, c1), T - r1 - c1
    mode = min(max((r1 + 1) * (c1 + 1) // (T + 2), lo), hi)
    terms = [(mode, 1.0)]
    P = 1.0
    for x in range(mode, lo, -1):
        P = P * float(x * (off + x)) / float((r1 - x + 1) * (c1 - x + 1))
        terms.append((x - 1, P))
    P = 1.0
    for x in range(mode, hi):
        P = P * float((r1 - x) * (c1 - x)) / float((x + 1) * (off + x + 1))
        terms.append((x + 1, P))
    total = 0.0
    for _, P in terms:
        total += P
    thr = dict(terms)[a] * (1.0 + 2.0 ** -30)
    tail = 0.0
    for _, P in terms:
        if P <= thr:
            tail += P
    return min(tail / total, 1.0)


def replay(tab, fisher_p=True):
    """(p, 11) fp64 as pg_cc_stats_dev writes them, from the replayed CMH sums: af_case, af_ctrl, or, chi2_allelic, chi2_trend, chi2_geno,
    chi2_dom, chi2_rec, p_fisher, chi2_cmh, or_mh."""
    t = tab.sum(axis=1).astype(np.int64)
    p = t.shape[0]
    r0, r1, r2, s0, s1, s2 = t[:, 0], t[:, 1], t[:, 2], t[:, 4], t[:, 5], t[:, 6]
    R, Sp = r0 + r1 + r2, s0 + s1 + s2
    N, n0, n1, n2 = R + Sp, r0 + s0, r1 + s1, r2 + s2
    a, c = r1 + 2 * r2, s1 + 2 * s2
    b, d, At = 2 * R - a, 2 * Sp - c, a + c
    o = np.full((p, 11), NAN)
    with np.errstate(invalid="ignore", divide="ignore"):
        o[:, 0], o[:, 1] = _d(a) / _d(2 * R), _d(c) / _d(2 * Sp)
        o[:, 2] = _d(a * d) / _d(b * c)
        o[:, 3] = _replay_2x2(a, b, c, d)
        U, Vi = _d(N * a - R * At), N * (n1 + 4 * n2) - At * At
        o[:, 4] = np.where(Vi == 0, NAN, (_d(N) * (U * U)) / (_d(R * Sp) * _d(Vi)))
        RS = _d(R * Sp)
        d0, d1, d2 = _d(r0 * N - R * n0), _d(r1 * N - R * n1), _d(r2 * N - R * n2)
        o[:, 5] = np.where((n0 == 0) | (n1 == 0) | (n2 == 0), NAN, (d0 * d0) / (RS * _d(n0)) + (d1 * d1) / (RS * _d(n1)) + (d2 * d2) / (RS * _d(n2)))
        o[:, 6] = _replay_2x2(r1 + r2, r0, s1 + s2, s0)
        o[:, 7] = _replay_2x2(r2, r0 + r1, s2, s0 + s1)
        cm = replay_cmh(tab)
        o[:, 9] = np.where(cm[:, 1] == 0, NAN, (cm[:, 0] * cm[:, 0]) / cm[:, 1])
        o[:, 10] = np.where(cm[:, 3] == 0, NAN, cm[:, 2] / cm[:, 3])
    dead = (R == 0) | (Sp == 0)
    if fisher_p:
        for g in np.flatnonzero(~dead):
            o[g, 8] = replay_fisher(int(a[g]), int(b[g]), int(c[g]), int(d[g]))
    o[dead] = NAN
    return o
