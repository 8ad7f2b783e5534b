"""The truth the fp16 x 2 tests compare against: NumPy only, written from the comments of csrc/rotate_geno.hip (absmax_kernel, scale_kernel,
split_u_kernel, split_x_kernel, the epilogue of geno_gemm_body) and of csrc/kinship.hip (its header, kin_encode_kernel,
pg_kinship_finish_dev), independently of pygemma_amd.

The kernels accumulate fp16 x fp16 products in float32 on the matrix pipe, in an order nobody specifies.  The order stops mattering when
nothing rounds: if every product of a pass lies on one power-of-two grid g and sum |terms| < 2^24 g, every partial sum of every order and
grouping is a float32, the accumulator is ONE number, and what the fp64 epilogue makes of it can be predicted bit for bit.  The panels
below are built so (terms_bound states the condition; the tests assert it for every output), each with the low plane it is about at work:

    prep      S = 2^k with S max|U| in [2^14, 2^15);  H1 = fp16(S u), H2 = fp16(S u - H1), round to nearest even;  colsum_k in fp64
    genotype  Xr[g][k] = float32(fma(dx_g / S, a, v0_g colsum_k)),  a = sum_i code_ig (H1 + H2)_ik
    indicator Xr[g][k] = float32(fma(dlt_g / S, a_ind, float64(Xr[g][k])))          (a second rounding)
    split     s_g = 2^k with s_g max|x_g| in [2^14, 2^15);  X1, X2 like H1, H2;  v0 = 0, dx = dlt = 1 / s_g;  pass 1 on X1, pass 2 adds X2
    kinship   per batch acc[i >= k] += fma(a, 1 / S, -v_k) in fp64;  K = float32(acc / p), mirrored

Where exactness is impossible (both low planes at work: a product needs 2^12 2^12 grid units) split_generic gives the exact value and a
derived bound instead."""
import numpy as np

import _rotate_i8_truth as I8      # encode_x and pack_bed: what the detect pass leaves, and .bed records of a panel

KT = 64             # samples per K-tile, and per partial of the fp64 column sums


# ---- conversions and scales ----------------------------------------------------------------------------------------------------------

def f16_rn(x):
    """float32 -> fp16, round to nearest even (NumPy's conversion), returned as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float64)


def f16_trunc(x):
    """float32 -> fp16 towards zero (a wrong model: test_host_f16x2_truth.py)"""
    x = np.asarray(x, np.float32)
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float64)


def split(x32, conv=f16_rn):
    """the two planes of float32 values: (h1, h2) as float64, h2 from the float32 residual x - h1 (exact)"""
    x32 = np.asarray(x32, np.float32)
    h1 = conv(x32)
    r = x32.astype(np.float64) - h1
    assert (r.astype(np.float32).astype(np.float64) == r).all()
    return h1, conv(r.astype(np.float32))


def pow2_scale(m):
    """(S, 1/S) of scale_kernel / split_scale: the power of two that puts the float32 m > 0 in [2^14, 2^15), the exponent field of S
    clamped to [1, 254]; m == 0 -> 1"""
    m = np.float32(m)
    if not m > 0:
        return 1.0, 1.0
    e = (int(np.array([m]).view(np.uint32)[0]) >> 23) & 0xFF
    se = min(max(127 + 14 - (e - 127), 1), 254)
    return 2.0 ** (se - 127), 2.0 ** (127 - se)


def colsum(U):
    """sum_i U[i, k] in fp64: 64-sample partials summed in order, then the partials in K-tile order"""
    U64 = np.asarray(U, np.float32).astype(np.float64)
    n = U64.shape[0]
    out = np.zeros(U64.shape[1], np.float64)
    for t in range(0, n, KT):
        s = np.zeros(U64.shape[1], np.float64)
        for i in range(t, min(t + KT, n)):
            s = s + U64[i]
        out = out + s
    return out


class Prep:
    """H1, H2 (n, n) float64 with eigenvector k in column k, S, invS, colsum (n,) float64"""

    def __init__(self, H1, H2, S, invS, cs):
        self.H1, self.H2, self.S, self.invS, self.colsum, self.n = H1, H2, S, invS, cs, H1.shape[0]

    @property
    def H(self):
        return self.H1 + self.H2          # 22 bits at the most: exact in float64


def prep(U, conv=f16_rn):
    U = np.ascontiguousarray(U)
    assert U.dtype == np.float32 and U.ndim == 2 and U.shape[0] == U.shape[1] and np.isfinite(U).all()
    S, invS = pow2_scale(np.abs(U).max())
    su = (U.astype(np.float64) * S).astype(np.float32)
    assert (su.astype(np.float64) == U.astype(np.float64) * S).all()          # a power of two: exact
    H1, H2 = split(su, conv)
    return Prep(H1, H2, S, invS, colsum(U))


# ---- the grid condition --------------------------------------------------------------------------------------------------------------

def _lowbit(x, unit=2.0 ** -24):
    """per row of x (K, m): the largest power of two that divides every non-zero entry of the row (entries are multiples of `unit`: 2^-24
    covers every fp16), as float64 (K,); inf for a row of zeros"""
    v = np.abs(np.atleast_2d(np.asarray(x, np.float64))) / unit
    q = v.astype(np.int64)
    assert (q == v).all()
    low = np.where(q != 0, q & -q, np.int64(1) << 62).min(axis=1)
    return np.where(low == np.int64(1) << 62, np.inf, low.astype(np.float64) * unit)


def terms_bound(A, H1, H2):
    """(bound (p, n), g): for every output of a pass on the operand A (K x SNPs) against the planes H1, H2 (K x eigen indices),
    sum_i |a_i| (|H1| + |H2|) in units of the grid g every non-zero product lies on: the smallest over the K index i of lowbit(A[i])
    lowbit(H1[i], H2[i]).  bound < 2^24 everywhere: the float32 accumulation is exact in any order."""
    gi = _lowbit(A) * np.minimum(_lowbit(H1), _lowbit(H2))
    gi = gi[np.isfinite(gi)]
    g = float(gi.min()) if gi.size else 1.0          # no non-zero product at all: every term is 0
    return np.abs(A).T @ (np.abs(H1) + np.abs(H2)) / g, g


def low_share(h2):
    return float(np.count_nonzero(h2)) / max(h2.size, 1)


def accumulate(A, pr):
    """the float32 accumulator of a pass, (p, n) float64: A' (H1 + H2).  Exact under terms_bound's condition, which is asserted, together
    with what it implies: the value is a float32."""
    bound, g = terms_bound(A, pr.H1, pr.H2)
    assert bound.max(initial=0) < 2.0 ** 24, f"sum |terms| reaches {bound.max() / 2.0 ** 24:.3f} x 2^24 grid units"
    acc = A.T @ pr.H                     # float64: exact a fortiori
    assert (acc.astype(np.float32).astype(np.float64) == acc).all()
    return acc, g


def epilogue(mul, invS, acc, g, base):
    """float32(fma(mul_g invS, acc, base)) over (p, n), the fma's single rounding included: the multiplier has few bits (asserted: at most
    29) and acc at most 24, so their float64 product is exact and the float64 addition is the one rounding of the fma"""
    m = np.asarray(mul, np.float32).astype(np.float64) * invS
    q = (np.frexp(np.abs(m))[0] * 2.0 ** 53).astype(np.int64)          # the significand as an integer: its width is 53 - trailing zeros
    assert ((q == 0) | ((q & -q) >= np.int64(1) << 24)).all() and np.abs(acc).max(initial=0) / g < 2.0 ** 24
    return (m[:, None] * acc + np.asarray(base, np.float64)).astype(np.float32)


# ---- the rotation ---------------------------------------------------------------------------------------------------------------------

def path_of(X):
    """1: genotype-valued (at most three equally spaced values and one other per column), 2: split planes, 0: NaN / Inf"""
    X = np.asarray(X)
    if not np.isfinite(X.astype(np.float32)).all():
        return 0
    try:
        I8.encode_x(X)
        return 1
    except ValueError:
        return 2


def rotate_geno(pr, X, round_between=True):
    """Xr (p, n) float32 of a genotype-valued block on the fp16 kernel: the codes and, when any column holds an other value, the
    indicator pass for every row.  round_between=False is a wrong model (one rounding for both passes)."""
    codes, v0, dx, ind, dlt = I8.encode_x(X)
    acc, g = accumulate(codes.astype(np.float64), pr)
    base = v0.astype(np.float64)[:, None] * pr.colsum[None, :]
    if not ind.any():
        return epilogue(dx, pr.invS, acc, g, base)
    acc2, g2 = accumulate(ind.astype(np.float64), pr)
    if round_between:
        xr = epilogue(dx, pr.invS, acc, g, base)
        return epilogue(dlt, pr.invS, acc2, g2, xr.astype(np.float64))
    both = dx.astype(np.float64)[:, None] * pr.invS * acc + dlt.astype(np.float64)[:, None] * pr.invS * acc2 + base
    return both.astype(np.float32)


def split_x(X, conv=f16_rn):
    """(X1, X2 (n, p) float64, inv (p,) float32 = 1 / s_g) of a finite block of any real dtype, read as float32"""
    X = np.asarray(X).astype(np.float32)
    n, p = X.shape
    X1, X2, inv = np.empty((n, p)), np.empty((n, p)), np.empty(p, np.float32)
    for j in range(p):
        lo, hi = X[:, j].min(), X[:, j].max()
        s, si = pow2_scale(max(abs(lo), abs(hi)))
        sx = (X[:, j].astype(np.float64) * s).astype(np.float32)
        X1[:, j], X2[:, j] = split(sx, conv)
        inv[j] = si
    return X1, X2, inv


def rotate_split(pr, X, skip_x2=False, conv=f16_rn):
    """Xr (p, n) float32 of a split-plane block: pass 1 on X1 (v0 = 0), pass 2 accumulates X2.  skip_x2 is a wrong model."""
    X1, X2, inv = split_x(X, conv)
    acc, g = accumulate(X1, pr)
    xr = epilogue(inv, pr.invS, acc, g, np.zeros_like(acc))
    if skip_x2:
        return xr
    acc2, g2 = accumulate(X2, pr)
    return epilogue(inv, pr.invS, acc2, g2, xr.astype(np.float64))


def split_generic(pr, X, conv=f16_rn):
    """A split-plane block on which exactness is impossible (S3): (exact (p, n) float64, bound (p, n) float64).  U holds so few non-zeros
    per eigenvector that the float64 sums below carry at most 2^-52 sum |terms|; `bound` is what the kernel may differ from `exact` by:
    t 2^-24 sum |terms| for each accumulator (t its non-zero terms: every float32 addition rounds a partial sum that sum |terms| bounds),
    scaled by 1 / (s S), one float32 rounding of Xr per pass, and the float64 slack of `exact` itself."""
    X1, X2, inv = split_x(X, conv)
    sc = inv.astype(np.float64)[:, None] * pr.invS
    nzH = (pr.H1 != 0).astype(np.float64) + (pr.H2 != 0)
    absH = np.abs(pr.H1) + np.abs(pr.H2)
    e = np.zeros((X1.shape[1], pr.n))
    parts = []
    for Xp in (X1, X2):
        a = Xp.T @ pr.H
        T = np.abs(Xp).T @ absH
        t = (Xp != 0).astype(np.float64).T @ nzH
        parts.append(a * sc)
        e += (t * 2.0 ** -24 + 2.0 ** -50) * T * sc
    exact = parts[0] + parts[1]
    bound = e * (1 + 2.0 ** -24) + 2.0 ** -24 * (np.abs(parts[0]) + np.abs(exact)) + 2.0 ** -52 * np.abs(exact)
    return exact, bound


# ---- the streamed kinship --------------------------------------------------------------------------------------------------------------

def kin_finish(acc, p, once=False):
    """K = float32(float64(acc / p)): two roundings, as pg_kinship_finish_dev takes them.  once=True is a wrong model: the quotient
    rounded to float32 directly (acc as an integer ratio: Python's division is correctly rounded, then placed on the float32 grid)."""
    acc = np.asarray(acc, np.float64)
    if not once:
        return (acc / np.float64(p)).astype(np.float32)
    from fractions import Fraction
    out = np.empty(acc.shape, np.float32)
    flat = out.reshape(-1)
    for j, a in enumerate(acc.reshape(-1).tolist()):
        q = Fraction(a) / p
        lo = np.float32(float(q))                               # within one float32 step of q: pick the nearer neighbour, ties to even
        cands = sorted({float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))},
                       key=lambda c: (abs(Fraction(c) - q), int(np.float32(c).view(np.uint32)) & 1))
        flat[j] = cands[0]
    return out


def kin_model(X, standardize, snp_batch, bed, fp32=False, conv=f16_rn, once=False, info=None, drop_low=False):
    """K (n, n) float32 of lmm.kinship's streamed path on the (n, p) dosages X (float64; NaN = a missing .bed call), in batches of
    snp_batch SNPs.  bed: the statistics of kin_bed_stats_kernel (integer counts), else those of kin_x_stats_kernel (two fp64 passes).
    fp32: the PG_KINSHIP_FP32=1 path (Zt in float32, an fp32 syrk per batch).  Every accumulation is asserted exact (terms_bound).
    drop_low is a wrong model (the low planes left out).  info (a dict) receives the largest sum |terms| / 2^24 and the share of non-zero
    entries in the low plane of (mu - r) R over the SNPs with a missing call."""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    acc = np.zeros((n, n), np.float64)
    worst, low, cnt = 0.0, 0, 0
    for b0 in range(0, p, snp_batch):
        Xb = X[:, b0:b0 + snp_batch]
        pb = Xb.shape[1]
        mis = np.isnan(Xb)
        called = (~mis).sum(0)
        Xz = np.where(mis, 0.0, Xb)
        if bed:
            tot, sq = Xz.sum(0), (Xz * Xz).sum(0)
            mu = np.where(called > 0, tot / np.maximum(called, 1), 0.0)
            var = np.where(called > 0, (called * sq - tot * tot) / (np.maximum(called, 1).astype(np.float64) * n), 0.0)
        else:
            assert not mis.any()
            mu = Xb.sum(0) / n
            var = ((Xb - mu) ** 2).sum(0) / n
        lo = np.where(called > 0, np.where(mis, np.inf, Xb).min(0), 0.0)
        hi = np.where(called > 0, np.where(mis, -np.inf, Xb).max(0), 0.0)
        s = mu if standardize else np.zeros(pb)
        ok = (var > 0) & bool(standardize)
        w = np.where(ok, 1.0 / np.where(ok, var, 1.0), 1.0)
        isd = np.where(ok, 1.0 / np.sqrt(np.where(ok, var, 1.0)), 1.0)
        r = np.rint(mu)
        xi = np.where(mis, mu[None, :], Xb)                      # the imputed values
        if fp32:
            Z = ((xi - s) * isd).astype(np.float32).astype(np.float64)
            g = _lowbit_any(Z) ** 2
            bound = np.abs(Z) @ np.abs(Z).T / g
            assert bound.max() < 2.0 ** 24
            worst = max(worst, bound.max() / 2.0 ** 24)
            a = Z @ Z.T
            assert (a.astype(np.float32) == a).all()
            acc = acc + a
            continue
        anymiss = mis.any(0)
        dev = np.maximum(np.abs(lo - s), np.abs(hi - s))
        dev = np.where(anymiss, np.maximum(dev, np.abs(mu - s)), dev)
        m = (w * dev * np.maximum(1.0, np.abs(mu - r))).astype(np.float32)
        m = m[(m > 0) & (m <= np.float32(3.0e38))]
        S, invS = pow2_scale(m.max()) if m.size else (2.0 ** 127, 2.0 ** -127)      # flag[1] stays 0: exponent field 0 -> clamped to 254
        c = np.where(mis, 0.0, Xb - r)
        R = w * (xi - s)
        RS = R * S
        r1 = conv(RS.astype(np.float32)); r2 = conv((RS - r1).astype(np.float32))
        A, H1, H2 = c, r1, r2
        if mis.any():
            MS = (mu - r) * RS
            m1 = conv(MS.astype(np.float32)); m2 = conv((MS - m1).astype(np.float32))
            A, H1, H2 = np.concatenate([c, mis.astype(np.float64)], 1), np.concatenate([r1, m1], 1), np.concatenate([r2, m2], 1)
        # operands are sample-major here: A (n, K), H (n, K); a[i, k] = sum_j A[i, j] H[k, j]
        if drop_low:
            H2 = np.zeros_like(H2)
        bound, g = terms_bound(A.T, H1.T, H2.T)
        assert bound.max() < 2.0 ** 24, f"kinship batch at SNP {b0}: sum |terms| reaches {bound.max() / 2.0 ** 24:.3f} x 2^24 grid units"
        worst = max(worst, bound.max() / 2.0 ** 24)
        if mis.any():      # the low plane that can matter: (mu - r) R of the SNPs with a missing call (the others meet a zero indicator)
            low += np.count_nonzero(m2[:, anymiss]); cnt += m2[:, anymiss].size
        a = A @ (H1 + H2).T
        assert (a.astype(np.float32) == a).all()
        # the rank-1 term: quarter sums of 16 SNPs in order, the four quarters left to right, then the K-tiles in order
        d = (s - r)[None, :] * R
        v = np.zeros(n)
        for t in range(0, pb, 64):
            q = []
            for u in range(t, t + 64, 16):
                qs = np.zeros(n)
                for j in range(u, min(u + 16, pb)):
                    qs = qs + d[:, j]
                q.append(qs)
            v = v + (((q[0] + q[1]) + q[2]) + q[3])
        acc = acc + (a * invS - v[None, :])                      # a / S is exact, so this is the fma's single rounding
    if info is not None:
        info.update(worst=worst, low_share=low / max(cnt, 1))
    K = kin_finish(np.tril(acc), p, once)
    return np.tril(K) + np.tril(K, -1).T


def _lowbit_any(x):
    """_lowbit for float32-valued data on a coarse grid (multiples of 2^-40)"""
    low = _lowbit(np.asarray(x, np.float64).reshape(1, -1), unit=2.0 ** -40)[0]
    return float(low) if np.isfinite(low) else 1.0


def kin_exact(X, standardize):
    """float32(float64(exact p K) / p) of a panel on which every z and R is dyadic: p K in float64 from values so short that the sum is
    exact (asserted through the integer grid), independent of batches, planes and scales"""
    X = np.asarray(X, np.float64)
    n, p = X.shape
    mis = np.isnan(X)
    called = (~mis).sum(0)
    mu = np.where(called > 0, np.where(mis, 0.0, X).sum(0) / np.maximum(called, 1), 0.0)
    xi = np.where(mis, mu[None, :], X)
    if standardize:
        var = ((xi - xi.mean(0)) ** 2).mean(0)
        Z = xi - mu
        R = Z / np.where(var > 0, var, 1.0)
    else:
        Z = R = xi
    g = _lowbit_any(Z) * _lowbit_any(R)
    assert (np.abs(Z) @ np.abs(R).T / g).max() < 2.0 ** 53
    return ((Z @ R.T) / np.float64(p)).astype(np.float32)


# ---- the panels ------------------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def basis_d(n, seed=0, density=1.0):
    """U = m 2^-12, m uniform in [-4095, 4095], one entry 4095 (S = 2^15: S u = 8 m has 12 bits above 2^14, so H2 = +-8 for odd |m| >=
    2048); not orthogonal on purpose.  density < 1 zeroes entries at random."""
    rng = _rng(11, n, seed)
    m = rng.integers(-4095, 4096, (n, n)).astype(np.float64)
    if density < 1:
        m[rng.random((n, n)) >= density] = 0
    m[rng.integers(n), rng.integers(n)] = 4095
    return (m * 2.0 ** -12).astype(np.float32)


def basis_s1(n, seed=0, density=1.0):
    """multiples of 1/32 in [-1, 1] with one entry 1: S = 2^14 and S u = 512 j, so H2 = 0"""
    rng = _rng(12, n, seed)
    m = rng.integers(-32, 33, (n, n)).astype(np.float64)
    if density < 1:
        m[rng.random((n, n)) >= density] = 0
    m[rng.integers(n), rng.integers(n)] = 32
    return (m / 32).astype(np.float32)


def basis_sparse(n, seed=0):
    """S3: at most two non-zeros per eigenvector at generic float32 values in +-[0.05, 1]; eigenvector k holds samples k and
    (k + 1 + n // 2) % n, so every sample index is hit (63 / 64, 127 / 128 and n - 1 among them)"""
    rng = _rng(13, n, seed)
    U = np.zeros((n, n), np.float32)
    k = np.arange(n)
    val = lambda: (rng.uniform(0.05, 1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    U[k, k] = val()
    U[(k + 1 + n // 2) % n, k] = val()
    return U


D_KINDS = ["raw", "dyadic", "other", "raw other"]


def block_d(n, p, dtype, seed=0):
    """genotype-valued columns, cycling through raw 0 / 1 / 2, v0 + dx code with v0 = -5537/8192 and dx = 2465/8192 (floats: pass 1
    rounds, its value has 12 + 13 fractional bits; 8-bit: -2 + 2 code for int8, 1 + code for uint8), and the same with one dyadic other
    value in a few rows (floats; 8-bit: calls two apart with a 1 between them), so that the indicator pass runs for the block as soon
    as p >= 3 and n >= 4"""
    dtype = np.dtype(dtype)
    rng = _rng(21, n, p, seed)
    X = np.empty((n, p), np.float64)
    for j in range(p):
        kind = D_KINDS[(j + n) % 4]
        c = rng.integers(0, 3, n).astype(np.float64)
        keep = rng.permutation(n)
        c[keep[:3]] = [0, 2, 1][:min(n, 3)]
        hole = (rng.random(n) < 0.1) & (n >= 4)
        if n >= 4:
            hole[keep[3]] = True
            hole[keep[:3]] = False
        if dtype.kind == "f":
            v0, dx, oth = (0.0, 1.0, 0.8125) if kind.startswith("raw") else (-5537 / 8192, 2465 / 8192, -0.25)
            x = v0 + dx * c
            if kind.endswith("other"):
                x[hole] = oth
        else:
            x = c.copy() if kind.startswith("raw") else (c + 1 if dtype.kind == "u" else 2 * c - 2)
            if kind.endswith("other"):
                x = 2 * c + (0 if dtype.kind == "u" else -2)
                x[hole] = 1 if dtype.kind == "u" else -1
        X[:, j] = x
    out = np.ascontiguousarray(X.astype(dtype))
    assert (out.astype(np.float64) == X).all()
    return out


def block_s1(n, p, dtype=np.float32, seed=0):
    """X = j / 8 + b 2^-11, j in 0 .. 16, b in {-1, 0, 1}, a 2 in every column: s = 2^13, s x = 1024 j + 4 b, and fp16 keeps steps of 8
    above 2^13: X2 = 4 b for j >= 8 (a tie each time: nearest even is 1024 j)"""
    rng = _rng(22, n, p, seed)
    X = rng.integers(0, 17, (n, p)) / 8 + rng.integers(-1, 2, (n, p)) * 2.0 ** -11
    X[rng.integers(n, size=p), np.arange(p)] = 2.0
    return np.ascontiguousarray(X.astype(dtype))


def block_s2(n, p, dtype=np.float32, seed=0, step=8):
    """X = j / step, j in 0 .. 2 step (8-bit: any integer up to 15 in magnitude): X2 = 0, the second pass adds zeros"""
    dtype = np.dtype(dtype)
    rng = _rng(23, n, p, seed)
    if dtype.kind == "f":
        X = rng.integers(0, 2 * step + 1, (n, p)) / step
        X[rng.integers(n, size=p), np.arange(p)] = 2.0
    else:
        X = rng.integers(0 if dtype.kind == "u" else -15, 16, (n, p)).astype(np.float64)
    return np.ascontiguousarray(X.astype(dtype))


def block_s3(n, p, dtype=np.float32, seed=0):
    """generic dosages in [0, 2]"""
    rng = _rng(24, n, p, seed)
    return np.ascontiguousarray((2 * rng.beta(0.5, 0.5, (n, p))).astype(dtype))


K_KINDS = ["raw", "pow2 called", "raw", "02", "01", "12"]


def kin_panel(n, p, standardize, seed=0, missing=True):
    """(n, p) float64 hard calls, NaN = missing, on which p K is dyadic.  standardize=False: random calls, and (missing) columns whose
    called count is a power of two (the largest below n, or 64) and whose sum is a multiple of called / 64, so that mu = k / 64 is
    dyadic and (mu - r) mu has up to 12 significant bits: the low plane of (mu - r) R is at work from n = 130 on.
    standardize=True (even n): balanced columns {0, 2}, {0, 1}, {1, 2} half and half — mu in {1, 1/2, 3/2}, variance 1 or 1/4 — and no
    missing call."""
    rng = _rng(31, n, p, int(standardize), seed)
    X = np.empty((n, p), np.float64)
    for j in range(p):
        if standardize:
            assert n % 2 == 0
            a, b = [(0, 2), (0, 1), (1, 2)][(j + n) % 3]
            col = np.array([a, b] * (n // 2), np.float64)
            X[:, j] = col[rng.permutation(n)]
        else:
            col = rng.integers(0, 3, n).astype(np.float64)
            col[rng.permutation(n)[:2]] = [0, 2][:min(n, 2)]
            if missing and j % 2 == 1 and n >= 3:
                called = 1 << ((n - 1).bit_length() - 1)                 # the largest power of two < n ...
                if j % 4 == 3 and n > 64:
                    called = 64                                          # ... or 64: most samples take the imputed value mu
                q = min(called, 64)                                      # mu = k / q: six fractional bits at the most
                tot = (called // q) * int(rng.integers(q // 4 + 1, 7 * q // 4 + 1))
                n2 = int(rng.integers(max(0, tot - called), tot // 2 + 1))
                col = np.array([2.0] * n2 + [1.0] * (tot - 2 * n2) + [0.0] * (called - tot + n2) + [np.nan] * (n - called))
                col = col[rng.permutation(n)]
            X[:, j] = col
    return X


def finish_panel(p, count=512, seed=0):
    """acc (5 count,) float64: the accumulators p mid (exact: p < 2^28) for midpoints `mid` of neighbouring float32, and their two fp64
    neighbours on either side — the values at which the two roundings of pg_kinship_finish_dev could part from one"""
    rng = _rng(41, p, count, seed)
    mid = (2 * rng.integers(1 << 23, 1 << 24, count) + 1).astype(np.float64) * 2.0 ** rng.integers(-40, -10, count)
    acc = mid * p
    assert (acc / p == mid).all()
    up1 = np.nextafter(acc, np.inf); dn1 = np.nextafter(acc, -np.inf)
    return np.concatenate([acc, up1, np.nextafter(up1, np.inf), dn1, np.nextafter(dn1, -np.inf)])


# ---- the shapes and cases the host and the device tests share ---------------------------------------------------------------------------

NS = [1, 3, 63, 64, 65, 129, 255, 256, 257, 1030]
PS = [1, 19, 255, 256, 257, 600]
DIAG = [(1, 19), (3, 1), (63, 255), (64, 257), (65, 256), (129, 600), (255, 19), (256, 257), (257, 255), (1030, 600)]
# a block of fewer than four samples is always genotype-valued (lowest, highest and one more value: the midpoint or the one other value), so
# the split path starts at n = 4: the two smallest sizes of the diagonal are 4 and 5 there
SPLIT_DIAG = [(4, 19), (5, 1)] + DIAG[2:]
SPARSE_FROM = 1030      # from this n on, S1 and S2 use U at density 1/8 (dense: sum |terms| reaches 2.3 and 1.1 x 2^24 at n = 1030)

_cache = {}


def basis(kind, n):
    """the float32 U of a panel kind at size n and its Prep: made once, left unchanged"""
    if (kind, n) not in _cache:
        density = 1 / 8 if n >= SPARSE_FROM else 1.0
        U = {"D": lambda: basis_d(n), "S1": lambda: basis_s1(n, density=density), "S2": lambda: basis_d(n, seed=1, density=density),
             "S3": lambda: basis_sparse(n)}[kind]()
        U.setflags(write=False)
        _cache[kind, n] = (U, prep(U))
    return _cache[kind, n]


def block(kind, n, p, dtype=np.float32, seed=0):
    return {"D": block_d, "S1": block_s1, "S2": block_s2, "S3": block_s3}[kind](n, p, dtype, seed)


def conditions(kind, pr, X):
    """The conditions a panel stands on, asserted: the path the block takes, the share of the low plane it claims, and sum |terms| < 2^24
    grid units for every output of every pass (S3: no such condition).  Returns the largest sum |terms| / 2^24 (S3: 0)."""
    want_path = 1 if kind == "D" else 2
    assert path_of(X) == want_path, (kind, X.shape, path_of(X))
    n = pr.n
    if kind in ("D", "S2", "S3") and n >= 63:
        assert low_share(pr.H2[pr.H1 != 0]) >= 0.20, (kind, n, low_share(pr.H2[pr.H1 != 0]))
    if kind == "S1":
        assert not pr.H2.any()
    if kind == "D":
        codes, _, _, ind, _ = I8.encode_x(X)
        ops = [codes.astype(np.float64)] + ([ind.astype(np.float64)] if ind.any() else [])
    else:
        X1, X2, _ = split_x(X)
        ops = [X1, X2]
        if kind in ("S1", "S3") and X.size >= 64:
            assert low_share(X2) >= 0.20, (kind, X.shape, low_share(X2))
        if kind == "S2":
            assert not X2.any()
    if kind == "S3":
        return 0.0
    worst = 0.0
    for A in ops:
        bound, _ = terms_bound(A, pr.H1, pr.H2)
        assert bound.max(initial=0) < 2.0 ** 24, (kind, X.shape, bound.max() / 2.0 ** 24)
        worst = max(worst, bound.max(initial=0) / 2.0 ** 24)
    return worst


def model(kind, pr, X):
    return rotate_geno(pr, X) if kind == "D" else rotate_split(pr, X)


KIN_NS = [2, 64, 130, 256, 258, 1030]
KIN_PS = [1, 64, 65, 200]


def kin_batches(p):
    """snp_batch below, at and above p"""
    return sorted({max(1, p // 3), p, p + 7})
