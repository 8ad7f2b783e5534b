"""The truth the int8 genotype-rotation tests compare against, bit for bit: NumPy and Python integers only, written from the comments of
csrc/rotate_geno.hip (the int8 digit-plane kernel, its prepare step and its detect / decode passes), independently of pygemma_amd.

The int8 path is exact integer arithmetic followed by one fp64 fma and one rounding to float32 per pass:

    prep      U[i, k] = w_k (q_ik + e), |e| <= 1/2: a 24-bit fixed point per eigenvector k, w_k = 2^(E_k - 22); colsum_k = sum_i U[i, k] in fp64
    encode    x_g = v0_g + dx_g code_g (+ dlt_g ind_g), code in {0, 1, 2}, ind in {0, 1}
    rotate    P = code' q (integers: exact);  Xr1 = float32(fma(f64(dx_g) w_k, P, f64(v0_g) colsum_k))
              and, when any column of the block has an indicator:  Xr = float32(fma(f64(dlt_g) w_k, code_ind' q, f64(Xr1)))

so every output bit can be predicted here.  The fma is formed exactly: both terms as integer ratios, one correctly rounded division."""
import numpy as np

KT = 64             # samples per partial of the fp64 column sums
QMAX = 8355711      # 127 * 65536 + 127 * 256 + 127: the largest q whose top digit stays <= 127


class Prep:
    """q (n, n) int32 with eigenvector k in column k, w (n,) float64 (NaN for an eigenvector with a NaN / Inf), colsum (n,) float64"""

    def __init__(self, q, w, colsum):
        self.q, self.w, self.colsum, self.n = q, w, colsum, q.shape[0]


def digits(q):
    """(d2, d1, d0) of q = 65536 d2 + 256 d1 + d0 by the kernel's rule: each low digit the residue in [-128, 127], the carry goes up"""
    q = np.asarray(q, np.int64)
    d0 = ((q + 128) & 255) - 128
    q1 = (q - d0) >> 8
    d1 = ((q1 + 128) & 255) - 128
    d2 = (q1 - d1) >> 8
    return d2, d1, d0


def prep(U):
    U = np.ascontiguousarray(U)
    assert U.dtype == np.float32 and U.ndim == 2 and U.shape[0] == U.shape[1]
    n = U.shape[0]
    U64 = U.astype(np.float64)
    key = (U.view(np.uint32) & np.uint32(0x7FFFFFFF)).max(axis=0)             # the bit pattern of max_i |U[i, k]| (a NaN sorts above Inf)
    q, w = np.zeros((n, n), np.int32), np.empty(n, np.float64)
    for k in range(n):
        mx = float(key[k:k + 1].view(np.float32)[0])
        field = int(key[k]) >> 23
        E = field - 127
        if field == 255:
            w[k] = np.nan
            continue
        if mx == 0.0 or E < -100:
            qscale = 1.0
            w[k] = 1.0
        else:
            if mx * 2.0 ** (22 - E) > QMAX:                                   # exact: mx scaled by a power of two
                E += 1
            qscale = 2.0 ** (22 - E)
            w[k] = 2.0 ** (E - 22)
        # the product is exact in float32 (|.| < 2^23 with at most 24 bits), or far below 1/2 where it is not: one rint, ties to even
        q[:, k] = np.rint((U64[:, k] * qscale).astype(np.float32)).astype(np.int32)
    colsum = np.zeros(n, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(0, n, KT):
            s = np.zeros(n, np.float64)
            for i in range(t, min(t + KT, n)):
                s = s + U64[i]
            colsum = colsum + s
    return Prep(q, w, colsum)


def _f2key(x):
    """the order-preserving integer key of a float32 array (-0.0 below +0.0)"""
    b = np.ascontiguousarray(x, np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def encode_x(X):
    """(codes (n, p) int64, v0 (p,) f32, dx (p,) f32, ind (n, p) int64, dlt (p,) f32) of an (n, p) array of any real dtype.  Raises
    ValueError for a block the genotype path does not take."""
    X = np.asarray(X).astype(np.float32)
    n, p = X.shape
    if not np.isfinite(X).all():
        raise ValueError("NaN / Inf in the block")
    codes, ind = np.zeros((n, p), np.int64), np.zeros((n, p), np.int64)
    v0, dx, dlt = np.zeros(p, np.float32), np.zeros(p, np.float32), np.zeros(p, np.float32)
    half = np.float32(0.5)
    for g in range(p):
        x = X[:, g]
        key = _f2key(x)
        lo, hv = x[np.argmin(key)], x[np.argmax(key)]
        mid = np.float32(lo + half * np.float32(hv - lo))
        tol = np.float32(np.float32(2.0 ** -20) * max(abs(lo), abs(hv)))       # 8 ulp of the larger extreme
        is_lo = x == lo
        is_hi = ~is_lo & (x == hv)
        is_mid = ~is_lo & ~is_hi & (np.abs((x - mid).astype(np.float32)) <= tol)
        oth = ~is_lo & ~is_hi & ~is_mid
        codes[:, g] = np.where(is_hi, 2, np.where(is_mid, 1, 0))
        v0[g], dx[g] = lo, half * np.float32(hv - lo)
        if oth.any():
            ob = np.unique(x[oth].view(np.uint32))
            if len(ob) != 1:
                raise ValueError(f"column {g} holds two other values")
            ind[:, g] = oth
            dlt[g] = np.float32(ob.view(np.float32)[0] - lo)
    return codes, v0, dx, ind, dlt


def encode_bed(data, n, count_a1):
    """The same five arrays of packed .bed records data (p, ldb >= ceil(n/4)) uint8: sample i of a record in bits 2 (i % 4) of byte i // 4,
    00 -> 0 (2 with count_a1), 10 -> 1, 11 -> 2 (0 with count_a1), 01 missing.  Only the n samples' bits are read."""
    data = np.asarray(data)
    assert data.dtype == np.uint8 and data.ndim == 2 and data.shape[1] >= (n + 3) // 4
    p = data.shape[0]
    i = np.arange(n)
    c = ((data[:, i >> 2] >> (2 * (i & 3)).astype(np.uint8)) & 3).T.astype(np.int64)      # (n, p)
    two = 0 if count_a1 else 3
    codes = np.where(c == 2, 1, np.where(c == two, 2, 0)).astype(np.int64)
    ind = (c == 1).astype(np.int64)
    nm = ind.sum(axis=0)
    called = n - nm
    tot = codes.sum(axis=0)                                                                # n1 + 2 n2
    mean = tot.astype(np.float64) / np.where(called > 0, called, 1).astype(np.float64)
    dlt = np.where((nm > 0) & (called > 0), mean, 0.0).astype(np.float32)
    return codes, np.zeros(p, np.float32), np.ones(p, np.float32), ind, dlt


def _dot(codes, q):
    """codes' q as int64 (p, n).  Every partial sum is an integer below 2^53, so the float64 product is exact in any order."""
    n = q.shape[0]
    assert int(np.abs(codes).max(initial=0)) * n * (QMAX + 1) < 2 ** 53
    return (codes.T.astype(np.float64) @ q.astype(np.float64)).astype(np.int64)


def _fma_rows(a, P, b):
    """float64 fma(a, P, b) with a single rounding, elementwise over 1-D arrays: a and b finite float64, P integer.  a P + b as one
    integer ratio with a power-of-two denominator; Python's int / int is correctly rounded (ties to even, subnormals included)."""
    out = np.empty(len(a), np.float64)
    for j, (aj, Pj, bj) in enumerate(zip(a.tolist(), P.tolist(), b.tolist())):
        an, ad = aj.as_integer_ratio()
        bn, bd = bj.as_integer_ratio()
        out[j] = (an * Pj * bd + bn * ad) / (ad * bd)
    return out


def _pass(a, P, base):
    """float32(fma(a, P, base)) over (p, n) arrays.  Where a term is zero or something is not finite (w_k NaN: the whole output column)
    the two IEEE operations of NumPy give the fma's result; everywhere else the sum is formed exactly."""
    Pf = P.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = a * Pf + base
    need = np.isfinite(a) & np.isfinite(base) & (a != 0) & (P != 0) & (base != 0)
    if need.any():
        out[need] = _fma_rows(a[need], P[need], base[need])
    with np.errstate(over="ignore"):
        return out.astype(np.float32)


def rotate(pr, codes, v0, dx, ind=None, dlt=None):
    """Xr (p, n) float32 of a block: pass 1 on the codes and, when any column has an indicator, the accumulating pass for every row"""
    w, cs = pr.w[None, :], pr.colsum[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        a1 = np.asarray(dx, np.float32).astype(np.float64)[:, None] * w
        base = np.asarray(v0, np.float32).astype(np.float64)[:, None] * cs
    xr = _pass(a1, _dot(codes, pr.q), base)
    if ind is not None and ind.any():
        with np.errstate(invalid="ignore", over="ignore"):
            a2 = np.asarray(dlt, np.float32).astype(np.float64)[:, None] * w
        xr = _pass(a2, _dot(ind, pr.q), xr.astype(np.float64))
    return xr


# ---- the inputs the host and the device tests share ----------------------------------------------------------------------------------

def basis(n, seed=0):
    """a random orthogonal float32 U (n, n)"""
    return np.linalg.qr(np.random.default_rng(1000 + 7 * n + seed).standard_normal((n, n)))[0].astype(np.float32)


ADVERSARIAL = ["pow2 max", "E++ top", "E++ just above", "E++ boundary", "ties and carries", "zero", "denormals", "max 2^-110", "max 2^-100",
               "dominant", "NaN", "Inf", "unit", "unit", "unit", "negative max"]


def adversarial_basis(n=257, seed=3):
    """basis(n) with its first len(ADVERSARIAL) columns replaced by the eigenvectors that steer the prepare step; returns (U, bad) with
    bad the columns that hold a NaN / Inf (the only outputs that may be NaN)"""
    assert n >= 64
    rng = np.random.default_rng(seed)
    U = basis(n, seed)
    two = lambda e: np.float32(2.0 ** e)

    def floor_col(scale):
        return (rng.uniform(-1, 1, n) * scale).astype(np.float32)

    U[:, 0] = floor_col(0.2); U[n - 1, 0] = two(-1)                                         # max_i |U| a power of two: top q = 2^22
    U[:, 1] = floor_col(0.2); U[0, 1] = np.float32(2.0 ** -2 * (2 - 2.0 ** -23))            # 2^23 - 1/2 > 8355711: E + 1
    U[:, 2] = floor_col(0.05); U[n // 2, 2] = np.float32(8355711.5 * 2.0 ** (-3 - 22))      # just above the largest q: E + 1
    U[:, 3] = floor_col(0.05); U[127, 3] = -np.float32(8355711.0 * 2.0 ** (-3 - 22))        # at it: digits (127, 127, 127), sign -
    # q scale 2^23 (max 1/2): half-integers of q (ties to even) and q at the digit carries, both signs
    t = [127.5, 128.5, -127.5, -128.5, 0.5, -0.5, 1.5, -1.5, 32767.5, 32768.5, -32767.5, -32768.5, 127, 128, 129, -127, -128, -129,
         384, -384, 32767, 32768, 32769, -32767, -32768, -32769, 98304, -98304, 65536 - 128, 65536 + 128, -65536 + 128, 8388608 / 2 - 1,
         -(8388608 / 2 - 1), 32768 + 128, -32768 - 128, 32768 - 128.5, 255.5, -255.5, 65535.5, -65535.5]
    col = np.rint(rng.uniform(-2.0 ** 21, 2.0 ** 21, n)) + rng.integers(0, 2, n) * 0.5
    col[1:1 + len(t)] = t
    col[0] = 2.0 ** 22
    U[:, 4] = (col * 2.0 ** -23).astype(np.float32)
    assert (U[:, 4].astype(np.float64) * 2.0 ** 23 == col).all()
    U[:, 5] = 0
    U[:, 6] = (rng.integers(1, 1 << 20, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** -149).astype(np.float32)
    U[:, 7] = floor_col(2.0 ** -112); U[3, 7] = two(-110)
    U[:, 8] = floor_col(2.0 ** -101); U[64, 8] = two(-100)                                  # the smallest exponent that is still scaled
    U[:, 9] = floor_col(1e-5); U[5, 9] = 1.0
    U[:, 10] = floor_col(0.1); U[128, 10] = np.nan
    U[:, 11] = floor_col(0.1); U[n - 1, 11] = np.inf
    for k in (12, 13, 14):
        U[:, k] = 0; U[[12, 128, n - 1][k - 12], k] = 1.0
    U[:, 15] = floor_col(0.3); U[85, 15] = -two(-1)
    bad = np.zeros(n, bool); bad[[10, 11]] = True
    return U, bad


def cancelling_basis(n=257, seed=12):
    """A matrix (not orthogonal: the rotation never asks) on which the fp64 steps of the kernel reach the float32 result.
    Even columns: c_k (1 + noise), what the leading eigenvector of a kinship matrix looks like; a centred column cancels against it,
    v0 colsum against dx w P, down to its own rounding, so the single rounding of the fma shows.  Odd columns: pairs +a, -a over 40
    binary orders of magnitude in random rows; their exact sum is 0 and the fp64 column sum is whatever its ORDER leaves, which a
    column with v0 != 0 multiplies into the output."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.5, 1, n) / np.sqrt(n)
    noise = np.array([0, 2.0 ** -22, 2.0 ** -20, 2.0 ** -18])[(np.arange(n) // 2) % 4]
    U = (c[None, :] * (1 + rng.uniform(-1, 1, (n, n)) * noise[None, :])).astype(np.float32)
    h = n // 2
    for k in range(1, n, 2):
        a = (rng.uniform(1, 2, h) * 2.0 ** -rng.uniform(0, 40, h)).astype(np.float32)
        col = np.zeros(n, np.float32); col[:h] = a; col[h:2 * h] = -a
        U[:, k] = col[rng.permutation(n)]
    return U


def cancelling_block(n, p, dtype, seed=1):
    """standardised calls (float64 statistics) with every third column one value: v0 != 0 everywhere"""
    rng = np.random.default_rng(seed)
    g = rng.binomial(2, rng.uniform(0.1, 0.5, p), (n, p)).astype(np.float64)
    g[:3] = [[0], [1], [2]]
    X = (g - g.mean(0)) / g.std(0)
    X[:, ::3] = rng.uniform(0.5, 2, (1, p))[:, ::3]
    return np.ascontiguousarray(X.astype(dtype))


SPECIALS = 7


def hard_calls(n, p, seed, miss=0.0, specials=True):
    """(n, p) float64 hard calls 0 / 1 / 2 with NaN = missing.  With `specials` the LAST min(p, 7) columns are, from the right end and
    starting at entry (n + p) % 7 of this list: monomorphic 0, 1 and 2, a singleton het, one called genotype, all missing, and an SNP
    whose only missing call is sample n - 1 — so a block of p >= 7 holds them all, and the blocks of a grid with p < 7 between them."""
    rng = np.random.default_rng(seed * 1000003 + 1009 * n + p)
    G = rng.binomial(2, rng.uniform(0.05, 0.5, p), (n, p)).astype(np.float64)
    if miss > 0:
        G[rng.random((n, p)) < miss] = np.nan
    if specials:
        for s in range(min(p, SPECIALS)):
            kind, j = (n + p + s) % SPECIALS, p - 1 - s
            if kind < 3:
                G[:, j] = kind
            elif kind == 3:
                G[:, j] = 0; G[n // 2, j] = 1
            elif kind == 4:
                G[:, j] = np.nan; G[n // 3, j] = 2
            elif kind == 5:
                G[:, j] = np.nan
            else:
                G[:, j] = rng.binomial(2, 0.4, n); G[n - 1, j] = np.nan
    return G


def pack_bed(G, count_a1, extra=0, seed=0):
    """(p, ceil(n/4) + extra) .bed records of hard_calls' G (the codes of encode_bed); the pad bits of the last byte of a record and its
    `extra` bytes are random bits"""
    n, p = G.shape
    rng = np.random.default_rng(seed + n + p)
    code = np.full((n, p), 1, np.uint8)
    code[G == 0] = 3 if count_a1 else 0
    code[G == 1] = 2
    code[G == 2] = 0 if count_a1 else 3
    pad = rng.integers(0, 4, ((-n) % 4, p)).astype(np.uint8)
    c = np.concatenate([code, pad], axis=0).T.reshape(p, -1, 4)
    rec = (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rec, rng.integers(0, 256, (p, extra)).astype(np.uint8)], axis=1))


FLOAT_KINDS = ["raw", "01", "12", "02", "one", "centred", "standardised", "imputed"]
INT_KINDS = ["raw", "01", "12", "02", "one", "imputed"]


def array_block(n, p, dtype, seed, imputed=True):
    """(n, p) array of dtype float32 / float64 / int8 / uint8 whose columns cycle through the kinds of genotype column: raw hard calls,
    columns holding only {0, 1}, {1, 2}, {0, 2} or one value, centred and standardised calls (floats: v0 and dx not trivial) and — with
    `imputed` — calls with one other value: the mean of the column in some rows (floats), or calls two apart with a 1 between them (8-bit)."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed * 7919 + 31 * n + p)
    kinds = FLOAT_KINDS if dtype.kind == "f" else INT_KINDS
    kinds = [k for k in kinds if imputed or k != "imputed"]
    X = np.empty((n, p), np.float64)
    for j in range(p):
        kind = kinds[(j + n) % len(kinds)]
        g = rng.binomial(2, rng.uniform(0.1, 0.5), n).astype(np.float64)
        g[rng.permutation(n)[:3]] = [0, 1, 2][:min(n, 3)]
        if kind == "01":
            g[g == 2] = 0
        elif kind == "12":
            g[g == 0] = 2
        elif kind == "02":
            g[g == 1] = 2
        elif kind == "one":
            g[:] = [2, 1, 0.75][j % 3] if dtype.kind == "f" else [2, 1, 0][j % 3]
        elif kind == "centred":
            g = g - g.mean()
        elif kind == "standardised":
            g = (g - g.mean()) / (g.std() if g.std() > 0 else 1.0)
        elif kind == "imputed":
            hole = rng.random(n) < 0.05
            hole[rng.integers(n)] = True
            if dtype.kind == "f":
                mu = g[~hole].mean() if (~hole).any() else 0.25
                g[hole] = mu if mu not in (0.0, 1.0, 2.0) else 0.3125
            else:
                g = 2 * g + (0 if dtype.kind == "u" else -2)
                g[hole] = 1
        X[:, j] = g
    return np.ascontiguousarray(X.astype(dtype))
