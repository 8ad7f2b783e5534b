"""The truth the LD tests compare against: NumPy integer arithmetic, written independently of pygemma_amd.

A genotype panel is a float64 (n, p) matrix G with NaN (or +-Inf) for a missing call.  A column is hard-call when every finite value is
exactly 0, 1 or 2; any other column counts as all missing."""
import numpy as np


def planes(G):
    """(m, x, x^2) as int64 (n, p) matrices: called, code (0 where missing), code squared."""
    G = np.asarray(G, np.float64)
    fin = np.isfinite(G)
    hard = np.all(~fin | (G == 0) | (G == 1) | (G == 2), axis=0)
    m = (fin & hard[None, :]).astype(np.int64)
    x = np.where(m == 1, G, 0.0).astype(np.int64)
    return m, x, x * x


def sums(GA, GB=None):
    """The six sums of every pair (a of GA, b of GB) as an int64 (pa, pb, 6) array in the order N, Sa, Sb, Saa, Sbb, Sab."""
    ma, xa, qa = planes(GA)
    mb, xb, qb = (ma, xa, qa) if GB is None else planes(GB)
    return np.stack([ma.T @ mb, xa.T @ mb, ma.T @ xb, qa.T @ mb, ma.T @ qb, xa.T @ xb], axis=-1)


def r_of(S):
    """float32 r of an array (..., 6) of sums by the definition: int64 products, one division, one square root, clamp, one rounding."""
    S = np.asarray(S, np.int64)
    N, Sa, Sb, Saa, Sbb, Sab = (S[..., t] for t in range(6))
    ca, cb, cab = N * Saa - Sa * Sa, N * Sbb - Sb * Sb, N * Sab - Sa * Sb
    ok = (ca > 0) & (cb > 0)
    den = np.sqrt(np.where(ok, ca, 1).astype(np.float64) * np.where(ok, cb, 1).astype(np.float64))
    r = np.clip(cab.astype(np.float64) / den, -1.0, 1.0)
    return np.where(ok, r, np.nan).astype(np.float32)


def r64_of(S):
    """The same r before the rounding to float32 (for the comparison with np.corrcoef)."""
    S = np.asarray(S, np.int64)
    N, Sa, Sb, Saa, Sbb, Sab = (S[..., t] for t in range(6))
    ca, cb, cab = N * Saa - Sa * Sa, N * Sbb - Sb * Sb, N * Sab - Sa * Sb
    ok = (ca > 0) & (cb > 0)
    den = np.sqrt(np.where(ok, ca, 1).astype(np.float64) * np.where(ok, cb, 1).astype(np.float64))
    return np.where(ok, np.clip(cab.astype(np.float64) / den, -1.0, 1.0), np.nan)


def band_of(R, w, fill=np.nan):
    """band[j, k] = R[j, j + 1 + k] of a square matrix (or of a (p, p, 6) array of sums), `fill` where j + 1 + k >= p."""
    p = R.shape[0]
    out = np.full((p, w) + R.shape[2:], fill, R.dtype)
    for j in range(p):
        k = min(w, p - 1 - j)
        out[j, :k] = R[j, j + 1:j + 1 + k]
    return out


def in_ld(r, r2):
    r = float(r)
    return (not np.isnan(r)) and r * r >= r2


def prune(R, window, r2):
    """Greedy forward pruning on the dense r matrix: plain loops."""
    p = R.shape[0]
    keep = [True] * p
    for j in range(p):
        for i in range(max(0, j - window), j):
            if keep[i] and in_ld(R[i, j], r2):
                keep[j] = False
                break
    return np.array(keep, bool)


def clump(R, pv, p1, p2, r2, window, chrom=None, pos=None):
    """PLINK-style clumping on the dense r matrix over ALL p SNPs: plain loops.  Returns [(index SNP, sorted list of members)] sorted by
    (p, index)."""
    p = len(pv)
    cand = [j for j in range(p) if pv[j] < p2]          # NaN < p2 is False
    order = sorted(cand, key=lambda j: (pv[j], j))
    done = set()
    out = []
    for j in order:
        if j in done or not pv[j] <= p1:
            continue
        done.add(j)
        mem = []
        for i in cand:
            if i in done:
                continue
            if chrom is not None and chrom[i] != chrom[j]:
                continue
            d = abs(i - j) if pos is None else abs(float(pos[i]) - float(pos[j]))      # Python numbers: an unsigned difference cannot wrap
            if d <= window and in_ld(R[min(i, j), max(i, j)], r2):
                mem.append(i)
        done.update(mem)
        out.append((j, sorted(mem)))
    return out


def ld_panel(n, p, seed, miss=0.07, specials=True):
    """A random LD-block panel: a column is a fresh binomial(2, maf) draw or its left neighbour with a tenth of the calls redrawn, `miss`
    of all calls missing.  With `specials` and room for them it also holds (at fixed columns from the right end, all distinct):
    a monomorphic SNP, an all-missing SNP, an exact copy and a flip 2 - x of column 0, and a dosage column (0.5 in it: not hard-call).
    Returns the float64 (n, p) matrix, NaN = missing."""
    rng = np.random.default_rng(seed)
    G = np.empty((n, p))
    for j in range(p):
        if j == 0 or j % 11 == 0 or rng.random() < 0.15:
            G[:, j] = rng.binomial(2, rng.uniform(0.2, 0.5), n)
        else:
            G[:, j] = G[:, j - 1]
            redo = rng.random(n) < 0.1
            G[redo, j] = rng.binomial(2, 0.4, int(redo.sum()))
    if miss > 0:
        G[rng.random((n, p)) < miss] = np.nan
    if specials and p >= 12:
        G[:, p - 2] = 1.0                                # monomorphic
        G[:, p - 3] = np.nan                             # all missing
        G[:, p - 5] = G[:, 0]                            # copy
        G[:, p - 6] = 2.0 - G[:, 0]                      # flip
        G[:, p - 8] = np.where(np.arange(n) % 2 == 0, 0.5, 1.0)      # dosage
    return G


def pack(G, count_a1=False):
    """(p, ceil(n/4)) PLINK .bed records of a panel: A2 counts 0/1/2 -> codes 00/10/11 (count_a1: 11/10/00), anything else -> 01."""
    G = np.asarray(G, np.float64)
    n, p = G.shape
    code = np.full(G.shape, 1, np.uint8)
    code[G == 0] = 3 if count_a1 else 0
    code[G == 1] = 2
    code[G == 2] = 0 if count_a1 else 3
    c = np.concatenate([code.T, np.zeros((p, (-n) % 4), np.uint8)], axis=1).reshape(p, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def bed_view(G):
    """What a .bed file keeps of a panel: a column that is not hard-call cannot be written as one; every call of it is missing."""
    m, x, _ = planes(G)
    return np.where(m == 1, x.astype(np.float64), np.nan)
