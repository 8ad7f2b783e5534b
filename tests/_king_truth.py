"""The truth the KING tests compare against: NumPy int64 arithmetic, written independently of pygemma_amd.

A genotype panel is a float64 (n, p) matrix G with NaN (or +-Inf) for a missing call.  A column is hard-call when every finite value is
exactly 0, 1 or 2; any other column counts as all missing for every sample (the rule of _ld_truth.planes)."""
import numpy as np

from _ld_truth import bed_view, ld_panel, pack, planes      # noqa: F401  (re-exported: the tests build their sources with them)


def indicators(G):
    """(m, h, a, b) as int64 (n, p) matrices: called, called and 1, called and 0, called and 2."""
    m, x, _ = planes(G)
    return m, ((x == 1) & (m == 1)).astype(np.int64), ((x == 0) & (m == 1)).astype(np.int64), ((x == 2) & (m == 1)).astype(np.int64)


def counts(G):
    """The pair counts of every pair of samples as a dict of int64 (n, n) matrices: N, HH, IBS0, Hij (row i: i's het calls where j is
    called; Hji is its transpose), IBS1, IBS2."""
    m, h, a, b = indicators(G)
    C = {"N": m @ m.T, "HH": h @ h.T, "IBS0": a @ b.T + b @ a.T, "Hij": h @ m.T}
    C["IBS1"] = C["Hij"] + C["Hij"].T - 2 * C["HH"]
    C["IBS2"] = C["N"] - C["IBS0"] - C["IBS1"]
    return C


def _ratio(num, den):
    ok = den != 0
    out = np.asarray(num).astype(np.float64) / np.where(ok, den, 1).astype(np.float64)
    return ok, out


def phi_of(C):
    """float32 KING-robust kinship by the definition: one fp64 division of the exact counts, one rounding; NaN when Hij + Hji == 0."""
    ok, v = _ratio(C["HH"] - 2 * C["IBS0"], C["Hij"] + C["Hij"].T)
    return np.where(ok, np.float32(v), np.float32(np.nan)).astype(np.float32)


def ibs_of(C):
    """float32 IBS similarity 1 - (IBS1 + 2 IBS0) / (2 N); NaN when N == 0."""
    ok, v = _ratio(C["IBS1"] + 2 * C["IBS0"], 2 * C["N"])
    return np.where(ok, np.float32(1.0 - v), np.float32(np.nan)).astype(np.float32)


def sample_counts(G, count_a1=False):
    """(n, 5) int64: n_obs, n_miss, n0, n1, n2 per sample; a column that is not hard-call adds 1 to every n_miss."""
    m, h, a, b = indicators(2.0 - np.asarray(G, np.float64) if count_a1 else G)
    obs = m.sum(axis=1)
    return np.stack([obs, m.shape[1] - obs, a.sum(axis=1), h.sum(axis=1), b.sum(axis=1)], axis=1)


def related_pairs(phi, cutoff):
    """[(i, j, phi)] of the pairs i < j with phi > cutoff, by descending phi, then i, then j: plain loops."""
    n = phi.shape[0]
    out = []
    for i in range(n):
        for j in range(i + 1, n):
            v = float(phi[i, j])
            if not np.isnan(v) and v > cutoff:
                out.append((i, j, v))
    return sorted(out, key=lambda t: (-t[2], t[0], t[1]))


def unrelated(phi, cutoff):
    """The greedy keep-mask: while an edge remains, drop the vertex of largest current degree, ties to the largest index.  Plain loops."""
    n = phi.shape[0]
    edges = {(i, j) for i, j, _ in related_pairs(phi, cutoff)}
    keep = [True] * n
    while edges:
        deg = [0] * n
        for i, j in edges:
            deg[i] += 1
            deg[j] += 1
        best = max(range(n), key=lambda v: (deg[v], v))
        keep[best] = False
        edges = {e for e in edges if best not in e}
    return np.array(keep, bool)


def king_panel(n, p, seed, miss=0.07, specials=True):
    """ld_panel(n, p, seed, miss) plus, where n leaves room (n >= 16), four special samples at the end: n - 1 an exact duplicate of
    sample 0, n - 2 with every call missing, n - 3 without a het call (its hets become 0 or 2), n - 4 a child of samples 1 and 2 (one
    allele drawn from each parent; missing where either parent is not a called 0, 1 or 2).  The panel's dosage column keeps its 0.5 in
    the other rows: it stays a column that is not hard-call."""
    G = ld_panel(n, p, seed, miss=miss, specials=specials)
    if n < 16:
        return G
    rng = np.random.default_rng(seed + 1000)
    par = G[1:3]
    ok = np.isin(par, (0.0, 1.0, 2.0)).all(axis=0)
    draw = rng.random((2, p)) < np.where(ok[None, :], par, 0.0) / 2.0      # the allele a parent hands on
    G[n - 4] = np.where(ok, draw.sum(axis=0).astype(np.float64), np.nan)
    row = G[n - 3]
    G[n - 3] = np.where(row == 1.0, np.where(rng.random(p) < 0.5, 0.0, 2.0), row)
    G[n - 2] = np.nan
    G[n - 1] = G[0]
    return G
