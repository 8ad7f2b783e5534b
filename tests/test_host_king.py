"""CPU checks of the KING feature: the truth helper against brute-force per-pair loops, its exact properties (a duplicate is 0.5, phi does
not see which allele is counted, the IBS counts add up), lmm.related_pairs and lmm.unrelated against plain loops, PackedBed.take_samples
against the decoded matrix, the public surface, every refusal before the device, and the C ABI's argument checks."""
import inspect

import numpy as np
import pytest

import _king_truth as T


def _lib_loaded():
    from pygemma_amd import _lib
    return _lib.load()


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


def brute(G):
    """Per-pair, per-SNP loops straight from the definition."""
    G = np.asarray(G, np.float64)
    n, p = G.shape
    hard = [all((not np.isfinite(v)) or v in (0.0, 1.0, 2.0) for v in G[:, g]) for g in range(p)]
    out = {k: np.zeros((n, n), np.int64) for k in ("N", "HH", "IBS0", "Hij")}
    for i in range(n):
        for j in range(n):
            for g in range(p):
                x, y = G[i, g], G[j, g]
                if not (hard[g] and np.isfinite(x) and np.isfinite(y)):
                    continue
                out["N"][i, j] += 1
                out["HH"][i, j] += x == 1 and y == 1
                out["IBS0"][i, j] += abs(x - y) == 2
                out["Hij"][i, j] += x == 1
    return out


def test_truth_is_the_brute_force_count():
    G = T.king_panel(17, 23, seed=3)
    C, B = T.counts(G), brute(G)
    for k in B:
        assert (C[k] == B[k]).all(), k
    num, den = B["HH"] - 2 * B["IBS0"], B["Hij"] + B["Hij"].T
    phi = T.phi_of(C)
    for i in range(17):
        for j in range(17):
            if den[i, j] == 0:
                assert np.isnan(phi[i, j])
            else:
                assert phi[i, j] == np.float32(np.float64(num[i, j]) / np.float64(den[i, j]))
    S = T.sample_counts(G)
    assert (S[:, 0] == np.diag(B["N"])).all() and (S[:, 3] == np.diag(B["HH"])).all() and (S[:, 0] + S[:, 1] == 23).all()
    assert (S[:, 2] + S[:, 3] + S[:, 4] == S[:, 0]).all()


@pytest.mark.parametrize("n,p", [(16, 40), (65, 129)])
def test_truth_properties(n, p):
    G = T.king_panel(n, p, seed=n)
    C = T.counts(G)
    phi, ibs = T.phi_of(C), T.ibs_of(C)
    assert (C["IBS0"] + C["IBS1"] + C["IBS2"] == C["N"]).all() and (C["IBS1"] >= 0).all() and (C["IBS2"] >= 0).all()
    assert not (C["Hij"] == C["Hij"].T).all()
    live = np.diag(C["HH"]) > 0
    assert live.sum() >= n - 2 and (np.diag(phi)[live] == 0.5).all() and (np.diag(ibs)[np.diag(C["N"]) > 0] == 1.0).all()
    assert phi[n - 1, 0] == 0.5 and phi[0, n - 1] == 0.5                         # the duplicate
    assert np.isnan(phi[n - 2]).all() and (C["N"][n - 2] == 0).all()             # the all-missing sample
    assert np.isnan(phi[n - 3, n - 3]) and C["Hij"][n - 3].sum() == 0            # the sample without a het call
    assert (phi.view(np.uint32) == phi.T.view(np.uint32)).all()
    # counting the other allele: phi and ibs keep their bits, n0 and n2 swap
    F = 2.0 - G
    CF = T.counts(F)
    assert (T.phi_of(CF).view(np.uint32) == phi.view(np.uint32)).all() and (T.ibs_of(CF).view(np.uint32) == ibs.view(np.uint32)).all()
    S, SF = T.sample_counts(G), T.sample_counts(F)
    assert (S[:, [0, 1, 3]] == SF[:, [0, 1, 3]]).all() and (S[:, 2] == SF[:, 4]).all() and (S[:, 4] == SF[:, 2]).all()
    assert (T.sample_counts(G, count_a1=True) == SF).all()


def test_the_child_is_first_degree_and_the_rest_unrelated():
    n, p = 64, 2000
    phi = T.phi_of(T.counts(T.king_panel(n, p, seed=2)))
    c = n - 4
    assert 0.177 < phi[c, 1] < 0.354 and 0.177 < phi[c, 2] < 0.354
    got = [(i, j) for i, j, _ in T.related_pairs(phi, 0.177)]
    assert sorted(got) == [(0, n - 1), (1, c), (2, c)]
    keep = T.unrelated(phi, 0.177)
    assert (~keep).sum() == 2 and not keep[c] and not keep[n - 1]


def sym(n, edges, value=0.3):
    phi = np.zeros((n, n), np.float32)
    for e in edges:
        i, j = e[:2]
        phi[i, j] = phi[j, i] = e[2] if len(e) > 2 else value
    np.fill_diagonal(phi, 0.5)
    return phi


HAND = {
    "star": (6, [(0, k) for k in range(1, 6)], [0]),                                 # the hub goes, the leaves stay
    "triangle": (4, [(0, 1), (1, 2), (0, 2)], [2, 1]),                               # ties: the largest index first, then of the rest
    "chain": (5, [(0, 1), (1, 2), (2, 3), (3, 4)], [3, 1]),                          # degree 2 ties: 3, then 1 (degree 1 against 0)
    "ties": (6, [(0, 1), (2, 3), (4, 5)], [5, 3, 1]),
    "none": (4, [], []),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_unrelated_on_hand_made_graphs(name):
    from pygemma_amd import lmm
    n, edges, dropped = HAND[name]
    phi = sym(n, edges)
    keep = lmm.unrelated(phi, 0.0884)
    assert keep.dtype == np.bool_ and keep.shape == (n,)
    assert sorted(np.flatnonzero(~keep).tolist()) == sorted(dropped)
    assert (keep == T.unrelated(phi, 0.0884)).all()
    left = phi[np.ix_(keep, keep)]
    assert not (np.triu(left, 1) > 0.0884).any()


@pytest.mark.parametrize("seed", range(6))
def test_related_pairs_and_unrelated_are_the_truth_loops(seed):
    from pygemma_amd import lmm
    rng = np.random.default_rng(seed)
    n = 40
    A = rng.choice(np.array([-0.02, 0.01, 0.05, 0.1, 0.2, 0.3, 0.5], np.float32), (n, n), p=[0.3, 0.3, 0.2, 0.08, 0.06, 0.04, 0.02])
    phi = np.triu(A, 1) + np.triu(A, 1).T + np.diag(np.full(n, 0.5, np.float32))     # many equal values: the order is by i, j among them
    phi[rng.integers(0, n, 5), rng.integers(0, n, 5)] = np.nan
    phi = np.where(np.isnan(phi) | np.isnan(phi.T), np.nan, phi).astype(np.float32)
    for cutoff in (0.0884, 0.177, 0.0, -1.0, 0.5):
        want = T.related_pairs(phi, cutoff)
        got = lmm.related_pairs(phi, cutoff)
        assert list(got.columns) == ["i", "j", "phi"] and got["i"].dtype == np.int64 and got["phi"].dtype == np.float32
        assert list(zip(got["i"].tolist(), got["j"].tolist())) == [(i, j) for i, j, _ in want]
        assert got["phi"].tolist() == [v for _, _, v in want]
        assert (lmm.unrelated(phi, cutoff) == T.unrelated(phi, cutoff)).all()
    assert len(lmm.related_pairs(phi, 0.5)) == 0 and lmm.unrelated(phi, 0.5).all()


@pytest.mark.parametrize("n", [5, 8, 13, 18])
def test_take_samples_is_the_decoded_selection(n):
    from pygemma_amd.bed import PackedBed
    p = 9
    G = T.ld_panel(n, p, seed=n, miss=0.2, specials=False)
    for a1 in (False, True):
        bed = PackedBed(T.pack(G, count_a1=a1), n, count_A1=a1, snps=[f"rs{j}" for j in range(p)])
        full = bed.to_float(impute=False)
        assert np.array_equal(full, G.astype(np.float32), equal_nan=True)
        mask = np.arange(n) % 3 != 1
        for index in (mask, np.flatnonzero(mask), np.array([n - 1, 0, -2, 0]), np.arange(n), np.array([2])):
            sub = bed.take_samples(index)
            want = full[index]
            assert isinstance(sub, PackedBed) and sub.n == want.shape[0] and sub.p == p and sub.count_A1 == a1 and sub.snps == bed.snps
            assert sub.snps is not bed.snps                                     # a copy, as PackedBed.take makes one
            assert sub.data.shape == (p, (sub.n + 3) // 4) and sub.data.dtype == np.uint8
            assert np.array_equal(sub.to_float(impute=False), want, equal_nan=True)
            if sub.n % 4:
                assert not (sub.data[:, -1] >> (2 * (sub.n % 4))).any()        # the pad bits of the last byte are zero
        for bad in (np.ones(n + 1, bool), np.ones((n, 1), bool), [n], [-n - 1], np.array([0.0, 1.0]), np.zeros((2, 2), np.int64), np.zeros(n, bool),
                    np.zeros(0, np.int64)):
            with pytest.raises(ValueError):
                bed.take_samples(bad)


def test_public_names_signatures_and_defaults():
    import pygemma.lmm as ref_style
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    names = ("king", "ibs", "sample_stats", "related_pairs", "unrelated")
    for name in names:
        assert name in lmm.__all__ and getattr(ref_style, name) is getattr(lmm, name)
    sig = {k: str(inspect.signature(getattr(lmm, k))) for k in names}
    assert sig["king"] == "(X, *, counts=False, device=0, snp_batch=None, verbose=0, stats=None)"
    assert sig["ibs"] == sig["king"]
    assert sig["sample_stats"] == "(X, samples=None, device=0, snp_batch=None, verbose=0, stats=None)"
    assert sig["related_pairs"] == "(phi, cutoff=0.0884)" and sig["unrelated"] == "(phi, cutoff=0.0884)"
    assert str(inspect.signature(PackedBed.take_samples)) == "(self, index)"
    for cut in ("0.354", "0.177", "0.0884", "0.0442"):
        assert cut in lmm.related_pairs.__doc__
    assert "plink2" in lmm.unrelated.__doc__.lower() and "NOT" in lmm.unrelated.__doc__


X0 = np.random.default_rng(0).integers(0, 3, (20, 6)).astype(np.float32)
BAD_X = {"X 1-D": X0[:, 0], "X 3-D": X0[:, :, None], "X int32": X0.astype(np.int32), "X float16": X0.astype(np.float16), "no SNPs": X0[:, :0],
         "no samples": X0[:0]}


@pytest.mark.parametrize("bad", sorted(BAD_X))
def test_bad_genotypes_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    X = BAD_X[bad]
    for call in (lambda: lmm.king(X), lambda: lmm.ibs(X), lambda: lmm.sample_stats(X), lambda: lmm.king(X, counts=True)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("sb", [0, -4, 64.0, True, "8"])
def test_bad_batch_and_names_are_refused_before_the_device(sb, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    for call in (lambda: lmm.king(X0, snp_batch=sb), lambda: lmm.ibs(X0, snp_batch=sb), lambda: lmm.sample_stats(X0, snp_batch=sb),
                 lambda: lmm.sample_stats(X0, samples=["a"] * 19)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("bad", ["1-D", "3-D", "not square", "cutoff high", "cutoff nan", "cutoff -inf", "cutoff str", "cutoff bool", "cutoff None"])
def test_bad_phi_and_cutoff_are_refused(bad):
    from pygemma_amd import lmm
    phi = sym(4, [(0, 1)])
    args = {"1-D": (phi[0],), "3-D": (phi[:, :, None],), "not square": (phi[:3],), "cutoff high": (phi, 0.51), "cutoff nan": (phi, float("nan")),
            "cutoff -inf": (phi, float("-inf")), "cutoff str": (phi, "0.1"), "cutoff bool": (phi, True), "cutoff None": (phi, None)}[bad]
    for fn in (lmm.related_pairs, lmm.unrelated):
        with pytest.raises(ValueError):
            fn(*args)


ENTRY = {
    "pg_king_bed_acc_dev": lambda L, c, p: L.pg_king_bed_acc_dev(c, 8, 1, p, 2, 0, p),
    "pg_king_x_acc_dev": lambda L, c, p: L.pg_king_x_acc_dev(c, 8, 1, p, 2, 8, 1, p),
    "pg_king_finish_dev": lambda L, c, p: L.pg_king_finish_dev(c, 8, p, 0, p),
    "pg_king_counts_dev": lambda L, c, p: L.pg_king_counts_dev(c, 8, p, p, p),
    "pg_sample_stats_bed_acc_dev": lambda L, c, p: L.pg_sample_stats_bed_acc_dev(c, 8, 1, p, 2, 0, p),
    "pg_sample_stats_x_acc_dev": lambda L, c, p: L.pg_sample_stats_x_acc_dev(c, 8, 1, p, 2, 8, 1, p),
}


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_device_entry_points_refuse_a_null_context_by_name(name):
    L = _lib_loaded()
    buf = np.zeros(4096, np.uint8)
    assert ENTRY[name](L, None, buf.ctypes.data) == -22          # PG_EINVAL
    assert name in L.pg_last_error().decode()
    assert not buf.any()


# the checks behind the NULL check never read the context: a dummy non-NULL pointer stands in for it, and nothing may be enqueued
BAD_CALLS = {
    "bed NULL records": lambda L, c, p: L.pg_king_bed_acc_dev(c, 8, 1, None, 2, 0, p),
    "bed NULL acc": lambda L, c, p: L.pg_king_bed_acc_dev(c, 8, 1, p, 2, 0, None),
    "bed n 0": lambda L, c, p: L.pg_king_bed_acc_dev(c, 0, 1, p, 2, 0, p),
    "bed n 2^20": lambda L, c, p: L.pg_king_bed_acc_dev(c, 1 << 20, 1, p, 1 << 18, 0, p),
    "bed pb 0": lambda L, c, p: L.pg_king_bed_acc_dev(c, 8, 0, p, 2, 0, p),
    "bed pb 2^31": lambda L, c, p: L.pg_king_bed_acc_dev(c, 8, 1 << 31, p, 2, 0, p),
    "bed short pitch": lambda L, c, p: L.pg_king_bed_acc_dev(c, 9, 1, p, 2, 0, p),
    "bed acc off 16": lambda L, c, p: L.pg_king_bed_acc_dev(c, 8, 1, p, 2, 0, p + 4),
    "x NULL block": lambda L, c, p: L.pg_king_x_acc_dev(c, 8, 1, None, 2, 8, 1, p),
    "x pb 0": lambda L, c, p: L.pg_king_x_acc_dev(c, 8, 0, p, 2, 8, 1, p),
    "x short SNP-major pitch": lambda L, c, p: L.pg_king_x_acc_dev(c, 8, 4, p, 2, 7, 1, p),
    "x short sample-major pitch": lambda L, c, p: L.pg_king_x_acc_dev(c, 8, 4, p, 2, 3, 0, p),
    "stats bed n 0": lambda L, c, p: L.pg_sample_stats_bed_acc_dev(c, 0, 1, p, 2, 0, p),
    "stats bed short pitch": lambda L, c, p: L.pg_sample_stats_bed_acc_dev(c, 9, 1, p, 2, 0, p),
    "stats bed NULL counts": lambda L, c, p: L.pg_sample_stats_bed_acc_dev(c, 8, 1, p, 2, 0, None),
    "stats x pb 0": lambda L, c, p: L.pg_sample_stats_x_acc_dev(c, 8, 0, p, 2, 8, 1, p),
    "stats x short pitch": lambda L, c, p: L.pg_sample_stats_x_acc_dev(c, 8, 4, p, 2, 3, 0, p),
    "finish NULL out": lambda L, c, p: L.pg_king_finish_dev(c, 8, p, 0, None),
    "finish n 0": lambda L, c, p: L.pg_king_finish_dev(c, 0, p, 0, p),
    "finish what 2": lambda L, c, p: L.pg_king_finish_dev(c, 8, p, 2, p),
    "counts NULL sample5": lambda L, c, p: L.pg_king_counts_dev(c, 8, p, p, None),
    "counts n 0": lambda L, c, p: L.pg_king_counts_dev(c, 0, p, p, p),
}


@pytest.mark.parametrize("name", sorted(BAD_CALLS))
def test_bad_arguments_are_refused_before_any_launch(name):
    L = _lib_loaded()
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    dummy_ctx = np.zeros(4096, np.uint8)
    assert BAD_CALLS[name](L, dummy_ctx.ctypes.data, base) == -22
    assert "pg_" in L.pg_last_error().decode()
    assert not buf.any() and not dummy_ctx.any()


@pytest.mark.parametrize("name", ["pg_king_x_acc_dev", "pg_sample_stats_x_acc_dev"])
@pytest.mark.parametrize("dtype", [-1, 4, 99])
def test_an_unknown_dtype_is_not_supported(name, dtype):
    L = _lib_loaded()
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    dummy_ctx = np.zeros(4096, np.uint8)
    assert getattr(L, name)(dummy_ctx.ctypes.data, 8, 1, base, dtype, 8, 1, base) == -95      # PG_ENOTSUP
    assert name in L.pg_last_error().decode() and "dtype" in L.pg_last_error().decode()


def test_last_batch_ms_refuses_null_and_starts_at_zero():
    import ctypes as C
    L = _lib_loaded()
    enc, pair = C.c_float(-1), C.c_float(-1)
    assert L.pg_king_last_batch_ms(None, C.byref(pair)) == -22 and L.pg_king_last_batch_ms(C.byref(enc), None) == -22
    assert "pg_king_last_batch_ms" in L.pg_last_error().decode() and enc.value == -1 and pair.value == -1
    assert L.pg_king_last_batch_ms(C.byref(enc), C.byref(pair)) == 0 and enc.value >= 0 and pair.value >= 0


def test_acc_bytes():
    L = _lib_loaded()
    for n, pb in ((0, 4), (-1, 4), (1 << 20, 4), (100, 0), (100, -3), (100, 1 << 31)):
        assert L.pg_king_acc_bytes(n, pb) == 0
    assert L.pg_king_zero_bytes(0) == 0 and L.pg_king_zero_bytes(1 << 20) == 0
    sizes = [L.pg_king_acc_bytes(1000, pb) for pb in (1, 129, 300, 10000)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))
    for n in (1, 63, 1000):
        z = L.pg_king_zero_bytes(n)
        assert 16 * n * n + 48 * n + 8 <= z <= L.pg_king_acc_bytes(n, 1) - 3 * 128 * n      # accumulators, totals and counts; then a batch's planes
    assert L.pg_king_acc_bytes(1000, 300) >= L.pg_king_zero_bytes(1000) + 3 * 384 * 1000


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    from pygemma_amd.bed import PackedBed
    _lib_loaded()
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    G = np.random.default_rng(0).integers(0, 3, (20, 6)).astype(np.float64)
    for X in (G.astype(np.float32), G.astype(np.int8), PackedBed(T.pack(G), 20)):
        for call in (lambda: lmm.king(X), lambda: lmm.ibs(X), lambda: lmm.sample_stats(X)):
            with pytest.raises(_lib.PgError):
                call()
