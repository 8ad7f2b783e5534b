"""The streamed kinship (lmm.kinship with a PackedBed or snp_batch, csrc/kinship.hip) against fp64 NumPy truth: packed .bed records
with missing calls and edge-case SNPs, 8-bit and float arrays in both layouts, the fp16 and the fp32 path, bit symmetry,
determinism, agreement with the original path and with pygemma fed by the fp64 K."""
import numpy as np
import pytest

from pygemma_amd.bed import PackedBed

pytestmark = pytest.mark.gpu


def _pack(D):
    """(n, p) dosages of A2 (0/1/2, NaN = missing) -> PackedBed (count_A1=False), as bed.write_bed encodes them."""
    n, p = D.shape
    code = np.full(D.shape, 1, np.uint8)
    code[D == 0] = 0; code[D == 1] = 2; code[D == 2] = 3
    c = np.concatenate([code.T, np.zeros((p, (-n) % 4), np.uint8)], axis=1).reshape(p, -1, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8)


def _decode(bed):
    """fp64 dosages of the bed's convention (NaN = missing)."""
    shifts = np.arange(4, dtype=np.uint8) * 2
    codes = ((bed.data[:, :, None] >> shifts[None, None, :]) & 3).reshape(bed.p, -1)[:, :bed.n]
    lut = np.array([2.0, np.nan, 1.0, 0.0] if bed.count_A1 else [0.0, np.nan, 1.0, 2.0])
    return lut[codes].T


def truth(X, standardize=True):
    """fp64 K of the mean-imputed X; an all-missing SNP contributes zeros (and counts in p)."""
    X = np.array(X, np.float64)
    mu = np.nanmean(np.where(np.isnan(X).all(0), 0.0, X), axis=0) if np.isnan(X).any() else X.mean(0)
    X = np.where(np.isnan(X), mu[None, :], X)
    if standardize:
        sd = X.std(0)
        sd[sd == 0] = 1
        X = (X - X.mean(0)) / sd
    return X @ X.T / X.shape[1]


def check_gate(K, ref, p):
    """the gates of test_gpu_kinship.test_kinship_matches_float64_reference.  The first is floored at four float32 half-ulps of the
    largest scale: below p = 4, sqrt(p)/8 allows fewer than the fp32 path's own roundings (z_i, z_k, the product and K each round
    once to float32; measured 2.3 ulps at p = 1, n = 1500)."""
    assert K.dtype == np.float32 and K.shape == ref.shape
    assert np.isfinite(K).all()
    scale = np.sqrt(np.abs(np.outer(np.diag(ref), np.diag(ref))))
    err = np.abs(K.astype(np.float64) - ref).max()
    assert err <= scale.max() * max(1e-6 * np.sqrt(p) / 8, 4 * 2.0 ** -24), (err, scale.max())
    assert err / np.abs(ref).max() <= 1e-6 + 6e-8 * np.sqrt(p), (err, np.abs(ref).max())


def bitsym(K):
    return (K.view(np.uint32) == K.T.copy().view(np.uint32)).all()


def make_dosages(n, p, miss, seed):
    rng = np.random.default_rng(seed)
    D = rng.binomial(2, rng.uniform(0.02, 0.5, p), size=(n, p)).astype(np.float64)
    if miss:
        D[rng.random((n, p)) < miss] = np.nan
    if p >= 6:
        D[:, 2] = 2.0                             # monomorphic
        D[:, 3] = 0.0; D[n // 2, 3] = 1.0         # singleton het
        if miss:
            D[:, 0] = np.nan; D[3, 0] = 1.0      # one call
            D[:, 1] = np.nan                      # all missing
            D[:, 4] = 2.0; D[1, 4] = 1.0; D[2, 4] = np.nan
    return D


@pytest.fixture(params=["fp16", "fp32"])
def path(request, monkeypatch):
    if request.param == "fp32":
        monkeypatch.setenv("PG_KINSHIP_FP32", "1")
    else:
        monkeypatch.delenv("PG_KINSHIP_FP32", raising=False)
    return request.param


@pytest.mark.parametrize("n", [37, 257, 1500, 4099])
@pytest.mark.parametrize("p,snp_batch", [(1, None), (333, 100), (333, 333), (333, 1000), (4100, 1024), (4100, None)])
@pytest.mark.parametrize("miss", [0.0, 0.02])
def test_packed_bed_matches_fp64_truth(n, p, snp_batch, miss, path):
    from pygemma_amd import lmm
    D = make_dosages(n, p, miss, seed=n + p)
    bed = PackedBed(_pack(D), n)
    K = lmm.kinship(bed, snp_batch=snp_batch)
    check_gate(K, truth(D), p)
    assert bitsym(K)


@pytest.mark.parametrize("count_a1", [False, True])
@pytest.mark.parametrize("standardize", [True, False])
def test_count_a1_and_standardize(count_a1, standardize, path):
    from pygemma_amd import lmm
    n, p = 513, 700
    D = make_dosages(n, p, 0.02, seed=11)
    bed = PackedBed(_pack(D), n, count_A1=count_a1)
    X = _decode(bed)
    K = lmm.kinship(bed, standardize=standardize, snp_batch=256)
    check_gate(K, truth(X, standardize), p)
    assert bitsym(K)


@pytest.mark.parametrize("kind", ["int8 codes", "uint8 codes", "int8 any", "uint8 any", "float32 C", "float32 F", "float64 C", "float64 F",
                                  "int8 F"])
@pytest.mark.parametrize("standardize", [True, False])
def test_arrays_with_snp_batch(kind, standardize, path):
    from pygemma_amd import lmm
    rng = np.random.default_rng(len(kind))
    n, p = 1100, 900
    if "codes" in kind:
        G = rng.binomial(2, rng.uniform(0.02, 0.5, p), size=(n, p))
    elif "int8 any" in kind:
        G = rng.integers(-128, 128, size=(n, p))
    elif "uint8 any" in kind:
        G = rng.integers(0, 256, size=(n, p))
    elif "int8 F" in kind:
        G = rng.integers(-128, 128, size=(n, p))
    else:
        G = rng.standard_normal((n, p)) * rng.uniform(0.1, 10, p) + rng.uniform(-5, 5, p)
    dt = {"int8": np.int8, "uint8": np.uint8, "float32": np.float32, "float64": np.float64}[kind.split()[0]]
    G = G.astype(dt)
    G[:, 5] = G[0, 5]                                   # constant column
    if kind.endswith("F"):
        G = np.asfortranarray(G)
    K = lmm.kinship(G, standardize=standardize, snp_batch=300)
    check_gate(K, truth(G, standardize), p)
    assert bitsym(K)


@pytest.mark.parametrize("n", [8191, 8192])
def test_hom2_singleton_beside_a_missing_call(n, path):
    """A singleton het among hom-2 calls has R ~ -n and mu R ~ -2n.  When another SNP of the batch has a missing call, the mu R
    planes are written for it too, so its fp16 scale must cover mu R (from n = 8 191 on it overflowed to -inf: K rows of NaN)."""
    from pygemma_amd import lmm
    rng = np.random.default_rng(n)
    p = 64
    D = rng.binomial(2, rng.uniform(0.05, 0.5, p), size=(n, p)).astype(np.float64)
    D[:, 0] = 2.0; D[n // 3, 0] = 1.0           # singleton het, no missing call
    D[7, 1] = np.nan                             # one missing call elsewhere in the batch
    K = lmm.kinship(PackedBed(_pack(D), n), snp_batch=p)
    assert np.isfinite(K).all()
    check_gate(K, truth(D), p)
    assert bitsym(K)


@pytest.mark.parametrize("n", [1500, 4099])
def test_common_allele_orientation(n, path):
    """Most SNPs with mean near 2 (count_A1=False with A2 the common allele): the fp32 sum of c R cancels most against the rank-1
    term sum s R there."""
    from pygemma_amd import lmm
    p = 4100
    D = 2.0 - make_dosages(n, p, 0.02, seed=n + 1)
    bed = PackedBed(_pack(D), n)
    for pb in (None, 1000):
        K = lmm.kinship(bed, snp_batch=pb)
        check_gate(K, truth(D), p)
        assert bitsym(K)


def test_deterministic_and_batch_independent():
    from pygemma_amd import lmm
    n, p = 1500, 4100
    D = make_dosages(n, p, 0.02, seed=3)
    bed = PackedBed(_pack(D), n)
    a = lmm.kinship(bed, snp_batch=1000)
    b = lmm.kinship(bed, snp_batch=1000)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    ref = truth(D)
    for pb in (64, 777, 5000):
        c = lmm.kinship(bed, snp_batch=pb)
        check_gate(c, ref, p)
        assert np.abs(c.astype(np.float64) - a).max() <= 1e-6 * np.abs(np.diag(ref)).max() * np.sqrt(p) / 8


def test_same_k_as_the_array_path():
    from pygemma_amd import lmm
    n, p = 1500, 4100
    D = make_dosages(n, p, 0.02, seed=5)
    D[:, 1] = 1.0                                       # no all-missing SNP, which to_float turns into NaN
    bed = PackedBed(_pack(D), n)
    K = lmm.kinship(bed)
    K0 = lmm.kinship(bed.to_float())                    # the original path: dense float32, fp32 syrk
    check_gate(K, K0.astype(np.float64), p)


def test_end_to_end_scan():
    from pygemma_amd import lmm
    rng = np.random.default_rng(9)
    n, p = 600, 2000
    D = make_dosages(n, p, 0.02, seed=9)
    bed = PackedBed(_pack(D), n)
    W = np.ones((n, 1), np.float32)
    Xs = np.nan_to_num(D[:, 10:60], nan=1.0).astype(np.float32)
    y = (0.4 * Xs[:, :1] + rng.standard_normal((n, 1))).astype(np.float32)
    K = lmm.kinship(bed)
    a = lmm.pygemma(y, bed, W, K)
    b = lmm.pygemma(y, bed, W, truth(D).astype(np.float32))
    # columns 0-4 are make_dosages' edge cases, constant after imputation (0, 1, 2) or nearly so: beta there is rounding noise
    np.testing.assert_allclose(a["beta"].to_numpy()[5:], b["beta"].to_numpy()[5:], rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(a["p_wald"].to_numpy()[5:], b["p_wald"].to_numpy()[5:], rtol=2e-2)


def test_full_size_pinned_bed():
    from pygemma_amd import lmm
    n, p = 10000, 50000
    rng = np.random.default_rng(12)
    D = rng.binomial(2, rng.uniform(0.05, 0.5, p), size=(n, p)).astype(np.int8)
    codes = np.where(D == 0, 0, np.where(D == 1, 2, 3)).astype(np.uint8)
    miss = rng.random((n, p), dtype=np.float32) < 0.01
    codes[miss] = 1
    del D
    c = np.concatenate([codes.T, np.zeros((p, (-n) % 4), np.uint8)], axis=1).reshape(p, -1, 4)
    data = lmm.pinned_empty((p, (n + 3) // 4), np.uint8)
    data[:] = c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)
    del c
    bed = PackedBed(data, n)
    K = lmm.kinship(bed)
    assert K.shape == (n, n) and np.isfinite(K).all() and bitsym(K)
    X = np.array([0.0, np.nan, 1.0, 2.0])[codes]        # fp64 dosages, then fp64 mean imputation and standardisation
    del codes
    mu = np.nanmean(X, axis=0)
    X = np.where(np.isnan(X), mu[None, :], X)
    X -= X.mean(0)
    sd = np.sqrt((X * X).mean(0))
    sd[sd == 0] = 1
    X /= sd
    rows = rng.choice(n, 64, replace=False)
    ref = X[rows] @ X.T / p
    scale = np.sqrt(np.outer(np.einsum("ij,ij->i", X[rows], X[rows]), np.einsum("ij,ij->i", X, X))) / p
    err = np.abs(K[rows].astype(np.float64) - ref).max()
    assert err <= 1e-6 * scale.max() * np.sqrt(p) / 8, err
    assert err / np.abs(ref).max() <= 1e-6 + 6e-8 * np.sqrt(p), err
