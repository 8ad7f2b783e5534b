"""GPU checks of the multi-phenotype scan (pg_assoc_pheno_dev, lmm.pygemma_multi) — run with -m gpu on an MI355X.

The bar is bit-identity: every phenotype's six outputs equal those of a single-phenotype run (pg_assoc_dev / lmm.pygemma) on
that phenotype alone, for chunk widths 1, 2, 4, 8 and a chunk boundary, the register-resident and slot-chunked covariate
paths, NaN and constant phenotypes, and every X input of lmm.pygemma."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = ("beta", "se_beta", "tau", "lambda", "F_wald", "p_wald")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _panel(n, c, p=48):
    """Eigen-basis inputs plus 17 phenotypes: the panel's own, one with NaNs, one constant, and mixtures of y, W and noise."""
    from pygemma_amd import synth
    rp = synth.rotated_panel(n, p, c, seed=100 + n + c)
    rng = np.random.default_rng(n * 31 + c)
    y = rp["Y"].reshape(-1)
    Ys = [y]
    nan = y.copy(); nan[rng.integers(0, n, 3)] = np.nan
    Ys += [nan, np.full(n, 1.5, np.float32)]
    while len(Ys) < 17:
        a, b = rng.standard_normal(2)
        Ys.append((a * y + b * rp["W"][:, rng.integers(0, c)] + rng.standard_normal(n)).astype(np.float32))
    return rp["d"], np.ascontiguousarray(rp["W"]), np.ascontiguousarray(np.stack(Ys)), np.ascontiguousarray(rp["X"].T), rp


def _outs(ctx, t, p):
    return [ctx.alloc(t * p * 4) for _ in range(4)] + [ctx.alloc(t * p * 8) for _ in range(2)]


def _download(bufs, t, p):
    return {col: b.download((t, p), np.float32 if k < 4 else np.float64) for k, (col, b) in enumerate(zip(COLS, bufs))}


def single(ctx, d, W, y, Xs, grid):
    from pygemma_amd import _lib
    L = _lib.load()
    n, c = W.shape
    p = Xs.shape[0]
    dd, dW, dy, dX = (ctx.to_device(a) for a in (d, W, y, Xs))
    o = _outs(ctx, 1, p)
    _lib.check(L.pg_assoc_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, dX.ptr, n, int(grid), *[b.ptr for b in o], None), "pg_assoc_dev")
    ctx.sync()
    r = _download(o, 1, p)
    for b in (dd, dW, dy, dX, *o):
        b.free()
    return {k: v[0] for k, v in r.items()}


def multi(ctx, d, W, Y, Xs, grid, stats=None):
    from pygemma_amd import _lib
    L = _lib.load()
    n, c = W.shape
    p, t = Xs.shape[0], Y.shape[0]
    ldy = n + 5                                   # a row pitch other than n
    Yp = np.zeros((t, ldy), np.float32); Yp[:, :n] = Y
    dd, dW, dY, dX = (ctx.to_device(a) for a in (d, W, Yp, Xs))
    o = _outs(ctx, t, p)
    ds = ctx.to_device(np.zeros(2, np.uint64))
    _lib.check(L.pg_assoc_pheno_dev(ctx.handle, n, c, p, t, dd.ptr, dW.ptr, dY.ptr, ldy, dX.ptr, n, int(grid), *[b.ptr for b in o], ds.ptr),
               "pg_assoc_pheno_dev")
    ctx.sync()
    r = _download(o, t, p)
    if stats is not None:
        stats[:] = ds.download((2,), np.uint64)
    for b in (dd, dW, dY, dX, ds, *o):
        b.free()
    return r


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("n", [37, 384, 2000])
@pytest.mark.parametrize("c", [1, 5, 10, 16, 30])
def test_kernel_bit_identical_to_single_phenotype_runs(c, n, grid, ctx):
    d, W, Y, Xs, _ = _panel(n, c)
    ref = [single(ctx, d, W, Y[k], Xs, grid) for k in range(Y.shape[0])]
    for t in (1, 2, 3, 8, 17):
        got = multi(ctx, d, W, Y[:t], Xs, grid)
        for k in range(t):
            for col in COLS:
                ne = bits(got[col][k]) != bits(ref[k][col])
                assert not ne.any(), (t, k, col, int(ne.sum()), got[col][k][ne][:3], ref[k][col][ne][:3])


@pytest.mark.parametrize("n,c,grid", [(384, 5, False), (2000, 10, True)])
def test_kernel_matches_oracle_in_kernel_order(n, c, grid, ctx):
    from oracle import oracle as O
    d, W, Y, Xs, rp = _panel(n, c)
    got = multi(ctx, d, W, Y[:4], Xs, grid)
    for k in (0, 3):
        orc = O.calculate(d, Y[k], W, Xs.T, grid=grid, order=1, nthreads=4)
        for col in ("beta", "se_beta", "tau", "lambda", "F_wald"):
            a, b = got[col][k], orc[col].astype(got[col].dtype)
            assert (bits(a) == bits(b)).all(), (k, col)
        np.testing.assert_allclose(got["p_wald"][k], orc["p_wald"], rtol=1e-9)


def test_kernel_stats_are_the_sum_of_single_runs(ctx):
    from pygemma_amd import ops
    d, W, Y, Xs, _ = _panel(384, 5)
    st = np.zeros(2, np.uint64)
    multi(ctx, d, W, Y[:3], Xs, False, stats=st)
    tot = sum(ops.assoc(d, W, Y[k], Xs.T, ctx=ctx, return_stats=True)["n_evals"] for k in range(3))
    assert (st.astype(np.int64) == tot).all()


def test_abi_misuse(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    f = ctx.alloc(1 << 16).ptr
    call = lambda n=64, c=2, p=4, t=2, Yr=f, ldy=64, ldx=64: L.pg_assoc_pheno_dev(ctx.handle, n, c, p, t, f, f, Yr, ldy, f, ldx, 0,
                                                                                   f, f, f, f, f, f, None)
    assert call(Yr=None) == -22
    assert call(t=0) == -22
    assert call(ldy=63) == -22
    assert call(ldx=63) == -22
    assert call(n=1) == -22
    assert call(c=0) == -95 and call(c=31) == -95
    assert call(n=4, c=3, ldy=4, ldx=4) == -22           # n - c - 1 = 0
    assert call(p=-1) == -22
    assert call(p=0) == 0                                  # no-op
    assert L.pg_assoc_pheno_warm(ctx.handle, 64, 31, 2, 8) == -95
    assert L.pg_assoc_pheno_warm(ctx.handle, 64, 2, 0, 8) == -22
    assert L.pg_assoc_pheno_warm(ctx.handle, 64, 2, 9, 100) == 0


# ---- the pipeline -------------------------------------------------------------------------------------------------------------
def _frames_equal(a, b):
    assert list(a.columns) == list(b.columns)
    for col in COLS:
        assert a[col].dtype == b[col].dtype, col
        assert (bits(a[col].to_numpy()) == bits(b[col].to_numpy())).all(), col
    if "SNPs" in a.columns:
        assert list(a["SNPs"]) == list(b["SNPs"])


def _raw(n=384, p=700, c=3, t=5, seed=3):
    from pygemma_amd import synth
    raw = synth.exact_panel(n, p, c, seed=seed)
    rng = np.random.default_rng(seed)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    G = raw["X"]
    Y = np.stack([G[:, :20] @ rng.standard_normal(20) + rng.standard_normal(n) * s for s in np.linspace(0.5, 3, t)], axis=1)
    Y[:, 1] = np.round(Y[:, 1])                                  # a float64 column of integers
    return Y, G, W, raw["K"]


def _compare(Y, X, W, K, **kw):
    from pygemma import lmm
    snps = [f"rs{i}" for i in range(X.shape[1])]
    st_m, st_s = {}, {}
    got = lmm.pygemma_multi(Y, X, W, K, snps=snps, stats=st_m, **kw)
    assert list(got) == list(range(Y.shape[1]))
    for k in range(Y.shape[1]):
        _frames_equal(got[k], lmm.pygemma(Y[:, k], X, W, K, snps=snps, stats=st_s, **kw))
    assert st_m["phenotypes"] == Y.shape[1] and st_m["bytes_in"] == st_s["bytes_in"] and st_m["batches"] == st_s["batches"]
    return got


@pytest.mark.parametrize("kind", ["f32", "f32_snp_major", "f64", "i8", "u8"])
def test_pipeline_bit_identical_for_every_x_layout(kind):
    Y, G, W, K = _raw()
    X = {"f32": G, "f32_snp_major": np.asfortranarray(G), "f64": G.astype(np.float64), "i8": G.astype(np.int8),
         "u8": G.astype(np.uint8)}[kind]
    _compare(Y, X, W, K)


def test_pipeline_packed_bed(tmp_path):
    from pygemma_amd.bed import PackedBed, write_bed
    Y, G, W, K = _raw(n=301, p=500)
    Gm = G.astype(np.float64)
    Gm[np.random.default_rng(1).random(Gm.shape) < 0.01] = np.nan
    write_bed(str(tmp_path / "toy"), Gm)
    _compare(Y, PackedBed.open(str(tmp_path / "toy")), W, K)


def test_pipeline_pre_rotated_eigenpairs_and_Z():
    from pygemma_amd import synth
    Y, G, W, K = _raw(p=300)
    # eigen=False: the rotated inputs and the eigenvalues
    rp = synth.rotated_panel(257, 300, 2, seed=9)
    Yr = np.concatenate([rp["Y"], rp["Y"][::-1], np.full((257, 1), 2.0, np.float32)], axis=1)
    _compare(Yr, rp["X"], rp["W"], rp["d"], eigen=False, grid=True)
    # eigenpairs=(d, U)
    dK, U = np.linalg.eigh(K.astype(np.float64))
    _compare(Y, G, W, None, eigenpairs=(dK, U.astype(np.float32)))
    # Z: K <- Z K Z' on the device
    rng = np.random.default_rng(4)
    q = 200
    Kq = synth.panel(q, 4, 1, seed=5)["K"]
    Z = np.zeros((Y.shape[0], q), np.float32)
    Z[np.arange(Y.shape[0]), rng.integers(0, q, Y.shape[0])] = 1.0
    _compare(Y[:, :3], G, W, Kq, Z=Z)


def test_pipeline_nan_phenotype_and_dataframe_labels():
    import pandas as pd
    from pygemma import lmm
    Y, G, W, K = _raw(p=200, t=3)
    Y[5, 1] = np.nan
    df = pd.DataFrame(Y, columns=["height", "bmi", "ldl"])
    got = lmm.pygemma_multi(df, G, W, K)
    assert list(got) == ["height", "bmi", "ldl"]
    for k, lab in enumerate(df.columns):
        _frames_equal(got[lab], lmm.pygemma(Y[:, k], G, W, K))
    with pytest.raises(ValueError, match="NaN"):
        lmm.pygemma_multi(df, G, W, K, disable_checks=False)
    # a single column (n,) is a one-phenotype run
    one = lmm.pygemma_multi(Y[:, 0], G, W, K)
    _frames_equal(one[0], lmm.pygemma(Y[:, 0], G, W, K))


def test_pipeline_full_size_n10000():
    """The flagship shape with a few phenotypes: n = 10 000, c = 5, t = 4, p = 4 096."""
    from pygemma_amd import synth
    n, p, c, t = 10000, 4096, 5, 4
    raw = synth.exact_panel(n, p, c, seed=2, p_k=4096)
    rng = np.random.default_rng(2)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    Y = raw["X"][:, :30] @ rng.standard_normal((30, t)) + rng.standard_normal((n, t)) * 2
    _compare(Y, raw["X"], W, raw["K"])


def test_pipeline_two_gpus_equal_one():
    from pygemma_amd import _lib
    from pygemma import lmm
    if _lib.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    Y, G, W, K = _raw(p=900)
    a = lmm.pygemma_multi(Y, G, W, K, nproc=1)
    b = lmm.pygemma_multi(Y, G, W, K, nproc=2)
    for k in a:
        _frames_equal(a[k], b[k])
