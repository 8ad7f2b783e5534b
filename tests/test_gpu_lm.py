"""GPU checks of the linear-model scan (pg_lm_setup_dev, pg_lm_x_dev, pg_lm_bed_dev, ops.lm, lmm.pygemma_lm) — run with -m gpu on an
MI355X.

The truth is ordinary least squares in fp64 NumPy on the same float32 inputs: W is orthogonalised by Householder QR (np.linalg.qr,
applied twice), not by the kernel's Cholesky route.  The gate is the score test's (test_gpu_score.py):
|F - F_t| / max(F_t, median F_t) <= 1e-9 max(1, cond(W'W) 1e-6) on every row, se_beta and tau within 1 float32 ulp of the rounded
truth, beta within 1 ulp (widened like there past cond 1e6), p_wald against scipy.stats.f.sf at rtol 1e-8."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = ("beta", "se_beta", "tau", "F_wald", "p_wald")
DTYPES = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def truth(W, Y, X):
    """fp64 OLS per SNP and phenotype.  W (n,c), Y (n,t), X (n,p): float32-valued.  Returns (t,p) fp64 columns and cond(W'W)."""
    W, Y, X = (np.asarray(a, np.float64) for a in (W, Y, X))
    Y = Y.reshape(Y.shape[0], -1)
    n, c = W.shape
    df = n - c - 1
    Q, _ = np.linalg.qr(W)
    Yt, Xt = Y - Q @ (Q.T @ Y), X - Q @ (Q.T @ X)
    Yt, Xt = Yt - Q @ (Q.T @ Yt), Xt - Q @ (Q.T @ Xt)         # twice is enough
    sxx, syy = np.einsum("ip,ip->p", Xt, Xt), np.einsum("ik,ik->k", Yt, Yt)
    sxy = Yt.T @ Xt
    with np.errstate(all="ignore"):
        rss = syy[:, None] - sxy ** 2 / sxx[None, :]
        out = {"beta": sxy / sxx, "se_beta": np.sqrt(rss / (df * sxx)), "tau": df / rss, "F_wald": df * sxy ** 2 / (sxx * rss)}
    return out, float(np.linalg.cond(W.T @ W))


def ulps(a32, t64):
    t32 = t64.astype(np.float32)
    ai, ti = a32.view(np.int32).astype(np.int64), t32.view(np.int32).astype(np.int64)
    return np.abs(ai - ti)


def gate(got, tr, kappa, n, c, tag=""):
    from scipy import stats
    tol = 1e-9 * max(1.0, kappa * 1e-6)
    for k in range(tr["F_wald"].shape[0]):
        F, Ft = got["F_wald"][k], tr["F_wald"][k]
        assert np.isfinite(F).all() and np.isfinite(Ft).all(), (tag, k)
        err = np.abs(F - Ft) / np.maximum(Ft, np.median(Ft))
        print(f"{tag} phenotype {k}: max F err {err.max():.3e} (tol {tol:.1e}, cond {kappa:.2e})")
        assert err.max() <= tol, (tag, k, err.max(), kappa)
        for col in ("se_beta", "tau"):
            assert ulps(got[col][k], tr[col][k]).max() <= 1, (tag, k, col)
        if kappa <= 1e6:
            assert ulps(got["beta"][k], tr["beta"][k]).max() <= 1, (tag, k)
        else:
            eb = np.abs(got["beta"][k] - tr["beta"][k]) / np.maximum(np.abs(tr["beta"][k]), np.median(np.abs(tr["beta"][k])))
            assert eb.max() <= 2.0 ** -23 * kappa * 1e-6, (tag, k, eb.max(), kappa)
        assert np.allclose(got["p_wald"][k], stats.f.sf(F, 1, n - c - 1), rtol=1e-8, atol=0), (tag, k)


@functools.lru_cache(maxsize=None)
def _panel(n, c, t, p=130, seed=0):
    """W (n,c) with an intercept, Y (n,t) with some signal, X (n,p): imputed dosages (a general float32 matrix)."""
    rng = np.random.default_rng(seed + 1000 * n + 10 * c + t)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    X = (rng.binomial(2, rng.uniform(0.1, 0.5, p), (n, p)) + 0.1 * rng.standard_normal((n, p))).astype(np.float32)
    Y = (rng.standard_normal((n, t)) + 0.2 * X[:, : min(p, 5)] @ rng.standard_normal((min(p, 5), t))).astype(np.float32)
    for a in (W, X, Y):
        a.flags.writeable = False
    return W, Y, X


@functools.lru_cache(maxsize=None)
def _panel_truth(n, c, t):
    return truth(*_panel(n, c, t))


@pytest.mark.parametrize("n", [37, 203, 384, 2000])
@pytest.mark.parametrize("c,t", [(1, 1), (5, 1), (30, 1), (10, 6), (10, 7), (30, 34)])
def test_kernel_against_fp64_truth(ctx, n, c, t):
    from pygemma_amd import ops
    W, Y, X = _panel(n, c, t)
    tr, kappa = _panel_truth(n, c, t)
    for order, Xk in (("C", X), ("F", np.asfortranarray(X))):
        got = ops.lm(W, Y, Xk, ctx=ctx)
        assert all(got[col].shape == (t, X.shape[1]) for col in COLS)
        gate(got, tr, kappa, n, c, f"n={n} c={c} t={t} {order}")


def _genotypes(n, p, seed, miss=0.0):
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, rng.uniform(0.1, 0.5, p), (n, p)).astype(np.float64)
    if miss:
        G[rng.random((n, p)) < miss] = np.nan
    return G


def test_every_storage_kind_meets_the_gate(ctx, tmp_path):
    from pygemma_amd import ops
    from pygemma_amd.bed import PackedBed, write_bed
    n, p, c, t = 203, 130, 5, 2
    W, Y, _ = _panel(n, c, t)
    G = _genotypes(n, p, 3)
    write_bed(str(tmp_path / "full"), G)
    Gf = G.astype(np.float32)
    tr, kappa = truth(W, Y, Gf)
    kinds = {"f32 C": Gf, "f32 F": np.asfortranarray(Gf), "f64 C": G, "f64 F": np.asfortranarray(G), "i8 C": G.astype(np.int8),
             "i8 F": np.asfortranarray(G.astype(np.int8)), "u8 C": G.astype(np.uint8), "u8 F": np.asfortranarray(G.astype(np.uint8)),
             "bed": PackedBed.open(str(tmp_path / "full"))}
    for tag, Xk in kinds.items():
        gate(ops.lm(W, Y, Xk, ctx=ctx), tr, kappa, n, c, tag)
    # ~3 % missing calls: the truth is the host decode with mean imputation; its float32 and float64 images meet the same truth
    Gm = _genotypes(n, p, 4, miss=0.03)
    assert np.isnan(Gm).any(axis=0).sum() > p // 2
    write_bed(str(tmp_path / "miss"), Gm)
    for a1 in (False, True):
        bed = PackedBed.open(str(tmp_path / "miss"), count_A1=a1)
        Xi = bed.to_float(impute=True)
        tr, kappa = truth(W, Y, Xi)
        gate(ops.lm(W, Y, bed, ctx=ctx), tr, kappa, n, c, f"bed missing count_A1={a1}")
        gate(ops.lm(W, Y, Xi, ctx=ctx), tr, kappa, n, c, f"imputed f32 count_A1={a1}")
        gate(ops.lm(W, Y, np.asfortranarray(Xi.astype(np.float64)), ctx=ctx), tr, kappa, n, c, f"imputed f64 count_A1={a1}")
    # float64 values that are not float32 numbers are rounded per element, as X.astype(np.float32) does
    X64 = Gf.astype(np.float64) * (1.0 + 1e-9) + 1e-10
    tr, kappa = truth(W, Y, X64.astype(np.float32))
    gate(ops.lm(W, Y, X64, ctx=ctx), tr, kappa, n, c, "f64 rounded C")
    gate(ops.lm(W, Y, np.asfortranarray(X64), ctx=ctx), tr, kappa, n, c, "f64 rounded F")


def kernel(ctx, W, Y, X, snp_major, ldX=None, ldo=None, bed=None, count_a1=0, want_p=True):
    """pg_lm_setup_dev + one scan call on a block copied into rows of pitch ldX whose pad holds NaN (0xff bytes for 8-bit and .bed
    blocks), with outputs of pitch ldo pre-filled with 0x7f: the pads of the outputs must come back untouched.
    X: (p, n) when snp_major else (n, p); bed: packed records (p, ceil(n/4)) instead.  Returns (t, p) columns."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, c = W.shape
    Yt = np.ascontiguousarray(np.asarray(Y, np.float32).reshape(n, -1).T)
    t = Yt.shape[0]
    src = bed if bed is not None else X
    rows, width = src.shape
    p = rows if (bed is not None or snp_major) else width
    ldX, ldo = ldX or width, ldo or p
    if src.dtype.kind == "f":
        Xp = np.full((rows, ldX), np.nan, src.dtype)
    else:
        Xp = np.full((rows, ldX), -1, np.int64).astype(src.dtype)
    Xp[:, :width] = src
    dW, dY, dX = ctx.to_device(np.ascontiguousarray(W, np.float32)), ctx.to_device(Yt), ctx.to_device(Xp)
    work = ctx.alloc(L.pg_lm_work_bytes(n, c, t))
    outs = [ctx.alloc(t * ldo * (4 if k < 3 else 8)) for k in range(5)]
    for k, b in enumerate(outs):
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, t * ldo * (4 if k < 3 else 8)), "pg_memset")
    _lib.check(L.pg_lm_setup_dev(ctx.handle, n, c, t, dW.ptr, dY.ptr, n, work.ptr), "pg_lm_setup_dev")
    ptrs = [b.ptr for b in outs]
    if not want_p:
        ptrs[4] = None
    if bed is not None:
        _lib.check(L.pg_lm_bed_dev(ctx.handle, n, c, t, p, dX.ptr, ldX, count_a1, work.ptr, *ptrs, ldo), "pg_lm_bed_dev")
    else:
        _lib.check(L.pg_lm_x_dev(ctx.handle, n, c, t, p, dX.ptr, DTYPES[X.dtype], ldX, int(snp_major), work.ptr, *ptrs, ldo), "pg_lm_x_dev")
    ctx.sync()
    res = {}
    for k, (col, b) in enumerate(zip(COLS, outs)):
        full = b.download((t, ldo), np.float32 if k < 3 else np.float64)
        pad = np.ascontiguousarray(full[:, p:]).view(np.uint8)
        assert (pad == 0x7f).all(), f"{col}: the pad of the output rows was written"
        if k == 4 and not want_p:
            assert (full.view(np.uint8) == 0x7f).all()
        res[col] = np.ascontiguousarray(full[:, :p])
    for b in (dW, dY, dX, work, *outs):
        b.free()
    return res


def test_rows_depend_only_on_their_snp(ctx):
    from pygemma import lmm
    n, p, c, t = 384, 4099, 5, 3
    W, Y, X = _panel(n, c, t, p=p, seed=5)
    Xs = np.ascontiguousarray(X.T)                                   # SNP-major (p, n)
    full = kernel(ctx, W, Y, Xs, True)
    assert np.isfinite(full["F_wald"]).all()
    sample_major = kernel(ctx, W, Y, X, False)
    for tag, r in (("ldX", kernel(ctx, W, Y, Xs, True, ldX=n + 64)), ("odd ldX", kernel(ctx, W, Y, Xs, True, ldX=n + 3)),
                   ("ldo", kernel(ctx, W, Y, Xs, True, ldo=p + 37)), ("no pval", kernel(ctx, W, Y, Xs, True, want_p=False))):
        for col in COLS[:4] if tag == "no pval" else COLS:
            assert same_bits(full[col], r[col]), (tag, col)
    padded = kernel(ctx, W, Y, X, False, ldX=p + 5, ldo=p + 1)
    for col in COLS:
        assert same_bits(sample_major[col], padded[col]), col
    rng = np.random.default_rng(0)
    for q in (1, 7, 130, 4099):
        idx = rng.permutation(p)[:q]
        sub = kernel(ctx, W, Y, Xs[idx], True, ldX=n + 3, ldo=q + 2)
        sub_s = kernel(ctx, W, Y, np.ascontiguousarray(X[:, idx]), False, ldX=q + 1)
        for col in COLS:
            assert same_bits(sub[col], full[col][:, idx]), (q, col)
            assert same_bits(sub_s[col], sample_major[col][:, idx]), (q, col)
    # the driver: any batch size, either memory order
    for Xk, ref in ((np.asfortranarray(X), full), (X, sample_major)):
        for sb in (64, 1000, None):
            st = {}
            fr = lmm.pygemma_lm(Y, Xk, W, snp_batch=sb, stats=st)
            assert list(fr) == [0, 1, 2]
            assert st["batches"] == (1 if sb is None else -(-p // sb)) and st["bytes_in"] == 4 * n * p
            for k in range(t):
                for col in COLS:
                    assert same_bits(fr[k][col].to_numpy(), ref[col][k]), (sb, k, col)


def _nan_row(r, k, g):
    return all(np.isnan(r[col][k, g]) for col in COLS)


def test_degenerate_rows(ctx, tmp_path):
    from pygemma_amd import ops
    from pygemma_amd.bed import PackedBed, write_bed
    n, c, t = 384, 3, 2
    W, Y, X = _panel(n, c, t, p=12, seed=9)
    assert (W[:, 0] == 1).all()                                      # the intercept
    X = X.copy()
    X[:, 0] = 0.0
    X[:, 1] = 2.0                                                    # constant
    X[:, 2] = np.float32(3.0) * W[:, 1]                              # a multiple of a covariate
    X[:, 3] = W[:, 0] - np.float32(2.0) * W[:, 1] + np.float32(0.5) * W[:, 2]     # in span(W)
    X[5, 4] = np.nan
    X[7, 5] = np.inf
    X[383, 6] = -np.inf                                              # in the last, partial k-group
    for Xk in (X, np.asfortranarray(X), X.astype(np.float64)):
        r = ops.lm(W, Y, Xk, ctx=ctx)
        for k in range(t):
            for g in range(7):
                assert _nan_row(r, k, g), (k, g)
            for g in range(7, 12):
                assert all(np.isfinite(r[col][k, g]) for col in COLS), (k, g)
    # an all-missing .bed record between called ones
    G = _genotypes(n, 12, 2, miss=0.03)
    G[:, 2] = np.nan
    write_bed(str(tmp_path / "am"), G)
    for a1 in (False, True):
        r = ops.lm(W, Y, PackedBed.open(str(tmp_path / "am"), count_A1=a1), ctx=ctx)
        for k in range(t):
            assert _nan_row(r, k, 2)
            assert all(np.isfinite(r[col][k, g]) for col in COLS for g in range(12) if g != 2), k
    # a duplicated covariate: NaN everywhere
    Wd = np.ascontiguousarray(np.concatenate([W, W[:, 1:2]], axis=1))
    r = ops.lm(Wd, Y, _panel(n, c, t, p=12, seed=9)[2], ctx=ctx)
    assert all(np.isnan(r[col]).all() for col in COLS)
    # a non-finite covariate too
    Wn = W.copy()
    Wn[3, 1] = np.nan
    r = ops.lm(Wn, Y, _panel(n, c, t, p=12, seed=9)[2], ctx=ctx)
    assert all(np.isnan(r[col]).all() for col in COLS)
    # a NaN in one phenotype: that phenotype only
    Yn = Y.copy()
    Yn[10, 1] = np.nan
    Xg = _panel(n, c, t, p=12, seed=9)[2]
    r, clean = ops.lm(W, Yn, Xg, ctx=ctx), ops.lm(W, Y, Xg, ctx=ctx)
    for col in COLS:
        assert np.isnan(r[col][1]).all(), col
        assert same_bits(r[col][0], clean[col][0]), col


def test_abi_misuse_launches_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, c, t, p = 64, 2, 2, 4
    bufs = [ctx.alloc(1 << 16) for _ in range(9)]
    for b in bufs:
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, 1 << 16), "pg_memset")
    ctx.sync()
    W, Y, X, work, beta, se, tau, F, pv = [b.ptr for b in bufs]
    good = dict(n=n, c=c, t=t, pb=p, X=X, dtype=2, ldX=n, sm=1, work=work, beta=beta, F=F, ldo=p, ldb=(n + 3) // 4)

    def x(**kw):
        a = {**good, **kw}
        return L.pg_lm_x_dev(ctx.handle, a["n"], a["c"], a["t"], a["pb"], a["X"], a["dtype"], a["ldX"], a["sm"], a["work"], a["beta"], se, tau,
                             a["F"], pv, a["ldo"])

    def bed(**kw):
        a = {**good, **kw}
        return L.pg_lm_bed_dev(ctx.handle, a["n"], a["c"], a["t"], a["pb"], a["X"], a["ldb"], 0, a["work"], a["beta"], se, tau, a["F"], pv, a["ldo"])

    def setup(**kw):
        a = {"W": W, "Y": Y, "ldy": n, **good, **kw}
        return L.pg_lm_setup_dev(ctx.handle, a["n"], a["c"], a["t"], a["W"], a["Y"], a["ldy"], a["work"])

    for call in (x, bed):
        assert call(X=None) == -22 and call(work=None) == -22 and call(beta=None) == -22 and call(F=None) == -22
        assert call(c=0) == -95 and call(c=31) == -95
        assert call(c=30, t=35, n=128) == -95
        assert call(t=0) == -22
        assert call(n=3, c=2) == -22
        assert call(ldo=p - 1) == -22
        assert call(pb=-1) == -22
    assert x(ldX=n - 1) == -22 and x(sm=0, ldX=p - 1) == -22
    assert x(dtype=4) == -22 and x(dtype=-1) == -22
    assert bed(ldb=(n + 3) // 4 - 1) == -22
    assert setup(W=None) == -22 and setup(Y=None) == -22 and setup(work=None) == -22
    assert setup(c=0) == -95 and setup(c=31) == -95 and setup(c=30, t=35, n=128) == -95
    assert setup(t=0) == -22 and setup(n=3, c=2) == -22 and setup(ldy=n - 1) == -22
    ctx.sync()
    for b in bufs[3:]:
        assert (b.download((1 << 16,), np.uint8) == 0x7f).all()       # neither the work area nor an output was written


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def test_agrees_with_the_mixed_model_at_zero_eigenvalues():
    """With d = 0 the mixed model is OLS: lmm.pygemma on (Y, X, W, d = 0, eigen=False) is the code that already exists."""
    from pygemma import lmm
    n, p, c = 2000, 1500, 4
    rng = np.random.default_rng(17)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    X = rng.binomial(2, rng.uniform(0.1, 0.5, p), (n, p)).astype(np.float32)
    Y = (0.1 * X[:, :10] @ rng.standard_normal(10) + rng.standard_normal(n)).astype(np.float32).reshape(-1, 1)
    lm = lmm.pygemma_lm(Y, X, W)
    mm = lmm.pygemma(Y, X, W, np.zeros(n, np.float32), eigen=False)
    tr, _ = truth(W, Y, X)
    keep = tr["F_wald"][0] >= 1e-2
    assert keep.mean() >= 0.8, keep.mean()
    rel = np.abs(lm["F_wald"].to_numpy()[keep] / mm["F_wald"].to_numpy()[keep] - 1)
    print(f"linear model against the Wald scan at d = 0: max |F/F_wald - 1| {rel.max():.3e} on {keep.sum()} of {p} rows")
    assert rel.max() <= 1e-4


def test_frames_and_several_phenotypes():
    import pandas as pd
    from pygemma import lmm
    from scipy import stats
    n, p, c, t = 384, 700, 3, 3
    W, Y, X = _panel(n, c, t, p=p, seed=2)
    snps = [f"rs{i}" for i in range(p)]
    st = {}
    one = lmm.pygemma_lm(Y[:, 0], X, W, snps=snps, stats=st)
    assert list(one.columns) == list(COLS) + ["SNPs"] and list(one["SNPs"]) == snps
    assert [str(one[col].dtype) for col in COLS] == ["float32", "float32", "float32", "float64", "float64"]
    assert lmm.pygemma_lm(Y[:, :1], X, W).shape == (p, 5)
    assert isinstance(st["lambda_gc"], list) and len(st["lambda_gc"]) == 1
    assert st["lambda_gc"][0] == float(np.median(stats.chi2.isf(one["p_wald"].to_numpy(), 1)) / 0.4549364)
    assert st["batches"] == 1 and st["bytes_in"] == 4 * n * p and st["seconds"] > 0
    st3 = {}
    many = lmm.pygemma_lm(Y, X, W, snps=snps, stats=st3)
    assert list(many) == [0, 1, 2] and len(st3["lambda_gc"]) == 3
    labelled = lmm.pygemma_lm(pd.DataFrame(np.asarray(Y), columns=["bmi", "ldl", "hdl"]), X, W, snps=snps)
    assert list(labelled) == ["bmi", "ldl", "hdl"]
    for k, lab in enumerate(["bmi", "ldl", "hdl"]):
        single = lmm.pygemma_lm(Y[:, k], X, W, snps=snps)
        for fr in (many[k], labelled[lab]):
            assert list(fr.columns) == list(single.columns) and list(fr["SNPs"]) == snps
            for col in COLS:
                assert fr[col].dtype == single[col].dtype
                assert same_bits(fr[col].to_numpy(), single[col].to_numpy()), (k, col)
        pv = many[k]["p_wald"].to_numpy()
        assert st3["lambda_gc"][k] == float(np.median(stats.chi2.isf(pv[~np.isnan(pv)], 1)) / 0.4549364)


def test_null_calibration():
    from pygemma import lmm
    n, p = 2000, 20000
    rng = np.random.default_rng(23)
    X = rng.binomial(2, rng.uniform(0.05, 0.5, p), (n, p)).astype(np.int8)       # unrelated samples
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, 2))], axis=1).astype(np.float32)
    Y = rng.standard_normal(n)
    st = {}
    df = lmm.pygemma_lm(Y, X, W, stats=st)
    frac = float((df["p_wald"] < 0.05).mean())
    print(f"null panel: fraction p < 0.05 = {frac:.4f}, lambda_GC = {st['lambda_gc'][0]:.4f}")
    assert 0.035 <= frac <= 0.065, frac
    assert 0.9 <= st["lambda_gc"][0] <= 1.1, st["lambda_gc"]
