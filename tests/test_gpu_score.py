"""GPU checks of the score test (pg_score_null_dev, pg_score_dev, ops.score, lmm.pygemma_score) — run with -m gpu on an MI355X.

The truth is the contract's formulas in fp64 NumPy (P0 from np.linalg.solve, not the kernel's Cholesky route) on the same float32
inputs and the same float32 lambda0."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS = ("beta", "se_beta", "tau", "lambda", "F_score", "p_score")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def truth(d, W, y, X, lam0):
    """Contract formulas in fp64: d (n,), W (n,c), y (n,), X (n,p) float32; lam0 float32.  Returns dict of fp64 columns."""
    d, W, y, X = (np.asarray(a, np.float64) for a in (d, W, y.reshape(-1), X))
    n, c = W.shape
    df = n - c - 1
    h = 1.0 / (np.float64(np.float32(lam0)) * d + 1.0)
    HW = h[:, None] * W
    G = W.T @ HW
    if n <= 2000:                                       # the dense P0 of the contract
        P0 = np.diag(h) - HW @ np.linalg.solve(G, HW.T)
        P0y, P0X = P0 @ y, P0 @ X
    else:                                               # the same operator applied without forming it
        P0y = h * y - HW @ np.linalg.solve(G, HW.T @ y)
        P0X = h[:, None] * X - HW @ np.linalg.solve(G, HW.T @ X)
    pyy, pxy, pxx = y @ P0y, X.T @ P0y, np.einsum("ip,ip->p", X, P0X)
    s = np.einsum("ip,ip->p", X, h[:, None] * X)
    with np.errstate(all="ignore"):
        ok = np.isfinite(s) & np.isfinite(pxx) & (pxx > 1e-10 * s)
        pxyy = pyy - pxy * pxy / pxx
        out = {"beta": pxy / pxx, "se_beta": np.sqrt(pxyy / (df * pxx)), "tau": df / pxyy, "F_score": n * pxy ** 2 / (pyy * pxx)}
    for k in out:
        out[k] = np.where(ok, out[k], np.nan)
    out["ok"] = ok
    return out


def ml_loglik(d, W, y, lam):
    """fp64 ML log-likelihood of y ~ W at lam (the contract's lambda0 check)."""
    d, W, y = (np.asarray(a, np.float64) for a in (d, W, y.reshape(-1)))
    n = len(d)
    h = 1.0 / (lam * d + 1.0)
    HW = h[:, None] * W
    pyy = y @ (h * y) - (HW.T @ y) @ np.linalg.solve(W.T @ HW, HW.T @ y)
    return n / 2 * np.log(n / (2 * np.pi)) - n / 2 - 0.5 * np.sum(np.log(lam * d + 1.0)) - n / 2 * np.log(pyy)


def null_lambda(ctx, d, W, y):
    from pygemma_amd import _lib
    L = _lib.load()
    n, c = W.shape
    dd, dW, dy, dl = ctx.to_device(d), ctx.to_device(W), ctx.to_device(y.reshape(-1)), ctx.alloc(4)
    _lib.check(L.pg_score_null_dev(ctx.handle, n, c, dd.ptr, dW.ptr, dy.ptr, dl.ptr), "pg_score_null_dev")
    ctx.sync()
    lam = dl.download((1,), np.float32)[0]
    for b in (dd, dW, dy, dl):
        b.free()
    return lam


def kernel(ctx, d, W, y, Xs, lam0, ldx=None):
    """pg_score_dev on SNP-major Xs (p, n) copied into rows of pitch ldx."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, c = W.shape
    p = Xs.shape[0]
    ldx = ldx or n
    Xp = np.full((max(p, 1), ldx), np.nan, np.float32)       # pad columns hold NaN: they must never be read
    Xp[:p, :n] = Xs
    dd, dW, dy, dX = ctx.to_device(d), ctx.to_device(W), ctx.to_device(y.reshape(-1)), ctx.to_device(Xp)
    o = [ctx.alloc(max(p, 1) * 4) for _ in range(4)] + [ctx.alloc(max(p, 1) * 8) for _ in range(2)]
    _lib.check(L.pg_score_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, float(lam0), dX.ptr, ldx, *[b.ptr for b in o]), "pg_score_dev")
    ctx.sync()
    r = {col: b.download((p,), np.float32 if k < 4 else np.float64) for k, (col, b) in enumerate(zip(COLS, o))}
    for b in (dd, dW, dy, dX, *o):
        b.free()
    return r


@functools.lru_cache(maxsize=None)
def _panel(n, c, p=64, seed=0):
    from pygemma_amd import synth
    rp = synth.fast_rotated_panel(n, p, c, seed=seed + 10 * n + c)
    return rp["d"], np.ascontiguousarray(rp["W"]), np.ascontiguousarray(rp["Y"].reshape(-1)), np.ascontiguousarray(rp["X"].T)


def ulps(a32, t64):
    t32 = t64.astype(np.float32)
    ai, ti = a32.view(np.int32).astype(np.int64), t32.view(np.int32).astype(np.int64)
    return np.abs(ai - ti)


@pytest.mark.parametrize("n", [37, 384, 2000, 10000])
@pytest.mark.parametrize("c", [1, 2, 5, 10, 26, 30])
def test_kernel_against_fp64_truth(ctx, n, c):
    from scipy import stats
    d, W, y, Xs = _panel(n, c)
    lam0 = null_lambda(ctx, d, W, y)
    assert np.isfinite(lam0) and lam0 > 0
    got = kernel(ctx, d, W, y, Xs, lam0)
    tr = truth(d, W, y, Xs.T, lam0)
    assert tr["ok"].all()
    # 1e-9 relative, measured against max(F, median F): F ~ P_xy^2, and the absolute error of P_xy (any fp64 route: the kernel's
    # Cholesky, the truth's solve) is eps cond(G) |x|_P0 |y|_P0, so a SNP with P_xy near 0 has a large RELATIVE error in both.  The
    # bound widens with cond(G) past 1e6: at n = 37, c = 30 (df = 6) cond(G) reaches 1.3e7 and the two fp64 routes differ by 1.3e-9
    # relative at F ~ 1 (a CPU replay of the kernel's arithmetic gives the same).
    F, Ft = got["F_score"], tr["F_score"]
    h = 1.0 / (np.float64(lam0) * d.astype(np.float64) + 1.0)
    kappa = np.linalg.cond(W.astype(np.float64).T @ (h[:, None] * W.astype(np.float64)))
    tol = 1e-9 * max(1.0, kappa * 1e-6)
    err = np.abs(F - Ft) / np.maximum(Ft, np.median(Ft))
    assert err.max() <= tol, (err.max(), kappa)
    for col in ("se_beta", "tau"):
        assert ulps(got[col], tr[col]).max() <= 1, col
    if kappa <= 1e6:
        assert ulps(got["beta"], tr["beta"]).max() <= 1
    else:     # beta ~ P_xy: the same widening, its error measured against max(|beta|, median |beta|) in float32 ulps of 1
        eb = np.abs(got["beta"] - tr["beta"]) / np.maximum(np.abs(tr["beta"]), np.median(np.abs(tr["beta"])))
        assert eb.max() <= 2.0 ** -23 * kappa * 1e-6, (eb.max(), kappa)
    assert (bits(got["lambda"]) == bits(np.full(len(got["lambda"]), lam0, np.float32))).all()
    ref_p = stats.f.sf(got["F_score"], 1, n - c - 1)
    assert np.allclose(got["p_score"], ref_p, rtol=1e-8, atol=0)


@pytest.mark.parametrize("n,c", [(384, 1), (384, 5), (2000, 5), (2000, 10), (10000, 5)])
def test_null_lambda_is_the_ml_maximum(ctx, n, c):
    from pygemma import lmm
    d, W, y, _ = _panel(n, c)
    lam0 = float(null_lambda(ctx, d, W, y))
    grid = np.logspace(-5, 5, 2001)
    best = max(ml_loglik(d, W, y, g) for g in grid)
    l0 = ml_loglik(d, W, y, lam0)
    assert l0 >= best - 1e-6 * abs(best), (lam0, l0, best)
    if 1e-5 < lam0 < 1e5:
        ref = lmm.calc_lambda(d, y.reshape(-1, 1), W)
        assert abs(lam0 - ref) <= 1e-4 * abs(ref), (lam0, ref)


def test_rows_depend_only_on_their_snp(ctx):
    n, c = 384, 5
    from pygemma_amd import synth
    rp = synth.fast_rotated_panel(n, 4099, c, seed=5)
    d, W, y, Xs = rp["d"], np.ascontiguousarray(rp["W"]), rp["Y"].reshape(-1), np.ascontiguousarray(rp["X"].T)
    lam0 = null_lambda(ctx, d, W, y)
    full = kernel(ctx, d, W, y, Xs, lam0)
    padded = kernel(ctx, d, W, y, Xs, lam0, ldx=n + 64)
    for col in COLS:
        assert (bits(full[col]) == bits(padded[col])).all(), col
    rng = np.random.default_rng(0)
    for p in (1, 7, 130, 4099):
        idx = rng.permutation(4099)[:p]
        sub = kernel(ctx, d, W, y, Xs[idx], lam0, ldx=n + 3)
        for col in COLS:
            assert (bits(sub[col]) == bits(full[col][idx])).all(), (p, col)


def _nan_row(r, g):
    return all(np.isnan(r[col][g]) for col in ("beta", "se_beta", "tau", "F_score", "p_score"))


def test_degenerate_snps_and_covariates(ctx):
    n, c = 384, 3
    d, W, y, Xs = _panel(n, c, p=8)
    W = W.copy()
    W[:, 0] = np.float32(1.0) + np.float32(0.1) * W[:, 0]          # an intercept-like column
    Xs = Xs.copy()
    Xs[0] = np.float32(2.0) * W[:, 0]                                # monomorphic: a multiple of the intercept
    Xs[1] = W[:, 0] - np.float32(2.0) * W[:, 1]                      # x in span(W)
    Xs[2, 5] = np.nan
    Xs[3, 7] = np.inf
    Xs[4] = 0.0
    lam0 = null_lambda(ctx, d, W, y)
    r = kernel(ctx, d, W, y, Xs, lam0)
    for g in (0, 1, 2, 3, 4):
        assert _nan_row(r, g), g
    for g in (5, 6, 7):
        assert np.isfinite(r["F_score"][g]) and np.isfinite(r["beta"][g])
    assert (r["lambda"] == lam0).all()
    # rank-deficient W: every row NaN except lambda
    Wd = np.ascontiguousarray(np.concatenate([W, W[:, 1:2]], axis=1))
    r = kernel(ctx, d, Wd, y, Xs, np.float32(1.0))
    assert all(_nan_row(r, g) for g in range(8)) and (r["lambda"] == np.float32(1.0)).all()


def test_degenerate_panels_never_raise(ctx):
    from pygemma_amd import synth
    full_rank_finite = {"plain", "d = 0", "d huge", "d half zero", "d tiny", "y = 0", "y * 1e20", "y * 1e-20", "y = w0", "y with NaN",
                        "W * 1e20"}
    for tag, d, W, y, X in synth.degenerate_panels():
        W = np.ascontiguousarray(W)
        lam0 = null_lambda(ctx, d, W, y)
        r = kernel(ctx, d, W, y, np.ascontiguousarray(X.T), lam0)
        assert (bits(r["lambda"]) == bits(np.full(X.shape[1], lam0, np.float32))).all(), tag
        for g in (8, 9, 10, 13):                                      # NaN / inf in x
            assert _nan_row(r, g), (tag, g)
        if tag in full_rank_finite:
            for g in (0, 1, 2, 3, 11):                                # zero, constant, = w0, = w_last, in span(W)
                assert _nan_row(r, g), (tag, g)
        if tag in ("W duplicate column", "W zero column", "W with NaN", "d with NaN"):
            assert all(_nan_row(r, g) for g in range(X.shape[1])), tag


def test_abi_misuse_launches_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, c, p = 64, 2, 4
    bufs = [ctx.alloc(4096) for _ in range(10)]
    for b in bufs:
        _lib.check(L.pg_memset(ctx.handle, b.ptr, 0x7f, 4096), "pg_memset")
    ctx.sync()
    d, W, y, X, beta, se, tau, lam, F, pv = [b.ptr for b in bufs]
    good = dict(n=n, c=c, p=p, ldx=n)
    def call(**kw):
        a = {**good, **kw}
        return L.pg_score_dev(ctx.handle, a["n"], a["c"], a["p"], a.get("d", d), W, y, 1.0, a.get("X", X), a["ldx"], beta, se, tau, lam, F, pv)
    assert call(d=None) == -22
    assert call(X=None) == -22
    assert call(c=0) == -95 and call(c=31) == -95
    assert call(n=3, c=2) == -22
    assert call(ldx=n - 1) == -22
    assert L.pg_score_null_dev(ctx.handle, n, 31, d, W, y, lam) == -95
    assert L.pg_score_null_dev(ctx.handle, 3, 2, d, W, y, lam) == -22
    assert L.pg_score_null_dev(ctx.handle, n, c, d, W, y, None) == -22
    ctx.sync()
    for b in bufs[5:]:
        assert (b.download((4096,), np.uint8) == 0x7f).all()          # no output was written


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------

def _frames_equal(a, b):
    assert list(a.columns) == list(b.columns)
    for col in a.columns:
        if col == "SNPs":
            assert list(a[col]) == list(b[col])
            continue
        assert a[col].dtype == b[col].dtype, col
        assert (bits(a[col].to_numpy()) == bits(b[col].to_numpy())).all(), col


def test_pipeline_eigen_false_matches_the_kernel(ctx):
    from pygemma import lmm
    from pygemma_amd import ops
    d, W, y, Xs = _panel(2000, 5, p=3000)
    st = {}
    df = lmm.pygemma_score(y.reshape(-1, 1), np.ascontiguousarray(Xs.T), W, d, eigen=False, stats=st)
    assert list(df.columns) == list(COLS)
    assert [str(df[col].dtype) for col in COLS] == ["float32", "float32", "float32", "float64", "float64", "float64"]
    k = ops.score(d, W, y, np.ascontiguousarray(Xs.T), ctx=ctx)
    assert np.float32(st["lambda_null"]) == np.float32(k["lambda_null"])
    for col in COLS:
        assert (bits(df[col].to_numpy()) == bits(k[col])).all(), col


def _raw(n=384, p=600, c=3, seed=3):
    from pygemma_amd import synth
    raw = synth.exact_panel(n, p, c, seed=seed)
    rng = np.random.default_rng(seed)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    G = raw["X"]
    y = G[:, :20] @ rng.standard_normal(20) + rng.standard_normal(n)
    return y.reshape(-1, 1), G, W, raw["K"]


def test_pipeline_x_kinds_agree_where_wald_does(tmp_path):
    from pygemma import lmm
    from pygemma_amd.bed import PackedBed, write_bed
    Y, G, W, K = _raw()
    write_bed(str(tmp_path / "toy"), G.astype(np.float64))
    kinds = {"f32": G, "f32_snp_major": np.asfortranarray(G), "f64": G.astype(np.float64), "i8": G.astype(np.int8),
             "u8": G.astype(np.uint8), "bed": PackedBed.open(str(tmp_path / "toy"))}
    wald = {k: lmm.pygemma(Y, X, W, K) for k, X in kinds.items()}
    score = {k: lmm.pygemma_score(Y, X, W, K) for k, X in kinds.items()}
    names = list(kinds)
    pairs = 0
    for i, a in enumerate(names):
        assert np.isfinite(score[a]["F_score"]).all(), a
        for b in names[i + 1:]:
            if all((bits(wald[a][col].to_numpy()) == bits(wald[b][col].to_numpy())).all() for col in wald[a].columns):
                _frames_equal(score[a], score[b])
                pairs += 1
    assert pairs >= 1


def _fp64_truth_eigen(Y, X, W, K, lam0):
    d, U = np.linalg.eigh(np.asarray(K, np.float64))
    d = np.maximum(d, 0.0)
    R = lambda A: U.T @ np.asarray(A, np.float64)
    return truth(d, R(W), R(Y).reshape(-1), R(X), lam0)


def test_pipeline_against_fp64_truth_with_eigenpairs_and_Z():
    from pygemma import lmm
    from pygemma_amd import synth
    n, p, c = 2000, 1500, 4
    raw = synth.panel(n, p, c, seed=11)
    st = {}
    df = lmm.pygemma_score(raw["Y"], raw["X"], raw["W"], raw["K"], stats=st)
    lam0 = np.float32(st["lambda_null"])
    tr = _fp64_truth_eigen(raw["Y"], raw["X"], raw["W"], raw["K"], lam0)
    F, Ft = df["F_score"].to_numpy(), tr["F_score"]
    big = Ft >= 1e-2
    rel = np.abs(F[big] / Ft[big] - 1)
    print(f"fp64 truth, n = {n}: max rel err of F_score (F >= 1e-2) {rel.max():.3e}, median {np.median(rel):.3e}")
    assert rel.max() <= 1e-4
    # precomputed eigenpairs: the same gate
    d, U = np.linalg.eigh(raw["K"].astype(np.float64))
    df_e = lmm.pygemma_score(raw["Y"], raw["X"], raw["W"], None, eigenpairs=(d, U))
    Fe = df_e["F_score"].to_numpy()
    assert np.all(np.abs(Fe[big] / Ft[big] - 1) <= 1e-4)
    # Z = I: K is what the eigensolver sees, bit for bit
    df_z = lmm.pygemma_score(raw["Y"], raw["X"], raw["W"], raw["K"], Z=np.eye(n, dtype=np.float32))
    _frames_equal(df, df_z)


def test_two_gpus_equal_one():
    from pygemma import lmm
    from pygemma_amd import _lib, synth
    if _lib.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    raw = synth.panel(512, 3001, 3, seed=4)
    snps = [f"rs{i}" for i in range(3001)]
    a = lmm.pygemma_score(raw["Y"], raw["X"], raw["W"], raw["K"], snps=snps, nproc=1)
    b = lmm.pygemma_score(raw["Y"], raw["X"], raw["W"], raw["K"], snps=snps, nproc=2)
    _frames_equal(a, b)


def test_null_calibration_and_agreement_with_wald():
    from pygemma import lmm
    from pygemma_amd import synth
    from scipy import stats
    rp = synth.fast_rotated_panel(2000, 20000, 3, seed=21, null=True)
    df = lmm.pygemma_score(rp["Y"], rp["X"], rp["W"], rp["d"], eigen=False)
    frac = float((df["p_score"] < 0.05).mean())
    assert 0.035 <= frac <= 0.065, frac
    rp = synth.fast_rotated_panel(2000, 5000, 3, seed=22)
    s = lmm.pygemma_score(rp["Y"], rp["X"], rp["W"], rp["d"], eigen=False)
    w = lmm.pygemma(rp["Y"], rp["X"], rp["W"], rp["d"], eigen=False)
    rho = stats.spearmanr(-np.log10(s["p_score"]), -np.log10(w["p_wald"])).correlation
    assert rho > 0.99, rho


def test_full_size():
    from pygemma import lmm
    from pygemma_amd import synth
    n, p, c = 10000, 100000, 5
    rp = synth.fast_rotated_panel(n, p, c, seed=31)
    st = {}
    df = lmm.pygemma_score(rp["Y"], rp["X"], rp["W"], rp["d"], eigen=False, stats=st)
    for col in COLS:
        assert np.isfinite(df[col].to_numpy()).all(), col
    idx = np.random.default_rng(0).choice(p, 256, replace=False)
    tr = truth(rp["d"], rp["W"], rp["Y"], rp["X"][:, idx], np.float32(st["lambda_null"]))
    F, Ft = df["F_score"].to_numpy()[idx], tr["F_score"]
    big = Ft >= 1e-2
    assert np.all(np.abs(F[big] / Ft[big] - 1) <= 1e-4)
