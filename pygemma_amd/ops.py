"""Array-level wrappers over the C ABI (host NumPy in / out).  HIP path only."""
import ctypes as C

import numpy as np

from . import _lib
from ._feed import _KIN_DTYPES, _call_dev, _describe, _genotypes     # noqa: F401  (_KIN_DTYPES: re-exported)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ldx(n):     # row pitch, in floats, of a rotated SNP-major block
    return (n + 63) // 64 * 64


def _six_alloc(ctx, p):     # device columns of a scan's p result rows: beta, se_beta, tau, lambda (float32), F, p (float64)
    return [ctx.alloc(max(p, 1) * 4) for _ in range(4)] + [ctx.alloc(max(p, 1) * 8) for _ in range(2)]


def _six_download(out, p, F, pv):     # ... as host arrays, the last two named `F` and `pv`, lambda widened as in the reference's frame
    res = {col: b.download((p,), np.float32 if k < 4 else np.float64) for k, (col, b) in enumerate(zip(("beta", "se_beta", "tau", "lambda", F, pv), out))}
    res["lambda"] = res["lambda"].astype(np.float64)
    return res


def assoc(d, Wr, yr, Xr, grid=False, ctx=None, want_p=True, return_stats=False):
    """calculate((eigenVals, Y, W, X_block, grid)) (lmm/lmm.py:461) on the GPU.
    d (n,), Wr (n,c), yr (n,) or (n,1), Xr (n,p) in the REFERENCE layout, all in the eigenbasis."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        d, Wr, yr, Xr = _f32(d), _f32(Wr), _f32(np.asarray(yr).reshape(-1)), _f32(Xr)
        n, c = Wr.shape
        p = Xr.shape[1]
        assert d.shape == (n,) and yr.shape == (n,) and Xr.shape[0] == n
        beta, se, tau, lam = (np.empty(p, np.float32) for _ in range(4))
        F, pv = np.empty(p, np.float64), np.empty(p, np.float64)
        stats = np.zeros(2, np.uint64)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        dpass = ctx.to_device(np.zeros(4, np.uint64)) if return_stats else None
        if return_stats:
            _lib.check(L.pg_assoc_set_pass_stats(ctx.handle, dpass.ptr), "pg_assoc_set_pass_stats")
        try:
            _lib.check(L.pg_assoc(ctx.handle, n, c, p, vp(d), vp(Wr), vp(yr), vp(Xr), int(bool(grid)), vp(beta), vp(se),
                                  vp(tau), vp(lam), vp(F), vp(pv) if want_p else None, vp(stats)), "pg_assoc")
        finally:
            if return_stats:
                L.pg_assoc_set_pass_stats(ctx.handle, None)
        out = {"beta": beta, "se_beta": se, "tau": tau, "lambda": lam.astype(np.float64), "F_wald": F,
               "p_wald": pv if want_p else None}
        if return_stats:
            out["n_evals"] = stats.astype(np.int64)
            # passes over n that produced P, Q, R (a fused pass counts once per power) and Newton starts on Brent's P and Q
            out["passes"] = dpass.download((4,), np.uint64).astype(np.int64)
        return out


def score(d, Wr, yr, Xr, lam0=None, ctx=None):
    """The score test at the null model's ML lambda (pg_score_null_dev + pg_score_dev) on the GPU.
    d (n,), Wr (n,c), yr (n,) or (n,1), Xr (n,p) in the REFERENCE layout, all in the eigenbasis.  lam0: the float32 lambda to
    evaluate at (None: the ML lambda of y ~ W, computed on the device).  Returns dict(beta, se_beta, tau, lambda, F_score,
    p_score, lambda_null)."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        d, Wr, yr, Xr = _f32(d), _f32(Wr), _f32(np.asarray(yr).reshape(-1)), _f32(Xr)
        n, c = Wr.shape
        p = Xr.shape[1]
        assert d.shape == (n,) and yr.shape == (n,) and Xr.shape[0] == n
        dd, dW, dy = ctx.to_device(d), ctx.to_device(Wr), ctx.to_device(yr)
        if lam0 is None:
            dl = ctx.alloc(4)
            _lib.check(L.pg_score_null_dev(ctx.handle, n, c, dd.ptr, dW.ptr, dy.ptr, dl.ptr), "pg_score_null_dev")
            ctx.sync()
            lam0 = dl.download((1,), np.float32)[0]
        lam0 = np.float32(lam0)
        dX = ctx.to_device(Xr)
        dXr = ctx.alloc(max(p, 1) * n * 4)
        out = _six_alloc(ctx, p)
        if p:
            _lib.check(L.pg_transpose_dev(ctx.handle, n, p, dX.ptr, p, dXr.ptr, n), "pg_transpose_dev")
        _lib.check(L.pg_score_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, float(lam0), dXr.ptr, n, *[b.ptr for b in out]),
                   "pg_score_dev")
        ctx.sync()
        res = _six_download(out, p, "F_score", "p_score")
        res["lambda_null"] = float(lam0)
        return res


LM_COLS = ("beta", "se_beta", "tau", "F_wald", "p_wald")


def lm(W, Y, X, ctx=None):
    """The plain linear model y_k ~ W + x per SNP (pg_lm_setup_dev + one pg_lm_{bed,x}_dev call) on the GPU, from raw
    genotypes.  W (n,c); Y (n,) or (n,t); X (n,p): a PackedBed, or an int8, uint8, float32 or float64 array that is handed over as
    it is stored (C order: sample-major, Fortran order: SNP-major; anything else is copied to C order, other dtypes are cast to
    float32).  Returns dict(beta, se_beta, tau, F_wald, p_wald) of (t, p) arrays (float32 x 3, float64 x 2)."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        W = _f32(W)
        Y = np.asarray(Y)
        Yt = _f32(Y.reshape(Y.shape[0], -1).T)                 # phenotype-major rows
        n, c = W.shape
        t = Yt.shape[0]
        src = _describe(_genotypes(X, "ops.lm", cast=True))
        assert Yt.shape[1] == n and src.n == n
        p = src.p
        dW, dY = ctx.to_device(W), ctx.to_device(Yt)
        work = ctx.alloc(max(int(L.pg_lm_work_bytes(n, c, t)), 256))
        _lib.check(L.pg_lm_setup_dev(ctx.handle, n, c, t, dW.ptr, dY.ptr, n, work.ptr), "pg_lm_setup_dev")
        out = [ctx.alloc(max(t * p, 1) * 4) for _ in range(3)] + [ctx.alloc(max(t * p, 1) * 8) for _ in range(2)]
        dX = ctx.to_device(src.src.data if src.packed else src.src.T if src.snp_major else src.src)     # the whole source, as it is stored
        _call_dev(L, "pg_lm_{}_dev", src, (ctx.handle, n, c, t, p), dX.ptr, p, (work.ptr, *[b.ptr for b in out], p))
        ctx.sync()
        return {col: b.download((t, p), np.float32 if k < 3 else np.float64) for k, (col, b) in enumerate(zip(LM_COLS, out))}


def gxe(d, Wr, yr, Xr, XEr, ctx=None, want_p=True, return_stats=False):
    """The SNP-by-environment Wald test (pg_assoc_gxe_dev) on the GPU: per SNP j, the REML Wald test of XEr[:, j] in
    y ~ Wr + Xr[:, j] + XEr[:, j], i.e. calculate(d, yr, [Wr, Xr[:, j]], XEr[:, j]) with lambda searched per SNP.
    d (n,), Wr (n,c) with U'e as its last column, yr (n,) or (n,1), Xr = U'X and XEr = U'(X o e), each (n,p) in the REFERENCE
    layout, all in the eigenbasis.  Returns dict(beta, se_beta, tau, lambda, F_wald, p_wald[, n_evals]); beta is beta_gxe and
    p_wald uses F(1, n - c - 2)."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        d, Wr, yr, Xr, XEr = _f32(d), _f32(Wr), _f32(np.asarray(yr).reshape(-1)), _f32(Xr), _f32(XEr)
        n, c = Wr.shape
        p = Xr.shape[1]
        assert d.shape == (n,) and yr.shape == (n,) and Xr.shape == (n, p) and XEr.shape == (n, p)
        dd, dW, dy = ctx.to_device(d), ctx.to_device(Wr), ctx.to_device(yr)
        dX, dXE = ctx.to_device(Xr), ctx.to_device(XEr)
        dXr, dXEr = ctx.alloc(max(p, 1) * n * 4), ctx.alloc(max(p, 1) * n * 4)
        out = _six_alloc(ctx, p)
        dst = ctx.alloc(16)
        _lib.check(L.pg_memset(ctx.handle, dst.ptr, 0, 16), "pg_memset")
        if p:
            _lib.check(L.pg_transpose_dev(ctx.handle, n, p, dX.ptr, p, dXr.ptr, n), "pg_transpose_dev")
            _lib.check(L.pg_transpose_dev(ctx.handle, n, p, dXE.ptr, p, dXEr.ptr, n), "pg_transpose_dev")
        _lib.check(L.pg_assoc_gxe_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, dXr.ptr, n, dXEr.ptr, n,
                                      *[b.ptr for b in out[:5]], out[5].ptr if want_p else None, dst.ptr), "pg_assoc_gxe_dev")
        ctx.sync()
        res = _six_download(out, p, "F_wald", "p_wald")
        if not want_p:
            res["p_wald"] = None
        if return_stats:
            res["n_evals"] = dst.download((2,), np.uint64).astype(np.int64)
        return res


def fdist_sf(F, dfd, ctx=None):
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        F = np.ascontiguousarray(F, np.float64).ravel()
        dF = ctx.to_device(F)
        dP = ctx.alloc(F.nbytes)
        _lib.check(L.pg_fdist_sf_dev(ctx.handle, F.size, dF.ptr, float(dfd), dP.ptr), "pg_fdist_sf_dev")
        ctx.sync()
        return dP.download(F.shape, np.float64)


def rotate(U, X, ctx=None, ldx=None):
    """X <- U' X (lmm/lmm.py:243-246) on the GPU; U (n,n) eigenvectors in columns, X (n,p).
    Returns the SNP-major rotated block (p, ldx) float32."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        U, X = _f32(U), _f32(X)
        n, p = X.shape
        ldx = ldx or _ldx(n)
        dU, dX = ctx.to_device(U), ctx.to_device(X)
        dXr = ctx.alloc(p * ldx * 4)
        _lib.check(L.pg_rotate_dev(ctx.handle, n, p, dU.ptr, n, dX.ptr, p, dXr.ptr, ldx), "pg_rotate_dev")
        ctx.sync()
        return dXr.download((p, ldx), np.float32)


def syevd(K, ctx=None, want64=False):
    """scipy.linalg.eigh(K) (lmm/lmm.py:152) on the GPU: lower triangle of K (n,n) float32 ->
    (evals f32 ascending clamped >= 0, U f32 with eigenvector j in column j[, evals f64, U f64])."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        K = _f32(K)
        n = K.shape[0]
        assert K.shape == (n, n)
        dK = ctx.to_device(K)
        dev, dU = ctx.alloc(n * 4), ctx.alloc(n * n * 4)
        d64 = ctx.alloc(n * 8) if want64 else None
        U64 = ctx.alloc(n * n * 8) if want64 else None
        _lib.check(L.pg_syevd_dev(ctx.handle, n, dK.ptr, dev.ptr, dU.ptr, d64.ptr if want64 else None,
                                  U64.ptr if want64 else None), "pg_syevd_dev")
        ctx.sync()
        out = [dev.download((n,), np.float32), dU.download((n, n), np.float32)]
        if want64:
            out += [d64.download((n,), np.float64), U64.download((n, n), np.float64)]
        return tuple(out)


def rotate_geno(U, X, ctx=None, ldx=None):
    """Genotype fast path of X <- U'X (pg_rotate_geno_dev).  Returns (Xr (p, ldx) float32, True) when every column of X
    takes <= 3 equally spaced values, else (None, False)."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        U, X = _f32(U), _f32(X)
        n, p = X.shape
        ldx = ldx or _ldx(n)
        dU, dX = ctx.to_device(U), ctx.to_device(X)
        dprep = ctx.alloc(L.pg_geno_prep_bytes(n))
        dwork = ctx.alloc(L.pg_geno_work_bytes(n, p))
        dXr = ctx.alloc(p * ldx * 4)
        _lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
        ok = C.c_int(0)
        _lib.check(L.pg_rotate_geno_dev(ctx.handle, n, p, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), "pg_rotate_geno_dev")
        ctx.sync()
        out = dXr.download((p, ldx), np.float32) if ok.value else None
        return out, int(ok.value)     # 1: genotype-valued block, 2: general finite block (X split in two fp16 planes)


def rotate_auto(U, X, ctx=None):
    """pg_rotate_auto_dev: the rotation of a float32 block with the path (genotype fp16x2 / split planes / fp32 MFMA for NaN
    blocks) chosen on the device.  Returns (Xr (p, ldx) float32, path) with path 1 / 2 / 0 like pg_rotate_geno_dev's flag."""
    L = _lib.load()
    with _lib.scope(ctx) as ctx:
        U, X = _f32(U), _f32(X)
        n, p = X.shape
        ldx = _ldx(n)
        dU, dX = ctx.to_device(U), ctx.to_device(X)
        dprep, dwork = ctx.alloc(L.pg_geno_prep_bytes(n)), ctx.alloc(L.pg_geno_work_bytes(n, p))
        dXr, dpath = ctx.alloc(p * ldx * 4), ctx.alloc(4)
        _lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
        _lib.check(L.pg_rotate_auto_dev(ctx.handle, n, p, dU.ptr, n, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, dpath.ptr),
                   "pg_rotate_auto_dev")
        ctx.sync()
        return dXr.download((p, ldx), np.float32), int(dpath.download((1,), np.int32)[0])
