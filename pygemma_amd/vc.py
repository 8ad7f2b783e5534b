"""lmm.reml / lmm.vc_kinship: REML variance components for several kinship matrices (GCTA --reml --mgrm, GEMMA -vc 2).

Several K's share no eigenvectors, so every evaluation is dense fp64 linear algebra on V = sum_i s_i K_i + s_e I on the device
(csrc/vc.hip: pg_vc_eval_dev); the iteration — a few (k + 1)-vectors and (k + 1) x (k + 1) matrices — runs here on the host."""
import ctypes as C
import time

import numpy as np
import pandas as pd

from . import _lib

_VC_MAX_K = 64           # VC_MAXK: matrices per call
_VC_MAX_C = 30           # PG_MAX_COVARIATES
_HALVINGS = 10
_LOGL_TOL = 1e-4         # GCTA's second convergence condition
_FLOOR = 1e-6            # a component driven below 0 is set to this share of Var(y)


class RemlResult:
    """What lmm.reml returns: sigma2 (k + 1, noise last), se, cov (the inverse average-information matrix), h2 (k) = sigma2_i / sum
    sigma2 with delta-method h2_se, h2_total and h2_total_se, logl, logl0 (the model without any K), lrt = 2 (logl - logl0), beta and
    beta_se (GLS), iters, converged, constrained (bool mask, k + 1), n.  frame() is GCTA's .hsq table."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"RemlResult(sigma2={np.array2string(self.sigma2, precision=6)}, h2_total={self.h2_total:.6g} +- {self.h2_total_se:.3g}, "
                f"logl={self.logl:.6f}, iters={self.iters}, converged={self.converged})")

    def frame(self):
        """The .hsq table: Source, Variance, SE — V(G1) .. V(Gk), V(e), Vp, V(Gi)/Vp, Sum of V(G)/Vp, then logL, logL0, LRT, df, Pval, n
        with SE NaN.  Pval is chi2(df = k).sf(LRT), halved for k = 1 (the boundary mixture GCTA reports)."""
        from scipy import stats
        k = len(self.h2)
        one = np.ones(k + 1)
        rows = [(f"V(G{i + 1})", self.sigma2[i], self.se[i]) for i in range(k)]
        rows += [("V(e)", self.sigma2[k], self.se[k]), ("Vp", float(self.sigma2.sum()), float(np.sqrt(max(one @ self.cov @ one, 0.0))))]
        rows += [(f"V(G{i + 1})/Vp", self.h2[i], self.h2_se[i]) for i in range(k)]
        if k > 1:
            rows.append(("Sum of V(G)/Vp", self.h2_total, self.h2_total_se))
        pval = float(stats.chi2.sf(max(self.lrt, 0.0), k)) * (0.5 if k == 1 else 1.0)
        nan = float("nan")
        rows += [("logL", self.logl, nan), ("logL0", self.logl0, nan), ("LRT", self.lrt, nan), ("df", float(k), nan), ("Pval", pval, nan), ("n", float(self.n), nan)]
        return pd.DataFrame(rows, columns=["Source", "Variance", "SE"])


def _check_ks(Ks, who):
    if isinstance(Ks, np.ndarray) and Ks.ndim == 2:
        Ks = [Ks]
    try:
        Ks = [np.asarray(K) for K in Ks]
    except TypeError:
        raise ValueError(f"{who}: Ks must be an (n, n) array or a sequence of them") from None
    if not 1 <= len(Ks) <= _VC_MAX_K:
        raise ValueError(f"{who} takes k = 1 to {_VC_MAX_K} kinship matrices, got {len(Ks)}")
    n = Ks[0].shape[0] if Ks[0].ndim == 2 else -1
    for i, K in enumerate(Ks):
        if K.ndim != 2 or K.shape != (n, n) or n < 1:
            raise ValueError(f"shape mismatch: K[{i}] is {K.shape}, not a square matrix of the first one's size")
        if K.dtype not in (np.float32, np.float64):
            raise ValueError(f"{who}: K[{i}] is {K.dtype}; float32 or float64 matrices are taken")
        if not np.isfinite(K).all():
            raise ValueError(f"{who}: K[{i}] holds NaN or Inf")
    return Ks, n


class _Mats:
    """The K's on the device in the caller's dtypes, and the host arrays the C entry points take."""

    def __init__(self, ctx, Ks):
        self.k, self.n = len(Ks), Ks[0].shape[0]
        self.bufs = [ctx.to_device(np.ascontiguousarray(K)) for K in Ks]
        self.ptrs = (C.c_void_p * self.k)(*[b.ptr for b in self.bufs])
        self.f64 = (C.c_int * self.k)(*[int(K.dtype == np.float64) for K in Ks])
        self.ldk = (C.c_int64 * self.k)(*[self.n] * self.k)

    def head(self, ctx):
        return ctx.handle, self.n, self.k, self.ptrs, self.f64, self.ldk


def _unpack(out, k, c):
    kk, o = k + 1, 4
    ev = {"logl": out[0], "logdet_v": out[1], "logdet_xvx": out[2], "ypy": out[3]}
    for name, size, shape in (("score", kk, (kk,)), ("ai", kk * kk, (kk, kk)), ("beta", c, (c,)), ("xvx_inv", c * c, (c, c)), ("tr_pk", kk, (kk,)),
                              ("ypkpy", kk, (kk,))):
        ev[name] = out[o:o + size].reshape(shape).copy()
        o += size
    return ev


def _active_step(ev, active):
    """The AI step over the active components (0 elsewhere), or None when their AI block is singular to working precision."""
    ai = ev["ai"][np.ix_(active, active)]
    d = np.sqrt(np.abs(np.diagonal(ai)))
    if not np.isfinite(ai).all() or (d == 0).any():
        return None
    w = np.linalg.eigvalsh(ai / np.outer(d, d))
    if w[0] < 1e-10 * max(w[-1], 1.0):
        return None
    step = np.zeros(len(active))
    step[active] = np.linalg.solve(ai, ev["score"][active])
    return step


def iterate(evaluate, start, vy, n, tol, max_iter, constrain, log=lambda msg: None):
    """GCTA's AI-REML from `start`: evaluate(sigma) -> (ev, info) with ev None when V is not positive definite (info = 1 + the pivot).
    Iteration 1 is an EM step, sigma_i += 2 sigma_i^2 score_i / n; later ones sigma += AI^-1 score over the components that are not
    held at the floor.  A step is halved (up to 10 times) while V is not positive definite or logL drops by more than 1e-10 (1 +
    |logL|).  constrain: a component below 0 is set to 1e-6 vy, flagged, and leaves the AI system until its score is positive again.
    Converged when max |d sigma| <= tol sum sigma and |d logL| <= 1e-4.  A singular AI block (collinear components) or ten halvings
    that do not stop a drop of logL end the iteration unconverged.  Returns (sigma, ev, iters, converged, constrained)."""
    sigma = np.array(start, np.float64)
    kk = len(sigma)
    constrained = np.zeros(kk, bool)
    ev, info = evaluate(sigma)
    if ev is None:
        raise _lib.PgError(f"reml: V is not positive definite at the starting values {sigma} (pivot {info - 1})")
    converged, iters = False, 0
    for it in range(1, int(max_iter) + 1):
        iters = it
        if it == 1:
            step = 2.0 * sigma ** 2 * ev["score"] / n
        else:
            active = ~(constrained & (ev["score"] < 0))
            step = _active_step(ev, active) if active.any() else np.zeros(kk)
            if step is None:
                log(f"reml: iteration {it}: the average-information matrix is singular (collinear components?)")
                break
        accepted = None
        for h in range(_HALVINGS + 1):
            new = sigma + step * 0.5 ** h
            flag = np.zeros(kk, bool)
            if constrain:
                flag = new < 0
                new = np.where(flag, _FLOOR * vy, new)
            ev_new, info = evaluate(new)
            if ev_new is not None and ev_new["logl"] >= ev["logl"] - 1e-10 * (1.0 + abs(ev["logl"])):
                accepted = (new, ev_new, flag)
                break
            log(f"reml: iteration {it}: step / {2 ** h} " + ("leaves V indefinite" if ev_new is None else f"lowers logL to {ev_new['logl']:.6f}"))
        if accepted is None:
            if ev_new is None:
                raise _lib.PgError(f"reml: V is not positive definite after {_HALVINGS} halvings of the step at iteration {it} (pivot {info - 1})")
            break
        new, ev_new, flag = accepted
        dsig, dlogl = np.max(np.abs(new - sigma)), abs(ev_new["logl"] - ev["logl"])
        sigma, ev, constrained = new, ev_new, flag | (constrained & (new <= _FLOOR * vy))
        log(f"reml: iteration {it}: logL {ev['logl']:.6f}, sigma2 {sigma}")
        if dsig <= tol * sigma.sum() and dlogl <= _LOGL_TOL:
            converged = True
            break
    return sigma, ev, iters, converged, constrained


def summarize(sigma, ev, k):
    """se, cov, h2, h2_se, h2_total, h2_total_se, beta_se from an evaluation at sigma (delta method for the ratios)."""
    try:
        cov = np.linalg.inv(ev["ai"])
    except np.linalg.LinAlgError:
        cov = np.full_like(ev["ai"], np.nan)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.diagonal(cov))
        S = sigma.sum()
        G = (np.eye(k + 1)[:k] * S - sigma[:k, None]) / S ** 2          # d h2_i / d sigma_j
        h2, h2_se = sigma[:k] / S, np.sqrt(np.einsum("ij,jl,il->i", G, cov, G))
        g = np.r_[np.full(k, sigma[k]), -sigma[:k].sum()] / S ** 2
        h2_total, h2_total_se = sigma[:k].sum() / S, np.sqrt(g @ cov @ g)
        beta_se = np.sqrt(np.diagonal(ev["xvx_inv"]))
    return dict(se=se, cov=cov, h2=h2, h2_se=h2_se, h2_total=float(h2_total), h2_total_se=float(h2_total_se), beta_se=beta_se)


def null_logl(y, W):
    """REML log likelihood of the model without any K, V = s I, at its maximum s = RSS / (n - c), in pg_vc_eval_dev's convention
    (no 2 pi term): -1/2 ((n - c) log s + log|W'W| + n - c)."""
    n, c = W.shape
    beta, *_ = np.linalg.lstsq(W, y, rcond=None)
    rss = float(np.sum((y - W @ beta) ** 2))
    s = rss / (n - c)
    sign, ld = np.linalg.slogdet(W.T @ W)
    return -0.5 * ((n - c) * np.log(s) + ld + (n - c))


def reml(Y, W, Ks, *, start=None, tol=1e-8, max_iter=50, constrain=True, device=0, verbose=0, stats=None):
    """REML variance components of  y = W beta + sum_i g_i + e,  g_i ~ N(0, s_i K_i), e ~ N(0, s_e I)  for k >= 1 kinship matrices —
    how much phenotypic variance each of several relatedness matrices explains, with standard errors (GCTA --reml --mgrm, GEMMA -vc 2).

    Ks: one (n, n) array or a sequence of k <= 64 of them, float32 or float64 (kept in their dtype on the device), symmetric; the lower
    triangle is used.  Y: (n,) or (n, 1).  W: (n, c), c = 1 .. 30 < n, with the intercept column if one is wanted.
    GCTA's AI-REML: every component starts at Var(y) / (k + 1) (or at `start`, k + 1 values, noise last); the first iteration is an EM
    step, the rest average-information steps with step halving while logL drops or V is not positive definite; with `constrain` a
    component driven below 0 is set to 1e-6 Var(y) and flagged; converged when max |d sigma2| <= tol sum sigma2 and |d logL| <= 1e-4.
    Collinear components (a singular AI matrix) end the iteration with converged = False.  Every evaluation — Cholesky factor, explicit
    inverse, traces, symmetric products: 3 n^2 doubles of work space beside the K's — runs on one GPU (csrc/vc.hip); nothing of size
    n^2 comes back.  Returns a RemlResult.  `stats` receives evaluations, seconds, seconds_eval.
    Refused with ValueError before any device work: Ks that are not 1 to 64 square float32 / float64 matrices of one size, shapes of
    Y or W that do not match, c outside 1 .. 30, n <= c, NaN or Inf anywhere, a bad start, tol or max_iter.  PgError: V not positive
    definite at the start or after 10 halvings (the message names the pivot), collinear covariates."""
    Ks, n = _check_ks(Ks, "reml")
    k = len(Ks)
    y = np.asarray(Y, np.float64)
    if y.ndim == 2 and y.shape[1] == 1:
        y = y[:, 0]
    W = np.asarray(W, np.float64)
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"shape mismatch: Y is {np.shape(Y)}, the kinship matrices are ({n}, {n})")
    if W.ndim != 2 or W.shape[0] != n:
        raise ValueError(f"shape mismatch: W is {W.shape}, the kinship matrices are ({n}, {n})")
    c = W.shape[1]
    if not 1 <= c <= _VC_MAX_C:
        raise ValueError(f"reml takes c = 1 to {_VC_MAX_C} covariates (the intercept included), got {c}")
    if n <= c:
        raise ValueError(f"reml needs more samples than covariates: n = {n}, c = {c}")
    if not np.isfinite(y).all() or not np.isfinite(W).all():
        raise ValueError("reml: Y or W holds NaN or Inf")
    if not (isinstance(tol, (int, float)) and tol > 0):
        raise ValueError(f"tol must be > 0, not {tol!r}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1:
        raise ValueError(f"max_iter must be an integer >= 1, not {max_iter!r}")
    vy = float(np.var(y, ddof=1))
    if not vy > 0:
        raise ValueError("reml: Y is constant")
    if start is None:
        start = np.full(k + 1, vy / (k + 1))
    else:
        start = np.asarray(start, np.float64)
        if start.shape != (k + 1,) or not np.isfinite(start).all() or (start < 0).any() or not start[k] > 0:
            raise ValueError(f"start must hold k + 1 = {k + 1} finite variances >= 0 with the last (noise) > 0, got {start!r}")
    V = _lib.load_vc()
    if _lib.device_count() < 1:
        raise _lib.PgError("no MI355X visible: pygemma_amd has no CPU path")
    t0, counts = time.time(), {"evaluations": 0, "seconds_eval": 0.0}
    with _lib.Context(device) as ctx:       # every buffer hangs off the context: freed on every way out
        mats = _Mats(ctx, Ks)
        dWy = ctx.to_device(np.ascontiguousarray(np.c_[W, y]))
        work = ctx.alloc(int(V.pg_vc_work_bytes(n, k)))
        out = np.empty(int(V.pg_vc_out_len(k, c)))
        info = C.c_int(0)

        def evaluate(sigma):
            t1 = time.time()
            s = (C.c_double * (k + 1))(*sigma)
            _lib.check(V.pg_vc_eval_dev(ctx.handle, n, k, c, mats.ptrs, mats.f64, mats.ldk, s, dWy.ptr, work.ptr, out.ctypes.data, None, C.byref(info)), "pg_vc_eval_dev")
            counts["evaluations"] += 1
            counts["seconds_eval"] += time.time() - t1
            return (None if info.value != 0 else _unpack(out, k, c)), info.value

        sigma, ev, iters, converged, constrained = iterate(evaluate, start, vy, n, tol, max_iter, constrain,
                                                           log=(lambda msg: print(msg, flush=True)) if verbose > 1 else (lambda msg: None))
    logl0 = float(null_logl(y, W))
    res = RemlResult(sigma2=sigma, logl=float(ev["logl"]), logl0=logl0, lrt=2.0 * (float(ev["logl"]) - logl0), beta=ev["beta"], iters=iters,
                     converged=bool(converged), constrained=constrained, n=n, **summarize(sigma, ev, k))
    if stats is not None:
        stats.update(counts, seconds=time.time() - t0)
    if verbose:
        print(f"REML: {k} components, n = {n}, c = {c}: {iters} iterations ({counts['evaluations']} evaluations) in {time.time() - t0:.3f} s, "
              f"converged = {converged}", flush=True)
    return res


def vc_kinship(Ks, res, *, device=0):
    """sum_i s_i K_i / sum_{i<k} s_i with s = res.sigma2 (a RemlResult, or k + 1 variances with the noise last, which is not used) as a
    float32 (n, n) matrix: the one kinship matrix to hand to lmm.pygemma for a scan under the fitted multi-component model.  The sum is
    formed in fp64 by the combine kernel from the lower triangles, in the order of Ks, rounded once and mirrored.
    Refused with ValueError before any device work: Ks as in reml, a sigma2 that is not k + 1 finite values >= 0, genetic variances
    that sum to 0."""
    Ks, n = _check_ks(Ks, "vc_kinship")
    k = len(Ks)
    sigma = np.asarray(getattr(res, "sigma2", res), np.float64)
    if sigma.shape != (k + 1,) or not np.isfinite(sigma).all() or (sigma < 0).any():
        raise ValueError(f"vc_kinship: sigma2 must hold k + 1 = {k + 1} finite variances >= 0, got {sigma!r}")
    tot = sigma[:k].sum()
    if not tot > 0:
        raise ValueError("vc_kinship: the genetic variances sum to 0")
    L, V = _lib.load(), _lib.load_vc()
    if _lib.device_count() < 1:
        raise _lib.PgError("no MI355X visible: pygemma_amd has no CPU path")
    with _lib.Context(device) as ctx:
        mats = _Mats(ctx, Ks)
        dV = ctx.alloc(8 * n * n)
        _lib.check(L.pg_memset(ctx.handle, dV.ptr, 0, 8 * n * n), "pg_memset")
        s = (C.c_double * (k + 1))(*(sigma[:k] / tot), 0.0)
        _lib.check(V.pg_vc_combine_dev(*mats.head(ctx), s, dV.ptr, n), "pg_vc_combine_dev")
        ctx.sync()
        M = np.tril(dV.download((n, n), np.float64))
    return (M + np.tril(M, -1).T).astype(np.float32)
