"""Plain NumPy fp64 model of lmm.reml: one evaluation of the REML objective for V = sum_i s_i K_i + s_e I by np.linalg.cholesky and
explicit solves, and GCTA's AI-REML iteration over it.  Nothing here is shared with pygemma_amd but the genotype generator of its synth module.

evaluate() also returns, for logL, every score_i and every AI_ij, `mag`: the sum of the magnitudes of the terms that were added to
form it.  An implementation that adds the same terms in another order, from a factor of V with relative error ~ n u kappa_2(V), differs
by a small multiple of n u kappa_2(V) mag — the unit of the tests' tolerances."""
import numpy as np

U = 2.0 ** -53
HALVINGS, LOGL_TOL, FLOOR = 10, 1e-4, 1e-6


def sym(K):
    """The symmetric matrix a lower triangle stands for, in fp64."""
    L = np.tril(np.asarray(K, np.float64))
    return L + np.tril(L, -1).T


def kin_matrices(n, k, seed, dtypes=None):
    """k kinship matrices K_i = Z_i Z_i' / p_i from synth genotypes, scaled to trace n, in the given dtypes (default: float32 and
    float64 alternating, so a call mixes them); exactly symmetric.  n = 1: the 1 x 1 matrix [1]."""
    from pygemma_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for i in range(k):
        p = 2 * n + 16 * i + 3
        Z = synth.genotypes(rng, n, p, np.float64) if n > 1 else np.ones((1, p))
        K = Z @ Z.T / p
        K = sym(K * (n / np.trace(K)))
        dt = (dtypes[i] if dtypes is not None else (np.float32, np.float64)[i % 2])
        out.append(sym(K.astype(dt)).astype(dt))
    return out


def phenotype(Ks, c, sigma, seed):
    """(y, W): W = [1, normal columns], y = W b + sum_i g_i + e drawn with the variances sigma (k + 1)."""
    rng = np.random.default_rng(seed)
    n = Ks[0].shape[0]
    W = np.c_[np.ones(n), rng.standard_normal((n, c - 1))]
    y = W @ rng.standard_normal(c)
    for s, K in zip(sigma, Ks):
        w, Q = np.linalg.eigh(sym(K))
        y = y + Q @ (np.sqrt(np.clip(w, 0, None) * s) * rng.standard_normal(n))
    return y + np.sqrt(sigma[-1]) * rng.standard_normal(n), W


def v_of(Ks, sigma):
    n = Ks[0].shape[0]
    V = sigma[-1] * np.eye(n)
    for s, K in zip(sigma, Ks):
        V = V + s * sym(K)
    return V


def evaluate(y, W, Ks, sigma):
    """logl = -1/2 (log|V| + log|W'V^-1 W| + y'Py), score_i = -1/2 (tr(P K_i) - y'P K_i P y), ai_ij = 1/2 y'P K_i P K_j P y with
    K_k = I, the GLS beta, xvx_inv, py, and mag_logl, mag_score (k + 1), mag_ai (k + 1, k + 1).  None when V is not positive definite."""
    sigma = np.asarray(sigma, np.float64)
    k, n, c = len(Ks), len(y), W.shape[1]
    V = v_of(Ks, sigma)
    try:
        Lc = np.linalg.cholesky(V)
    except np.linalg.LinAlgError:
        return None
    Vi = np.linalg.solve(Lc.T, np.linalg.solve(Lc, np.eye(n)))
    Vi = (Vi + Vi.T) / 2
    Zw, viy = Vi @ W, Vi @ y
    xvx = W.T @ Zw
    xvx = (xvx + xvx.T) / 2
    Lx = np.linalg.cholesky(xvx)
    H = np.linalg.inv(xvx)
    H = (H + H.T) / 2
    xvy = W.T @ viy
    beta = H @ xvy
    py = viy - Zw @ beta
    ypy = y @ viy - xvy @ beta
    ld_v, ld_x = 2 * np.log(np.diagonal(Lc)), 2 * np.log(np.diagonal(Lx))
    out = {"logl": -0.5 * (ld_v.sum() + ld_x.sum() + ypy), "beta": beta, "xvx_inv": H, "py": py, "ypy": ypy,
           "mag_logl": 0.5 * (np.abs(ld_v).sum() + np.abs(ld_x).sum() + np.abs(y) @ np.abs(viy) + np.abs(xvy) @ np.abs(beta))}
    mats = [sym(K) for K in Ks] + [np.eye(n)]
    score, mag_s, us, zus = np.empty(k + 1), np.empty(k + 1), [], []
    for i, K in enumerate(mats):
        u = K @ py
        T = Zw.T @ K @ Zw
        score[i] = -0.5 * (np.sum(Vi * K) - np.sum(H * T) - py @ u)
        mag_s[i] = 0.5 * (np.sum(np.abs(Vi) * np.abs(K)) + np.sum(np.abs(H) * np.abs(T)) + np.abs(py) @ np.abs(K) @ np.abs(py))
        us.append(u)
        zus.append(Zw.T @ u)
    ai, mag_a = np.empty((k + 1, k + 1)), np.empty((k + 1, k + 1))
    for i in range(k + 1):
        for j in range(k + 1):
            ai[i, j] = 0.5 * (us[i] @ Vi @ us[j] - zus[i] @ H @ zus[j])
            mag_a[i, j] = 0.5 * (np.abs(us[i]) @ np.abs(Vi) @ np.abs(us[j]) + np.abs(zus[i]) @ np.abs(H) @ np.abs(zus[j]))
    out.update(score=score, ai=(ai + ai.T) / 2, mag_score=mag_s, mag_ai=mag_a)
    return out


def ai_step(ev, active=None):
    """AI^-1 score over the active components (all by default), 0 elsewhere."""
    kk = len(ev["score"])
    active = np.ones(kk, bool) if active is None else active
    step = np.zeros(kk)
    step[active] = np.linalg.solve(ev["ai"][np.ix_(active, active)], ev["score"][active])
    return step


def iterate(y, W, Ks, start=None, tol=1e-8, max_iter=50, constrain=True):
    """GCTA's AI-REML, the rule lmm.reml documents: an EM step first, then AI steps over the components not held at the floor, a step
    halved while V is indefinite or logL drops by more than 1e-10 (1 + |logL|), negative components set to 1e-6 Var(y).
    Returns (sigma, ev, iters, converged, constrained)."""
    k, n = len(Ks), len(y)
    vy = np.var(y, ddof=1)
    sigma = np.full(k + 1, vy / (k + 1)) if start is None else np.array(start, np.float64)
    constrained = np.zeros(k + 1, bool)
    ev = evaluate(y, W, Ks, sigma)
    assert ev is not None
    converged, iters = False, 0
    for it in range(1, max_iter + 1):
        iters = it
        if it == 1:
            step = 2.0 * sigma ** 2 * ev["score"] / n
        else:
            active = ~(constrained & (ev["score"] < 0))
            a = ev["ai"][np.ix_(active, active)]
            d = np.sqrt(np.abs(np.diagonal(a)))
            w = np.linalg.eigvalsh(a / np.outer(d, d))
            if w[0] < 1e-10 * max(w[-1], 1.0):
                break
            step = ai_step(ev, active)
        got = None
        for h in range(HALVINGS + 1):
            new = sigma + step * 0.5 ** h
            flag = (new < 0) if constrain else np.zeros(k + 1, bool)
            new = np.where(flag, FLOOR * vy, new)
            ev_new = evaluate(y, W, Ks, new)
            if ev_new is not None and ev_new["logl"] >= ev["logl"] - 1e-10 * (1.0 + abs(ev["logl"])):
                got = (new, ev_new, flag)
                break
        if got is None:
            break
        new, ev_new, flag = got
        dsig, dlogl = np.max(np.abs(new - sigma)), abs(ev_new["logl"] - ev["logl"])
        sigma, ev, constrained = new, ev_new, flag | (constrained & (new <= FLOOR * vy))
        if dsig <= tol * sigma.sum() and dlogl <= LOGL_TOL:
            converged = True
            break
    return sigma, ev, iters, converged, constrained


def summarize(sigma, ev):
    """se, h2, h2_se, h2_total, h2_total_se, beta_se at sigma from the evaluation there (delta method)."""
    k = len(sigma) - 1
    cov = np.linalg.inv(ev["ai"])
    S = sigma.sum()
    out = {"cov": cov, "se": np.sqrt(np.diagonal(cov)), "h2": sigma[:k] / S, "h2_se": np.empty(k), "beta_se": np.sqrt(np.diagonal(ev["xvx_inv"]))}
    for i in range(k):
        g = -sigma[i] * np.ones(k + 1) / S ** 2
        g[i] += 1.0 / S
        out["h2_se"][i] = np.sqrt(g @ cov @ g)
    g = np.r_[np.full(k, sigma[k]), -sigma[:k].sum()] / S ** 2
    out["h2_total"], out["h2_total_se"] = sigma[:k].sum() / S, np.sqrt(g @ cov @ g)
    return out
