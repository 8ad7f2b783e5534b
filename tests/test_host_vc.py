"""CPU-only checks of the variance-component fit (lmm.reml, lmm.vc_kinship): the NumPy truth against two independent forms of the same
objective, the host iteration of pygemma_amd/vc.py driven by the truth's evaluations, and every refusal before any device call.

Tolerances.  U = 2^-53.  The truth's logL, score_i and AI_ij come with `mag`, the sum of the magnitudes of their terms (tests/_vc_truth.py);
another route to the same number through a factor of V differs by a multiple of n U kappa_2(V) mag: 64 of them here and on the GPU.
The central difference D(h) = (f(s + h e_i) - f(s - h e_i)) / 2h with h = eps^(1/3) s_i has truncation error C h^2: D(2h) - D(h) = 3 C h^2
estimates it (doubled here), and each of its two evaluations carries a rounding error of up to 8 n U kappa_2 mag_logl, divided by 2h."""
import numpy as np
import pytest

import _vc_truth as T

U = 2.0 ** -53


def problem(n, k, c, seed, sigma=None):
    Ks = T.kin_matrices(n, k, seed)
    sigma = np.r_[np.full(k, 0.6 / k), 0.4] if sigma is None else np.asarray(sigma, np.float64)
    y, W = T.phenotype(Ks, c, sigma, seed + 1)
    return Ks, y, W, sigma


def kappa(Ks, sigma):
    w = np.linalg.eigvalsh(T.v_of(Ks, sigma))
    return w[-1] / w[0]


@pytest.mark.parametrize("n,c", [(65, 1), (200, 5), (129, 30)])
def test_truth_logl_equals_the_eigenvalue_form(n, c):
    Ks, y, W, _ = problem(n, 1, c, 11)
    for sigma in ([0.6, 0.4], [0.2, 1.3], [1.5, 0.5]):
        ev = T.evaluate(y, W, Ks, sigma)
        d, Q = np.linalg.eigh(T.sym(Ks[0]))
        h = 1.0 / (sigma[0] * d + sigma[1])
        yr, Wr = Q.T @ y, Q.T @ W
        xvx = Wr.T @ (h[:, None] * Wr)
        b = Wr.T @ (h * yr)
        ypy = yr @ (h * yr) - b @ np.linalg.solve(xvx, b)
        logl = -0.5 * (np.sum(np.log(sigma[0] * d + sigma[1])) + np.linalg.slogdet(xvx)[1] + ypy)
        tol = 64 * n * U * kappa(Ks, sigma) * ev["mag_logl"]
        print(f"n={n} c={c} sigma={sigma}: |diff| {abs(logl - ev['logl']):.3e} of {tol:.3e}")
        assert abs(logl - ev["logl"]) <= tol


@pytest.mark.parametrize("n,k,c", [(65, 1, 1), (129, 2, 5), (100, 5, 3)])
def test_truth_score_is_the_derivative_of_its_logl(n, k, c):
    Ks, y, W, sigma = problem(n, k, c, 23)
    sigma = sigma * np.linspace(0.8, 1.3, k + 1)
    ev, kap = T.evaluate(y, W, Ks, sigma), kappa(Ks, sigma)
    for i in range(k + 1):
        h = (2.0 ** -52) ** (1.0 / 3.0) * sigma[i]

        def diff(step):
            e = np.zeros(k + 1)
            e[i] = step
            return (T.evaluate(y, W, Ks, sigma + e)["logl"] - T.evaluate(y, W, Ks, sigma - e)["logl"]) / (2 * step)
        d1, d2 = diff(h), diff(2 * h)
        tol = 2 * abs(d2 - d1) / 3 + 2 * 8 * n * U * kap * ev["mag_logl"] / (2 * h) + 64 * n * U * kap * ev["mag_score"][i]
        print(f"n={n} k={k} component {i}: score {ev['score'][i]:.6e}, difference {d1:.6e}, |diff| {abs(d1 - ev['score'][i]):.3e} of {tol:.3e}")
        assert abs(d1 - ev["score"][i]) <= tol
        assert tol <= 1e-3 * ev["mag_score"][i]            # the check can tell a wrong sign or a missing factor


def test_truth_ai_is_symmetric_positive_definite():
    Ks, y, W, sigma = problem(100, 3, 4, 5)
    ev = T.evaluate(y, W, Ks, sigma)
    assert np.array_equal(ev["ai"], ev["ai"].T) and np.linalg.eigvalsh(ev["ai"])[0] > 0


# ---- the host iteration of the product, on the truth's evaluations ----------------------------------------------------------------------

def run_product_iteration(Ks, y, W, **kw):
    from pygemma_amd import vc
    calls = []

    def evaluate(s):
        calls.append(np.array(s))
        ev = T.evaluate(y, W, Ks, s)
        if ev is None:
            return None, 1
        return {"logl": ev["logl"], "score": ev["score"], "ai": ev["ai"], "beta": ev["beta"], "xvx_inv": ev["xvx_inv"]}, 0
    vy = float(np.var(y, ddof=1))
    start = kw.pop("start", np.full(len(Ks) + 1, vy / (len(Ks) + 1)))
    return vc.iterate(evaluate, start, vy, len(y), kw.pop("tol", 1e-8), kw.pop("max_iter", 50), kw.pop("constrain", True)), calls


@pytest.mark.parametrize("n,k,c", [(150, 1, 2), (200, 2, 3), (257, 3, 1)])
def test_iteration_follows_the_truths_rule(n, k, c):
    Ks, y, W, _ = problem(n, k, c, 31)
    (sigma, ev, iters, converged, constrained), calls = run_product_iteration(Ks, y, W)
    ts, tev, titers, tconv, tcons = T.iterate(y, W, Ks)
    assert converged and tconv and iters == titers
    assert np.array_equal(sigma, ts) and np.array_equal(constrained, tcons)      # the same evaluations, the same arithmetic
    assert np.array_equal(calls[0], np.full(k + 1, np.var(y, ddof=1) / (k + 1)))
    # the first step is the EM step  s_i <- (s_i^2 y'P K_i P y + tr(s_i I - s_i^2 P K_i)) / n
    ev0 = T.evaluate(y, W, Ks, calls[0])
    trpk = np.array([-2 * ev0["score"][i] + ev0["py"] @ K @ ev0["py"] for i, K in enumerate([T.sym(K) for K in Ks] + [np.eye(n)])])
    em = np.array([(calls[0][i] ** 2 * (ev0["py"] @ K @ ev0["py"]) + (n * calls[0][i] - calls[0][i] ** 2 * trpk[i])) / n
                   for i, K in enumerate([T.sym(K) for K in Ks] + [np.eye(n)])])
    np.testing.assert_allclose(calls[1], em, rtol=1e-12)
    # stationary: the next AI step is far below the tolerance
    assert np.max(np.abs(T.ai_step(ev))) <= 2e-8 * sigma.sum()


def test_iteration_flags_a_component_held_at_the_floor():
    """y drawn without the second component; the seed is one at which the truth's unconstrained estimate of it is negative."""
    Ks, y, W, _ = problem(200, 2, 2, 52, sigma=[0.6, 0.0, 0.4])
    ts, _, _, tconv, tcons = T.iterate(y, W, Ks)
    assert tcons[1] and not tcons[0] and not tcons[2], "the fixture must put component 2 on the boundary"
    (sigma, ev, iters, converged, constrained), _ = run_product_iteration(Ks, y, W)
    assert constrained[1] and sigma[1] == 1e-6 * np.var(y, ddof=1) and np.array_equal(constrained, tcons)
    assert converged == tconv and np.array_equal(sigma, ts)


def test_iteration_reports_collinear_components():
    Ks, y, W, _ = problem(150, 1, 2, 3)
    (sigma, ev, iters, converged, constrained), _ = run_product_iteration([Ks[0], Ks[0].copy()], y, W)
    assert not converged and np.isfinite(sigma).all() and iters <= 3


def test_iteration_names_the_pivot_when_v_stays_indefinite():
    from pygemma_amd import _lib, vc
    good = {"logl": -1.0, "score": np.array([1.0, 1.0]), "ai": np.eye(2), "beta": np.zeros(1), "xvx_inv": np.eye(1)}
    seen = []

    def evaluate(s):
        seen.append(s)
        return (good, 0) if len(seen) <= 2 else (None, 8)
    with pytest.raises(_lib.PgError, match="pivot 7"):
        vc.iterate(evaluate, np.array([1.0, 1.0]), 2.0, 10, 1e-8, 50, True)
    assert len(seen) == 2 + 11                              # the start, the EM step, then the full step and its 10 halvings
    with pytest.raises(_lib.PgError, match="starting values"):
        vc.iterate(lambda s: (None, 3), np.array([1.0, 1.0]), 2.0, 10, 1e-8, 50, True)


def test_summary_and_null_model_against_the_truth():
    from pygemma_amd import vc
    Ks, y, W, sigma = problem(120, 2, 3, 9)
    ev = T.evaluate(y, W, Ks, sigma)
    got, want = vc.summarize(sigma, ev, 2), T.summarize(sigma, ev)
    for key in ("se", "h2", "h2_se", "beta_se", "cov"):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12)
    np.testing.assert_allclose([got["h2_total"], got["h2_total_se"]], [want["h2_total"], want["h2_total_se"]], rtol=1e-12)
    # the model without any K is the model with a zero K at s_e = RSS / (n - c)
    n, c = W.shape
    rss = np.sum((y - W @ np.linalg.lstsq(W, y, rcond=None)[0]) ** 2)
    ev0 = T.evaluate(y, W, [np.zeros((n, n))], [0.0, rss / (n - c)])
    assert abs(vc.null_logl(y, W) - ev0["logl"]) <= 64 * n * U * ev0["mag_logl"]
    assert abs(ev0["score"][1]) <= 64 * n * U * ev0["mag_score"][1]      # ... where its REML score vanishes


def test_result_frame():
    from pygemma_amd import lmm
    Ks, y, W, sigma = problem(80, 2, 2, 2)
    ev = T.evaluate(y, W, Ks, sigma)
    from pygemma_amd import vc
    res = lmm.RemlResult(sigma2=sigma, logl=ev["logl"], logl0=ev["logl"] - 3.0, lrt=6.0, beta=ev["beta"], iters=4, converged=True,
                         constrained=np.zeros(3, bool), n=80, **vc.summarize(sigma, ev, 2))
    f = res.frame()
    assert list(f.columns) == ["Source", "Variance", "SE"]
    assert list(f["Source"]) == ["V(G1)", "V(G2)", "V(e)", "Vp", "V(G1)/Vp", "V(G2)/Vp", "Sum of V(G)/Vp", "logL", "logL0", "LRT", "df", "Pval", "n"]
    assert f["Variance"][3] == sigma.sum() and f["Variance"][9] == 6.0 and 0 < f["Variance"][11] < 1 and "converged=True" in repr(res)


# ---- refusals: ValueError before any device call ---------------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    from pygemma_amd import _lib

    def touched(*a, **kw):
        raise AssertionError("a device call was made before the arguments were refused")
    monkeypatch.setattr(_lib, "Context", touched)
    monkeypatch.setattr(_lib, "device_count", touched)


def test_reml_refusals_come_before_any_device_call(no_device):
    from pygemma import lmm
    rng = np.random.default_rng(0)
    n = 12
    K = np.eye(n)
    y, W = rng.standard_normal(n), np.c_[np.ones(n), rng.standard_normal(n)]
    nan_k, nan_y, nan_w = K.copy(), y.copy(), W.copy()
    nan_k[3, 2], nan_y[4], nan_w[5, 1] = np.nan, np.inf, np.nan
    bad = [
        dict(Ks=[]), dict(Ks=[K] * 65), dict(Ks=np.ones((n, n + 1))), dict(Ks=[K, np.eye(n + 1)]), dict(Ks=K.astype(np.int32)),
        dict(Ks=np.ones((2, n, n))[0:0]), dict(Ks=nan_k), dict(Ks=[K, nan_k.astype(np.float32)]), dict(Ks=3.0), dict(Ks=[np.ones(n)]),
        dict(Y=y[:-1]), dict(Y=np.c_[y, y]), dict(Y=nan_y), dict(Y=np.zeros(n)),
        dict(W=W[:-1]), dict(W=W[:, :0]), dict(W=rng.standard_normal((n, 31))), dict(W=rng.standard_normal((n, n))), dict(W=nan_w), dict(W=y),
        dict(start=[1.0]), dict(start=[1.0, -1.0]), dict(start=[1.0, 0.0]), dict(start=[np.nan, 1.0]), dict(start=[[1.0, 1.0]]),
        dict(tol=0.0), dict(tol=-1e-8), dict(tol=None), dict(max_iter=0), dict(max_iter=2.5), dict(max_iter=True),
    ]
    for kw in bad:
        args = dict(Y=y, W=W, Ks=K)
        args.update(kw)
        with pytest.raises(ValueError):
            lmm.reml(args.pop("Y"), args.pop("W"), args.pop("Ks"), **args)
    with pytest.raises(ValueError):                         # more than 30 covariates at a size that has the samples for them
        lmm.reml(rng.standard_normal(40), rng.standard_normal((40, 31)), np.eye(40))


def test_vc_kinship_refusals_come_before_any_device_call(no_device):
    from pygemma import lmm
    K = np.eye(5)
    for Ks, s in [([K, K], [1.0, 1.0]), ([K], [1.0, 1.0, 1.0]), ([K], [-1.0, 1.0]), ([K], [np.nan, 1.0]), ([K], [0.0, 1.0]), ([K, K], [0.0, 0.0, 2.0]),
                  ([K, np.eye(6)], [1.0, 1.0, 1.0]), ([K.astype(np.int64)], [1.0, 1.0]), ([], [1.0]), ([K], [[1.0, 1.0]])]:
        with pytest.raises(ValueError):
            lmm.vc_kinship(Ks, np.array(s))
    with pytest.raises(ValueError):
        lmm.vc_kinship([K], lmm.RemlResult(sigma2=np.array([1.0, 1.0, 1.0])))


def test_vc_library_exports_what_its_header_declares_and_nothing_else():
    """libpygemma_vc.so against include/pygemma_vc.h, as tests/test_host_abi.py holds the main library to its header; the main
    library carries none of the unit's entry points."""
    import re
    import subprocess
    from pygemma_amd import _lib
    V = _lib.load_vc()
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.VC_HEADER).read(), flags=re.S)
    decl = re.findall(r"\b(pgx?_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert [name for name, _ in decl] == _lib.VC_SYMBOLS and len(decl) == 10
    for name, params in decl:
        assert len(getattr(V, name).argtypes) == params.count(",") + 1, name

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(("pg_", "pgx_"))}
    assert exported(_lib.VC_LIB_PATH) == set(_lib.VC_SYMBOLS)
    assert not exported(_lib.LIB_PATH) & set(_lib.VC_SYMBOLS)
    import ctypes as C
    assert V.pg_vc_eval_dev.argtypes == [C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 9
    assert V.pg_potri_work_bytes.restype is C.c_size_t and V.pg_vc_out_len(3, 5) == 4 + 3 * 4 + 16 + 5 + 25


def test_no_gpu_is_an_error_not_a_fallback():
    from pygemma_amd import _lib, lmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(_lib.PgError):
        lmm.reml(np.arange(6.0), np.ones((6, 1)), np.eye(6))
    with pytest.raises(_lib.PgError):
        lmm.vc_kinship([np.eye(6)], np.array([1.0, 1.0]))
