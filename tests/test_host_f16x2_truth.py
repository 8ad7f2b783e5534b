"""CPU checks of the host model of the fp16 x 2 kernels (tests/_f16x2_truth.py), the reference a device comparison holds
rotate_geno_kernel<16>, <32>, the split-plane rotation and kin_geno_kernel to: the plane split recomposes the scaled value, the panels
stand on their conditions at every shape of the device grids, the model agrees with an evaluation in fractions.Fraction, and wrong
models — the ways these kernels can be wrong — each change the outputs of some panel.

Outputs changed by each wrong model on the 129 x 40 panels (5 160 outputs each; test_wrong_models_change_outputs prints the counts and
holds them to a stated minimum) and on the 256 x 65 kinship panel:

    wrong model                                         D       S1      S2      S3
    low plane dropped in K-tile 1                       4 855   0       5 116   5 064      (S1's U has no low plane)
    interleave read as [plane][K-tile]                  5 160   5 159   5 160   5 160
    sample 64 dropped                                   3 354   4 953   5 160   80         (S3: the two eigenvectors that hold it)
    eigen index shifted by one                          5 160   5 160   5 160   5 160
    truncation instead of ties to even                  0       0       0       3 636      (H1 + H2 is the same sum on an exact panel)
    X2 pass skipped                                     -       5 140   0       -          (S2's X2 is 0)
    second pass not rounded through float32             362     -       -       -          (of the 1 290 outputs of columns it can touch)
    low planes of R and (mu - r) R dropped              K: 28 279 of 65 536
    acc / p rounded once instead of twice               none, and none can exist: test_one_rounding_of_the_quotient_is_the_same_function

Swapping H1 and H2 of one K-tile is no wrong model: both planes meet the same genotype fragment in one accumulator, so the sum is the
same; what can go wrong with the interleave Up[k][kt][plane][j] is its index order, which is the wrong model above."""
from fractions import Fraction

import numpy as np
import pytest

import _f16x2_truth as T


# ---- the split and the scales ------------------------------------------------------------------------------------------------------------

def test_scale_rule():
    for m, S in [(1.0, 2.0 ** 14), (0.999, 2.0 ** 15), (2.0, 2.0 ** 13), (4095 / 4096, 2.0 ** 15), (2.0 ** -20, 2.0 ** 34), (3.0e38, 2.0 ** -113)]:
        s, inv = T.pow2_scale(np.float32(m))
        assert s == S and s * inv == 1.0
        assert 2.0 ** 14 <= float(np.float32(m)) * s < 2.0 ** 15
    assert T.pow2_scale(0.0) == (1.0, 1.0)
    s, inv = T.pow2_scale(np.float32(1e-45))           # a subnormal maximum: the exponent field of S is clamped at 254
    assert s == 2.0 ** 127 and inv == 2.0 ** -127


@pytest.mark.parametrize("kind,n", [("D", 129), ("S1", 129), ("S2", 1030), ("D", 1030)])
def test_planes_recompose_the_scaled_value_exactly_on_the_exact_panels(kind, n):
    U, pr = T.basis(kind, n)
    assert (pr.H1 + pr.H2 == U.astype(np.float64) * pr.S).all()
    X = T.block("S1" if kind == "S1" else "S2", n, 19)
    X1, X2, inv = T.split_x(X)
    assert (X1 + X2 == X.astype(np.float64) / inv.astype(np.float64)[None, :]).all()


def test_planes_of_generic_input_are_within_2_to_minus_23():
    rng = np.random.default_rng(5)
    u = (rng.standard_normal((200, 200)) * 10.0 ** rng.uniform(-3, 0, (200, 200))).astype(np.float32)
    pr = T.prep(u)
    su = u.astype(np.float64) * pr.S
    # the residual is at most half a step of H1 and, unless it is a power of two, starts a bit lower: H2 loses bit 23 alone.  Where H2 is
    # an fp16 subnormal (|S u| < 2^-2, steps of 2^-24) the error is half such a step instead.
    assert (np.abs(su - pr.H1 - pr.H2) <= np.maximum(2.0 ** -23 * np.abs(su), 2.0 ** -25)).all()
    assert (np.abs(su - pr.H1 - pr.H2) <= 2.0 ** -23 * np.abs(su))[np.abs(su) >= 0.25].all() and (np.abs(su) >= 0.25).mean() > 0.98
    assert np.abs(pr.H2).max() < 2.0 ** 5 and np.abs(pr.H1).max() < 2.0 ** 15
    X = T.block_s3(200, 30)
    X1, X2, inv = T.split_x(X)
    sx = X.astype(np.float64) / inv.astype(np.float64)[None, :]
    assert (np.abs(sx - X1 - X2) <= np.maximum(2.0 ** -23 * np.abs(sx), 2.0 ** -25)).all()


def test_ties_go_to_even_and_truncation_differs():
    x = np.float32([16384 + 4, 16384 + 12, 16384 - 2, -(16384 + 4), 2049, 2051, 5.5])
    assert T.f16_rn(x).tolist() == [16384, 16400, 16384, -16384, 2048, 2052, 5.5]
    assert T.f16_trunc(x).tolist() == [16384, 16384, 16376, -16384, 2048, 2050, 5.5]
    h1, h2 = T.split(x)
    assert h2.tolist() == [4, -4, -2, -4, 1, -1, 0]


def test_colsum_in_kernel_order():
    rng = np.random.default_rng(3)
    U = (rng.standard_normal((200, 5)) * 10.0 ** rng.uniform(-8, 8, (200, 5))).astype(np.float32)
    want = np.zeros(5)
    for t in range(0, 200, 64):
        s = np.zeros(5)
        for i in range(t, min(t + 64, 200)):
            s += U[i].astype(np.float64)
        want += s
    assert (T.colsum(U) == want).all()
    assert (T.colsum(U) != U.astype(np.float64).sum(0)).any()          # NumPy's pairwise sum is another order


# ---- the conditions, at every shape of the device grids ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,p", T.DIAG)
def test_conditions_d(n, p):
    _, pr = T.basis("D", n)
    worst = 0.0
    for dtype in (np.float32, np.int8, np.uint8):
        worst = max(worst, T.conditions("D", pr, T.block("D", n, p, dtype)))
    print(f"D n={n} p={p}: largest sum |terms| / 2^24 = {worst:.4f}")
    if n >= 4 and p >= 4:
        assert T.I8.encode_x(T.block("D", n, p))[3].any()          # the indicator pass runs


def test_conditions_full_grids():
    for n in T.NS:
        for kind in ("D", "S1"):
            if kind == "S1" and n < 4:
                continue
            _, pr = T.basis(kind, n)
            for p in T.PS:
                T.conditions(kind, pr, T.block(kind, n, p))


@pytest.mark.parametrize("n,p", T.SPLIT_DIAG)
def test_conditions_split(n, p):
    for kind, dtypes in (("S1", [np.float32]), ("S2", [np.float32, np.int8, np.uint8]), ("S3", [np.float32])):
        _, pr = T.basis(kind, n)
        for dtype in dtypes:
            worst = T.conditions(kind, pr, T.block(kind, n, p, dtype))
            print(f"{kind} {np.dtype(dtype).name} n={n} p={p}: largest sum |terms| / 2^24 = {worst:.4f}")


def test_no_block_of_fewer_than_four_samples_takes_the_split_path():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3):
        for _ in range(50):
            assert T.path_of(rng.standard_normal((n, 7)).astype(np.float32)) == 1
    assert T.path_of(rng.standard_normal((4, 7)).astype(np.float32)) == 2


def test_sparse_basis_hits_every_sample():
    for n in (4, 65, 129, 1030):
        U = T.basis("S3", n)[0]
        assert ((U != 0).sum(0) <= 2).all() and ((U != 0).sum(1) >= 1).all()
        for i in {min(63, n - 1), min(64, n - 1), min(127, n - 1), min(128, n - 1), n - 1}:
            assert U[i].any()


@pytest.mark.parametrize("p", T.KIN_PS)
@pytest.mark.parametrize("n", T.KIN_NS)
def test_conditions_kinship_and_the_exact_truth(n, p):
    """kin_model asserts sum |terms| < 2^24 for every batch; its K carries the bits of float32(float64(exact p K) / p) on both paths and
    at every batch size, and the panels with missing calls have the low plane of (mu - r) R at work"""
    for standardize in (False, True):
        X = T.kin_panel(n, p, standardize)
        want = T.kin_exact(X, standardize)
        for batch in T.kin_batches(p):
            for fp32 in (False, True):
                info = {}
                K = T.kin_model(X, standardize, batch, bed=True, fp32=fp32, info=info)
                assert (K.view(np.uint32) == want.view(np.uint32)).all(), (standardize, batch, fp32)
                assert info["worst"] < 1.0
                if not standardize and not fp32 and n >= 130 and p >= 64:          # mu = k / 64: (mu - r) mu reaches 12 bits
                    assert info["low_share"] > 0.02, info
        Xa = T.kin_panel(n, p, standardize, missing=False)
        Ka = T.kin_model(Xa, standardize, p, bed=False)
        assert (Ka.view(np.uint32) == T.kin_exact(Xa, standardize).view(np.uint32)).all()


# ---- the model against exact rational arithmetic ------------------------------------------------------------------------------------------

def _f32(q):
    """a Fraction rounded to fp64 (Python's division is correctly rounded) and then to float32: the two roundings of an epilogue"""
    return np.float32(q.numerator / q.denominator)


def _frac_rotate(pr, v0, ops):
    """the passes of a block in Fractions: ops = [(A (n, p), mul (p,)), ...], the first on the base v0 colsum, the others accumulating"""
    n, p = pr.n, ops[0][0].shape[1]
    out = np.zeros((p, n), np.float32)
    H = [[Fraction(float(pr.H1[i, k])) + Fraction(float(pr.H2[i, k])) for k in range(n)] for i in range(n)]
    for g in range(p):
        for k in range(n):
            x = None
            for A, m in ops:
                a = sum(Fraction(float(A[i, g])) * H[i][k] for i in range(n))
                base = Fraction(float(v0[g])) * Fraction(float(pr.colsum[k])) if x is None else Fraction(float(x))
                x = _f32(Fraction(float(m[g])) * Fraction(pr.invS) * a + base)
            out[g, k] = x
    return out


@pytest.mark.parametrize("n,p", [(5, 6), (9, 4)])
def test_model_agrees_with_fractions_on_small_panels(n, p):
    pr = T.prep(T.basis_d(n, seed=2))
    X = T.block_d(n, p, np.float32, seed=2)
    codes, v0, dx, ind, dlt = T.I8.encode_x(X)
    assert ind.any()
    want = _frac_rotate(pr, v0, [(codes, dx), (ind, dlt)])
    got = T.rotate_geno(pr, X)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    pr = T.prep(T.basis_s1(n, seed=2))
    X = T.block_s1(n, p, seed=2)
    X1, X2, inv = T.split_x(X)
    assert X2.any()
    want = _frac_rotate(pr, np.zeros(p), [(X1, inv), (X2, inv)])
    got = T.rotate_split(pr, X)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (got.astype(np.float64) == X.astype(np.float64).T @ T.basis_s1(n, seed=2).astype(np.float64)).all()      # short dyadics: U'x itself


def test_generic_split_agrees_with_fractions():
    n, p = 9, 4
    pr = T.prep(T.basis_sparse(n))
    X = T.block_s3(n, p)
    exact, bound = T.split_generic(pr, X)
    X1, X2, inv = T.split_x(X)
    for g in range(p):
        for k in range(n):
            q = sum((Fraction(float(X1[i, g])) + Fraction(float(X2[i, g]))) * (Fraction(float(pr.H1[i, k])) + Fraction(float(pr.H2[i, k])))
                    for i in range(n)) * Fraction(float(inv[g])) * Fraction(pr.invS)
            assert abs(Fraction(float(exact[g, k])) - q) <= Fraction(2.0 ** -50) * abs(q)
            assert bound[g, k] >= 2.0 ** -24 * abs(exact[g, k])


def test_kinship_model_agrees_with_fractions():
    for standardize in (False, True):
        n, p = 6, 9
        X = T.kin_panel(n, p, standardize)
        mis = np.isnan(X)
        K = T.kin_model(X, standardize, 4, bed=True)
        for i in range(n):
            for k in range(n):
                tot = Fraction(0)
                for j in range(p):
                    col = [Fraction(float(v)) for v in X[~mis[:, j], j]]
                    mu = sum(col) / len(col)
                    xi = [mu if mis[r, j] else Fraction(float(X[r, j])) for r in range(n)]
                    if standardize:
                        m = sum(xi) / n
                        var = sum((v - m) ** 2 for v in xi) / n
                        tot += (xi[i] - m) * (xi[k] - m) / (var if var > 0 else 1)
                    else:
                        tot += xi[i] * xi[k]
                assert K[i, k] == np.float32(np.float64(tot.numerator / tot.denominator) / np.float64(p)), (i, k)


# ---- wrong models ---------------------------------------------------------------------------------------------------------------------------

def _mutated(pr, what):
    """a Prep that is wrong in one stated way"""
    n = pr.n
    H1, H2 = pr.H1.copy(), pr.H2.copy()
    if what == "low plane dropped in K-tile 1":
        H2[64:128] = 0
    elif what == "interleave read as [plane][K-tile]":
        kt = (n + 63) // 64
        pad = lambda H: np.concatenate([H, np.zeros((kt * 64 - n, n))]).reshape(kt, 64, n)
        chunks = np.stack([pad(H1), pad(H2)], axis=1).reshape(2 * kt, 64, n)          # memory order: [K-tile][plane]
        H1 = np.concatenate([chunks[0 * kt + t] for t in range(kt)])[:n]               # stage (t, plane) reads chunk plane * kt + t
        H2 = np.concatenate([chunks[1 * kt + t] for t in range(kt)])[:n]
    elif what == "sample 64 dropped":
        H1[64] = 0; H2[64] = 0
    elif what == "eigen index shifted by one":
        H1, H2 = np.roll(H1, -1, axis=1), np.roll(H2, -1, axis=1)
    else:
        raise AssertionError(what)
    return T.Prep(H1, H2, pr.S, pr.invS, pr.colsum)


def _changed(a, b):
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~((a == 0) & (b == 0))).sum())


GEMM_MUTANTS = ["low plane dropped in K-tile 1", "interleave read as [plane][K-tile]", "sample 64 dropped", "eigen index shifted by one"]


def test_wrong_models_change_outputs():
    """the table of the module docstring"""
    n, p = 129, 40
    size = n * p
    report = {}
    right, prs, Xs = {}, {}, {}
    for kind in ("D", "S1", "S2", "S3"):
        U, prs[kind] = T.basis(kind, n)
        Xs[kind] = T.block(kind, n, p)
        T.conditions(kind, prs[kind], Xs[kind])
        right[kind] = T.model(kind, prs[kind], Xs[kind]) if kind != "S3" else T.split_generic(prs[kind], Xs[kind])[0].astype(np.float32)
    for what in GEMM_MUTANTS:
        for kind in ("D", "S1", "S2", "S3"):
            m = _mutated(prs[kind], what)
            wrong = T.model(kind, m, Xs[kind]) if kind != "S3" else T.split_generic(m, Xs[kind])[0].astype(np.float32)
            report[what, kind] = _changed(wrong, right[kind])
    for kind in ("D", "S1", "S2", "S3"):
        U = T.basis(kind, n)[0]
        m = T.prep(U, conv=T.f16_trunc)
        if kind == "D":
            wrong = T.rotate_geno(m, Xs[kind])
        elif kind == "S3":
            wrong = T.split_generic(m, Xs[kind], conv=T.f16_trunc)[0].astype(np.float32)
        else:
            wrong = T.rotate_split(m, Xs[kind], conv=T.f16_trunc)
        report["truncation instead of ties to even", kind] = _changed(wrong, right[kind])
    report["X2 pass skipped", "S1"] = _changed(T.rotate_split(prs["S1"], Xs["S1"], skip_x2=True), right["S1"])
    report["X2 pass skipped", "S2"] = _changed(T.rotate_split(prs["S2"], Xs["S2"], skip_x2=True), right["S2"])
    report["second pass not rounded through float32", "D"] = _changed(T.rotate_geno(prs["D"], Xs["D"], round_between=False), right["D"])
    for key, count in report.items():
        print(f"{key[0]:45s} {key[1]:3s} {count:6d} of {size}")
    tenth = size // 10
    assert report["low plane dropped in K-tile 1", "D"] >= tenth and report["low plane dropped in K-tile 1", "S2"] >= tenth
    assert report["low plane dropped in K-tile 1", "S3"] >= tenth
    assert report["low plane dropped in K-tile 1", "S1"] == 0                       # S1's U has no low plane: D, S2 and S3 are there for it
    for what in GEMM_MUTANTS[1:]:
        for kind in ("D", "S1", "S2", "S3"):
            if (what, kind) == ("sample 64 dropped", "S3"):
                assert report[what, kind] == 2 * p          # two eigenvectors hold sample 64: every SNP of both
            else:
                assert report[what, kind] >= tenth, (what, kind)
    for kind in ("D", "S1", "S2"):
        assert report["truncation instead of ties to even", kind] == 0              # H1 + H2 is the same sum: exact panels cannot see it
    assert report["truncation instead of ties to even", "S3"] >= size // 2
    assert report["X2 pass skipped", "S1"] >= size // 2 and report["X2 pass skipped", "S2"] == 0
    assert report["second pass not rounded through float32", "D"] >= size // 20      # a quarter of the columns have an other value and v0 != 0


def test_wrong_kinship_model_changes_outputs():
    n, p = 256, 65          # 128 of the 256 samples called in every second SNP: the (mu - r) R planes carry a quarter of K's entries
    X = T.kin_panel(n, p, False)
    right = T.kin_model(X, False, 64, bed=True)
    count = _changed(T.kin_model(X, False, 64, bed=True, drop_low=True), right)
    print(f"{'low planes of R and (mu - r) R dropped':45s} K   {count:6d} of {n * n}")
    assert count >= n * n // 10


@pytest.mark.parametrize("p", [1, 3, 7, 19, 200, 4100, 999983])
def test_one_rounding_of_the_quotient_is_the_same_function(p):
    """pg_kinship_finish_dev rounds acc / p to fp64 and then to float32.  For p < 2^28 that IS float32(acc / p): the two differ only if
    the fp64 quotient lands on the midpoint `mid` of two float32 while acc / p != mid, i.e. 0 < |acc - p mid| <= p ulp64(mid) / 2; but
    p mid has at most 25 + 28 bits, so it is an fp64 itself, and the next fp64 beside it is ulp64(p mid) > p ulp64(mid) / 2 away.  So a
    model that rounds once is no wrong model, and no panel can tell it from the kernel; checked here on the accumulators where it would
    show (T.finish_panel: p mid and its neighbours)."""
    acc = T.finish_panel(p)
    twice, once = T.kin_finish(acc, p), T.kin_finish(acc, p, once=True)
    assert (twice.view(np.uint32) == once.view(np.uint32)).all()
