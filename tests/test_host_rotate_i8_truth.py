"""CPU checks of the host model of the int8 genotype rotation (tests/_rotate_i8_truth.py), the reference tests/test_gpu_rotate_i8_exact.py
holds the kernel to bit for bit: the digit planes recompose q with every digit an int8, the fixed point is within half a unit of U, the
exact fma agrees with fractions.Fraction, the rotation stays within the representation's own error of an fp64 U'x, and the .bed decode
equals PackedBed's at every n % 4 with garbage in the pad bits."""
from fractions import Fraction

import numpy as np
import pytest

import _rotate_i8_truth as T


@pytest.fixture(scope="module")
def adversarial():
    U, bad = T.adversarial_basis()
    return U, bad, T.prep(U)


def _bases():
    yield "adversarial", T.adversarial_basis()[0]
    yield "identity", np.eye(86, dtype=np.float32)
    for n in (1, 3, 64, 130):
        yield f"random {n}", T.basis(n)
    rng = np.random.default_rng(9)
    yield "graded", (T.basis(200).astype(np.float64) * 10.0 ** rng.uniform(-30, 30, (1, 200))).astype(np.float32)


@pytest.mark.parametrize("name,U", list(_bases()), ids=lambda v: v if isinstance(v, str) else "")
def test_digits_are_int8_and_recompose_q(name, U):
    pr = T.prep(U)
    d2, d1, d0 = T.digits(pr.q)
    for d in (d2, d1, d0):
        assert d.min() >= -128 and d.max() <= 127
    assert (65536 * d2 + 256 * d1 + d0 == pr.q).all()
    assert np.abs(pr.q).max() <= T.QMAX


def test_digit_carries_on_chosen_q():
    q = np.array([0, 127, 128, 129, -127, -128, -129, 255, 256, 32767, 32768, 32769, -32768, -32769, 32768 + 128, T.QMAX, -T.QMAX, 1 << 22])
    d2, d1, d0 = T.digits(q)
    assert (65536 * d2 + 256 * d1 + d0 == q).all()
    assert list(zip(d2[:7], d1[:7], d0[:7])) == [(0, 0, 0), (0, 0, 127), (0, 1, -128), (0, 1, -127), (0, 0, -127), (0, 0, -128), (0, -1, 127)]
    assert (d2[15], d1[15], d0[15]) == (127, 127, 127) and (d2[16], d1[16], d0[16]) == (-127, -127, -127)
    assert (d2[11], d1[11], d0[11]) == (1, -128, 1) and (d2[14], d1[14], d0[14]) == (1, -127, -128)


@pytest.mark.parametrize("name,U", list(_bases()), ids=lambda v: v if isinstance(v, str) else "")
def test_fixed_point_is_within_half_a_unit(name, U):
    pr = T.prep(U)
    ok = np.isfinite(pr.w)
    # U / w and q are exact in float64 (w a power of two, |q| < 2^24), so is their difference
    e = U.astype(np.float64)[:, ok] / pr.w[ok] - pr.q[:, ok]
    assert (np.abs(e) <= 0.5).all()
    assert (pr.q[:, ~ok] == 0).all()


def test_prepare_step_on_the_adversarial_columns(adversarial):
    U, bad, pr = adversarial
    name = T.ADVERSARIAL
    w, q = pr.w, pr.q
    assert w[name.index("pow2 max")] == 2.0 ** -23 and q[:, 0].max() == 1 << 22
    assert w[1] == 2.0 ** -23 and q[0, 1] == 1 << 22                    # (2 - 2^-23) 2^-2 on the raised scale: 2^22 - 1/4 -> 2^22
    assert w[2] == 2.0 ** -24 and q[U.shape[0] // 2, 2] == 4177856      # 8355711.5 / 2 = 4177855.75 -> ...56
    assert w[3] == 2.0 ** -25 and q[127, 3] == -T.QMAX
    t = U[:, 4].astype(np.float64) * 2.0 ** 23
    assert w[4] == 2.0 ** -23 and (q[:, 4] == np.rint(t)).all()
    assert [int(v) for v in q[1:13, 4]] == [128, 128, -128, -128, 0, 0, 2, -2, 32768, 32768, -32768, -32768]      # ties to even
    for k in (5, 6, 7):
        assert w[k] == 1.0 and (q[:, k] == 0).all()
    assert w[8] == 2.0 ** -122 and q[64, 8] == 1 << 22
    assert w[9] == 2.0 ** -22 and q[5, 9] == 1 << 22 and np.abs(q[:, 9]).sum() - (1 << 22) > 0
    assert np.isnan(w[bad]).all() and np.isfinite(w[~bad]).all()
    assert np.isnan(pr.colsum[10]) and np.isinf(pr.colsum[11]) and np.isfinite(pr.colsum[~bad]).all()
    assert q[85, 15] == -(1 << 22)
    assert pr.colsum[6] != 0 and abs(pr.colsum[6]) < 2.0 ** -120          # the denormals' sum is kept in fp64


def test_colsum_in_kernel_order():
    """tiles of 64 samples summed in sequence, then the partials in sequence: not NumPy's pairwise sum, and equal to plain loops"""
    n = 200
    U = (T.basis(n).astype(np.float64) * 10.0 ** np.random.default_rng(2).uniform(-3, 3, (n, 1))).astype(np.float32)
    pr = T.prep(U)
    for k in (0, 63, 199):
        tot = 0.0
        for t0 in range(0, n, 64):
            s = 0.0
            for i in range(t0, min(t0 + 64, n)):
                s += float(U[i, k])
            tot += s
        assert pr.colsum[k] == tot
    exact = np.array([float(sum(Fraction(float(v)) for v in U[:, k])) for k in range(n)])
    assert np.abs(pr.colsum - exact).max() <= 200 * 2.0 ** -53 * np.abs(U.astype(np.float64)).sum(0).max()


def test_exact_fma_agrees_with_fraction():
    rng = np.random.default_rng(4)
    m = 4000
    a = (rng.standard_normal(m).astype(np.float32).astype(np.float64)) * 2.0 ** rng.integers(-130, -10, m)
    P = rng.integers(-2 ** 34, 2 ** 34, m)
    b = rng.standard_normal(m) * np.abs(a * P) * 10.0 ** rng.uniform(-17, 3, m)
    b[:50] = -(a[:50] * P[:50])                                         # cancellation: the result is the product's own rounding error
    a[50:60] = 2.0 ** -1074; P[50:60] = rng.integers(-9, 9, 10); b[50:60] = rng.integers(-9, 9, 10) * 2.0 ** -1074 + 2.0 ** -1070
    got = T._fma_rows(a, P, b)
    want = np.array([float(Fraction(x) * int(k) + Fraction(y)) for x, k, y in zip(a, P, b)])
    assert (got.view(np.uint64) == want.view(np.uint64)).all()
    two = a * P + b                                                     # two roundings differ somewhere: the exact path is not idle
    assert (two != want).any()


def test_fp64_steps_reach_the_result_on_the_cancelling_basis():
    """what the device test can tell apart: on T.cancelling_basis another order of the fp64 column sum, or an fma rounded twice, changes
    float32 outputs (on a random orthogonal basis neither does: the sums are exact in fp64 and nothing cancels)"""
    n, p = 257, 130
    U = T.cancelling_basis(n)
    pr = T.prep(U)
    enc = T.encode_x(T.cancelling_block(n, p, np.float64))
    true = T.rotate(pr, *enc)
    assert np.isfinite(true).all()
    plain = np.zeros(n)
    for i in range(n):
        plain = plain + U[i].astype(np.float64)
    for cs in (plain, U.astype(np.float64).sum(0)):                     # one sequential sum; NumPy's pairwise sum
        other = T.rotate(T.Prep(pr.q, pr.w, cs), *enc)
        assert (other.view(np.uint32) != true.view(np.uint32)).sum() > 1000
    keep = T._fma_rows
    try:
        T._fma_rows = lambda a, P, b: a * P.astype(np.float64) + b
        twice = T.rotate(pr, *enc)
    finally:
        T._fma_rows = keep
    assert (twice.view(np.uint32) != true.view(np.uint32)).sum() > 30


def _x64(enc):
    codes, v0, dx, ind, dlt = enc
    f = lambda v: v.astype(np.float64)[None, :]
    return f(v0) + f(dx) * codes + f(dlt) * ind


def _check_within_representation(U, pr, enc, ok=None):
    """|model - U'x| <= dx sum_i |code_i| w_k / 2 + |dlt| sum_i ind_i w_k / 2   (|U - w q| <= w / 2 per entry)
                      + half a float32 ulp per pass (the roundings of Xr1 and Xr)
                      + 2^-50 sum_i |u_ik| |x_i| + 2^-50 |v0| sum_i |u_ik|        (the fp64 steps of both sides: n <= 2^9 roundings of 2^-53,
                                                                                   the column sum carries |v0| times its own)
    with x = v0 + dx code + dlt ind in fp64, the values the codes stand for."""
    codes, v0, dx, ind, dlt = enc
    ok = np.isfinite(pr.w) if ok is None else ok
    got = T.rotate(pr, *enc).astype(np.float64)[:, ok]
    U64, X64 = U.astype(np.float64)[:, ok], _x64(enc)
    ref = (U64.T @ X64).T
    w = pr.w[ok][None, :]
    quant = (np.abs(dx.astype(np.float64))[:, None] * np.abs(codes).sum(0)[:, None] + np.abs(dlt.astype(np.float64))[:, None] * ind.sum(0)[:, None]) * w / 2
    passes = 2 if ind.any() else 1
    half_ulp = passes * np.spacing((np.abs(ref) + quant).astype(np.float32)).astype(np.float64) / 2
    fp64 = 2.0 ** -50 * (np.abs(X64).T @ np.abs(U64) + np.abs(v0.astype(np.float64))[:, None] * np.abs(U64).sum(0)[None, :])
    err = np.abs(got - ref)
    assert (err <= quant + half_ulp + fp64).all(), float((err / (quant + half_ulp + fp64)).max())
    return err, quant


@pytest.mark.parametrize("n,p", [(1, 2), (3, 9), (85, 130), (129, 257), (257, 40)])
def test_model_within_the_representation_of_fp64_rotation(n, p):
    U = T.basis(n)
    pr = T.prep(U)
    for count_a1 in (0, 1):
        G = T.hard_calls(n, p, 1, miss=0.02)
        err, quant = _check_within_representation(U, pr, T.encode_bed(T.pack_bed(G, count_a1, extra=3), n, count_a1))
    for dtype in (np.float32, np.float64, np.int8, np.uint8):
        _check_within_representation(U, pr, T.encode_x(T.array_block(n, p, dtype, 2)))


def test_model_on_the_adversarial_basis(adversarial):
    U, bad, pr = adversarial
    n = U.shape[0]
    for enc in (T.encode_bed(T.pack_bed(T.hard_calls(n, 70, 3, miss=0.02), 0), n, 0), T.encode_x(T.array_block(n, 70, np.float32, 3))):
        xr = T.rotate(pr, *enc)
        assert np.isnan(xr[:, bad]).all() and np.isfinite(xr[:, ~bad]).all()
        _check_within_representation(U, pr, enc)
    codes, v0, dx, ind, dlt = T.encode_bed(T.pack_bed(T.hard_calls(n, 70, 3), 0), n, 0)
    xr = T.rotate(pr, codes, v0, dx, ind, dlt)
    for k, i in ((12, 12), (13, 128), (14, n - 1)):                     # unit eigenvectors: the output is the call itself (0 where missing)
        assert (xr[:, k] == (codes[i] + dlt * ind[i]).astype(np.float32)).all()
    assert (xr[:, [5, 6, 7]] == 0).all()                                # q = 0 and v0 = 0
    X = T.array_block(86, 50, np.float32, 5, imputed=False)
    eye = T.rotate(T.prep(np.eye(86, dtype=np.float32)), *T.encode_x(X))
    kinds = [k for k in T.FLOAT_KINDS if k != "imputed"]
    raw = np.array([kinds[(j + 86) % len(kinds)] in ("raw", "01", "12", "02", "one") for j in range(50)])      # v0 + dx code is exact
    assert (eye[raw] == X.T[raw]).all()


def test_encode_x_kinds_and_refusals():
    n = 40
    x = np.zeros((n, 6), np.float32)
    x[:, 0] = np.arange(n) % 3                                          # raw
    x[:, 1] = np.arange(n) % 2 + 1                                      # {1, 2}: v0 = 1, dx = 1/2, codes 0 / 2
    x[:, 2] = 1.25                                                      # one value
    x[:, 3] = np.arange(n) % 3; x[7, 3] = x[9, 3] = 0.75                # imputed
    x[:, 4] = (np.arange(n) % 3 - 1.0) / 3                              # centred: the midpoint rounds
    x[:, 5] = np.where(np.arange(n) % 2 == 0, -0.0, 2.0)                # -0.0 is the lowest key, equal to +0.0 by value
    x[1, 5] = 0.0
    codes, v0, dx, ind, dlt = T.encode_x(x)
    assert (codes[:, 0] == np.arange(n) % 3).all() and v0[0] == 0 and dx[0] == 1
    assert set(codes[:, 1]) == {0, 2} and v0[1] == 1 and dx[1] == 0.5
    assert (codes[:, 2] == 0).all() and v0[2] == np.float32(1.25) and dx[2] == 0
    assert ind[:, 3].sum() == 2 and ind[7, 3] == ind[9, 3] == 1 and codes[7, 3] == 0 and dlt[3] == np.float32(0.75) and dlt[0] == 0
    assert (codes[:, 4] == np.arange(n) % 3).all() and not ind[:, 4].any()
    assert np.signbit(v0[5]) and codes[1, 5] == 0 and not ind[:, 5].any()
    assert (T.encode_x(x.astype(np.float64))[0] == codes).all()
    y = x.copy(); y[11, 3] = 0.5
    with pytest.raises(ValueError):
        T.encode_x(y)
    y = x.copy(); y[0, 0] = np.nan
    with pytest.raises(ValueError):
        T.encode_x(y)


@pytest.mark.parametrize("count_a1", [False, True])
@pytest.mark.parametrize("n", [8, 9, 10, 11, 1, 2, 3, 257])
def test_encode_bed_equals_packed_bed_decode(n, count_a1):
    from pygemma_amd.bed import PackedBed
    p = 23
    G = T.hard_calls(n, p, 7, miss=0.1)
    data = T.pack_bed(G, count_a1, extra=0, seed=1)
    if n % 4:
        assert (data[:, -1] >> (2 * (n % 4))).any()                     # the pad bits are not all zero
    want = PackedBed(data, n, count_A1=count_a1).to_float(impute=False).astype(np.float64)      # (n, p), NaN = missing
    np.testing.assert_array_equal(want, G)
    for extra in (0, 3):
        wide = T.pack_bed(G, count_a1, extra=extra, seed=1)
        assert (wide[:, :data.shape[1]] == data).all()
        codes, v0, dx, ind, dlt = T.encode_bed(wide, n, count_a1)
        assert (ind == np.isnan(want)).all() and (codes == np.nan_to_num(want)).all()
        assert (v0 == 0).all() and (dx == 1).all()
        called = (~np.isnan(want)).sum(0)
        for g in range(p):
            mean = np.float32(np.nansum(want[:, g]) / called[g]) if 0 < called[g] < n else np.float32(0)
            assert dlt[g] == mean
    # garbage where nothing may be read changes nothing: other pad bits, other extra bytes
    other = T.pack_bed(G, count_a1, extra=3, seed=2)
    a, b = T.encode_bed(wide, n, count_a1), T.encode_bed(other, n, count_a1)
    assert all((u == v).all() for u, v in zip(a, b))
