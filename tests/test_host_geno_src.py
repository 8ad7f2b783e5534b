"""CPU checks of the one genotype-source dispatch (csrc/geno_src.hpp): every entry point that takes an array of a PG_DTYPE_* keeps its own
refusal of an unknown dtype — the code that include/pygemma_hip.h documents for it, under its own name, before anything is touched."""
import numpy as np
import pytest

EINVAL, ENOTSUP = -22, -95

# otherwise valid small arguments (n = 8, pb = 1, pitch 8 in either storage order); c: the context, p: a buffer on 16 bytes, d: the dtype,
# sm: snp_major
X_ENTRY = {
    "pg_kinship_x_acc_dev": (EINVAL, lambda L, c, p, d, sm: L.pg_kinship_x_acc_dev(c, 8, 1, p, d, 8, sm, 0, p)),
    "pg_lm_x_dev": (EINVAL, lambda L, c, p, d, sm: L.pg_lm_x_dev(c, 8, 1, 1, 1, p, d, 8, sm, p, p, p, p, p, p, 1)),
    "pg_snp_stats_x_dev": (ENOTSUP, lambda L, c, p, d, sm: L.pg_snp_stats_x_dev(c, 8, 1, p, d, 8, sm, p, p, p)),
    "pg_prs_x_acc_dev": (ENOTSUP, lambda L, c, p, d, sm: L.pg_prs_x_acc_dev(c, 8, 1, p, d, 8, sm, 1, p, 1, 0, p, p, p, 8)),
    "pg_ld_encode_x_dev": (ENOTSUP, lambda L, c, p, d, sm: L.pg_ld_encode_x_dev(c, 8, 1, p, d, 8, sm, p, 1, 0)),
    "pg_king_x_acc_dev": (ENOTSUP, lambda L, c, p, d, sm: L.pg_king_x_acc_dev(c, 8, 1, p, d, 8, sm, p)),
    "pg_sample_stats_x_acc_dev": (ENOTSUP, lambda L, c, p, d, sm: L.pg_sample_stats_x_acc_dev(c, 8, 1, p, d, 8, sm, p)),
}


@pytest.mark.parametrize("dtype", [-1, 4])
@pytest.mark.parametrize("name", sorted(X_ENTRY))
def test_an_unknown_dtype_is_refused_with_the_entry_points_own_code(name, dtype):
    from pygemma_amd import _lib
    L = _lib.load()
    code, call = X_ENTRY[name]
    buf = np.zeros(8192, np.uint8)
    base = (buf.ctypes.data + 15) // 16 * 16
    dummy_ctx = np.zeros(4096, np.uint8)          # the checks never read the context
    for snp_major in (0, 1):
        assert call(L, dummy_ctx.ctypes.data, base, dtype, snp_major) == code
        msg = L.pg_last_error().decode()
        assert name in msg and "dtype" in msg and str(dtype) in msg
        assert not buf.any() and not dummy_ctx.any()
