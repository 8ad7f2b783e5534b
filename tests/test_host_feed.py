"""CPU checks of the streamed entry points' shared transport (pygemma_amd/_feed.py): what _describe reads off every kind of
genotype source, what _genotypes makes of a raw argument, and that lmm and ops share one dtype table."""
import numpy as np
import pytest

from pygemma_amd.bed import PackedBed

N, P = 21, 7
CODES = {"int8": 0, "uint8": 1, "float32": 2, "float64": 3}       # PG_DTYPE_* of include/pygemma_hip.h


@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("dtype", list(CODES))
def test_describe_array(dtype, order):
    from pygemma_amd import _feed
    X = np.zeros((N, P), dtype, order=order)
    d = _feed._describe(X)
    esz = np.dtype(dtype).itemsize
    assert d.src is X and d.packed is False and d.snp_major is (order == "F")
    assert (d.esz, d.row_bytes, d.n, d.p) == (esz, N * esz, N, P)
    assert d.dtype_code == CODES[dtype] and d.count_a1 is None
    assert d.direct is False                                       # ordinary memory: staged


@pytest.mark.parametrize("count_a1", [False, True])
@pytest.mark.parametrize("strided", [False, True])
def test_describe_packed_bed(strided, count_a1):
    from pygemma_amd import _feed
    bpr = (N + 3) // 4
    data = np.zeros((P, bpr + 5), np.uint8)[:, :bpr] if strided else np.zeros((P, bpr), np.uint8)
    assert data.flags.c_contiguous is (not strided)
    bed = PackedBed(data, N, count_A1=count_a1)
    d = _feed._describe(bed)
    assert d.src is bed and d.packed is True and d.snp_major is True
    assert (d.esz, d.row_bytes, d.n, d.p) == (1, bpr, N, P)
    assert d.dtype_code is None and d.count_a1 == int(count_a1)
    assert d.direct is False


def test_a_single_row_or_column_is_sample_major():
    from pygemma_amd import _feed
    for shape in ((1, P), (N, 1)):                                 # both C- and F-contiguous: read as C order, like _put_window
        assert _feed._describe(np.zeros(shape, np.float32, order="F")).snp_major is False


def test_genotypes_normalises_a_raw_argument():
    from pygemma_amd import _feed
    bed = PackedBed(np.zeros((P, (N + 3) // 4), np.uint8), N)
    assert _feed._genotypes(bed, "f") is bed
    for dtype in CODES:
        for order in "CF":
            X = np.zeros((N, P), dtype, order=order)
            assert _feed._genotypes(X, "f") is X                   # no copy, no cast
    wide = np.arange(N * 2 * P, dtype=np.float32).reshape(N, 2 * P)
    Y = _feed._genotypes(wide[:, ::2], "f")
    assert Y.flags.c_contiguous and (Y == wide[:, ::2]).all()
    assert _feed._genotypes([[1.0, 2.0], [3.0, 4.0]], "f").dtype == np.float64
    for bad in (np.zeros(N, np.int8), np.zeros((2, N, P), np.float32)):
        with pytest.raises(ValueError, match="2-D"):
            _feed._genotypes(bad, "f", cast=True)
    for dtype in (np.int16, np.float16, bool, np.int64):
        with pytest.raises(ValueError, match="entry_point takes .* not " + np.dtype(dtype).name):
            _feed._genotypes(np.zeros((N, P), dtype), "entry_point")
        Z = _feed._genotypes(np.ones((N, P), dtype), "entry_point", cast=True)
        assert Z.dtype == np.float32 and (Z == 1).all()


def test_one_dtype_table_and_one_column_list():
    from pygemma_amd import _feed, lmm, ops
    assert {str(k): v for k, v in _feed._KIN_DTYPES.items()} == CODES
    assert lmm._KIN_DTYPES is _feed._KIN_DTYPES and ops._KIN_DTYPES is _feed._KIN_DTYPES
    assert lmm._LM_COLS is ops.LM_COLS and not hasattr(ops, "_LM_DTYPES")
    assert lmm._Pinned is _feed._Pinned and lmm._put_window is _feed._put_window
    assert lmm._U_PANEL_BYTES == 256 << 20


class _Recorder:
    """Stands in for the loaded library: every entry point records (name, arguments) and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def test_one_bed_or_x_fork_passes_what_the_entry_points_take():
    """_call_dev on the ragged last batch (SNPs [8, 10) of p = 10 at pb = 4, n = 13) of a PackedBed, a C-order and an F-order
    array: for the three streamed consumers, the entry point's name and every argument in ABI order, written out."""
    from pygemma_amd import _feed
    n, p, s, e = 13, 10, 8, 10
    H, SLOT, ACC, WORK, DC, DM, O = 0x10, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, (0x71, 0x72, 0x73, 0x74, 0x75)
    c, t, std = 3, 2, 1
    bed = _feed._describe(PackedBed(np.zeros((p, 4), np.uint8), n, count_A1=True))
    xc = _feed._describe(np.zeros((n, p), np.float64))
    xf = _feed._describe(np.zeros((n, p), np.float32, order="F"))
    want = {
        ("pg_kinship_{}_acc_dev", "bed"): ("pg_kinship_bed_acc_dev", (H, 13, 2, SLOT, 4, 1, 1, ACC)),
        ("pg_kinship_{}_acc_dev", "C"): ("pg_kinship_x_acc_dev", (H, 13, 2, SLOT, 3, 2, 0, 1, ACC)),
        ("pg_kinship_{}_acc_dev", "F"): ("pg_kinship_x_acc_dev", (H, 13, 2, SLOT, 2, 13, 1, 1, ACC)),
        ("pg_lm_{}_dev", "bed"): ("pg_lm_bed_dev", (H, 13, 3, 2, 2, SLOT, 4, 1, WORK, 0x71, 0x72, 0x73, 0x74, 0x75, 10)),
        ("pg_lm_{}_dev", "C"): ("pg_lm_x_dev", (H, 13, 3, 2, 2, SLOT, 3, 2, 0, WORK, 0x71, 0x72, 0x73, 0x74, 0x75, 10)),
        ("pg_lm_{}_dev", "F"): ("pg_lm_x_dev", (H, 13, 3, 2, 2, SLOT, 2, 13, 1, WORK, 0x71, 0x72, 0x73, 0x74, 0x75, 10)),
        ("pg_snp_stats_{}_dev", "bed"): ("pg_snp_stats_bed_dev", (H, 13, 2, SLOT, 4, 1, WORK, DC, DM)),
        ("pg_snp_stats_{}_dev", "C"): ("pg_snp_stats_x_dev", (H, 13, 2, SLOT, 3, 2, 0, WORK, DC, DM)),
        ("pg_snp_stats_{}_dev", "F"): ("pg_snp_stats_x_dev", (H, 13, 2, SLOT, 2, 13, 1, WORK, DC, DM)),
    }
    for kind, src in (("bed", bed), ("C", xc), ("F", xf)):
        L = _Recorder()
        _feed._call_dev(L, "pg_kinship_{}_acc_dev", src, (H, n, e - s), SLOT, e - s, (std, ACC))
        _feed._call_dev(L, "pg_lm_{}_dev", src, (H, n, c, t, e - s), SLOT, e - s, (WORK, *O, p))
        _feed._call_dev(L, "pg_snp_stats_{}_dev", src, (H, n, e - s), SLOT, e - s, (WORK, DC, DM))
        assert L.calls == [want[stem, kind] for stem in ("pg_kinship_{}_acc_dev", "pg_lm_{}_dev", "pg_snp_stats_{}_dev")], kind
        assert all(type(a) is int for _, args in L.calls for a in args), kind


def test_a_failing_entry_point_is_reported_by_its_name(monkeypatch):
    from pygemma_amd import _feed, _lib
    seen = []
    monkeypatch.setattr(_lib, "check", lambda rc, what="": seen.append((rc, what)))
    L = _Recorder()
    _feed._call_dev(L, "pg_lm_{}_dev", _feed._describe(np.zeros((5, 3), np.int8)), (1,), 2, 3, (4,))
    assert seen == [(0, "pg_lm_x_dev")] and L.calls == [("pg_lm_x_dev", (1, 2, 0, 3, 0, 4))]
