"""CPU-only checks of the boundary: the C-ABI library loads and exports every symbol include/pygemma_hip.h
declares (no compute without a GPU), every function is bound with the signature the header declares, the host logic mirrors the reference's (SampleIter split, casts, error
behaviour), and the product never reaches for the oracle."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(pgx?_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.load()
    decl = _declared_symbols()
    assert len(decl) >= 20
    for sym in decl:
        assert hasattr(L, sym), f"{sym} declared in include/pygemma_hip.h but not exported"
    assert set(_lib.SYMBOLS) <= set(decl)
    assert b"gfx950" in L.pg_version()
    # and nothing of ours is exported that the header does not declare (VERDICT r1 hygiene: pgx_* test hooks are declared now)
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(("pg_", "pgx_"))}
    assert exported <= set(decl), sorted(exported - set(decl))


def _loaded():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load()


def test_every_declared_function_is_bound_with_its_parameter_count():
    """Counted here independently of _lib's parser: the names in header order, the commas of every parameter list."""
    _lib, L = _loaded()
    hdr = open(os.path.join(ROOT, "include", "pygemma_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = re.findall(r"\b(pgx?_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)
    assert len(decl) >= 89 and [name for name, _ in decl] == _lib.SYMBOLS
    for name, params in decl:
        f = getattr(L, name)
        assert f.argtypes is not None, f"{name}: no argtypes"
        assert len(f.argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name


def test_pinned_signatures_one_per_type_class():
    """Written out by hand from include/pygemma_hip.h."""
    import ctypes as C
    _lib, L = _loaded()
    vp, i64, i32, sz, f32, f64 = C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_float, C.c_double
    pinned = {
        "pg_assoc_dev": (i32, [vp, i64, i32, i64, vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp]),
        "pg_score_dev": (i32, [vp, i64, i32, i64, vp, vp, vp, f32, vp, i64, vp, vp, vp, vp, vp, vp]),
        "pgx_dgemm_ex_dev": (i32, [vp, i32, i32, i64, i64, i64, f64, vp, i64, vp, i64, f64, vp, i64]),
        "pg_memcpy2d_h2d_async": (i32, [vp, vp, sz, vp, sz, sz, sz]),
        "pg_geno_prep_bytes": (sz, [i64]),
        "pg_ctx_destroy": (None, [vp]),
        "pg_last_error": (C.c_char_p, []),
        "pg_comm_init_all": (i32, [i32, vp, vp]),              # pg_ctx *const *, pg_comm **
        "pg_stage_rows": (i32, [vp, sz, vp, sz, sz, sz, i32]),  # no context argument
        "pgx_ring_stamps": (i32, [vp]),                         # long long *
    }
    assert len(pinned["pg_assoc_dev"][1]) == 17
    for name, (restype, argtypes) in pinned.items():
        f = getattr(L, name)
        assert f.restype is restype, (name, f.restype)
        assert list(f.argtypes) == argtypes, (name, f.argtypes)


def test_header_parser_on_a_text_of_its_own():
    import ctypes as C
    from pygemma_amd import _lib
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    text = """
    #ifdef __cplusplus
    extern "C" {
    #endif
    #define PG_X (-1)   /* pg_not_a_call(int) */
    typedef struct pg_ctx pg_ctx;
    enum { PG_A = 0, PG_B = 1 };
    int pg_init_all(int ndev, pg_ctx *const *ctxs, pg_comm **out /* [ndev] */);
    int pg_three(pg_ctx *ctx, int64_t n,
                 const float *d, unsigned long long *stats,
                 double alpha);   /* pg_in_a_comment(int x); */
    size_t pgx_bytes(int64_t n);
    const char *pg_text(void);
    void pg_close(pg_ctx *ctx);
    #ifdef __cplusplus
    }
    #endif
    """
    assert _lib.parse_header(text) == [("pg_init_all", i32, [i32, vp, vp]), ("pg_three", i32, [vp, i64, vp, vp, C.c_double]),
                                       ("pgx_bytes", C.c_size_t, [i64]), ("pg_text", C.c_char_p, []), ("pg_close", None, [vp])]
    # a type outside the table is an error that names the function and the type, never ctypes' default int
    for bad, ctype in (("int pg_bad(pg_ctx *ctx, long double x);", "long double"), ("long double pg_bad(void);", "long double"),
                       ("int pg_bad(unsigned n);", "unsigned"), ("int pg_bad(long long n);", "long long"), ("pg_bad(int n);", "")):
        with pytest.raises(_lib.PgError, match=f"pg_bad: C type '{ctype}'"):
            _lib.parse_header(bad)
    with pytest.raises(_lib.PgError, match="pg_bad: C type 'long double'"):
        _lib.parse_header(text.replace("size_t pgx_bytes", "int pg_bad(long double x);\n    size_t pgx_bytes"))


def test_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    _lib, _ = _loaded()
    gone = str(tmp_path / "include" / "pygemma_hip.h")
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER", gone)
    with pytest.raises(_lib.PgError, match=re.escape(gone)):
        _lib.load()


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(_lib.PgError):
        _lib.Context(0)
    rng = np.random.default_rng(0)
    with pytest.raises(_lib.PgError):
        lmm.pygemma(rng.standard_normal((20, 1)), rng.standard_normal((20, 4)), np.ones((20, 1)), np.ones(20), eigen=False)


def test_product_does_not_import_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pygemma_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(import oracle|from oracle)", src, flags=re.M), f
                code = re.sub(r"//.*|#.*", "", src)   # comments may cite the oracle; code may not load it
                assert "liboracle" not in code and "oracle/" not in code, f


def test_sampleiter_matches_reference_split():
    """lmm/lmm.py:427-434: cols_per_proc = ceil(p/nproc), blocks [r*cols, min((r+1)*cols, p))."""
    from pygemma_amd.lmm import SampleIter
    for p, nproc in [(10, 3), (12226, 8), (100000, 8), (7, 7), (5, 1), (9, 4)]:
        blocks = list(SampleIter(p, nproc))
        cols = int(np.ceil(p / nproc))
        exp = [(r * cols, min((r + 1) * cols, p)) for r in range(nproc) if r * cols < p]
        assert blocks == exp
        assert blocks[0][0] == 0 and blocks[-1][1] == p
        assert all(b0[1] == b1[0] for b0, b1 in zip(blocks, blocks[1:]))


def test_de_mode_raises_like_a_broken_reference_path():
    from pygemma_amd import lmm
    with pytest.raises(NotImplementedError):
        lmm.pygemma(np.zeros((4, 1)), np.zeros((4, 2)), np.ones((4, 1)), np.eye(4), de=True)


def test_drop_in_import_path():
    from pygemma import lmm
    import inspect
    sig = inspect.signature(lmm.pygemma)
    ref = ["Y", "X", "W", "K", "Z", "snps", "verbose", "disable_checks", "de", "grid", "eigen", "nproc"]      # lmm/lmm.py:87
    names = list(sig.parameters)
    assert names[:len(ref)] == ref              # positional order and names of the reference, so every reference call site works
    # extensions come after the reference's parameters, keyword-style, default off: restartable runs, the LRT
    # columns (N2), host-supplied eigenpairs (BASELINE config 5), streaming counters
    assert names[len(ref):] == ["checkpoint", "lrt", "eigenpairs", "stats"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect._empty}
    assert d == {"Z": None, "snps": None, "verbose": 0, "disable_checks": True, "de": False, "grid": False, "eigen": True, "nproc": 1,
                 "checkpoint": None, "lrt": False, "eigenpairs": None, "stats": None}
    for name in ("precompute_mat", "calc_lambda_restricted", "calc_beta_vg_ve_restricted_overload", "newton",
                 "likelihood_restricted_lambda_overload", "likelihood_derivative1_restricted_lambda_overload",
                 "likelihood_derivative2_restricted_lambda_overload"):                                   # tests/test_pygemma.py:256-294
        assert callable(getattr(lmm, name))


def test_packed_bed_roundtrip(tmp_path):
    """bed.py: write_bed -> PackedBed.open -> to_float reproduces the dosages (both allele conventions, NaN for missing)."""
    import numpy as np
    from pygemma_amd.bed import PackedBed, write_bed
    rng = np.random.default_rng(5)
    n, p = 37, 19
    G = rng.integers(0, 3, size=(n, p)).astype(np.float64)
    G[rng.random((n, p)) < 0.1] = np.nan
    prefix = str(tmp_path / "t")
    packed = write_bed(prefix, G)
    assert packed.shape == (p, (n + 3) // 4)
    b = PackedBed.open(prefix)
    assert b.shape == (n, p) and b.snps[3] == "rs3"
    np.testing.assert_array_equal(b.to_float(impute=False), G.astype(np.float32))
    b1 = PackedBed.open(prefix + ".bed", count_A1=True)
    np.testing.assert_array_equal(b1.to_float(impute=False), (2 - G).astype(np.float32))
    with open(prefix + ".bed", "r+b") as f:
        f.write(b"\x00")
    import pytest
    with pytest.raises(ValueError):
        PackedBed.open(prefix)
