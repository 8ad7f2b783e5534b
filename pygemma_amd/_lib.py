"""ctypes binding of libpygemma_hip.so (C ABI: include/pygemma_hip.h).

The MI355X path has NO CPU fallback: if the shared library is missing or no GPU is visible the
calls raise.  The checker (the CPU oracle) is test infrastructure and is never imported from here.
"""
import contextlib
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYGEMMA_HIP_LIB") or os.path.join(_HERE, "lib", "libpygemma_hip.so")   # env: A/B builds
_lib = None

HEADER = os.path.join(os.path.dirname(_HERE), "include", "pygemma_hip.h")
VC_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libpygemma_vc.so")     # the variance-component unit: a library of its own
VC_HEADER = os.path.join(os.path.dirname(_HERE), "include", "pygemma_vc.h")
VC_SYMBOLS = []  # the functions VC_HEADER declares, in its order: filled by load_vc()
_vc = None
CC_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libpygemma_cc.so")     # the case/control unit: a library of its own
CC_HEADER = os.path.join(os.path.dirname(_HERE), "include", "pygemma_cc.h")
CC_SYMBOLS = []  # the functions CC_HEADER declares, in its order: filled by load_cc()
_cc = None
PERM_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libpygemma_perm.so")     # the permutation unit: a library of its own
PERM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "pygemma_perm.h")
PERM_SYMBOLS = []  # the functions PERM_HEADER declares, in its order: filled by load_perm()
_perm = None
SYMBOLS = []     # the functions HEADER declares, in its order: filled by load()
_CTYPES = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}


class PgError(RuntimeError):
    pass


def _ctype(decl, fn, ret=False):
    """ctypes type of one parameter ('const float *Xr', 'int64_t n') or return type ('const char *', 'void') of function fn.
    Every pointer is a c_void_p: it takes byref(), ctypes arrays, ndarray.ctypes pointers, ints, c_void_p and None."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return C.c_char_p if ret and words == ["char", "*"] else C.c_void_p
    if not ret and len(words) > 1:
        words = words[:-1]                   # the parameter's name
    ctype = " ".join(words)
    if ret and ctype == "void":
        return None
    if ctype not in _CTYPES:                 # never ctypes' default int: it would truncate whatever this is
        raise PgError(f"{fn}: C type '{ctype}' of '{decl.strip()}' has no ctypes mapping (pygemma_amd/_lib.py)")
    return _CTYPES[ctype]


def parse_header(text):
    """[(name, restype, argtypes)] of the pg_* / pgx_* functions a C header declares, in its order.  The header is plain C
    (include/pygemma_hip.h): comments and preprocessor lines go, typedefs and the enum hold no call, 'ret name(params);' is left."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{', "", text, flags=re.M)
    out = []
    for stmt in text.split(";"):
        m = re.fullmatch(r"(.*?)\b(pgx?_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if m:
            ret, fn, params = m.groups()
            args = [] if params.strip() == "void" else [_ctype(a, fn) for a in params.split(",")]
            out.append((fn, _ctype(ret, fn, ret=True), args))
    return out


def load():
    """Load the HIP library (build it first with __graft_entry__.build() / make -C pygemma_amd/csrc) and give every function
    the signature include/pygemma_hip.h declares: the header is the one place an entry point is registered."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PgError(f"{LIB_PATH} not found: build the HIP extension (python -c 'import __graft_entry__ as g; g.build()'). "
                      "pygemma_amd has no CPU fallback.")
    if not os.path.exists(HEADER):
        raise PgError(f"{HEADER} not found: the signatures of {LIB_PATH} are read from it")
    L = C.CDLL(LIB_PATH)
    with open(HEADER) as hdr:
        decls = parse_header(hdr.read())
    for fn, restype, argtypes in decls:
        f = getattr(L, fn)
        f.restype, f.argtypes = restype, argtypes
    SYMBOLS[:] = [fn for fn, _, _ in decls]
    _lib = L
    return L


def load_vc():
    """Load libpygemma_vc.so (csrc/vc.hip: lmm.reml's kernels) beside the main library, which it needs, and bind it from
    include/pygemma_vc.h.  Called by lmm.reml and lmm.vc_kinship, not at import: a process that fits no variance components
    never maps it."""
    global _vc
    if _vc is not None:
        return _vc
    load()
    for path in (VC_LIB_PATH, VC_HEADER):
        if not os.path.exists(path):
            raise PgError(f"{path} not found: build the HIP extension (python -c 'import __graft_entry__ as g; g.build()')")
    V = C.CDLL(VC_LIB_PATH)
    with open(VC_HEADER) as hdr:
        decls = parse_header(hdr.read())
    for fn, restype, argtypes in decls:
        f = getattr(V, fn)
        f.restype, f.argtypes = restype, argtypes
    VC_SYMBOLS[:] = [fn for fn, _, _ in decls]
    _vc = V
    return V


def load_cc():
    """Load libpygemma_cc.so (csrc/case_control.hip: lmm.case_control's kernels) beside the main library, which it needs, and bind
    it from include/pygemma_cc.h.  Called by lmm.case_control, not at import, as load_vc is."""
    global _cc
    if _cc is not None:
        return _cc
    load()
    for path in (CC_LIB_PATH, CC_HEADER):
        if not os.path.exists(path):
            raise PgError(f"{path} not found: build the HIP extension (python -c 'import __graft_entry__ as g; g.build()')")
    K = C.CDLL(CC_LIB_PATH)
    with open(CC_HEADER) as hdr:
        decls = parse_header(hdr.read())
    for fn, restype, argtypes in decls:
        f = getattr(K, fn)
        f.restype, f.argtypes = restype, argtypes
    CC_SYMBOLS[:] = [fn for fn, _, _ in decls]
    _cc = K
    return K


def load_perm():
    """Load libpygemma_perm.so (csrc/perm.hip: lmm.case_control_perm's kernels) beside the main library, which it needs, and bind
    it from include/pygemma_perm.h.  Called by lmm.case_control_perm, not at import, as load_vc is."""
    global _perm
    if _perm is not None:
        return _perm
    load()
    for path in (PERM_LIB_PATH, PERM_HEADER):
        if not os.path.exists(path):
            raise PgError(f"{path} not found: build the HIP extension (python -c 'import __graft_entry__ as g; g.build()')")
    P = C.CDLL(PERM_LIB_PATH)
    with open(PERM_HEADER) as hdr:
        decls = parse_header(hdr.read())
    for fn, restype, argtypes in decls:
        f = getattr(P, fn)
        f.restype, f.argtypes = restype, argtypes
    PERM_SYMBOLS[:] = [fn for fn, _, _ in decls]
    _perm = P
    return P


def check(rc, what=""):
    if rc != 0:
        raise PgError(f"{what} failed (code {rc}): {load().pg_last_error().decode()}")


class DeviceBuffer:
    """hipMalloc'd buffer owned by a Context (freed with it or by .free())."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        check(load().pg_malloc(ctx.handle, self.nbytes, C.byref(p)), "pg_malloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            load().pg_free(self.ctx.handle, self.ptr)
            self.ptr = None
        if self in self.ctx._bufs:
            self.ctx._bufs.remove(self)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(load().pg_memcpy_h2d(self.ctx.handle, self.ptr, arr.ctypes.data, arr.nbytes), "pg_memcpy_h2d")
        return self

    def download(self, shape, dtype, offset=0):
        out = np.empty(shape, dtype)
        check(load().pg_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr + offset, out.nbytes), "pg_memcpy_d2h")
        return out


class Context:
    """One per (process, GPU): wraps pg_ctx (device id + stream + scratch)."""

    def __init__(self, device=0, stream=None):
        L = load()
        h = C.c_void_p()
        if stream is None:
            check(L.pg_ctx_create(int(device), C.byref(h)), "pg_ctx_create")
        else:
            check(L.pg_ctx_create_on_stream(int(device), C.c_void_p(stream), C.byref(h)), "pg_ctx_create_on_stream")
        self.handle = h
        self.device = device
        self._bufs = []

    def alloc(self, nbytes):
        b = DeviceBuffer(self, nbytes)
        self._bufs.append(b)
        return b

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.alloc(max(arr.nbytes, 4)).upload(arr)

    def sync(self):
        check(load().pg_ctx_sync(self.handle), "pg_ctx_sync")

    def mem_info(self):
        """(free, total) bytes of this context's device."""
        f, t = C.c_size_t(), C.c_size_t()
        check(load().pg_mem_info(self.handle, C.byref(f), C.byref(t)), "pg_mem_info")
        return int(f.value), int(t.value)

    def close(self):
        if self.handle:
            for b in list(self._bufs):
                b.free()
            load().pg_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextlib.contextmanager
def scope(ctx=None, device=0):
    """The context and device buffers of one wrapper call: yields ctx, or a Context(device) of its own that is closed on exit.
    On exit from a borrowed ctx every DeviceBuffer allocated on it since entry is freed (hipFree waits for the device, so after
    the wrapper's downloads) and leaves ctx._bufs, whether the body returned or raised; what the caller had allocated stays.
    Scopes on one context nest (model._ml_scalars around precompute_mat).  A Context is used by one thread at a time — lmm.py
    gives every worker thread its own — so every buffer that appears between entry and exit is this scope's."""
    if ctx is None:
        with Context(device) as own:
            yield own
        return
    before = set(ctx._bufs)
    try:
        yield ctx
    finally:
        for b in [b for b in ctx._bufs if b not in before]:
            b.free()


def device_count():
    return load().pg_device_count()


# ---- pinned host memory (S1: streaming SNP batches / eigenvectors from the host) ---------------------------------------
_pinned = {}     # base address -> nbytes of every live pinned range this process made (pinned_empty / pin)


class _PinnedBlock:
    """Owner of one hipHostMalloc'd range; freed when the last NumPy view of it goes away."""

    def __init__(self, nbytes, device=0):
        import weakref
        self.ctx = Context(device)
        p = C.c_void_p()
        check(load().pg_host_alloc(self.ctx.handle, max(int(nbytes), 1), C.byref(p)), "pg_host_alloc")
        self.ptr, self.nbytes = p.value, int(nbytes)
        _pinned[self.ptr] = self.nbytes
        self._fin = weakref.finalize(self, _PinnedBlock._release, self.ctx, self.ptr)

    @staticmethod
    def _release(ctx, ptr):
        _pinned.pop(ptr, None)
        try:
            load().pg_host_free(ctx.handle, ptr)
            ctx.close()
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float32, device=0):
    """np.empty in page-locked host memory (hipHostMalloc, portable): the array to np.fromfile()/copy a genotype or
    eigenvector matrix into so that lmm.pygemma streams it by DMA without a staging copy."""
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    blk = _PinnedBlock(nbytes, device)
    buf = (C.c_char * max(nbytes, 1)).from_address(blk.ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=nbytes // dtype.itemsize).reshape(shape)
    arr.flags.writeable = True
    # arr.base -> memoryview -> buf: tie the block's life to the buffer object the array is based on
    buf._pg_block = blk
    return arr


def pin(arr, device=0):
    """Page-lock an existing contiguous (C- or Fortran-ordered) NumPy array in place (hipHostRegister).  Returns a handle whose
    .close() unpins; pinning costs ~5 ms/GB (tools/bench_h2d.py)."""
    assert arr.flags.c_contiguous or arr.flags.f_contiguous
    ctx = Context(device)
    check(load().pg_host_register(ctx.handle, arr.ctypes.data, arr.nbytes), "pg_host_register")
    _pinned[arr.ctypes.data] = arr.nbytes

    class _Pin:
        def close(self_inner):
            if _pinned.pop(arr.ctypes.data, None) is not None:
                load().pg_host_unregister(ctx.handle, arr.ctypes.data)
                ctx.close()
    return _Pin()


def is_pinned(arr):
    """True when the array's bytes lie inside a range pinned through this module."""
    try:
        from numpy.lib.array_utils import byte_bounds
    except ImportError:          # NumPy 1.x
        byte_bounds = np.byte_bounds
    lo, hi = byte_bounds(arr)
    for base, nb in list(_pinned.items()):
        if base <= lo and hi <= base + nb:
            return True
    return False
