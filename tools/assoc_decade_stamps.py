"""Share of a SNP's wave that assoc_kernel spends in the decade sweeps (the 11 sweeps at the shared lambdas and their scalars, or
decade_lanes in their place): s_memtime at wave entry, before and after the decade sweeps and at wave exit, 1024 SNPs spread over the launch.
Needs the stamped build: tools/build_variant.sh astamps assoc -DPG_ASSOC_STAMPS [-DPG_ASSOC_DECADE_HOIST=0],
PYGEMMA_HIP_LIB=pygemma_amd/lib_dev/astamps/libpygemma_hip.so
usage: assoc_decade_stamps.py [n] [p] [c]"""
import os, sys, ctypes as C
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pygemma_amd import _lib, ops, synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
p = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
c = int(sys.argv[3]) if len(sys.argv) > 3 else 5
L = _lib.load(); ctx = _lib.Context(0)
z = synth.fast_rotated_panel(n, p, c, seed=0)
for _ in range(2):
    ops.assoc(z["d"], z["W"], z["Y"], z["X"], ctx=ctx, want_p=False)
buf = (C.c_longlong * 4096)()
L.pgx_assoc_stamps.argtypes = [C.c_void_p]; L.pgx_assoc_stamps.restype = C.c_int
assert L.pgx_assoc_stamps(buf) == 0
st = np.array(buf, dtype=np.int64).reshape(1024, 4)
st = st[(st[:, 3] > st[:, 0])]
whole, scan, dec = st[:, 3] - st[:, 0], st[:, 1] - st[:, 0], st[:, 2] - st[:, 1]
print("n %d p %d c %d: %d stamped waves; s_memtime ticks per SNP" % (n, p, c, len(st)))
print("  whole wave       median %9.0f mean %9.0f" % (np.median(whole), whole.mean()))
print("  decade scan      median %9.0f mean %9.0f (%.2f %% of the waves' time)" % (np.median(scan), scan.mean(), 100 * scan.sum() / whole.sum()))
print("  decade sweeps    median %9.0f mean %9.0f (%.2f %% of the waves' time; median of the per-wave shares %.2f %%)" % (
    np.median(dec), dec.mean(), 100 * dec.sum() / whole.sum(), 100 * np.median(dec / whole)))
