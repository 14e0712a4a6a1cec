"""ctypes loader of the test-only device probe (halogen-pathtracer_amd/csrc/hg_devprobe.hip, `make devprobe`): one
elementwise kernel over the device building blocks of hg_device.h / hg_fmath.h / hg_pack.h.  A helper module of
tests/test_gpu_device_units.py; the function codes and element layouts are documented in hg_devprobe.hip."""
import ctypes as C
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
LIB_PATH = ROOT / "halogen-pathtracer_amd" / "halogen" / "devprobe" / "libhg_devprobe.so"

FMIN, FMAX, RCP, PCG, GET1, GET2, AABB, TRI, TRI_FLAT, SPHERES, PACK_R11G11B10, PACK_RGBA16F = 12, 13, 20, 21, 22, 23, 30, 31, 32, 33, 40, 41
# fn: (input words, output words) per element
WORDS = {**{fn: (1, 1) for fn in range(12)}, FMIN: (2, 1), FMAX: (2, 1), RCP: (1, 1), PCG: (1, 1), GET1: (4, 1), GET2: (4, 2), AABB: (12, 1),
         TRI: (16, 5), TRI_FLAT: (16, 5), SPHERES: (20, 2), PACK_R11G11B10: (3, 1), PACK_RGBA16F: (4, 2)}

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} not built (make -C halogen-pathtracer_amd devprobe)"
        L = C.CDLL(str(LIB_PATH))
        L.hg_devprobe.restype = C.c_int
        L.hg_devprobe.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int64]
        _lib = L
    return _lib


def run(fn: int, x: np.ndarray) -> np.ndarray:
    """Evaluate device function `fn` on the elements of x ((n,) or (n, words_in), float32 or uint32); returns the
    output words as uint32, (n,) or (n, words_out)."""
    wi, wo = WORDS[fn]
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.uint32) and x.size % wi == 0, (x.dtype, x.shape, wi)
    n = x.size // wi
    out = np.full(n * wo, 0xDEADBEEF, np.uint32)
    rc = lib().hg_devprobe(fn, x.ctypes.data, x.nbytes, out.ctypes.data, out.nbytes, n)
    assert rc == 0, f"hg_devprobe(fn={fn}, n={n}) returned HIP status {rc}"
    return out if wo == 1 else out.reshape(n, wo)
