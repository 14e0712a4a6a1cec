"""ctypes loader of the test-only device probe (halogen-pathtracer_amd/csrc/hg_devprobe.hip, `make devprobe`): one
elementwise kernel over the device building blocks of hg_device.h (the hg_dev_*.h headers) / hg_fmath.h / hg_pack.h.  A helper module of
tests/test_gpu_device_units.py and tests/test_gpu_shading_units.py; the function codes and element layouts are documented
in hg_devprobe.hip."""
import ctypes as C
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
LIB_PATH = ROOT / "halogen-pathtracer_amd" / "halogen" / "devprobe" / "libhg_devprobe.so"

FMIN, FMAX, RCP, PCG, GET1, GET2, AABB, TRI, TRI_FLAT, SPHERES, PACK_R11G11B10, PACK_RGBA16F = 12, 13, 20, 21, 22, 23, 30, 31, 32, 33, 40, 41
# fn: (input words, output words) per element
WORDS = {**{fn: (1, 1) for fn in range(12)}, FMIN: (2, 1), FMAX: (2, 1), RCP: (1, 1), PCG: (1, 1), GET1: (4, 1), GET2: (4, 2), AABB: (12, 1),
         TRI: (16, 5), TRI_FLAT: (16, 5), SPHERES: (20, 2), PACK_R11G11B10: (3, 1), PACK_RGBA16F: (4, 2)}
# the shading half; SKY needs a cubemap, MEDIUM_OPS and EVALUATE_HIT a material table (run_tables)
SKY, SKY_LEVEL, LAMBERT, REFLECT, SCHLICK, REFRACT, MEDIUM_OPS, EVALUATE_HIT, INV_BH = 50, 51, 52, 53, 54, 55, 56, 57, 58
# SKY: direction, level -> rgb; SKY_LEVEL: default_mip, acc_rough -> level; LAMBERT: n, rv -> direction; REFLECT: i, n ->
# direction; SCHLICK: n1, n2, normal, incident, min, max -> value; REFRACT: incident, normal, n1, n2 -> direction, tir;
# MEDIUM_OPS: sp, stack bytes lo, hi, 16 ops (kind << 30 | value; 1 push material, 2 pop id, 0 nothing) -> 16 x (sp, 8 ids);
# EVALUATE_HIT: frame, pixel, offset, sp, stack bytes lo, hi, ray o, d, hit t, orient, pos, n, mat -> att, ray.o, ray.d,
# bt_out, sp, 8 ids; INV_BH: x -> y
WORDS.update({SKY: (4, 3), SKY_LEVEL: (2, 1), LAMBERT: (6, 3), REFLECT: (6, 3), SCHLICK: (10, 1), REFRACT: (8, 4),
              MEDIUM_OPS: (19, 144), EVALUATE_HIT: (21, 19), INV_BH: (1, 1)})
OP_PUSH, OP_POP = 1 << 30, 2 << 30

_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        assert LIB_PATH.exists(), f"{LIB_PATH} not built (make -C halogen-pathtracer_amd devprobe)"
        L = C.CDLL(str(LIB_PATH))
        L.hg_devprobe.restype = C.c_int
        L.hg_devprobe.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int64]
        L.hg_devprobe_tables.restype = C.c_int
        L.hg_devprobe_tables.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int64, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32]
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


def run_tables(fn: int, x: np.ndarray, materials=None, cubemap=None) -> np.ndarray:
    """run() for the functions that read tables in device memory: materials is a ctypes array of PackedHalogenMaterial
    (packed by the probe with the product's hg_pack_spheres_materials), cubemap a halogen.envmap.Cubemap."""
    wi, wo = WORDS[fn]
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.uint32) and x.size % wi == 0, (x.dtype, x.shape, wi)
    n = x.size // wi
    out = np.full(n * wo, 0xDEADBEEF, np.uint32)
    tex = np.ascontiguousarray(cubemap.texels, np.float32) if cubemap is not None else None
    rc = lib().hg_devprobe_tables(fn, x.ctypes.data, x.nbytes, out.ctypes.data, out.nbytes, n,
                                  C.addressof(materials) if materials is not None else None,
                                  len(materials) if materials is not None else 0,
                                  tex.ctypes.data if tex is not None else None, tex.size if tex is not None else 0,
                                  cubemap.face_size if cubemap is not None else 0,
                                  cubemap.n_mips if cubemap is not None else 0)
    assert rc == 0, f"hg_devprobe_tables(fn={fn}, n={n}) returned HIP status {rc}"
    return out if wo == 1 else out.reshape(n, wo)
