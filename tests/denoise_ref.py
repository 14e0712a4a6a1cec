"""The display denoiser (csrc/hg_atrous.h, include/halogen_abi.h) restated in numpy float32, for test_denoise.py and
test_gpu_denoise.py.  One IEEE operation per numpy operation, in the header's order; hg_expf comes from the oracle
(hgo_fmath(5, ...), the function tests/test_fmath.py holds to the device's)."""
import ctypes as C

import numpy as np

import hg_oracle
from halogen import abi

F = np.float32
K = (F(0.375), F(0.25), F(0.0625))


def expf(x):
    L = hg_oracle.lib()
    L.hgo_fmath.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]
    x = np.ascontiguousarray(x, F)
    y = np.empty_like(x)
    L.hgo_fmath(5, x.ctypes.data, y.ctypes.data, x.size)
    return y


def params(iterations=3, sigma_color=0.0, sigma_normal=0.0, sigma_depth=0.0, demodulate=0, flags=0):
    return abi.DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth),
                             int(demodulate), int(flags))


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def restate(rgba, guide0, guide1, p):
    """hg_denoise_host's contract over (h, w, 4) float32 arrays."""
    rgba, guide0, guide1 = (np.ascontiguousarray(a, F) for a in (rgba, guide0, guide1))
    H, W, _ = rgba.shape
    c = rgba[..., :3].copy()
    n, t = guide0[..., :3], guide0[..., 3]
    miss = t == F(np.inf)
    a = np.maximum(guide1[..., :3], F(1e-3))
    if p.demodulate:
        c = c / a
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(p.iterations):
            s = 1 << i
            sc = F(p.sigma_color) * F(2.0 ** -i)
            r_c = F(1.0) / (sc * sc) if p.sigma_color > 0 else None
            r_n = F(1.0) / (F(p.sigma_normal) * F(p.sigma_normal)) if p.sigma_normal > 0 else None
            r_z = F(1.0) / (F(p.sigma_depth) * F(p.sigma_depth)) if p.sigma_depth > 0 else None
            acc = np.zeros((H, W, 3), F)
            wsum = np.zeros((H, W), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    y0, y1 = max(0, -s * dy), min(H, H - s * dy)
                    x0, x1 = max(0, -s * dx), min(W, W - s * dx)
                    if y0 >= y1 or x0 >= x1:
                        continue  # every such tap lies outside the image
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                    h = K[abs(dy)] * K[abs(dx)]
                    e = np.zeros((y1 - y0, x1 - x0), F)
                    if r_c is not None:
                        e = e + _sq3(c[P] - c[Q]) * r_c
                    if r_n is not None:
                        e = e + _sq3(n[P] - n[Q]) * r_n
                    if r_z is not None:
                        dz = t[P] - t[Q]
                        e = np.where(t[P] != t[Q], e + (dz * dz) * r_z, e)
                    e = np.where(miss[P] != miss[Q], F(np.inf), e).astype(F)
                    w = h * expf(-e)
                    acc[P] = acc[P] + w[..., None] * c[Q]
                    wsum[P] = wsum[P] + w
            c = acc / wsum[..., None]
    out = np.empty_like(rgba)
    out[..., :3] = c * a if p.demodulate else c
    out[..., 3] = rgba[..., 3]
    return out


def random_case(W, H, seed, c_max=1e3):
    """Colours up to c_max, normals from a few directions, t from a few depths with some misses, albedos with zeros."""
    rng = np.random.default_rng(seed)
    dirs = np.array([[0, 1, 0], [1, 0, 0], [0.6, 0, 0.8], [0, 0.6, -0.8]], F)
    depths = np.array([1.0, 1.25, 3.0], F)
    miss = rng.random((H, W)) < 0.15
    g0 = np.zeros((H, W, 4), F)
    g0[..., :3] = dirs[rng.integers(0, len(dirs), (H, W))]
    g0[..., 3] = depths[rng.integers(0, len(depths), (H, W))]
    g0[miss] = (0, 0, 0, np.inf)
    g1 = np.zeros((H, W, 4), F)
    g1[..., :3] = rng.random((H, W, 3)) * (rng.random((H, W, 1)) > 0.1)
    g1[..., 3] = 1
    g1[miss] = (1, 1, 1, 0)
    rgba = np.ones((H, W, 4), F)
    rgba[..., :3] = rng.random((H, W, 3)) * np.where(rng.random((H, W, 1)) < 0.05, c_max, 2.0)
    rgba[..., 3] = rng.random((H, W))
    return rgba, g0, g1


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
