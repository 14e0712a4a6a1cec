"""Triangle sets shared by tests/test_lbvh.py and tests/test_gpu_rebuild.py: ctypes arrays of HalogenTriangle."""
import functools

import numpy as np

from halogen import abi, scene as hs, scenes
from halogen.unity import Transform, unity_cube, unity_plane

f32 = np.float32


def from_corners(corners):
    """(n, 3, 3) corner coordinates -> HalogenTriangle array (normals: +y)."""
    c = np.asarray(corners, f32).reshape(-1, 9)
    t18 = np.concatenate([c, np.tile(f32([0, 1, 0, 0, 1, 0, 0, 1, 0]), (len(c), 1))], axis=1).astype(f32)
    return from_rows(t18)


def from_rows(t18):
    t18 = np.ascontiguousarray(t18, f32)
    return (abi.HalogenTriangle * len(t18)).from_buffer_copy(t18.tobytes())


@functools.lru_cache(maxsize=None)
def mesh_triangles(kind):
    """Unity's Plane (200 triangles) and Cube (12), the 8.7k dragon: the mesh's packed triangles."""
    v, n, t = {"plane": unity_plane, "cube": unity_cube, "dragon": lambda: scenes.dragon_mesh(1)}[kind]()
    return hs.RayTracingMesh(kind, v, n, t, Transform((0, 0, 0))).packed_triangles


def random_triangles(n, seed=0):
    """Small triangles in the unit cube, plus (from 3 triangles on) two point triangles at its corners (0, 0, 0) and
    (1, 1, 1): key points 0 and 2 on every axis, so the extent is 2, the scale exactly 512 and the point at pmax lands,
    unclamped, exactly on 1024."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.1, 0.9, (n, 1, 3)) + rng.uniform(-0.05, 0.05, (n, 3, 3))
    if n >= 3:
        c[0], c[n - 1] = 0.0, 1.0
    return from_corners(c)


def identical_triangles(n):
    return from_corners(np.tile(f32([[0.25, 0.5, 1.0], [1.25, 0.5, 1.0], [0.25, 1.5, 2.0]]), (n, 1, 1)))


def flat_triangles(n, flat_axes, seed=3):
    c = np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 3, 3))
    for axis in flat_axes:
        c[:, :, axis] = 0.25
    return from_corners(c)


def extreme_triangles(what, n=60, seed=4):
    rng = np.random.default_rng(seed)
    if what == "tiny":
        return from_corners(rng.uniform(0.0, 1e-30, (n, 3, 3)))
    if what == "huge":
        return from_corners(rng.uniform(-1e30, 1e30, (n, 3, 3)))
    if what == "denormal":  # every coordinate denormal; one point triangle at 0, so a key point sits at pmin exactly
        c = rng.uniform(0.0, 1e-40, (n, 3, 3))
        c[5] = 0.0
        return from_corners(c)
    assert what == "overflow"  # lo + hi overflows for half the triangles, on every axis
    c = rng.uniform(-1.0, 1.0, (n, 3, 3))
    c[::2] = rng.uniform(3.0e38, 3.3e38, (n // 2, 3, 3))
    return from_corners(c)


def ulp_triangles(seed=6):
    """Ten triangles; 3 and 4 are point triangles one ulp apart in x (key points 1.0 and the next float)."""
    c = np.random.default_rng(seed).uniform(-1.0, 3.0, (10, 3, 3)).astype(f32)
    c[3] = f32([0.5, 0.75, 0.25])
    c[4] = f32([np.nextafter(f32(0.5), f32(1.0)), 0.75, 0.25])
    return from_corners(c)
