"""Scenes and deformations shared by tests/test_refit.py and tests/test_gpu_refit.py."""
import ctypes as C

import numpy as np

from halogen import abi, scene as hs
from halogen.unity import Transform, euler_to_quat, unity_plane

f32 = np.float32


def _soup(tris):
    """(n, 3, 3) triangle corners -> vertices, normals, indices of an unshared-vertex mesh."""
    t = np.asarray(tris, f32)
    v = t.reshape(-1, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-20)
    return v, np.repeat(n, 3, axis=0).astype(f32), np.arange(len(v), dtype=np.int32).reshape(-1, 3)


def hazard_scene() -> hs.Scene:
    """Four meshes that together hold every hazard of a refit:
      0  3 triangles: the root is a leaf (no records, not cullable)
      1  40 triangles around one centroid (one leaf of 40: the leaf table, a long leaf loop) beside 60 spread ones
         (unequal child heights)
      2  Unity's flat 10 x 10 plane (every box padded)
      3  a bumpy 25 x 10 grid of 500 triangles, which hazard_packed instances twice at a non-zero triangle offset"""
    rng = np.random.default_rng(5)
    sc = hs.Scene()
    few = rng.uniform(-1, 1, (3, 3, 3))
    sc.add(hs.RayTracingMesh("few", *_soup(few), Transform((-3.0, 0.0, 6.0))))
    a = rng.uniform(0, 2 * np.pi, 40)
    r = rng.uniform(0.2, 1.0, 40)
    ring = []
    for ai, ri in zip(a, r):  # three points 120 degrees apart about the origin: every centroid is (0, 0, 0) +- rounding
        ring.append([[ri * np.cos(ai + k * 2 * np.pi / 3), ri * np.sin(ai + k * 2 * np.pi / 3), 0.0] for k in range(3)])
    ring = np.array(ring)
    ring[:, :, 2] = np.repeat(rng.uniform(-0.3, 0.3, (40, 1)), 3, axis=1) * [[1, -0.5, -0.5]]  # tilt, centroid z kept
    spread = rng.uniform(-0.2, 0.2, (60, 3, 3)) + rng.uniform([1.5, -3, -1], [8, 3, 1], (60, 1, 3))
    sc.add(hs.RayTracingMesh("cluster", *_soup(np.concatenate([ring, spread])), Transform((0.0, 0.0, 9.0))))
    sc.add(hs.RayTracingMesh("plane", *unity_plane(), Transform((0.0, -2.0, 8.0), (0, 0, 0, 1), (0.5, 1, 0.5))))
    gx, gz = np.meshgrid(np.arange(26, dtype=f32) * 0.2, np.arange(11, dtype=f32) * 0.2, indexing="ij")
    gv = np.stack([gx, rng.uniform(0, 0.4, gx.shape), gz], axis=-1).reshape(-1, 3).astype(f32)
    gi = []
    for i in range(25):
        for j in range(10):
            p = i * 11 + j
            gi += [(p, p + 1, p + 11), (p + 1, p + 12, p + 11)]
    gn = np.tile(f32([0, 1, 0]), (len(gv), 1))
    sc.add(hs.RayTracingMesh("grid", gv, gn, np.array(gi, np.int32), Transform((-2.5, -1.0, 7.0))))
    return sc


def hazard_packed(sc: hs.Scene) -> hs.PackedScene:
    """sc.pack() plus a fifth mesh record: a second instance of mesh 3's tree (both buffer offsets shared) under
    another matrix."""
    p = sc.pack()
    meshes = (abi.HalogenMeshData * (len(p.meshes) + 1))()
    C.memmove(meshes, p.meshes, C.sizeof(p.meshes))
    twin = hs.RayTracingMesh.__new__(hs.RayTracingMesh)
    twin.__dict__.update(sc.meshes[3].__dict__)
    twin.transform = Transform((1.5, 0.5, 10.0), euler_to_quat(0, 40, 10), (0.8, 1.2, 0.8))
    meshes[len(p.meshes)] = twin.mesh_data(p.meshes[3].materialIndex, p.meshes[3].triangleBufferOffset,
                                          p.meshes[3].accelerationBufferOffset)
    p.meshes = meshes
    return p


def twist(v, strength=0.6, axis=1):
    """The vertices rotated about `axis` by an angle growing along it."""
    v = np.asarray(v, f32)
    a, b = [k for k in range(3) if k != axis]
    ang = (v[:, axis] * f32(strength)).astype(f32)
    out = v.copy()
    out[:, a] = v[:, a] * np.cos(ang) - v[:, b] * np.sin(ang)
    out[:, b] = v[:, a] * np.sin(ang) + v[:, b] * np.cos(ang)
    return out.astype(f32)


def noise(v, scale, seed=1):
    v = np.asarray(v, f32)
    return (v + np.random.default_rng(seed).normal(0, scale, v.shape)).astype(f32)
