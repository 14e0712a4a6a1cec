"""Meshes and the numpy restatement of csrc/hg_normals.h, shared by tests/test_normals.py and
tests/test_gpu_normals.py."""
import numpy as np

import refit_cases
from halogen import scene as hs
from halogen.unity import Transform

f32 = np.float32
FAN = 4   # the fan's mesh index in fan_scene(); the grid stays 3
GRID2 = 5  # ... and the grid's second instance moves up to 5 (refit_cases.hazard_packed appends it)


def normals_numpy(positions, indices):
    """csrc/hg_normals.h restated: every operation one float32 numpy operation, in the header's association; a vertex's
    corners in ascending order of their triangles' index triples, one addition per corner"""
    p = np.asarray(positions, f32).reshape(-1, 3)
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    a, b, c = p[idx[:, 0]], p[idx[:, 1]], p[idx[:, 2]]
    e1, e2 = b - a, c - a
    assert e1.dtype == f32 and e2.dtype == f32
    f = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                  e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    assert f.dtype == f32
    face = np.repeat(np.arange(len(idx)), 3)  # the face of every corner, and the vertex it names
    vert = idx.reshape(-1)
    triple = idx[face]
    order = np.lexsort((triple[:, 2], triple[:, 1], triple[:, 0], vert))  # by vertex, then by triple
    face, vert = face[order], vert[order]
    start = np.searchsorted(vert, np.arange(len(p)))
    count = np.bincount(vert, minlength=len(p))
    s = np.zeros((len(p), 3), f32)
    for k in range(int(count.max()) if len(count) else 0):  # the k-th corner of every vertex that has one
        has = np.flatnonzero(count > k)
        s[has] = s[has] + f[face[start[has] + k]]
    d = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = f32(1.0) / np.sqrt(d)
        scaled = s * r[:, None]
    out = np.where((d > 0)[:, None], scaled, f32(0.0))
    assert out.dtype == f32
    return np.ascontiguousarray(out)


def fan(n=300, seed=8):
    """n triangles round vertex 0 (n + 1 vertices, the rim closed): one list of n corners, bumpy so no two faces are
    parallel"""
    rng = np.random.default_rng(seed)
    ang = np.arange(n) * (2 * np.pi / n)
    rim = np.stack([np.cos(ang), rng.uniform(-0.2, 0.2, n), np.sin(ang)], axis=1)
    v = np.concatenate([[[0.0, 0.5, 0.0]], rim]).astype(f32)
    idx = np.array([(0, 1 + (k + 1) % n, 1 + k) for k in range(n)], np.int32)  # wound so the normals point up
    return v, idx


def fan_scene():
    """refit_cases.hazard_scene() plus the fan as mesh 4"""
    sc = refit_cases.hazard_scene()
    v, idx = fan()
    sc.add(hs.RayTracingMesh("fan", v, normals_numpy(v, idx), idx, Transform((3.0, -0.5, 7.0))))
    return sc


def valences(indices, n_vertices):
    return np.bincount(np.asarray(indices).reshape(-1), minlength=n_vertices)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)
