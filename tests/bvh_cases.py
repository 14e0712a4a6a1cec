"""Meshes shared by the BLAS builder tests (test_bvh.py, test_bvh_sah.py), and the digests that pin hg_build_blas_sah's
exact tree (tests/golden/blas_sah_digests.json)."""
import ctypes as C
import hashlib

import numpy as np

from halogen import abi
from halogen.scenes import dragon_mesh
from halogen.unity import unity_cube, unity_plane


def grid_ties():
    """A lattice of coincident centroids and +-0 coordinates, with degenerate triangles: ties on the split plane and in
    the folds.  Returns (vertices, triangles)."""
    g = np.stack(np.meshgrid(np.arange(-20, 21), np.arange(-20, 21), np.arange(-20, 21)), -1).reshape(-1, 3)
    v = (g * 0.5).astype(np.float32)
    v[v == 0] = -0.0
    rng = np.random.default_rng(5)
    t = rng.integers(0, len(v), size=(60000, 3)).astype(np.int32)
    t[::7] = t[::7, :1]  # degenerate triangles: all three vertices equal
    return v, t


def shuffled(t, seed):
    return np.random.default_rng(seed).permutation(np.asarray(t)).astype(np.int32)


def build_sah(verts, tris, max_leaf=2, max_depth=48):
    """hg_build_blas_sah: (its return value, the node array, the reordered index list)."""
    verts = np.ascontiguousarray(verts, np.float32)
    idx = np.ascontiguousarray(tris, np.int32).copy()
    cap = 2 * len(idx) + 2
    nodes = (abi.BVHEntry * cap)()
    n = abi.lib().hg_build_blas_sah(verts.ctypes.data, len(verts), idx.ctypes.data, len(idx), max_leaf, max_depth,
                                    C.cast(nodes, C.c_void_p), cap)
    return n, nodes, idx


def sah_pin_meshes():
    """name -> (vertices, triangles) of the meshes whose SAH trees are pinned."""
    out = {}
    for name, (v, _, t) in (("plane", unity_plane()), ("cube", unity_cube()), ("dragon_x1", dragon_mesh(1))):
        out[name] = (v, t)
    v, _, t = dragon_mesh(3)
    out["dragon_x3_shuffled"] = (v, shuffled(t, 3))
    out["grid_ties"] = grid_ties()
    return out


def sah_digests():
    """"mesh/leafN" -> SHA-256 of the bytes of the n entries hg_build_blas_sah returned, then of the index list, for
    max_leaf 2 and 4 at max_depth 48 on every pinned mesh."""
    out = {}
    for name, (v, t) in sah_pin_meshes().items():
        for max_leaf in (2, 4):
            n, nodes, idx = build_sah(v, t, max_leaf, 48)
            assert n > 0, (name, max_leaf, n)
            out[f"{name}/leaf{max_leaf}"] = hashlib.sha256(bytes(nodes)[: n * 32] + idx.tobytes()).hexdigest()
    return out
