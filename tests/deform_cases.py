"""Bones, influences and the numpy restatement of csrc/hg_skin.h, shared by tests/test_skin.py and
tests/test_gpu_deform.py."""
import numpy as np

f32 = np.float32


def rotation(axis, angle):
    """The 3 x 3 rotation by `angle` about `axis` (Rodrigues), float64"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def bone(R=None, t=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """12 floats, row-major 3 x 4: (R * diag(scale) | t)"""
    m = np.zeros((3, 4))
    m[:, :3] = (np.eye(3) if R is None else R) @ np.diag(scale)
    m[:, 3] = t
    return m.astype(f32).reshape(12)


def rigid_palette(n_bones, seed=0, swing=0.5, shift=0.3):
    """n_bones rigid bones: small rotations about random axes and small translations; bone 0 is the identity"""
    rng = np.random.default_rng(seed)
    out = [bone()]
    for _ in range(n_bones - 1):
        out.append(bone(rotation(rng.normal(size=3), rng.uniform(-swing, swing)), rng.uniform(-shift, shift, 3)))
    return np.stack(out).astype(f32)


def influences(n_vertices, n_bones, seed=0):
    """Four bone indices and four weights per vertex; the weights of a vertex sum to 1 up to rounding, some are zero, and
    the last bone is used"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_bones, (n_vertices, 4)).astype(np.uint16)
    idx[0] = n_bones - 1
    w = rng.uniform(0, 1, (n_vertices, 4))
    w[rng.uniform(size=w.shape) < 0.3] = 0.0
    w[:, 0] += 0.1
    w /= w.sum(axis=1, keepdims=True)
    return idx, w.astype(f32)


def skin_numpy(positions, normals, bone_indices, weights, bones):
    """csrc/hg_skin.h restated: every operation one float32 numpy operation, in the header's association"""
    p = np.asarray(positions, f32).reshape(-1, 3)
    n = np.asarray(normals, f32).reshape(-1, 3)
    w = np.asarray(weights, f32).reshape(-1, 4)
    B = np.asarray(bones, f32).reshape(-1, 12)[np.asarray(bone_indices).reshape(-1, 4).astype(np.int64)]  # (n, 4, 12)
    assert B.dtype == f32
    M = ((w[:, 0, None] * B[:, 0] + w[:, 1, None] * B[:, 1]) + w[:, 2, None] * B[:, 2]) + w[:, 3, None] * B[:, 3]
    assert M.dtype == f32
    M = M.reshape(-1, 3, 4)
    x, y, z = p[:, 0, None], p[:, 1, None], p[:, 2, None]
    out_p = ((M[:, :, 0] * x + M[:, :, 1] * y) + M[:, :, 2] * z) + M[:, :, 3]
    x, y, z = n[:, 0, None], n[:, 1, None], n[:, 2, None]
    out_n = (M[:, :, 0] * x + M[:, :, 1] * y) + M[:, :, 2] * z
    d = (out_n[:, 0] * out_n[:, 0] + out_n[:, 1] * out_n[:, 1]) + out_n[:, 2] * out_n[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = f32(1.0) / np.sqrt(d)
        scaled = out_n * s[:, None]
    out_n = np.where((d > 0)[:, None], scaled, out_n)
    assert out_p.dtype == f32 and out_n.dtype == f32
    return np.ascontiguousarray(out_p), np.ascontiguousarray(out_n)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)
