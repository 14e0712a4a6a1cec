"""Hand-built packed scenes for tests/test_tree_cases.py (CPU) and tests/test_gpu_trees.py: BVHEntry trees written entry by
entry, not by a builder, at the extremes the C-ABI accepts and no builder produces.

  chain62      the deepest accepted tree (62 levels, stack_depth 64), instanced twice, one instance turned 180 degrees
  leaf_ladder  leaves of 1 .. 17, 31, 32, 33, 63, 64, 65 and 130 triangles
  ties         identical sibling boxes, one triangle in several places (a leaf, two leaves, two meshes), zero-area ones
  transforms   one tree under the identity, a mirror, an anisotropic and two uniform scales of 1e3 and 1e-3

Every material emits, so a frame's colour shows which copy of a triangle a camera ray met even without a sky."""
from dataclasses import dataclass, field, replace
from functools import lru_cache

import numpy as np

from halogen import abi, render_pass as rp, scene as hs
from halogen.unity import Transform, euler_to_quat, to_unity_floats, trs
from test_refit import BVH_DT

f32 = np.float32
INF = f32(np.inf)
W, H = 40, 24
LADDER = list(range(1, 18)) + [31, 32, 33, 63, 64, 65, 130]


# ---- raw arrays -> PackedScene ----------------------------------------------------------------------------------------
def packed_scene(tris18, bvh, meshes, materials, spheres=()) -> hs.PackedScene:
    """A PackedScene from raw arrays: (n, 18) float32 triangles (three points, three normals), BVH_DT entries, mesh
    records as dicts (triangleBufferOffset, accelerationBufferOffset, materialIndex, localToWorld as a 4 x 4 matrix and
    optionally worldToLocal, else its inverse) and HalogenMaterial objects.  The mesh record's world box (which no
    traversal reads) is the root entry's box under localToWorld."""
    t = np.ascontiguousarray(tris18, f32).reshape(-1, 18)
    b = np.ascontiguousarray(bvh, BVH_DT)
    recs = (abi.HalogenMeshData * len(meshes))()
    for r, m in zip(recs, meshes):
        l2w = np.asarray(m["localToWorld"], np.float64)
        w2l = np.asarray(m["worldToLocal"], np.float64) if "worldToLocal" in m else np.linalg.inv(l2w)
        r.triangleBufferOffset, r.accelerationBufferOffset = m["triangleBufferOffset"], m["accelerationBufferOffset"]
        r.materialIndex = m["materialIndex"]
        r.localToWorld.m[:] = to_unity_floats(l2w)
        r.worldToLocal.m[:] = to_unity_floats(w2l)
        root = b[m["accelerationBufferOffset"]]
        c = np.array([[x, y, z, 1.0] for x in (root["lo"][0], root["hi"][0]) for y in (root["lo"][1], root["hi"][1])
                      for z in (root["lo"][2], root["hi"][2])], np.float64)
        w = (l2w @ c.T).T[:, :3]
        r.boundingCornerA, r.boundingCornerB = abi.Vec3(*w.min(axis=0)), abi.Vec3(*w.max(axis=0))
    mats = [hs.pack_material(m, i) for i, m in enumerate(materials)]
    return hs.PackedScene(spheres=(abi.HalogenSphere * len(spheres))(*spheres), meshes=recs,
                          materials=(abi.PackedHalogenMaterial * len(mats))(*mats),
                          triangles=(abi.HalogenTriangle * len(t)).from_buffer_copy(t.tobytes()),
                          blas=(abi.BVHEntry * len(b)).from_buffer_copy(b.tobytes()))


def glow(r, g, b, intensity=1.0) -> hs.HalogenMaterial:
    return hs.HalogenMaterial(color=(r, g, b, 1.0), specularColor=(r, g, b, 1.0), subsurfaceColor=(r, g, b, 1.0),
                              emissionColor=(r, g, b, 1.0), emissionIntensity=intensity)


def tri18(p, n=None, rng=None):
    """One triangle record from (3, 3) points; normals given, or the face normal bent a little per vertex by rng."""
    p = np.asarray(p, np.float64)
    if n is None:
        face = np.cross(p[1] - p[0], p[2] - p[0])
        face = face / max(np.linalg.norm(face), 1e-30) if np.linalg.norm(face) > 0 else np.array([0.0, 0.0, 1.0])
        n = face[None, :] + (rng.normal(0, 0.15, (3, 3)) if rng is not None else np.zeros((3, 3)))
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
    return np.concatenate([p.reshape(-1), np.asarray(n, np.float64).reshape(-1)]).astype(f32)


@dataclass
class Node:
    """A BVHEntry to be: a leaf (first, count) or an inner entry (a, b); the box is given or the children's union."""
    lo: object = None
    hi: object = None
    first: int = 0
    count: int = 0
    a: "Node | None" = None
    b: "Node | None" = None


def leaf_of(tris, first, count, pad=0.0, box=None) -> Node:
    if box is not None:
        return Node(np.asarray(box[0], f32), np.asarray(box[1], f32), first, count)
    pts = np.asarray(tris, f32)[first:first + count, :9].reshape(-1, 3)
    return Node(pts.min(axis=0) - f32(pad), pts.max(axis=0) + f32(pad), first, count)


def inner_of(a: Node, b: Node, box=None) -> Node:
    if box is not None:
        return Node(np.asarray(box[0], f32), np.asarray(box[1], f32), a=a, b=b)
    return Node(np.minimum(a.lo, b.lo), np.maximum(a.hi, b.hi), a=a, b=b)


def flatten(root: Node) -> np.ndarray:
    """The tree as BVH_DT entries, the root at 0, an inner entry's children at indexA and indexA + 1."""
    out = [None]
    todo = [(root, 0)]
    while todo:
        node, at = todo.pop()
        if node.a is None:
            out[at] = (node.first, node.count, node.lo, node.hi)
        else:
            ia = len(out)
            out += [None, None]
            out[at] = (ia, 0, node.lo, node.hi)
            todo += [(node.b, ia + 1), (node.a, ia)]
    return np.array(out, BVH_DT)


def balanced(leaves) -> Node:
    if len(leaves) == 1:
        return leaves[0]
    half = (len(leaves) + 1) // 2
    return inner_of(balanced(leaves[:half]), balanced(leaves[half:]))


# ---- the cases ---------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    packed: hs.PackedScene
    camera: rp.Camera
    settings: rp.HalogenSettings
    info: dict = field(default_factory=dict)

    def params(self, frame=1, camera=None, **overrides) -> abi.HgParams:
        s = rp.clamp_settings(replace(self.settings, **overrides))
        return rp.make_params(s, camera or self.camera, frame, len(self.packed.spheres), len(self.packed.meshes), False)


SETTINGS = rp.HalogenSettings(useHDRISky=False)
CHAIN_X, CHAIN_Y, CHAIN_DZ, CHAIN_PAD = 1.4, 1.2, 0.1, 0.045


def chain_tree(levels: int, seed: int = 62):
    """Triangles and entries of a chain of `levels` inner entries: inner k has the children leaf k and inner k + 1 (in
    either order, alternating), the last one two leaves.  Leaf k lies at z = 0.1 * (levels - k): leaf 0 at the back, the
    last leaf in front.  Every box spans the same x and y, a leaf's box its own thin z slab, an inner entry's box all
    slabs from its nearest leaf's to the front.  So a ray along +z enters inner k + 1 before leaf k at every level and
    leaf k waits on the stack; a ray along -z meets leaf k first and the stack never holds more than two."""
    rng = np.random.default_rng(seed)
    tris, leaves = [], []
    for k in range(levels + 1):
        z = CHAIN_DZ * (levels - k)
        first = len(tris)
        for _ in range(1 + k % 3):
            c = rng.uniform([-CHAIN_X + 0.2, -CHAIN_Y + 0.2], [CHAIN_X - 0.2, CHAIN_Y - 0.2])
            ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
            xy = c + rng.uniform(0.15, 0.7) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
            xy = np.clip(xy, [-CHAIN_X + 0.02, -CHAIN_Y + 0.02], [CHAIN_X - 0.02, CHAIN_Y - 0.02])
            p = np.concatenate([xy, z + rng.uniform(-0.03, 0.03, (3, 1))], axis=1)
            tris.append(tri18(p, rng=rng))
        leaves.append(leaf_of(tris, first, len(tris) - first,
                              box=((-CHAIN_X, -CHAIN_Y, z - CHAIN_PAD), (CHAIN_X, CHAIN_Y, z + CHAIN_PAD))))
    node = None
    for k in range(levels - 1, -1, -1):
        box = ((-CHAIN_X, -CHAIN_Y, -CHAIN_PAD), (CHAIN_X, CHAIN_Y, CHAIN_DZ * (levels - k) + CHAIN_PAD))
        deeper = leaves[levels] if node is None else node
        node = inner_of(deeper, leaves[k], box) if k % 2 == 0 else inner_of(leaves[k], deeper, box)
    return np.array(tris, f32), flatten(node)


def chain_case(levels: int = 62) -> Case:
    """A small quad (a leaf root, so the chain's two buffer offsets are not 0), the chain seen from its front by the
    camera, covering the left three quarters of the image, and the same tree again turned 180 degrees about y on the
    right: the camera sees that one from behind.  Rays through both, through one and through neither share waves."""
    ctris, cbvh = chain_tree(levels)
    quad = np.array([[-1.9, -1.1, 50.0], [-0.9, -1.1, 50.0], [-0.9, -0.3, 50.0], [-1.9, -0.3, 50.0]])
    qtris = np.array([tri18(quad[[0, 1, 2]]), tri18(quad[[0, 2, 3]])], f32)
    qbvh = flatten(leaf_of(qtris, 0, 2, pad=0.01))
    meshes = [
        dict(triangleBufferOffset=0, accelerationBufferOffset=0, materialIndex=0, localToWorld=np.eye(4)),
        dict(triangleBufferOffset=2, accelerationBufferOffset=1, materialIndex=1,
             localToWorld=trs((-0.55, 0.0, 40.0), (0, 0, 0, 1), (1, 1, 1))),
        dict(triangleBufferOffset=2, accelerationBufferOffset=1, materialIndex=2,
             localToWorld=trs((1.9, 0.0, 47.0), (0, 1, 0, 0), (1, 1, 1))),
    ]
    packed = packed_scene(np.concatenate([qtris, ctris]), np.concatenate([qbvh, cbvh]), meshes,
                          [glow(0.9, 0.9, 0.2), glow(0.2, 0.6, 1.0, 0.7), glow(1.0, 0.3, 0.2, 0.5)])
    # 2.8 degrees: at the chain's far end (z = 46.3) the frame is 2 x 1.13 high and 2 x 1.89 wide, inside every box's y
    camera = rp.Camera(Transform((0, 0, 0)), 2.8, W, H)
    # behind the first instance and narrower, so that no camera ray reaches the turned instance's boxes (x >= 0.5)
    behind = rp.Camera(Transform((-0.75, 0.0, 86.0), (0, 1, 0, 0)), 1.6, W, H)
    return Case(f"chain{levels}", packed, camera, SETTINGS,
                dict(behind=behind, levels=levels, chain_mesh=1, chain_tris=(2, len(ctris)), chain_nodes=(1, len(cbvh))))


def ladder_case() -> Case:
    """One mesh of 24 leaves on a 6 x 4 grid of unit cells, leaf i a zig-zag strip of LADDER[i] triangles across its cell."""
    rng = np.random.default_rng(15)
    tris, leaves = [], []
    for i, n in enumerate(LADDER):
        x0, y0 = -3.0 + (i % 6) + 0.04, -2.0 + (i // 6) + 0.04
        w = 0.92 / ((n + 1) // 2 + 0.5)
        first = len(tris)
        for j in range(n):
            k = j // 2
            bottom = lambda q: [x0 + q * w, y0]
            top = lambda q: [x0 + (q + 0.5) * w, y0 + 0.92]
            xy = [bottom(k), bottom(k + 1), top(k)] if j % 2 == 0 else [top(k), bottom(k + 1), top(k + 1)]
            tris.append(tri18(np.concatenate([np.array(xy), rng.uniform(-0.05, 0.05, (3, 1))], axis=1), rng=rng))
        leaves.append(leaf_of(tris, first, n))
    tris = np.array(tris, f32)
    l2w = trs((0.2, -0.1, 12.0), euler_to_quat(5, 10, 3), (1, 1, 1))
    packed = packed_scene(tris, flatten(balanced(leaves)),
                          [dict(triangleBufferOffset=0, accelerationBufferOffset=0, materialIndex=0, localToWorld=l2w)],
                          [glow(0.8, 0.7, 0.6)])
    return Case("leaf_ladder", packed, rp.Camera(Transform((0, 0, 0)), 20.0, W, H), SETTINGS,
                dict(leaf_first=[l.first for l in leaves], leaf_count=[l.count for l in leaves]))


def ties_case() -> Case:
    """Identity matrices throughout, so a mesh-local ray is the world ray and copies of a triangle give equal t bit for bit.
    Mesh order V, T, U.  T: root -> (X, Y), X -> (A, B), Y -> (C, D), every one of the seven boxes the same.  Eight
    triangles T0..T7 tile the square; A (20 triangles, a table leaf) holds each of them twice with different normals, two
    zero-area triangles and two small ones in front; B, C and D hold further copies, and copies of two nearer triangles
    N0, N1 that A does not hold (N0: first met in B; N1: in C and D only).  U is a second instance of T's tree with
    another material.  V, the first mesh, holds copies of T2 and T5 and a triangle beside the square."""
    rng = np.random.default_rng(7)
    corners = {}
    for ix in range(3):
        for iy in range(3):
            corners[ix, iy] = [ix - 1.0, iy - 1.0, float(rng.uniform(-0.05, 0.05))]
    base = []
    for ix in range(2):
        for iy in range(2):
            a, b, c, d = corners[ix, iy], corners[ix + 1, iy], corners[ix + 1, iy + 1], corners[ix, iy + 1]
            base += [np.array([a, b, c]), np.array([a, d, c])]  # the second one wound the other way
    near = [np.array([[-0.7, -0.2, -0.3], [-0.1, -0.3, -0.3], [-0.4, 0.4, -0.3]]),
            np.array([[0.2, -0.6, -0.3], [0.8, -0.5, -0.3], [0.5, 0.1, -0.3]])]
    front = [np.array([[-0.2, 0.5, -0.5], [0.1, 0.5, -0.5], [0.0, 0.8, -0.5]]),
             np.array([[0.5, 0.5, -0.5], [0.9, 0.6, -0.5], [0.7, 0.9, -0.5]])]
    point = np.tile([[0.3, 0.3, -0.4]], (3, 1))
    line_x = np.array([[-0.5, -0.5, -0.4], [0.0, -0.5, -0.4], [0.5, -0.5, -0.4]])
    line_d = np.array([[-0.5, 0.0, -0.4], [0.0, 0.5, -0.4], [0.25, 0.75, -0.4]])
    copy = lambda p: tri18(p, rng=rng)  # the same points, other normals every time
    leaf_a = [copy(p) for p in base] + [copy(p) for p in base] + [copy(point), copy(line_x)] + [copy(p) for p in front]
    leaf_a = [leaf_a[i] for i in rng.permutation(len(leaf_a))]
    leaf_b = [copy(p) for p in base[:4]] + [copy(near[0]), copy(line_d)]
    leaf_c = [copy(p) for p in base] + [copy(near[0]), copy(near[1])] + [copy(p) for p in base[2:8]]
    leaf_c = [leaf_c[i] for i in rng.permutation(len(leaf_c))]
    leaf_d = [copy(near[1])]
    assert (len(leaf_a), len(leaf_b), len(leaf_c), len(leaf_d)) == (20, 6, 16, 1)
    t_tris = np.array(leaf_a + leaf_b + leaf_c + leaf_d, f32)
    box = ((-1.0, -1.0, -0.6), (1.0, 1.0, 0.2))
    la, lb = leaf_of(t_tris, 0, 20, box=box), leaf_of(t_tris, 20, 6, box=box)
    lc, ld = leaf_of(t_tris, 26, 16, box=box), leaf_of(t_tris, 42, 1, box=box)
    t_bvh = flatten(inner_of(inner_of(la, lb, box), inner_of(lc, ld, box), box))
    v_tris = np.array([copy(base[2]), copy(base[5]),
                       copy(np.array([[1.1, -0.8, 0.0], [1.8, -0.6, 0.1], [1.4, 0.7, -0.1]]))], f32)
    vbox = ((-1.0, -1.0, -0.6), (1.9, 1.0, 0.2))
    v_bvh = flatten(inner_of(leaf_of(v_tris, 0, 2, box=vbox), leaf_of(v_tris, 2, 1, box=vbox), vbox))
    eye = np.eye(4)
    meshes = [dict(triangleBufferOffset=0, accelerationBufferOffset=0, materialIndex=0, localToWorld=eye),
              dict(triangleBufferOffset=3, accelerationBufferOffset=3, materialIndex=1, localToWorld=eye),
              dict(triangleBufferOffset=3, accelerationBufferOffset=3, materialIndex=2, localToWorld=eye)]
    packed = packed_scene(np.concatenate([v_tris, t_tris]), np.concatenate([v_bvh, t_bvh]), meshes,
                          [glow(1.0, 0.2, 0.2), glow(0.2, 1.0, 0.2, 0.8), glow(0.2, 0.2, 1.0, 0.6)])
    all_tris = np.concatenate([v_tris, t_tris])
    p = all_tris[:, :9].reshape(-1, 3, 3).astype(np.float64)
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    return Case("ties", packed, rp.Camera(Transform((0.0, 0.0, -6.0)), 22.0, W, H), SETTINGS,
                dict(zero_area=np.flatnonzero(area == 0.0)))


TRANSFORM_NAMES = ("identity", "mirror", "anisotropic", "times_1000", "times_0.001")


def transforms_case() -> Case:
    """One tree of 16 triangles in 4 leaves, in a slab 2 x 2 wide and 0.002 thick, under five matrices.  The camera at
    (0, -1, -8) sees each instance about a quarter radian wide: the identity's at the origin, the mirrored one beside
    it, the (1e-3, 1, 1e3) one turned so that the camera looks along its thin axis (the slab's thickness times 1e3 is
    its width then), the 1e3 one 8,000 away and the 1e-3 one 0.008 away.  The far plane is 1e6."""
    rng = np.random.default_rng(5)
    tris = []
    for k in range(16):
        c = np.array([-0.75 + 0.5 * (k % 4), -0.75 + 0.5 * (k // 4)]) + rng.uniform(-0.1, 0.1, 2)
        xy = np.clip(c + rng.uniform(-0.7, 0.7, (3, 2)), -1.0, 1.0)
        tris.append(tri18(np.concatenate([xy, rng.uniform(-1e-3, 1e-3, (3, 1))], axis=1), rng=rng))
    tris = np.array(tris, f32)
    bvh = flatten(balanced([leaf_of(tris, 4 * i, 4) for i in range(4)]))
    cam = np.array([0.0, -1.0, -8.0])
    at = lambda tx, ty, d: tuple(cam + np.array([tx, ty, 1.0]) * d)
    l2w = [np.eye(4),
           trs((-3.2, 0.0, 0.0), (0, 0, 0, 1), (-1, 1, 1)),
           trs((3.2, 0.0, 0.0), euler_to_quat(10, 80, 5), (1e-3, 1, 1e3)),
           trs(at(-0.22, -0.2, 8000.0), (0, 0, 0, 1), (1e3, 1e3, 1e3)),
           trs(at(0.22, -0.2, 0.008), (0, 0, 0, 1), (1e-3, 1e-3, 1e-3))]
    meshes = [dict(triangleBufferOffset=0, accelerationBufferOffset=0, materialIndex=i, localToWorld=m)
              for i, m in enumerate(l2w)]
    mats = [glow(1, 1, 1, 0.5), glow(1, 0.3, 0.3), glow(0.3, 1, 0.3), glow(0.3, 0.3, 1), glow(1, 1, 0.2)]
    return Case("transforms", packed_scene(tris, bvh, meshes, mats), rp.Camera(Transform(tuple(cam)), 40.0, W, H),
                replace(SETTINGS, FarPlaneDistance=1.0e6), {})


CASES = ("chain62", "leaf_ladder", "ties", "transforms")


@lru_cache(maxsize=None)
def case(name: str) -> Case:
    return {"chain62": chain_case, "leaf_ladder": ladder_case, "ties": ties_case, "transforms": transforms_case}[name]()


# ---- rays ---------------------------------------------------------------------------------------------------------------
def all_pixels(w=W, h=H):
    return np.stack(np.meshgrid(np.arange(w), np.arange(h)), axis=-1).reshape(-1, 2).astype(np.int32)  # row-major


def bvh_np(packed):
    return np.frombuffer(bytes(packed.blas), dtype=BVH_DT)


def tris_np(packed):
    return np.frombuffer(bytes(packed.triangles), dtype=f32).reshape(-1, 18)


def _l2w(mesh_record):
    return np.array(mesh_record.localToWorld.m[:], np.float64).reshape(4, 4).T


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def special_rays(c: Case, camera_hits, seed=11) -> np.ndarray:
    """Seeded rays a camera never sends, as an (n, 8) float32 array: for every mesh, through its root entry and two of
    its leaves, the six axis directions with every sign of the two zero components, from the box's centre, from the
    centre of its low-z face and from outside; for eight triangles, origins on the triangle's plane with directions
    leaving it, lying in it and random; and every third camera ray with t_max at 0.5, 0.99995, 1, 1.00005 and 2 times the
    distance in camera_hits (the oracle's answers for the case's camera rays, 1.5 where it found none)."""
    rng = np.random.default_rng(seed)
    packed = c.packed
    nodes, tris = bvh_np(packed), tris_np(packed)
    rays = []

    def add(o, d, t_max=INF):
        rays.append(np.concatenate([np.asarray(o, f32), [t_max], np.asarray(d, f32), [0.0]]).astype(f32))

    axis_dirs = []
    for ax in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    d = [z1, z2]
                    d.insert(ax, s)
                    axis_dirs.append(np.array(d, f32))
    for m in packed.meshes:
        l2w = _l2w(m)
        off = m.accelerationBufferOffset
        reach = [off]
        todo = [off]
        while todo:  # the mesh's entries, root first
            e = nodes[todo.pop()]
            if e["count"] == 0:
                kids = [off + int(e["indexA"]), off + int(e["indexA"]) + 1]
                reach += kids
                todo += kids
        leaves = [g for g in reach if nodes[g]["count"] > 0]
        for g in dict.fromkeys([off, leaves[0], leaves[-1]]):
            lo, hi = nodes[g]["lo"].astype(np.float64), nodes[g]["hi"].astype(np.float64)
            centre, face = (lo + hi) / 2, np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, lo[2]])
            size = float(np.linalg.norm(l2w[:3, :3] @ (hi - lo)))
            for local in (centre, face):
                o = (l2w @ np.append(local, 1.0))[:3]
                for d in axis_dirs:
                    add(o, d)
            o = (l2w @ np.append(centre, 1.0))[:3]
            for d in axis_dirs:  # from outside, aimed at the centre
                add(o - d.astype(np.float64) * 2.0 * size, d)
    for g in rng.choice(len(tris), min(8, len(tris)), replace=False):
        l2w = _l2w([m for m in packed.meshes if m.triangleBufferOffset <= g][-1])  # (any mesh holding it will do)
        p = (l2w @ np.concatenate([tris[g, :9].reshape(3, 3).astype(np.float64), np.ones((3, 1))], axis=1).T).T[:, :3]
        e1, e2 = p[1] - p[0], p[2] - p[0]
        if np.linalg.norm(np.cross(e1, e2)) == 0.0:
            continue
        normal = _unit(np.cross(e1, e2))
        for o in (p.mean(axis=0), p.mean(axis=0) + 0.7 * e1, p[0]):
            add(o, normal)
            add(o, -normal)
            add(o, _unit(e2))
            for _ in range(3):
                add(o, _unit(rng.normal(0, 1, 3)))
    cam = camera_hits
    for i in range(0, len(cam["rays"]), 3):
        r = cam["rays"][i]
        t = cam["hits"]["t"][i] if cam["hits"]["kind"][i] else f32(1.5)
        for s in (0.5, 0.99995, 1.0, 1.00005, 2.0):
            add(r["origin"], r["direction"], f32(np.float64(t) * s))
    out = np.array(rays, f32)
    d = out[:, 4:7].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) < 1e-6) and np.isfinite(out[:, :3]).all()
    return out
