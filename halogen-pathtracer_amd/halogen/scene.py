"""Host-side scene objects and buffer packing — the mirror of the reference's C# host data producers.

  HalogenMaterial        Assets/Scripts/RayTracingManager.cs:6-38   (authoring struct + defaults)
  RayTracingMesh         Assets/Scripts/RayTracingMesh.cs           (cache mesh data, build BLAS, pack tris)
  RayTracingSphere       Assets/Scripts/RayTracingSphere.cs
  Scene (registry)       Assets/Scripts/RayTracingManager.cs:40-145 (enumeration order = buffer order)
  pack_scene             HalogenRenderPass.UpdateObjectBuffers / PackHalogenMaterial / PackMaterialToList
                         (Render Features/HalogenRenderPass.cs:425-537)

The BLAS build and triangle packing run in the native library (hg_build_blas / hg_pack_triangles,
restating BVHGenerator.cs and RayTracingMesh.UpdateTriangleList); all float32 arithmetic the C# code does
on packed values (1/subsurface * absorption, bounds centre/extents) is done in float32 here as well.
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .unity import Transform, mesh_bounds_min_max, to_unity_floats

f32 = np.float32


def _c(v) -> float:
    return float(f32(v))


@dataclass(frozen=True)
class HalogenMaterial:
    """RayTracingManager.cs:6-38.  Colors are linear RGBA (the project uses linear space)."""

    color: tuple = (1.0, 1.0, 1.0, 1.0)
    roughness: float = 1.0
    metallic: float = 0.0
    specularColor: tuple = (1.0, 1.0, 1.0, 1.0)
    subsurfaceColor: tuple = (1.0, 1.0, 1.0, 1.0)
    indexOfRefraction: float = 1.0
    absorption: float = 0.0
    dielectricPriority: int = 0
    emissionColor: tuple = (0.0, 0.0, 0.0, 1.0)  # Color.black
    emissionIntensity: float = 0.0

    def __post_init__(self):  # store exactly what a C# float field would hold
        for name in ("color", "specularColor", "subsurfaceColor", "emissionColor"):
            object.__setattr__(self, name, tuple(_c(v) for v in getattr(self, name)))
        for name in ("roughness", "metallic", "indexOfRefraction", "absorption", "emissionIntensity"):
            object.__setattr__(self, name, _c(getattr(self, name)))
        object.__setattr__(self, "dielectricPriority", int(self.dielectricPriority))

    @staticmethod
    def default(color=(1.0, 1.0, 1.0, 1.0)) -> "HalogenMaterial":
        """new HalogenMaterial(defaultColor): color = specular = subsurface = defaultColor (:24-37)."""
        return HalogenMaterial(color=color, specularColor=color, subsurfaceColor=color)


def pack_material(m: HalogenMaterial, material_id: int) -> abi.PackedHalogenMaterial:
    """PackHalogenMaterial, RP:425-446."""
    p = abi.PackedHalogenMaterial()
    p.materialID = material_id
    p.albedo = abi.Vec4(*m.color)
    p.specularAlbedo = abi.Vec4(*m.specularColor)
    p.metallic = m.metallic
    p.roughness = m.roughness
    p.emissive = abi.Vec4(m.emissionColor[0], m.emissionColor[1], m.emissionColor[2], m.emissionIntensity)
    sub = [f32(v) for v in m.subsurfaceColor[:3]]
    amax = f32(max(m.absorption, 0.0))  # Mathf.Max(material.absorption, 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        absorb = [float((f32(1.0) / s) * amax) for s in sub]  # new Vector3(1/x,1/y,1/z) * max(...)
    p.rayMedium.indexOfRefraction = m.indexOfRefraction
    p.rayMedium.absorption = abi.Vec3(*absorb)
    p.rayMedium.priority = m.dielectricPriority
    p.rayMedium.materialID = material_id
    return p


# BLAS builder of the meshes constructed from here on: "reference" (BVHGenerator.cs, the drop-in's parity path) or
# "sah" (hg_build_blas_sah: a binned-SAH hierarchy in the same format, NOT the reference's images)
BLAS_BUILDERS = ("reference", "sah")
_blas_builder = "reference"
SAH_MAX_LEAF = 2


def set_blas_builder(name: str) -> str:
    """Select the BLAS builder for meshes built afterwards; returns the previous one."""
    global _blas_builder
    if name not in BLAS_BUILDERS:
        raise ValueError(f"unknown BLAS builder {name!r}")
    prev, _blas_builder = _blas_builder, name
    return prev


_CACHE_TOKENS = itertools.count(1)


class RayTracingMesh:
    """RayTracingMesh.cs: submesh-0 triangles, vertices and normals of a mesh + its transform + material.

    CacheRaytracingData (:51-68) runs at construction: the BLAS is built (reordering the triangle list in
    place, exactly as the C# builder does) and the 72-B triangles are packed from the reordered list.
    """

    def __init__(self, name: str, vertices, normals, triangles, transform: Transform,
                 material: HalogenMaterial | None = None, max_hierarchy_depth: int = 32):
        self.name = name
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        self.normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        self.triangles = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3).copy()
        if self.normals.shape != self.vertices.shape:
            raise ValueError("normals must match vertices")
        self.transform = transform
        self.material = material if material is not None else HalogenMaterial.default()
        self.max_hierarchy_depth = int(max_hierarchy_depth)
        self.blas_builder = _blas_builder
        self.deform_serial = 0  # deform() calls since the geometry was cached
        # deform(rebuild=True) calls, and of the last one: its input (the moved triangles in the order before it, which
        # is the device's until the pass rebuilds), its leaf size, and deform_serial right after it
        self.rebuild_serial, self.rebuild_input, self.rebuild_leaf, self.rebuild_at = 0, None, 0, 0
        self.rebuild_node_cost = None  # of a deform(rebuild="sah"): the node cost its twin used
        self.normals_recomputed = False  # the last deform() took normals="recompute"
        self._cache()

    def _cache(self):
        # a new token whenever the geometry is (re)cached, as the reference's manager ID is new on every OnEnable
        # (RayTracingManager.cs:74-79): the pass's geometry generation keys on it (id() of a collected mesh is reused)
        self.cache_token = next(_CACHE_TOKENS)
        L = abi.lib()
        n_tris = len(self.triangles)
        mn, mx = mesh_bounds_min_max(self.vertices) if len(self.vertices) else (np.zeros(3, f32), np.zeros(3, f32))
        mn = np.ascontiguousarray(mn, dtype=np.float32)
        mx = np.ascontiguousarray(mx, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        cap = 2 * n_tris + 2
        nodes = (abi.BVHEntry * cap)()
        # the parallel build returns the same nodes and triangle order (tests/test_bvh.py); 8 workers measured
        # best on the GPU box's host (tools/bench_build.py: 871k triangles 0.12 s -> 0.05 s)
        if self.blas_builder == "sah":
            n = L.hg_build_blas_sah(self.vertices.ctypes.data, len(self.vertices), self.triangles.ctypes.data, n_tris,
                                    SAH_MAX_LEAF, 48, C.cast(nodes, C.c_void_p), cap)
        else:
            n = L.hg_build_blas_mt(self.vertices.ctypes.data, len(self.vertices), self.triangles.ctypes.data, n_tris,
                                   mn.ctypes.data_as(fp), mx.ctypes.data_as(fp), self.max_hierarchy_depth,
                                   C.cast(nodes, C.c_void_p), cap, min(8, len(os.sched_getaffinity(0))))
        if n < 0:
            raise abi.HalogenError(f"hg_build_blas failed for {self.name}: {n}")
        self.bvh = (abi.BVHEntry * n)()
        C.memmove(self.bvh, nodes, n * C.sizeof(abi.BVHEntry))
        # inner entries of the current tree: the records a device rebuild may certainly use (the device keeps the record
        # span of the tree it was last given in full, which is never smaller than the current tree's)
        self.bvh_inner = int((np.frombuffer(self.bvh, dtype=np.uint32).reshape(-1, 8)[:, 1] == 0).sum()) if n else 0
        self.packed_triangles = (abi.HalogenTriangle * n_tris)()
        rc = L.hg_pack_triangles(self.vertices.ctypes.data, self.normals.ctypes.data, len(self.vertices),
                                 self.triangles.ctypes.data, n_tris, C.cast(self.packed_triangles, C.c_void_p))
        if rc != 0:
            raise abi.HalogenError(f"hg_pack_triangles failed for {self.name}: {rc}")

    def deform(self, vertices, normals=None, rebuild=False, leaf_size: int = 0, node_cost: float = 0.0) -> None:
        """Move the vertices (same count; skinning, cloth, a morph target) and keep the topology: the triangles are
        repacked through the index list the BLAS build already permuted, and the BLAS is refitted on the host
        (hg_refit_blas: every box from the moved triangles, the tree as it was), so pack() is always current.  The
        cache token stays (the geometry generation does not change); deform_serial tells the pass to refit the device
        (Context.refit_mesh) instead of rebuilding.  A refitted tree is valid for any deformation and as tight as the
        builder's boxes, but its split planes are the rest pose's: large deformations trace slower than a rebuild.

        rebuild=True gives the mesh a new tree over the moved triangles instead (abi.build_blas_lbvh, the host twin of
        Context.rebuild_mesh: a linear BVH with leaves of leaf_size; 0: the smallest of 4..15 whose tree fits).  A tree
        fits when it has no more inner entries than the mesh's current tree: that many records the device certainly
        has for it, whether or not a full upload came in between, so the room never grows back after a rebuild with
        larger leaves; a leaf size that does not fit raises ValueError before anything is changed.  The triangle order changes: the index list is permuted with it, so later plain deforms repack in
        the new order.  The BVH array keeps its length (entries past the new tree are unreachable padding) and the cache
        token stays, so the pass rebuilds on the device (rebuild_serial) and its next upload is still vouched.

        rebuild="sah" is the rebuild with leaves chosen by surface area (abi.build_blas_lbvh_sah, the host twin of
        Context.rebuild_mesh_sah) at node_cost (0: the library's value, doubled until the tree fits), under the same
        rule of fit; rebuild_node_cost keeps the cost the twin used, which is what the pass gives the device.

        normals="recompute" takes the normals from the moved faces (abi.vertex_normals, the host twin of
        Context.deform_mesh(recompute_normals=True): area-weighted, independent of the triangles' order);
        normals_recomputed remembers it, and a pass with recompute_normals then sends the positions alone."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        recompute = isinstance(normals, str)
        if recompute:
            if normals != "recompute":
                raise ValueError(f"normals must be an array, None or 'recompute', not {normals!r}")
            if v.shape != self.vertices.shape:
                raise ValueError("deform keeps the vertex count")
            n = abi.vertex_normals(v, self.triangles) if len(self.triangles) else np.zeros_like(v)
        else:
            n = self.normals if normals is None else np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        if v.shape != self.vertices.shape or n.shape != v.shape:
            raise ValueError("deform keeps the vertex count")
        fit = []
        sah = None
        if isinstance(rebuild, str):
            if rebuild != "sah":
                raise ValueError(f"rebuild must be False, True or 'sah', not {rebuild!r}")
            if len(self.triangles):
                n_tris = len(self.triangles)
                moved = (abi.HalogenTriangle * n_tris)()
                rc = abi.lib().hg_pack_triangles(v.ctypes.data, n.ctypes.data, len(v), self.triangles.ctypes.data, n_tris,
                                                 C.cast(moved, C.c_void_p))
                if rc != 0:
                    raise abi.HalogenError(f"hg_pack_triangles failed for {self.name}: {rc}")
                try:
                    sah = abi.build_blas_lbvh_sah(moved, node_cost, self.bvh_inner)
                except abi.HalogenError as e:
                    if e.rc != abi.HG_E_UNSUPPORTED:
                        raise
                    raise ValueError(f"{self.name}: no tree at node cost {node_cost or 'automatic'} fits the "
                                     f"{self.bvh_inner} inner entries of its tree") from None
        elif rebuild and len(self.triangles):
            n_tris = len(self.triangles)
            sizes = [int(leaf_size)] if leaf_size else range(4, 16)
            fit = [k for k in sizes if 1 <= k <= 15 and (n_tris + k - 1) // k - 1 <= self.bvh_inner]
            if not fit:
                raise ValueError(f"{self.name}: no LBVH with leaf size {leaf_size or '4..15'} fits the {self.bvh_inner} "
                                 f"inner entries of its tree")
        self.vertices, self.normals = v, n
        self.normals_recomputed = recompute
        rc = abi.lib().hg_pack_triangles(v.ctypes.data, n.ctypes.data, len(v), self.triangles.ctypes.data,
                                         len(self.triangles), C.cast(self.packed_triangles, C.c_void_p))
        if rc != 0:
            raise abi.HalogenError(f"hg_pack_triangles failed for {self.name}: {rc}")
        if fit:
            moved = (abi.HalogenTriangle * n_tris)()
            C.memmove(moved, self.packed_triangles, C.sizeof(moved))
            order, self.packed_triangles, nodes = abi.build_blas_lbvh(moved, fit[0])
            self.triangles = np.ascontiguousarray(self.triangles[order])
            C.memset(self.bvh, 0, C.sizeof(self.bvh))
            C.memmove(self.bvh, nodes, C.sizeof(nodes))
            self.bvh_inner = (n_tris + fit[0] - 1) // fit[0] - 1
            self.rebuild_serial += 1
            self.rebuild_input, self.rebuild_leaf, self.rebuild_at = moved, fit[0], self.deform_serial + 1
            self.rebuild_node_cost = None
        elif sah:
            order, self.packed_triangles, nodes, used = sah
            self.triangles = np.ascontiguousarray(self.triangles[order])
            C.memset(self.bvh, 0, C.sizeof(self.bvh))
            C.memmove(self.bvh, nodes, C.sizeof(nodes))
            self.bvh_inner = (len(nodes) - 1) // 2
            self.rebuild_serial += 1
            self.rebuild_input, self.rebuild_leaf, self.rebuild_at = moved, 0, self.deform_serial + 1
            self.rebuild_node_cost = used  # the rung the twin used: the device is given it, not its own ladder
        elif len(self.triangles):
            abi.refit_blas(self.packed_triangles, self.bvh)
        self.deform_serial += 1

    def set_skin(self, bone_indices, weights) -> None:
        """Make the mesh skinnable: its current vertices and normals become the rest pose, with per vertex four bone
        indices and four weights ((n_vertices, 4) each; the weights are used as given)."""
        b = np.ascontiguousarray(bone_indices, dtype=np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
        if len(b) != len(self.vertices) or len(w) != len(self.vertices):
            raise ValueError("set_skin takes four bone indices and four weights per vertex")
        self.rest_vertices, self.rest_normals = self.vertices.copy(), self.normals.copy()
        self.bone_indices, self.bone_weights = b, w

    def pose(self, bones, rebuild=False, leaf_size: int = 0, node_cost: float = 0.0, normals=None) -> None:
        """Pose the skinned mesh (set_skin) by a bone palette, (n_bones, 12) row-major 3 x 4 matrices: the rest pose goes
        through abi.skin_vertices (the host twin of Context.skin_mesh) and the result through deform() as it is, so the
        host arrays stay current.  rebuild, leaf_size, node_cost: deform's.  normals="recompute": the skinned normals are
        replaced by those of the skinned faces (the twin of Context.skin_mesh(recompute_normals=True))."""
        if getattr(self, "bone_indices", None) is None:
            raise ValueError(f"{self.name}: pose needs set_skin")
        v, n = abi.skin_vertices(self.rest_vertices, self.rest_normals, self.bone_indices, self.bone_weights, bones)
        if normals is not None and not (isinstance(normals, str) and normals == "recompute"):
            raise ValueError(f"normals must be None or 'recompute', not {normals!r}")
        self.deform(v, n if normals is None else normals, rebuild=rebuild, leaf_size=leaf_size, node_cost=node_cost)

    @property
    def triangle_count(self) -> int:
        return len(self.triangles)

    def world_bounds(self):
        """meshRenderer.bounds padded as GetBounds (:106-117): world AABB of the transformed local box."""
        mn, mx = mesh_bounds_min_max(self.vertices)
        corners = np.array([[x, y, z, 1.0] for x in (mn[0], mx[0]) for y in (mn[1], mx[1]) for z in (mn[2], mx[2])])
        w = (self.transform.local_to_world @ corners.T).T[:, :3]
        return unity_bounds(w.min(axis=0), w.max(axis=0), pad=True)

    def mesh_data(self, material_index: int, tri_offset: int, node_offset: int) -> abi.HalogenMeshData:
        """GetRefreshedMeshData, RayTracingMesh.cs:89-104."""
        d = abi.HalogenMeshData()
        bmin, bmax = self.world_bounds()
        d.boundingCornerA = abi.Vec3(*bmin)
        d.boundingCornerB = abi.Vec3(*bmax)
        d.triangleBufferOffset = tri_offset
        d.accelerationBufferOffset = node_offset
        d.materialIndex = material_index
        d.localToWorld.m[:] = to_unity_floats(self.transform.local_to_world)
        d.worldToLocal.m[:] = to_unity_floats(self.transform.world_to_local)
        return d


class RayTracingSphere:
    """RayTracingSphere.cs: centre = transform.position (world), radius = the serialized field."""

    def __init__(self, name: str, transform: Transform, radius: float, material: HalogenMaterial | None = None):
        self.name = name
        self.transform = transform
        self.radius = _c(radius)
        self.material = material if material is not None else HalogenMaterial.default()


def unity_bounds(mn, mx, pad: bool):
    """UnityEngine.Bounds round trip (SetMinMax -> min/max), optionally with the thin-box pad."""
    fp = C.POINTER(C.c_float)
    a = np.ascontiguousarray(mn, dtype=np.float32)
    b = np.ascontiguousarray(mx, dtype=np.float32)
    o1 = np.zeros(3, np.float32)
    o2 = np.zeros(3, np.float32)
    abi.lib().hg_unity_bounds(a.ctypes.data_as(fp), b.ctypes.data_as(fp), 1 if pad else 0, o1.ctypes.data_as(fp),
                              o2.ctypes.data_as(fp))
    return o1, o2


@dataclass
class PackedScene:
    spheres: object
    meshes: object
    materials: object
    triangles: object
    blas: object
    names: list = field(default_factory=list)

    def counts(self) -> dict:
        return {"spheres": len(self.spheres), "meshes": len(self.meshes), "materials": len(self.materials),
                "triangles": len(self.triangles), "blas": len(self.blas)}

    def as_numpy(self) -> dict:
        """Raw bytes of each buffer (for hashing / fixtures)."""
        return {k: np.frombuffer(bytes(getattr(self, k)), dtype=np.uint8)
                for k in ("spheres", "meshes", "materials", "triangles", "blas")}


class Scene:
    """The RayTracingManager registries: spheres and meshes in enumeration (= buffer) order."""

    def __init__(self):
        self.spheres: list[RayTracingSphere] = []
        self.meshes: list[RayTracingMesh] = []

    def add(self, obj):
        (self.spheres if isinstance(obj, RayTracingSphere) else self.meshes).append(obj)
        return obj

    def pack(self) -> PackedScene:
        """UpdateObjectBuffers, RP:448-509 (with PackMaterialToList's struct-equality dedup, :524-537)."""
        unpacked: list[HalogenMaterial] = []
        materials: list[abi.PackedHalogenMaterial] = []

        def material_index(m: HalogenMaterial) -> int:
            if m in unpacked:
                return unpacked.index(m)
            unpacked.append(m)
            materials.append(pack_material(m, len(materials)))
            return len(materials) - 1

        sph = []
        for s in self.spheres:
            hs = abi.HalogenSphere()
            c = s.transform.position
            r = f32(s.radius)
            hs.center = abi.Vec3(*c)
            hs.radius = float(r)
            hs.materialIndex = material_index(s.material)
            hs.boundingCornerA = abi.Vec3(*(c - np.array([r, r, r], np.float32)))
            hs.boundingCornerB = abi.Vec3(*(c + np.array([r, r, r], np.float32)))
            sph.append(hs)
        mesh_records, tri_chunks, node_chunks = [], [], []
        n_tris = n_nodes = 0
        for m in self.meshes:
            mi = material_index(m.material)
            tri_chunks.append(m.packed_triangles)
            mesh_records.append(m.mesh_data(mi, n_tris, n_nodes))
            node_chunks.append(m.bvh)
            n_tris += m.triangle_count
            n_nodes += len(m.bvh)
        tris = (abi.HalogenTriangle * n_tris)()
        nodes = (abi.BVHEntry * n_nodes)()
        ot = on = 0
        for tc, nc in zip(tri_chunks, node_chunks):
            C.memmove(C.addressof(tris) + ot * C.sizeof(abi.HalogenTriangle), tc, C.sizeof(tc))
            C.memmove(C.addressof(nodes) + on * C.sizeof(abi.BVHEntry), nc, C.sizeof(nc))
            ot += len(tc)
            on += len(nc)
        return PackedScene(
            spheres=(abi.HalogenSphere * len(sph))(*sph),
            meshes=(abi.HalogenMeshData * len(mesh_records))(*mesh_records),
            materials=(abi.PackedHalogenMaterial * len(materials))(*materials),
            triangles=tris,
            blas=nodes,
            names=[s.name for s in self.spheres] + [m.name for m in self.meshes],
        )
