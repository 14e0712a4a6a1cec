"""ctypes mirror of include/halogen_abi.h and a thin, error-checked wrapper around libhalogen_hip.so.

The structs below are byte-identical to the reference's C# blittable structs
(Assets/Scripts/Render Features/HalogenRenderPass.cs:10-76); test_abi.py checks every size and offset
against the header.  There is no fallback: if the shared library is missing, importing `lib()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
# HALOGEN_LIB selects an alternative build of the same library (A/B variants in tools/sweep.sh)
LIB_PATH = Path(os.environ["HALOGEN_LIB"]) if os.environ.get("HALOGEN_LIB") else _HERE / "libhalogen_hip.so"


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Vec4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Mat4(C.Structure):
    """UnityEngine.Matrix4x4 field order (m00, m10, m20, m30, m01, ...): column-major."""

    _fields_ = [("m", C.c_float * 16)]


class HalogenSphere(C.Structure):  # RP:10-19, 44 B
    _fields_ = [("center", Vec3), ("radius", C.c_float), ("materialIndex", C.c_uint32),
                ("boundingCornerA", Vec3), ("boundingCornerB", Vec3)]


class HalogenMeshData(C.Structure):  # RP:21-34, 164 B
    _fields_ = [("triangleBufferOffset", C.c_uint32), ("accelerationBufferOffset", C.c_uint32),
                ("boundingCornerA", Vec3), ("boundingCornerB", Vec3), ("materialIndex", C.c_uint32),
                ("worldToLocal", Mat4), ("localToWorld", Mat4)]


class PackedRayMedium(C.Structure):  # RP:36-42, 24 B
    _fields_ = [("indexOfRefraction", C.c_float), ("absorption", Vec3), ("priority", C.c_int32),
                ("materialID", C.c_uint32)]


class PackedHalogenMaterial(C.Structure):  # RP:44-55, 84 B
    _fields_ = [("materialID", C.c_uint32), ("albedo", Vec4), ("specularAlbedo", Vec4), ("metallic", C.c_float),
                ("roughness", C.c_float), ("emissive", Vec4), ("rayMedium", PackedRayMedium)]


class HalogenTriangle(C.Structure):  # RP:57-66, 72 B
    _fields_ = [("pointA", Vec3), ("pointB", Vec3), ("pointC", Vec3), ("normalA", Vec3), ("normalB", Vec3),
                ("normalC", Vec3)]


class BVHEntry(C.Structure):  # RP:68-76, 32 B
    _fields_ = [("indexA", C.c_uint32), ("triangleCount", C.c_uint32), ("boundingCornerA", Vec3),
                ("boundingCornerB", Vec3)]


class HgParams(C.Structure):  # every uniform of HalgoenCompute.compute:26-68,185
    _fields_ = [
        ("camLocalToWorld", Mat4), ("screenParameters", Vec4), ("viewParameters", Vec4),
        ("cameraParameters", Vec4), ("frameCount", C.c_int32), ("samplesPerPixel", C.c_uint32),
        ("maxBounces", C.c_uint32), ("maxDiffuseBounces", C.c_uint32), ("maxGlossyBounces", C.c_uint32),
        ("maxTransmissionBounces", C.c_uint32), ("halogenDebugMode", C.c_uint32),
        ("triangleDebugDisplayRange", C.c_uint32), ("boxDebugDisplayRange", C.c_uint32),
        ("defaultHDRIMipLevel", C.c_int32), ("focalPlaneDistance", C.c_float), ("focalConeAngle", C.c_float),
        ("filterRadius", C.c_float), ("useEnvironmentCubemap", C.c_int32), ("bufferCounts", Vec4),
    ]


class HgCounters(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("rays", C.c_uint64), ("tri_tests", C.c_uint64),
                ("aabb_tests", C.c_uint64), ("mesh_visits", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("hits", C.c_uint64), ("kernel_ms", C.c_double), ("launches", C.c_uint64),
                ("trace_ms", C.c_double), ("trace_launches", C.c_uint64), ("node_rounds", C.c_uint64),
                ("tri_rounds", C.c_uint64), ("last_kernel", C.c_uint64),
                ("trace_cycles", C.c_uint64), ("shade_cycles", C.c_uint64),
                ("shade_detail", C.c_uint64 * 4), ("shade_rounds", C.c_uint64), ("primary_misses", C.c_uint64),
                ("exec_fallbacks", C.c_uint64), ("trace_busy_ms", C.c_double), ("order_faults", C.c_uint64),
                ("scene_uploads", C.c_uint64), ("scene_uploads_skipped", C.c_uint64),
                ("scene_uploads_partial", C.c_uint64), ("scene_uploads_vouched", C.c_uint64),
                ("server_launches", C.c_uint64),
                ("server_frames", C.c_uint64), ("server_refused", C.c_uint64), ("frames_lost", C.c_uint64),
                ("server_ahead", C.c_uint64)]

    def as_dict(self) -> dict:
        return {name: (list(v) if isinstance(v, C.Array) else v)
                for name, v in ((name, getattr(self, name)) for name, _ in self._fields_)}


class HgRay(C.Structure):  # hg_ray, 32 B: a unit-length direction; t_max = +inf for an unbounded ray
    _fields_ = [("origin", Vec3), ("t_max", C.c_float), ("direction", Vec3), ("flags", C.c_uint32)]


class HgRayHit(C.Structure):  # hg_ray_hit, 48 B
    _fields_ = [("t", C.c_float), ("kind", C.c_uint32), ("object", C.c_uint32), ("primitive", C.c_uint32),
                ("u", C.c_float), ("v", C.c_float), ("material", C.c_uint32), ("orientation", C.c_float),
                ("normal", Vec3), ("reserved", C.c_uint32)]


# numpy views of the two records (Context.trace_rays / camera_rays): the same bytes as the ctypes mirrors
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_max", np.float32), ("direction", np.float32, 3),
                      ("flags", np.uint32)])
RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("kind", np.uint32), ("object", np.uint32), ("primitive", np.uint32),
                          ("u", np.float32), ("v", np.float32), ("material", np.uint32), ("orientation", np.float32),
                          ("normal", np.float32, 3), ("reserved", np.uint32)])
HG_HIT_NONE, HG_HIT_MESH, HG_HIT_SPHERE = 0, 1, 2


class DenoiseParams(C.Structure):  # hg_denoise_params, 24 B (include/halogen_abi.h, csrc/hg_atrous.h)
    """The display denoiser's settings: 1..6 a-trous iterations (step 1, 2, 4, ...), the three edge-stopping sigmas
    (<= 0: term off; the colour sigma is the one at iteration 0 and halves every iteration) and albedo demodulation."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("demodulate", C.c_int32), ("flags", C.c_uint32)]


HG_RAYS_CLOSEST, HG_RAYS_ANY = 0, 1
RAY_MODES = {"closest": HG_RAYS_CLOSEST, "any": HG_RAYS_ANY}

HG_OK = 0
HG_KERNEL_MEGA,HG_KERNEL_WAVEFRONT, HG_KERNEL_MEGA_REGEN, HG_KERNEL_MEGA_STREAM, HG_KERNEL_MEGA_POOL = 0, 1, 2, 3, 4
HG_KERNEL_AUTO = 5
HG_OPT_KERNEL, HG_OPT_BLOCK, HG_OPT_COUNTERS, HG_OPT_TIMING, HG_OPT_REFILL, HG_OPT_FRAME_SPLIT = 1, 2, 3, 4, 5, 6
HG_OPT_DESCENT_T = 7
HG_OPT_TILE_ORDER = 8
HG_OPT_COALESCE = 9
HG_OPT_READBACK_DEPTH = 10
HG_OPT_READBACK_STREAM = 11
HG_OPT_WAVE_UNITS = 12
HG_OPT_LANE_PICK = 14
HG_OPT_SERVER = 15
HG_OPT_SERVER_IDLE_US = 16
HG_OPT_SERVER_GATE_US = 17
HG_OPT_QUEUE_FILL = 18
HG_OPT_SERVER_AHEAD = 19
HG_E_INVALID, HG_E_HIP, HG_E_NOMEM, HG_E_NOSCENE, HG_E_NOTARGET, HG_E_UNSUPPORTED, HG_E_COMM = -1, -2, -3, -4, -5, -6, -7
HG_E_FRAME_LOST = -8
HG_READBACK_MAX = 16
# display formats of readback_begin(format=...) (include/halogen_abi.h, csrc/hg_pack.h): bytes per pixel and numpy view
HG_DISPLAY_RGBA32F, HG_DISPLAY_RGBA16F, HG_DISPLAY_R11G11B10F = 0, 1, 2
DISPLAY_FORMATS = {"rgba32f": HG_DISPLAY_RGBA32F, "rgba16f": HG_DISPLAY_RGBA16F, "r11g11b10f": HG_DISPLAY_R11G11B10F}
DISPLAY_BPP = {HG_DISPLAY_RGBA32F: 16, HG_DISPLAY_RGBA16F: 8, HG_DISPLAY_R11G11B10F: 4}

# every symbol include/halogen_abi.h declares (test_abi.py checks the .so exports exactly these)
EXPORTS = [
    "hg_abi_version", "hg_create", "hg_destroy", "hg_last_error", "hg_upload_scene", "hg_upload_scene_gen",
    "hg_upload_cubemap",
    "hg_set_params", "hg_resize", "hg_set_tiling", "hg_clear_accumulation", "hg_render", "hg_synchronize",
    "hg_readback", "hg_readback_begin", "hg_readback_end", "hg_readback_begin_format", "hg_readback_end_data",
    "hg_pack_display", "hg_set_accumulation", "hg_copy_tiles_device", "hg_local_tile_count", "hg_get_counters", "hg_reset_counters",
    "hg_set_option", "hg_selftest", "hg_trace_rays", "hg_trace_rays_device", "hg_camera_rays",
    "hg_update_guides", "hg_readback_guides", "hg_readback_begin_denoised", "hg_denoise_host", "hg_build_blas", "hg_build_blas_mt", "hg_build_blas_sah", "hg_unity_bounds", "hg_pack_triangles",
    "hg_comm_unique_id", "hg_comm_init_rank", "hg_comm_init_all", "hg_comm_gather", "hg_comm_synchronize",
    "hg_comm_readback", "hg_comm_readback_begin", "hg_comm_readback_end", "hg_comm_set_timeout_ms", "hg_comm_transport", "hg_comm_last_error", "hg_comm_destroy",
    "hg_comm_assemble_host",
    "hg_refit_blas", "hg_refit_mesh", "hg_refit_mesh_device", "hg_scene_readback",
    "hg_build_blas_lbvh", "hg_rebuild_mesh", "hg_rebuild_mesh_device",
    "hg_build_blas_lbvh_sah", "hg_rebuild_mesh_sah", "hg_rebuild_mesh_sah_device",
    "hg_set_mesh_vertices", "hg_deform_mesh", "hg_deform_mesh_device", "hg_set_mesh_skin", "hg_skin_mesh",
    "hg_skin_mesh_device", "hg_skin_vertices", "hg_mesh_vertices_readback",
    "hg_set_mesh_vertices_opt", "hg_vertex_normals",
]
# hg_deform_mesh / hg_skin_mesh: what follows the pack (Context.deform_mesh(how=...))
HG_DEFORM_REFIT, HG_DEFORM_REBUILD, HG_DEFORM_REBUILD_SAH = 0, 1, 2
DEFORM_KINDS = {"refit": HG_DEFORM_REFIT, "lbvh": HG_DEFORM_REBUILD, "sah": HG_DEFORM_REBUILD_SAH}
HG_DEFORM_NORMALS = 0x100  # OR-ed into `how`: the vertex normals are recomputed on the device (recompute_normals=True)
HG_BIND_ADJACENCY = 1  # hg_set_mesh_vertices_opt: what HG_DEFORM_NORMALS needs (set_mesh_vertices(adjacency=True))
HG_SKIN_LDS_BONES = 256  # csrc/hg_tunables.h: the largest bone palette the skin kernel keeps in LDS
# hg_scene_readback: the device scene's arrays (layouts private to the library, csrc/hg_layout.h)
HG_SCENE_NODES, HG_SCENE_LEAVES, HG_SCENE_TRIS, HG_SCENE_NORMALS, HG_SCENE_MESHES = 0, 1, 2, 3, 4
SCENE_ARRAYS = {"nodes": HG_SCENE_NODES, "leaves": HG_SCENE_LEAVES, "tris": HG_SCENE_TRIS,
                "normals": HG_SCENE_NORMALS, "meshes": HG_SCENE_MESHES}
HG_COMM_ID_BYTES = 128
HG_COMM_RCCL, HG_COMM_PEER = 1, 2
HG_SELFTEST_RCP = 1
HG_SELFTEST_BUILD = 2
HG_BUILD_CHECK_EXEC = 1
HG_BUILD_NO_REGEN_ITEMS = 2

_lib = None


def lib() -> C.CDLL:
    """Load libhalogen_hip.so (built in-tree by `make -C halogen-pathtracer_amd`).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} not built: run `make -C halogen-pathtracer_amd` (no CPU fallback exists)")
    L = C.CDLL(str(LIB_PATH))
    P = C.c_void_p
    i32, i64, sz, f32p = C.c_int32, C.c_int64, C.c_size_t, C.POINTER(C.c_float)
    sig = {
        "hg_abi_version": (C.c_int, []),
        "hg_create": (C.c_int, [C.c_int, C.POINTER(P)]),
        "hg_destroy": (None, [P]),
        "hg_last_error": (C.c_char_p, [P]),
        "hg_upload_scene": (C.c_int, [P, P, i32, P, i32, P, i32, P, i32, P, i32]),
        "hg_upload_scene_gen": (C.c_int, [P, C.c_uint64, P, i32, P, i32, P, i32, P, i32, P, i32]),
        "hg_upload_cubemap": (C.c_int, [P, i32, i32, P, sz]),
        "hg_set_params": (C.c_int, [P, C.POINTER(HgParams)]),
        "hg_resize": (C.c_int, [P, i32, i32]),
        "hg_set_tiling": (C.c_int, [P, i32, i32]),
        "hg_clear_accumulation": (C.c_int, [P]),
        "hg_render": (C.c_int, [P, i32, i32]),
        "hg_synchronize": (C.c_int, [P]),
        "hg_readback": (C.c_int, [P, f32p, sz]),
        "hg_readback_begin": (C.c_int, [P]),
        "hg_readback_end": (C.c_int, [P, C.POINTER(f32p), C.POINTER(sz)]),
        "hg_readback_begin_format": (C.c_int, [P, i32]),
        "hg_readback_end_data": (C.c_int, [P, C.POINTER(P), C.POINTER(sz), C.POINTER(i32)]),
        "hg_pack_display": (C.c_int, [f32p, sz, i32, P]),
        "hg_set_accumulation": (C.c_int, [P, f32p, sz, i32]),
        "hg_copy_tiles_device": (C.c_int, [P, P, sz]),
        "hg_local_tile_count": (i32, [P]),
        "hg_get_counters": (C.c_int, [P, C.POINTER(HgCounters)]),
        "hg_reset_counters": (C.c_int, [P]),
        "hg_set_option": (C.c_int, [P, i32, i32]),
        "hg_selftest": (i64, [P, i32, C.POINTER(i64)]),
        "hg_trace_rays": (C.c_int, [P, P, i64, i32, P]),
        "hg_trace_rays_device": (C.c_int, [P, P, i64, i32, P]),
        "hg_camera_rays": (C.c_int, [P, C.POINTER(HgParams), i32, P, i64, P]),
        "hg_update_guides": (C.c_int, [P, C.POINTER(HgParams), i32]),
        "hg_readback_guides": (C.c_int, [P, f32p, f32p, sz]),
        "hg_readback_begin_denoised": (C.c_int, [P, i32, C.POINTER(DenoiseParams)]),
        "hg_denoise_host": (C.c_int, [f32p, f32p, f32p, i32, i32, C.POINTER(DenoiseParams), f32p]),
        "hg_build_blas": (i64, [P, i32, P, i32, f32p, f32p, i32, P, i64]),
        "hg_build_blas_mt": (i64, [P, i32, P, i32, f32p, f32p, i32, P, i64, i32]),
        "hg_build_blas_sah": (i64, [P, i32, P, i32, i32, i32, P, i64]),
        "hg_unity_bounds": (None, [f32p, f32p, i32, f32p, f32p]),
        "hg_pack_triangles": (C.c_int, [P, P, i32, P, i32, P]),
        "hg_comm_unique_id": (C.c_int, [C.c_char_p]),
        "hg_comm_init_rank": (C.c_int, [P, i32, C.c_char_p, i32, C.POINTER(P)]),
        "hg_comm_init_all": (C.c_int, [C.POINTER(P), i32, C.POINTER(P)]),
        "hg_comm_gather": (C.c_int, [P, i32]),
        "hg_comm_synchronize": (C.c_int, [P]),
        "hg_comm_readback": (C.c_int, [P, f32p, sz]),
        "hg_comm_readback_begin": (C.c_int, [P, i32]),
        "hg_comm_readback_end": (C.c_int, [P, C.POINTER(P), C.POINTER(sz), C.POINTER(i32)]),
        "hg_comm_set_timeout_ms": (C.c_int, [P, i64]),
        "hg_comm_assemble_host": (C.c_int, [f32p, i64, i32, i32, i32, f32p, sz]),
        "hg_comm_transport": (C.c_int, [P]),
        "hg_comm_last_error": (C.c_char_p, [P]),
        "hg_comm_destroy": (None, [P]),
        "hg_refit_blas": (C.c_int, [P, i32, P, i32]),
        "hg_refit_mesh": (C.c_int, [P, i32, P, i32, C.c_uint64]),
        "hg_refit_mesh_device": (C.c_int, [P, i32, P, i32, C.c_uint64]),
        "hg_scene_readback": (C.c_int, [P, i32, P, sz, C.POINTER(sz)]),
        "hg_build_blas_lbvh": (i64, [P, i32, i32, P, P, P, i64]),
        "hg_rebuild_mesh": (C.c_int, [P, i32, P, i32, i32, P, C.c_uint64]),
        "hg_rebuild_mesh_device": (C.c_int, [P, i32, P, i32, i32, P, C.c_uint64]),
        "hg_build_blas_lbvh_sah": (i64, [P, i32, C.c_float, i64, P, P, P, i64, f32p]),
        "hg_rebuild_mesh_sah": (C.c_int, [P, i32, P, i32, C.c_float, P, C.c_uint64]),
        "hg_rebuild_mesh_sah_device": (C.c_int, [P, i32, P, i32, C.c_float, P, C.c_uint64]),
        "hg_set_mesh_vertices": (C.c_int, [P, i32, P, i32, i32]),
        "hg_deform_mesh": (C.c_int, [P, i32, P, P, i32, i32, i32, C.c_float, P, C.c_uint64]),
        "hg_deform_mesh_device": (C.c_int, [P, i32, P, P, i32, i32, i32, C.c_float, P, C.c_uint64]),
        "hg_set_mesh_skin": (C.c_int, [P, i32, P, P, P, P, i32, i32]),
        "hg_skin_mesh": (C.c_int, [P, i32, P, i32, i32, i32, C.c_float, P, C.c_uint64]),
        "hg_skin_mesh_device": (C.c_int, [P, i32, P, i32, i32, i32, C.c_float, P, C.c_uint64]),
        "hg_skin_vertices": (C.c_int, [P, P, P, P, i32, P, i32, P, P]),
        "hg_mesh_vertices_readback": (C.c_int, [P, i32, P, P, i32]),
        "hg_set_mesh_vertices_opt": (C.c_int, [P, i32, P, i32, i32, C.c_uint32]),
        "hg_vertex_normals": (C.c_int, [P, i32, P, i32, P]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if not os.environ.get("HALOGEN_LIB"):
                raise
            continue  # an older A/B build (tools/sweeps) without this entry point
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class HalogenError(RuntimeError):
    def __init__(self, msg: str, rc: int = 0):
        super().__init__(msg)
        self.rc = rc  # the HG_E_* code (0 when not from an entry point)


def _ptr(a) -> C.c_void_p:
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.cast(a, C.c_void_p)


def _display_view(ptr: C.c_void_p, n_bytes: int, fmt: int, w: int, h: int, copy: bool) -> np.ndarray:
    """A display image (hg_readback_end_data) as (h, w, 4) float32 / (h, w, 4) float16 / (h, w) uint32."""
    bpp = DISPLAY_BPP.get(fmt)
    if bpp is None or n_bytes != w * h * bpp:
        raise HalogenError(f"display readback: {n_bytes} bytes of format {fmt} for a {w}x{h} target")
    raw = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n_bytes,))
    if fmt == HG_DISPLAY_RGBA32F:
        view = raw.view(np.float32).reshape(h, w, 4)
    elif fmt == HG_DISPLAY_RGBA16F:
        view = raw.view(np.float16).reshape(h, w, 4)
    else:
        view = raw.view(np.uint32).reshape(h, w)
    return view.copy() if copy else view


def as_struct_array(struct_type, n: int):
    return (struct_type * max(n, 0))()


class Context:
    """One HIP device + stream (hg_ctx).  Not thread-safe; one per GPU."""

    def __init__(self, device: int = 0):
        L = lib()
        h = C.c_void_p()
        rc = L.hg_create(int(device), C.byref(h))
        if rc != HG_OK:
            raise HalogenError(f"hg_create(device={device}) failed with {rc} (no usable HIP device?)")
        self._h = h
        self.device = device
        self._size = None  # (w, h) of the last resize (guides())

    def _check(self, rc: int, what: str):
        if rc != HG_OK:
            msg = lib().hg_last_error(self._h)
            raise HalogenError(f"{what} failed ({rc}): {msg.decode() if msg else ''}", rc)

    def close(self):
        if getattr(self, "_h", None):
            lib().hg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- API -----------------------------------------------------------------------------------------
    def upload_scene(self, packed, generation: int = 0) -> None:
        """packed: halogen.scene.PackedScene (ctypes arrays of the reference structs).  generation: the caller's
        geometry generation (hg_upload_scene_gen; 0 = compare every array)."""
        self._check(lib().hg_upload_scene_gen(
            self._h, int(generation), _ptr(packed.spheres), len(packed.spheres), _ptr(packed.meshes), len(packed.meshes),
            _ptr(packed.materials), len(packed.materials), _ptr(packed.triangles), len(packed.triangles),
            _ptr(packed.blas), len(packed.blas)), "hg_upload_scene_gen")

    def upload_cubemap(self, face_size: int, n_mips: int, texels: np.ndarray) -> None:
        t = np.ascontiguousarray(texels, dtype=np.float32)
        self._check(lib().hg_upload_cubemap(self._h, face_size, n_mips, _ptr(t), t.size), "hg_upload_cubemap")

    def set_params(self, p: HgParams) -> None:
        self._check(lib().hg_set_params(self._h, C.byref(p)), "hg_set_params")

    def resize(self, w: int, h: int) -> None:
        self._check(lib().hg_resize(self._h, w, h), "hg_resize")
        self._size = (int(w), int(h))

    def set_tiling(self, rank: int, n_ranks: int) -> None:
        self._check(lib().hg_set_tiling(self._h, rank, n_ranks), "hg_set_tiling")

    def clear_accumulation(self) -> None:
        self._check(lib().hg_clear_accumulation(self._h), "hg_clear_accumulation")

    def render(self, n_frames: int, accumulate: bool = True) -> None:
        self._check(lib().hg_render(self._h, int(n_frames), 1 if accumulate else 0), "hg_render")

    def synchronize(self) -> None:
        self._check(lib().hg_synchronize(self._h), "hg_synchronize")

    def readback(self, w: int, h: int, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros((h, w, 4), dtype=np.float32)
        self._check(lib().hg_readback(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "hg_readback")
        return out

    def readback_begin(self, fmt: int | None = None, denoise: "DenoiseParams | None" = None) -> None:
        """hg_readback_begin(_format): enqueue the display readback of every frame rendered so far (at most
        HG_OPT_READBACK_DEPTH outstanding), as RGBA32F or another HG_DISPLAY_* format.  denoise: the image goes through
        the edge-avoiding a-trous filter first (hg_readback_begin_denoised; needs update_guides)."""
        if denoise is not None:
            self._check(lib().hg_readback_begin_denoised(self._h, HG_DISPLAY_RGBA32F if fmt is None else int(fmt),
                                                         C.byref(denoise)), "hg_readback_begin_denoised")
        elif fmt is None:
            self._check(lib().hg_readback_begin(self._h), "hg_readback_begin")
        else:
            self._check(lib().hg_readback_begin_format(self._h, int(fmt)), "hg_readback_begin_format")

    def readback_end(self, w: int, h: int, copy: bool = True) -> np.ndarray:
        """hg_readback_end_data: the image of the oldest begun readback, as (h, w, 4) float32 (RGBA32F), (h, w, 4)
        float16 (RGBA16F) or (h, w) uint32 (R11G11B10F).  copy=False returns a view of the context's pinned host image,
        valid until the depth-th readback_begin after the one it came from."""
        ptr, n, fmt = C.c_void_p(), C.c_size_t(0), C.c_int32(-1)
        self._check(lib().hg_readback_end_data(self._h, C.byref(ptr), C.byref(n), C.byref(fmt)), "hg_readback_end_data")
        return _display_view(ptr, n.value, fmt.value, w, h, copy)

    def set_accumulation(self, image: np.ndarray, frame_count: int) -> None:
        """Checkpoint resume (hg_set_accumulation): the (h, w, 4) image hg_readback returned and the FrameCount of
        the next frame."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        self._check(lib().hg_set_accumulation(self._h, img.ctypes.data_as(C.POINTER(C.c_float)), img.size,
                                              int(frame_count)), "hg_set_accumulation")

    def local_tile_count(self) -> int:
        return int(lib().hg_local_tile_count(self._h))

    def copy_tiles_device(self, dst_ptr: int, n_bytes: int) -> None:
        self._check(lib().hg_copy_tiles_device(self._h, C.c_void_p(dst_ptr), n_bytes), "hg_copy_tiles_device")

    def counters(self) -> dict:
        c = HgCounters()
        self._check(lib().hg_get_counters(self._h, C.byref(c)), "hg_get_counters")
        return c.as_dict()

    def reset_counters(self) -> None:
        self._check(lib().hg_reset_counters(self._h), "hg_reset_counters")

    def set_option(self, option: int, value: int) -> None:
        self._check(lib().hg_set_option(self._h, option, value), "hg_set_option")

    # --- ray queries (hg_trace_rays, hg_trace_rays_device, hg_camera_rays) --------------------------------------------
    def trace_rays(self, rays, mode="closest"):
        """Closest-hit ("closest") or occlusion ("any") query of n rays over the uploaded scene.

        rays on the host: an (n, 8) float32 array (origin xyz, t_max, unit direction xyz, 0) or a RAY_DTYPE array;
        returns a RAY_HIT_DTYPE array of n hits.  rays as a contiguous (n, 8) float32 torch tensor on the context's
        device: traced in place through the device entry point (no copy); returns an (n, 12) float32 tensor on that
        device, rows laid out as hg_ray_hit (view it as int32 for kind / object / primitive / material).  (A process
        that uses both imports torch before it creates its first Context, so that both share one HIP runtime.)"""
        m = RAY_MODES[mode] if isinstance(mode, str) else int(mode)
        if hasattr(rays, "data_ptr") and not isinstance(rays, np.ndarray):
            import torch

            if not (rays.is_cuda and rays.device.index == self.device and rays.dtype == torch.float32 and
                    rays.dim() == 2 and rays.shape[1] == 8 and rays.is_contiguous()):
                raise ValueError(f"device rays must be a contiguous (n, 8) float32 tensor on cuda:{self.device}")
            hits = torch.empty((rays.shape[0], 12), dtype=torch.float32, device=rays.device)
            torch.cuda.current_stream(rays.device).synchronize()  # the rays are complete before the call
            self._check(lib().hg_trace_rays_device(self._h, C.c_void_p(rays.data_ptr()), rays.shape[0], m,
                                                   C.c_void_p(hits.data_ptr())), "hg_trace_rays_device")
            return hits
        a = np.asarray(rays)
        if a.dtype != RAY_DTYPE:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != 8:
                raise ValueError(f"rays must be (n, 8) float32 or a RAY_DTYPE array, got {a.shape}")
        a = np.ascontiguousarray(a).reshape(-1) if a.dtype == RAY_DTYPE else a
        n = a.shape[0]
        hits = np.zeros(n, dtype=RAY_HIT_DTYPE)
        self._check(lib().hg_trace_rays(self._h, _ptr(a) if n else None, n, m, _ptr(hits) if n else None),
                    "hg_trace_rays")
        return hits

    def camera_rays(self, params: HgParams, frame_count: int, pixels) -> np.ndarray:
        """The first camera ray (sample 0) frame `frame_count` traces for each (x, y) of `pixels` ((n, 2) integers),
        as a RAY_DTYPE array with t_max = +inf (hg_camera_rays; `params` is explicit, the context's are not read)."""
        px = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1, 2)
        rays = np.zeros(px.shape[0], dtype=RAY_DTYPE)
        self._check(lib().hg_camera_rays(self._h, C.byref(params), int(frame_count), _ptr(px), px.shape[0], _ptr(rays)),
                    "hg_camera_rays")
        return rays

    # --- deforming geometry (hg_refit_mesh, hg_refit_mesh_device, hg_scene_readback) ----------------------------------
    def refit_mesh(self, mesh_index: int, triangles, generation: int = 0) -> None:
        """Replace the triangles of mesh `mesh_index` of the uploaded scene and refit its BVH boxes on the device,
        topology unchanged.  triangles on the host: a ctypes array of HalogenTriangle, or a numpy array of 72 bytes per
        triangle ((n, 18) float32).  triangles as a contiguous (n, 18) float32 torch tensor on the context's device: read
        in place through the device entry point.  generation: the geometry generation the next (vouched) upload_scene
        will carry.  The accumulation is not cleared."""
        keep, ptr, n, dev = self._triangles(triangles)  # (keep: what ptr points into, alive through the call)
        if dev:
            self._stream_done(keep)
            self._check(lib().hg_refit_mesh_device(self._h, int(mesh_index), ptr, n, int(generation)),
                        "hg_refit_mesh_device")
        else:
            self._check(lib().hg_refit_mesh(self._h, int(mesh_index), ptr, n, int(generation)), "hg_refit_mesh")

    def rebuild_mesh(self, mesh_index: int, triangles, leaf_size: int = 0, generation: int = 0):
        """Give mesh `mesh_index` of the uploaded scene a new tree over its moved triangles, built on the device in place
        (hg_rebuild_mesh, hg_rebuild_mesh_device): a linear BVH with leaves of `leaf_size` (0: the smallest of 4..15
        whose records fit the tree's capacity).  triangles: as refit_mesh takes them, in the mesh's current order.
        Returns the new order: order[k] is the index, in `triangles`, of the triangle now at position k; a torch int32
        tensor on the device for a torch tensor, a numpy int32 array otherwise.  The mesh's triangles are in that order
        from now on (later refit_mesh / rebuild_mesh calls, hg_ray_hit.primitive).  The accumulation is not cleared."""
        return self._rebuild("hg_rebuild_mesh", mesh_index, triangles, int(leaf_size), generation)

    def rebuild_mesh_sah(self, mesh_index: int, triangles, node_cost: float = 0.0, generation: int = 0):
        """rebuild_mesh with leaves chosen by surface area (hg_rebuild_mesh_sah, hg_rebuild_mesh_sah_device): the radix
        tree over single triangles, every subtree of at most 15 triangles made one leaf where that is no dearer at
        `node_cost` per inner node against 1 per leaf triangle (0: the library's value, doubled until the records fit
        the tree's capacity).  Arguments, the returned order and everything else as rebuild_mesh."""
        return self._rebuild("hg_rebuild_mesh_sah", mesh_index, triangles, float(node_cost), generation)

    def _rebuild(self, name, mesh_index, triangles, arg, generation):
        """hg_rebuild_mesh / hg_rebuild_mesh_sah (`arg`: the leaf size / the node cost), or the _device form for a
        torch tensor."""
        keep, ptr, n, dev = self._triangles(triangles)
        if dev:
            import torch

            order = torch.empty(n, dtype=torch.int32, device=keep.device)
            name, order_ptr = name + "_device", C.c_void_p(order.data_ptr())
            self._stream_done(keep)
        else:
            order = np.zeros(n, dtype=np.int32)
            order_ptr = _ptr(order)
        self._check(getattr(lib(), name)(self._h, int(mesh_index), ptr, n, arg, order_ptr, int(generation)), name)
        return order

    def _triangles(self, triangles):
        """`triangles` as (the array kept alive, pointer, count, is_device): a contiguous (n, 18) float32 torch tensor on
        the context's device (the caller waits for its stream, _stream_done), a numpy array of 72 bytes per triangle, or
        a ctypes array of HalogenTriangle"""
        if hasattr(triangles, "data_ptr") and not isinstance(triangles, np.ndarray):
            return self._device_floats(triangles, 18, "triangles")
        if isinstance(triangles, np.ndarray):
            a = np.ascontiguousarray(triangles)
            if a.nbytes % C.sizeof(HalogenTriangle):
                raise ValueError("triangles must hold 72 bytes per triangle")
            return a, _ptr(a), a.nbytes // C.sizeof(HalogenTriangle), False
        return triangles, _ptr(triangles), len(triangles), False

    @staticmethod
    def _stream_done(tensor) -> None:
        """Wait for torch's current stream on the tensor's device: what it holds is complete before the library reads it"""
        import torch

        torch.cuda.current_stream(tensor.device).synchronize()

    # --- deforming a mesh from its vertices (hg_set_mesh_vertices, hg_deform_mesh, hg_set_mesh_skin, hg_skin_mesh) ----
    def set_mesh_vertices(self, mesh_index: int, indices, n_vertices: int, adjacency: bool = False, flags=None) -> None:
        """Bind the index list of mesh `mesh_index` ((n, 3) integers: its triangles in their current order, as they were
        uploaded) to its tree on the device, for deform_mesh / skin_mesh.  The library keeps the list in step with every
        later rebuild of the tree; the binding lives until the next full upload of the scene.  adjacency=True
        (hg_set_mesh_vertices_opt, HG_BIND_ADJACENCY) also binds what recompute_normals=True of those calls needs: the
        vertices' face lists, built here on the host, and room for the normals.  `flags`: the call's flags as given."""
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        ip = _ptr(idx) if idx.size else None
        if not adjacency and flags is None:
            self._check(lib().hg_set_mesh_vertices(self._h, int(mesh_index), ip, idx.shape[0], int(n_vertices)),
                        "hg_set_mesh_vertices")
            return
        f = int(flags) if flags is not None else HG_BIND_ADJACENCY
        self._check(lib().hg_set_mesh_vertices_opt(self._h, int(mesh_index), ip, idx.shape[0], int(n_vertices), f),
                    "hg_set_mesh_vertices_opt")

    def _device_floats(self, a, cols, what):
        """`a` as (the array kept alive, pointer, rows, is_device): a contiguous (rows, cols) float32 torch tensor on the context's device
        (its stream synchronised: the data is complete before the call), or anything numpy takes"""
        if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray):
            import torch

            if not (a.is_cuda and a.device.index == self.device and a.dtype == torch.float32 and a.dim() == 2 and
                    a.shape[1] == cols and a.is_contiguous()):
                raise ValueError(f"device {what} must be a contiguous (n, {cols}) float32 tensor on cuda:{self.device}")
            return a, C.c_void_p(a.data_ptr()), a.shape[0], True
        h = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)
        return h, (_ptr(h) if h.size else None), h.shape[0], False

    def _n_bound_triangles(self, mesh_index: int) -> int:
        """The triangles from the mesh's offset to the next mesh's (or the scene's end) in the device scene: room for a
        rebuild's order, which is never longer (no other tree shares a rebuilt mesh's triangles)"""
        m = self.scene_readback("meshes").view(np.uint32).reshape(-1, 36)
        if not 0 <= int(mesh_index) < len(m):
            return 0  # (the entry point refuses the index before it writes an order)
        start = int(m[int(mesh_index), 17])
        later = [int(o) for o in m[:, 17] if int(o) > start]
        n = C.c_size_t(0)
        self._check(lib().hg_scene_readback(self._h, HG_SCENE_TRIS, None, 0, C.byref(n)), "hg_scene_readback")
        return (min(later) if later else n.value // 36) - start  # (the device keeps 9 floats a triangle)

    def _order_buffer(self, mesh_index, kind, source, dev):
        """(order, its pointer) for a deform of `kind` from `source`: a torch int32 tensor beside a device source (whose
        stream is synchronised here: the source is complete before the call), a numpy int32 array otherwise; (None, None)
        for a refit, which has no order"""
        order = order_ptr = None
        if kind != HG_DEFORM_REFIT:
            n_tris = self._n_bound_triangles(mesh_index)
            if dev:
                import torch

                order = torch.empty(n_tris, dtype=torch.int32, device=source.device)
                order_ptr = C.c_void_p(order.data_ptr())
            else:
                order = np.zeros(n_tris, dtype=np.int32)
                order_ptr = _ptr(order)
        if dev:
            self._stream_done(source)
        return order, order_ptr

    def deform_mesh(self, mesh_index: int, positions, normals=None, how="refit", leaf_size: int = 0,
                    node_cost: float = 0.0, generation: int = 0, recompute_normals: bool = False):
        """Move mesh `mesh_index` (bound by set_mesh_vertices) to new vertex positions and normals, (n_vertices, 3) float32
        each: the triangles are packed on the device from the bound index list, then the mesh's tree is refitted
        (how="refit": refit_mesh), rebuilt as a linear BVH (how="lbvh", leaf_size: rebuild_mesh) or rebuilt with leaves
        chosen by surface area (how="sah", node_cost: rebuild_mesh_sah).  Both arrays on the host (numpy), or both
        contiguous float32 torch tensors on the context's device, read in place.  The rebuild kinds return the new
        order as rebuild_mesh does (a torch int32 tensor for tensors, a numpy int32 array otherwise); "refit" returns
        None.  recompute_normals=True (HG_DEFORM_NORMALS; a binding with adjacency=True): the normals are recomputed
        on the device from the moved faces, vertex_normals' bits; `normals` is ignored and may be None."""
        kind = DEFORM_KINDS[how] if isinstance(how, str) else int(how)
        p, pp, n, dev = self._device_floats(positions, 3, "positions")
        q = qp = None
        if recompute_normals:
            kind |= HG_DEFORM_NORMALS
        elif normals is not None:
            q, qp, nq, dev_q = self._device_floats(normals, 3, "normals")
            if dev != dev_q or n != nq:
                raise ValueError("positions and normals must both be numpy arrays or both device tensors, of one length")
        order, order_ptr = self._order_buffer(mesh_index, kind & ~HG_DEFORM_NORMALS, p, dev)
        name = "hg_deform_mesh_device" if dev else "hg_deform_mesh"
        self._check(getattr(lib(), name)(self._h, int(mesh_index), pp, qp, n, kind, int(leaf_size), float(node_cost),
                                         order_ptr, int(generation)), name)
        return order

    def set_mesh_skin(self, mesh_index: int, rest_positions, rest_normals, bone_indices, weights, n_bones: int) -> None:
        """Give a bound mesh its rest pose ((n_vertices, 3) positions and normals) and influences ((n_vertices, 4) bone
        indices below n_bones and (n_vertices, 4) weights, used as given) for skin_mesh.  Host arrays."""
        p = np.ascontiguousarray(rest_positions, dtype=np.float32).reshape(-1, 3)
        q = np.ascontiguousarray(rest_normals, dtype=np.float32).reshape(-1, 3)
        b = np.asarray(bone_indices)
        if b.size and (b.min() < 0 or b.max() > 65535):
            raise ValueError("bone indices must fit 16 bits")
        b = np.ascontiguousarray(b, dtype=np.uint16).reshape(-1, 4)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
        if not (len(p) == len(q) == len(b) == len(w)):
            raise ValueError("rest positions, rest normals, bone indices and weights must hold one row per vertex")
        self._check(lib().hg_set_mesh_skin(self._h, int(mesh_index), _ptr(p), _ptr(q), _ptr(b), _ptr(w), len(p),
                                           int(n_bones)), "hg_set_mesh_skin")

    def skin_mesh(self, mesh_index: int, bones, how="refit", leaf_size: int = 0, node_cost: float = 0.0,
                  generation: int = 0, recompute_normals: bool = False):
        """Pose a skinned mesh (set_mesh_skin) by a bone palette, (n_bones, 12) float32: row-major 3 x 4 matrices, on the
        host or as a contiguous torch tensor on the context's device.  The vertices are skinned on the device
        (linear blend, abi.skin_vertices' arithmetic bit for bit) and then go the way of deform_mesh; `how`, the other
        arguments and the returned order are deform_mesh's.  recompute_normals=True: the skinned normals are replaced
        by those recomputed from the skinned positions (right for any bones, non-uniformly scaled ones too)."""
        kind = DEFORM_KINDS[how] if isinstance(how, str) else int(how)
        if recompute_normals:
            kind |= HG_DEFORM_NORMALS
        b, bp, n_bones, dev = self._device_floats(bones, 12, "bones")
        order, order_ptr = self._order_buffer(mesh_index, kind & ~HG_DEFORM_NORMALS, b, dev)
        name = "hg_skin_mesh_device" if dev else "hg_skin_mesh"
        self._check(getattr(lib(), name)(self._h, int(mesh_index), bp, n_bones, kind, int(leaf_size), float(node_cost),
                                         order_ptr, int(generation)), name)
        return order

    def mesh_vertices_readback(self, mesh_index: int, n_vertices: int) -> tuple[np.ndarray, np.ndarray]:
        """A diagnostic copy of the vertices the last skin_mesh of the mesh produced: (n_vertices, 3) float32 positions
        and normals."""
        p = np.zeros((int(n_vertices), 3), dtype=np.float32)
        q = np.zeros((int(n_vertices), 3), dtype=np.float32)
        self._check(lib().hg_mesh_vertices_readback(self._h, int(mesh_index), _ptr(p), _ptr(q), int(n_vertices)),
                    "hg_mesh_vertices_readback")
        return p, q

    def scene_readback(self, which) -> np.ndarray:
        """A diagnostic copy of one array of the device scene ("nodes", "leaves", "tris", "normals", "meshes" or an
        HG_SCENE_* value) as bytes: two contexts hold the same scene exactly when all five are equal."""
        w = SCENE_ARRAYS[which] if isinstance(which, str) else int(which)
        n = C.c_size_t(0)
        self._check(lib().hg_scene_readback(self._h, w, None, 0, C.byref(n)), "hg_scene_readback")
        out = np.zeros(n.value, dtype=np.uint8)
        self._check(lib().hg_scene_readback(self._h, w, _ptr(out) if n.value else None, n.value, C.byref(n)),
                    "hg_scene_readback")
        return out

    # --- denoised display (hg_update_guides, hg_readback_guides; readback_begin(denoise=...)) -------------------------
    def update_guides(self, params: HgParams, frame_count: int) -> None:
        """Trace the guide images (first-hit normal + distance, albedo + kind) of the camera rays frame `frame_count`
        traces under `params` (explicit, as in camera_rays); filterRadius = focalConeAngle = 0 gives guides that do not
        change from frame to frame."""
        self._check(lib().hg_update_guides(self._h, C.byref(params), int(frame_count)), "hg_update_guides")

    def guides(self) -> tuple[np.ndarray, np.ndarray]:
        """The guide images of the last update_guides: two (h, w, 4) float32 arrays, (normal.xyz, t) with t = +inf for
        a miss and (albedo.rgb, kind as 0.0 / 1.0 / 2.0)."""
        if self._size is None:
            raise HalogenError("guides: resize not called", HG_E_NOTARGET)
        w, h = self._size
        g0 = np.zeros((h, w, 4), dtype=np.float32)
        g1 = np.zeros((h, w, 4), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._check(lib().hg_readback_guides(self._h, g0.ctypes.data_as(fp), g1.ctypes.data_as(fp), g0.size),
                    "hg_readback_guides")
        return g0, g1

    def selftest(self, test: int = HG_SELFTEST_RCP) -> tuple[int, int]:
        """(mismatches, inputs tested) of a device arithmetic self-test."""
        tested = C.c_int64(0)
        r = lib().hg_selftest(self._h, test, C.byref(tested))
        if r < 0:
            self._check(int(r), "hg_selftest")
        return int(r), int(tested.value)


def comm_unique_id() -> bytes:
    """A fresh communicator id (hg_comm_unique_id): made once by the root process and sent to every rank."""
    buf = C.create_string_buffer(HG_COMM_ID_BYTES)
    rc = lib().hg_comm_unique_id(buf)
    if rc != HG_OK:
        raise HalogenError(f"hg_comm_unique_id failed ({rc})")
    return buf.raw


class Comm:
    """hg_comm: the multi-GPU gather of the ranks' tiles to a root.  Comm.rank(ctx, n, id, r) joins
    one process's rank (one process per GPU); Comm.all(ctxs) covers every rank of this process.  Destroy it (close)
    before its contexts."""

    def __init__(self, handle: C.c_void_p, ctxs):
        self._h = handle
        self._ctxs = list(ctxs)  # kept alive while the comm exists

    @classmethod
    def rank(cls, ctx: "Context", n_ranks: int, uid: bytes, rank: int) -> "Comm":
        h = C.c_void_p()
        rc = lib().hg_comm_init_rank(ctx._h, n_ranks, uid, rank, C.byref(h))
        if rc != HG_OK:
            msg = lib().hg_last_error(ctx._h)
            raise HalogenError(f"hg_comm_init_rank failed ({rc}): {msg.decode() if msg else ''}")
        return cls(h, [ctx])

    @classmethod
    def all(cls, ctxs) -> "Comm":
        arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
        h = C.c_void_p()
        rc = lib().hg_comm_init_all(arr, len(ctxs), C.byref(h))
        if rc != HG_OK:
            msg = lib().hg_last_error(ctxs[0]._h)
            raise HalogenError(f"hg_comm_init_all failed ({rc}): {msg.decode() if msg else ''}")
        return cls(h, ctxs)

    def _check(self, rc: int, what: str):
        if rc != HG_OK:
            msg = lib().hg_comm_last_error(self._h)
            raise HalogenError(f"{what} failed ({rc}): {msg.decode() if msg else ''}", rc)

    @property
    def transport(self) -> int:
        return int(lib().hg_comm_transport(self._h))

    def gather(self, root: int = 0) -> None:
        self._check(lib().hg_comm_gather(self._h, root), "hg_comm_gather")

    def synchronize(self) -> None:
        """Wait for this process's part of the last gather, bounded by the deadline (HalogenError on a dead peer)."""
        self._check(lib().hg_comm_synchronize(self._h), "hg_comm_synchronize")

    def set_timeout_ms(self, ms: int) -> None:
        self._check(lib().hg_comm_set_timeout_ms(self._h, int(ms)), "hg_comm_set_timeout_ms")

    def readback(self, w: int, h: int, out: np.ndarray | None = None) -> np.ndarray:
        if out is None:
            out = np.zeros((h, w, 4), dtype=np.float32)
        self._check(lib().hg_comm_readback(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size),
                    "hg_comm_readback")
        return out

    def readback_begin(self, fmt: int = HG_DISPLAY_RGBA32F) -> None:
        """hg_comm_readback_begin: the pipelined display of the last gather's image (into the root context's ring)."""
        self._check(lib().hg_comm_readback_begin(self._h, int(fmt)), "hg_comm_readback_begin")

    def readback_end(self, w: int, h: int, copy: bool = True) -> np.ndarray:
        """hg_comm_readback_end: the oldest begun display image (bounded wait), shaped as Context.readback_end's."""
        ptr, n, fmt = C.c_void_p(), C.c_size_t(0), C.c_int32(-1)
        self._check(lib().hg_comm_readback_end(self._h, C.byref(ptr), C.byref(n), C.byref(fmt)), "hg_comm_readback_end")
        return _display_view(ptr, n.value, fmt.value, w, h, copy)

    def close(self):
        if getattr(self, "_h", None):
            lib().hg_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def assemble_host(slabs: np.ndarray, width: int, height: int, n_ranks: int) -> np.ndarray:
    """hg_comm_assemble_host: (n_ranks, slab_tiles, 64, 4) float32 tiles (slab r = rank r's local tiles) -> the
    (height, width, 4) image, through the mapping the device gather uses (csrc/hg_tiling.h).  Needs no GPU."""
    s = np.ascontiguousarray(slabs, dtype=np.float32)
    if s.ndim != 4 or s.shape[0] != n_ranks or s.shape[2:] != (64, 4):
        raise ValueError(f"slabs must be (n_ranks={n_ranks}, slab_tiles, 64, 4), got {s.shape}")
    out = np.empty((height, width, 4), np.float32)
    fp = C.POINTER(C.c_float)
    rc = lib().hg_comm_assemble_host(s.ctypes.data_as(fp), s.shape[1], width, height, n_ranks, out.ctypes.data_as(fp),
                                     out.size)
    if rc != HG_OK:
        raise HalogenError(f"hg_comm_assemble_host failed ({rc}): slabs {s.shape} for {width}x{height}, {n_ranks} ranks")
    return out


def denoise_host(rgba: np.ndarray, guide0: np.ndarray, guide1: np.ndarray, params: DenoiseParams) -> np.ndarray:
    """hg_denoise_host: the display denoiser on the host (no device work), bit-identical to
    Context.readback_begin(denoise=params).  rgba, guide0, guide1: (h, w, 4) float32; returns (h, w, 4) float32."""
    img = np.ascontiguousarray(rgba, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f"denoise_host: rgba must be (h, w, 4), got {img.shape}")
    g0 = np.ascontiguousarray(guide0, dtype=np.float32)
    g1 = np.ascontiguousarray(guide1, dtype=np.float32)
    if g0.shape != img.shape or g1.shape != img.shape:
        raise ValueError(f"denoise_host: guides {g0.shape} {g1.shape} do not match the image {img.shape}")
    out = np.empty_like(img)
    fp = C.POINTER(C.c_float)
    rc = lib().hg_denoise_host(img.ctypes.data_as(fp), g0.ctypes.data_as(fp), g1.ctypes.data_as(fp), img.shape[1],
                               img.shape[0], C.byref(params), out.ctypes.data_as(fp))
    if rc != HG_OK:
        raise HalogenError(f"hg_denoise_host failed ({rc}): bad size or parameters", rc)
    return out


def refit_blas(triangles, nodes) -> None:
    """hg_refit_blas: rewrite, in place, the boxes of one mesh's tree (`nodes`: a ctypes array of BVHEntry, root at 0)
    from its triangles in tree order (a ctypes array of HalogenTriangle), topology unchanged: what the device holds after
    Context.refit_mesh of the same triangles.  Needs no GPU."""
    rc = lib().hg_refit_blas(_ptr(triangles), len(triangles), _ptr(nodes), len(nodes))
    if rc != HG_OK:
        raise HalogenError(f"hg_refit_blas failed ({rc}): a range, the depth or a cycle of the tree", rc)


def vertex_normals(positions, indices) -> np.ndarray:
    """hg_vertex_normals, the host twin of deform_mesh / skin_mesh with recompute_normals=True: area-weighted vertex
    normals of (n, 3) positions under an (m, 3) index list, each vertex's faces summed in the order of their index
    triples (csrc/hg_normals.h), so the result does not depend on the order of the list; (0, 0, 0) for a vertex no
    triangle with an area names.  Returns (n, 3) float32.  Needs no GPU."""
    p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
    out = np.empty_like(p)
    rc = lib().hg_vertex_normals(_ptr(p) if p.size else None, len(p), _ptr(idx) if idx.size else None, len(idx),
                                 _ptr(out) if out.size else None)
    if rc != HG_OK:
        raise HalogenError(f"hg_vertex_normals failed ({rc}): no vertices, no triangles, or an index outside the "
                           f"{len(p)} vertices", rc)
    return out


def skin_vertices(rest_positions, rest_normals, bone_indices, weights, bones):
    """hg_skin_vertices, the host twin of Context.skin_mesh: linear-blend skinning of (n, 3) rest positions and normals
    by (n, 4) bone indices and weights (used as given) over `bones`, (n_bones, 12) row-major 3 x 4 matrices.  Normals go
    through the 3 x 3 block (rigid and uniformly scaled bones) and are normalised where their length is not zero.
    Returns (positions, normals), (n, 3) float32 each.  Needs no GPU."""
    p = np.ascontiguousarray(rest_positions, dtype=np.float32).reshape(-1, 3)
    q = np.ascontiguousarray(rest_normals, dtype=np.float32).reshape(-1, 3)
    bi = np.asarray(bone_indices)
    if bi.size and (bi.min() < 0 or bi.max() > 65535):
        raise HalogenError("hg_skin_vertices: bone indices must fit 16 bits", HG_E_INVALID)
    bi = np.ascontiguousarray(bi, dtype=np.uint16).reshape(-1, 4)
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1, 4)
    b = np.ascontiguousarray(bones, dtype=np.float32).reshape(-1, 12)
    if not (len(p) == len(q) == len(bi) == len(w)):
        raise ValueError("rest positions, rest normals, bone indices and weights must hold one row per vertex")
    out_p, out_q = np.empty_like(p), np.empty_like(q)
    rc = lib().hg_skin_vertices(_ptr(p), _ptr(q), _ptr(bi), _ptr(w), len(p), _ptr(b), len(b), _ptr(out_p), _ptr(out_q))
    if rc != HG_OK:
        raise HalogenError(f"hg_skin_vertices failed ({rc}): no vertices, no bones, or a bone index not below "
                           f"{len(b)} bones", rc)
    return out_p, out_q


def build_blas_lbvh(triangles, leaf_size: int):
    """hg_build_blas_lbvh, the host twin of Context.rebuild_mesh: one mesh's triangles (a ctypes array of
    HalogenTriangle) -> (order, triangles in that order, nodes): a numpy int32 array and two ctypes arrays; the tree has
    its root at entry 0 and mesh-relative indices, as hg_upload_scene takes it.  Needs no GPU."""
    n = len(triangles)
    leaves = (n + int(leaf_size) - 1) // int(leaf_size) if 1 <= int(leaf_size) <= 15 else 1
    order = np.zeros(max(n, 1), dtype=np.int32)
    out = (HalogenTriangle * max(n, 1))()
    nodes = (BVHEntry * (2 * max(leaves, 1) - 1))()
    rc = lib().hg_build_blas_lbvh(_ptr(triangles), n, int(leaf_size), _ptr(order), _ptr(out), _ptr(nodes), len(nodes))
    if n == 0 or rc != len(nodes):
        raise HalogenError(f"hg_build_blas_lbvh failed ({rc}): no triangles, or leaf_size outside 1..15", int(rc))
    return order[:n], out, nodes


def build_blas_lbvh_sah(triangles, node_cost: float = 0.0, max_records: int = -1):
    """hg_build_blas_lbvh_sah, the host twin of Context.rebuild_mesh_sah: one mesh's triangles (a ctypes array of
    HalogenTriangle) -> (order, triangles in that order, nodes, the node cost used).  max_records plays the device
    tree's capacity (negative: no limit); node_cost 0 climbs the library's ladder until the records fit.  The tree has
    its root at entry 0 and 2M + 1 entries for M inner nodes.  Needs no GPU."""
    n = len(triangles)
    order = np.zeros(max(n, 1), dtype=np.int32)
    out = (HalogenTriangle * max(n, 1))()
    nodes = (BVHEntry * (2 * max(n, 1) - 1))()
    used = C.c_float(0.0)
    rc = lib().hg_build_blas_lbvh_sah(_ptr(triangles), n, float(node_cost), int(max_records), _ptr(order), _ptr(out),
                                      _ptr(nodes), len(nodes), C.byref(used))
    if rc < 1:
        raise HalogenError(f"hg_build_blas_lbvh_sah failed ({rc}): no triangles, a node cost that is negative or not "
                           f"finite, or more than {max_records} records", int(rc))
    fit = (BVHEntry * rc)()
    C.memmove(fit, nodes, C.sizeof(fit))
    return order[:n], out, fit, used.value


def pack_display(rgba: np.ndarray, fmt: int) -> np.ndarray:
    """hg_pack_display: (..., 4) float32 pixels in a display format on the host, the device's conversion (no GPU):
    (..., 4) float32, (..., 4) float16 or (...) uint32 (R11G11B10F)."""
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    if a.shape[-1] != 4:
        raise ValueError("rgba must have 4 channels")
    n = a.size // 4
    shape = {HG_DISPLAY_RGBA32F: (a.shape, np.float32), HG_DISPLAY_RGBA16F: (a.shape, np.float16),
             HG_DISPLAY_R11G11B10F: (a.shape[:-1], np.uint32)}
    if fmt not in shape:
        raise ValueError(f"unknown display format {fmt}")
    out = np.empty(*shape[fmt])
    rc = lib().hg_pack_display(a.ctypes.data_as(C.POINTER(C.c_float)), n, int(fmt), C.c_void_p(out.ctypes.data))
    if rc != HG_OK:
        raise HalogenError(f"hg_pack_display failed ({rc})")
    return out


def gpu_available() -> bool:
    """True when a HIP device is visible (without initialising torch)."""
    if os.environ.get("HIP_VISIBLE_DEVICES") == "":
        return False
    try:
        L = lib()
    except RuntimeError:
        return False
    h = C.c_void_p()
    if L.hg_create(0, C.byref(h)) != HG_OK:
        return False
    L.hg_destroy(h)
    return True
