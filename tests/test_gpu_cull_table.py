"""GPU parity over the cull table (csrc/hg_cull.h; hg_dev_isect.h mesh_live_mask walks it at every ray start).

Every kernel that starts a ray — stream, regen, lockstep (HG_OPT_KERNEL) and the ray queries, closest and occlusion —
against the CPU oracle, bit for bit and with equal work counters, at 64 x 36 with 1 and 3 frames, on the scenes where the
table has something to get wrong:
  c2        C2's nine meshes: every one has a single entry (an odd number of entries: the zero pad is fetched);
  odd       a leaf-root mesh and a singular-matrix mesh among cullable ones: no entry, always live;
  many      66 small cubes in the box, 75 meshes: entries for meshes below 64 only;
  moved     a mesh moved by a partial re-upload between two renders: the table is refreshed with the mesh records;
  refit     one refit of a mesh, then a render: the table follows the refitted root's children.
The ray queries are chained to the oracle as tests/test_gpu_query.py does: the camera rays of every pixel, traced by the
closest query, name the normals of the oracle's debug view and its primary misses; the occlusion query reports a hit
for exactly the same rays.  The oracle's images are computed once per scene and frame count and shared by the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before the library's first context (tests/test_gpu_query.py has why)

import hg_oracle
import refit_cases
from halogen import abi, render_pass as rp, scenes
from halogen.scene import PackedScene, RayTracingMesh
from halogen.unity import Transform
from test_gpu_mesh_paths import _cubes_scene
from test_gpu_parity import KERNELS, assert_bitwise

W, H = 64, 36
F = np.float32
KERNEL_NAMES = ["mega", "regen", "stream"]  # lockstep, regenerating, streaming
SCENES = ["c2", "odd", "many", "moved", "refit"]
_cache = {}


def _params(packed, first_frame=1):
    s = rp.clamp_settings(scenes.settings_for(scenes.CONFIGS["C1"]))
    return rp.make_params(s, scenes.cornell_camera(W, H), first_frame, len(packed.spheres), len(packed.meshes), False)


def _copy(packed):
    arrays = {}
    for k in ("spheres", "meshes", "materials", "triangles", "blas"):
        a = getattr(packed, k)
        b = (type(a)._type_ * len(a))()
        C.memmove(b, a, C.sizeof(a))
        arrays[k] = b
    return PackedScene(**arrays)


def _odd_scene():
    """The Cornell box plus a 3-triangle mesh (its root is a leaf), and interior cube 7 under a matrix that ignores
    world y (a zero column: not invertible, so the cube has no cull boxes and is an endless prism to every ray)."""
    sc = scenes.cornell_box()
    tris = np.random.default_rng(11).uniform(-0.6, 0.6, (3, 3, 3))
    sc.add(RayTracingMesh("few", *refit_cases._soup(tris), Transform((0.0, 0.4, 17.2), parent=Transform(scenes.CORNELL_ROOT))))
    packed = sc.pack()
    leaf = packed.meshes[len(packed.meshes) - 1]
    assert packed.blas[leaf.accelerationBufferOffset].triangleCount == 3
    for i in range(4, 8):
        packed.meshes[7].worldToLocal.m[i] = 0.0
    return packed


def scene_states(name):
    """The uploads / updates that lead to the scene's final state, as (before, apply(ctx), final packed arrays)."""
    if name not in _cache:
        if name == "c2":
            final = scenes.cornell_box().pack()
            assert len(final.meshes) == 9
            _cache[name] = (final, None, final)
        elif name == "odd":
            final = _odd_scene()
            _cache[name] = (final, None, final)
        elif name == "many":
            final = _cubes_scene(66)
            assert len(final.meshes) == 75
            _cache[name] = (final, None, final)
        elif name == "moved":
            before = scenes.cornell_box().pack()
            final = _copy(before)
            for k in (12, 13):  # interior cube 7 moved in world x and y: its matrix alone changes
                final.meshes[7].worldToLocal.m[k] += 0.35
                final.meshes[7].localToWorld.m[k] -= 0.35
            _cache[name] = (before, lambda ctx: ctx.upload_scene(final), final)
        else:
            sc = scenes.cornell_box()
            before = sc.pack()
            sc.meshes[7].deform(refit_cases.twist(sc.meshes[7].vertices, 0.9))
            final = sc.pack()
            tris = sc.meshes[7].packed_triangles
            _cache[name] = (before, lambda ctx: ctx.refit_mesh(7, tris), final)
    return _cache[name]


def oracle(name, frames):
    key = (name, frames)
    if key not in _cache:
        final = scene_states(name)[2]
        img, cnt = hg_oracle.render(final, _params(final), frames, True)
        img.setflags(write=False)
        _cache[key] = (img, cnt)
    return _cache[key]


def prepared(ctx, name):
    """The context brought to the scene's final state; where that takes an update, one frame is rendered before it, so
    the update meets a table that launches have used."""
    before, apply, final = scene_states(name)
    ctx.upload_scene(before)
    ctx.resize(W, H)
    if apply is not None:
        ctx.set_params(_params(before))
        ctx.render(1, True)
        uploads = ctx.counters()
        apply(ctx)
        if name == "moved":
            assert ctx.counters()["scene_uploads_partial"] == uploads["scene_uploads_partial"] + 1
        ctx.clear_accumulation()
        ctx.reset_counters()
    return final


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNEL_NAMES)
@pytest.mark.parametrize("name", SCENES)
def test_gpu_cull_table_render_matches_oracle(gpu, name, kernel):
    for frames in (1, 3):
        ref, rcnt = oracle(name, frames)
        with abi.Context(0) as ctx:
            ctx.set_option(abi.HG_OPT_KERNEL, KERNELS[kernel])
            final = prepared(ctx, name)
            ctx.set_params(_params(final))
            ctx.render(frames, True)
            img = ctx.readback(W, H)
            cnt = ctx.counters()
        assert_bitwise(img, ref, f"{name}, kernel {kernel}, {frames} frame(s)")
        for k in ("rays", "tri_tests", "aabb_tests", "hits"):
            assert cnt[k] == rcnt[k], (name, kernel, frames, k, cnt[k], rcnt[k])
        assert rcnt["hits"] > 0.3 * rcnt["paths"], "the scene is not in view: not a parity check"


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_gpu_cull_table_queries_match_oracle(gpu, name):
    with abi.Context(0) as ctx:
        final = prepared(ctx, name)
        params = _params(final, first_frame=3)
        px = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
        rays = ctx.camera_rays(params, 3, px)
        hits = ctx.trace_rays(rays, "closest")
        occ = ctx.trace_rays(rays, "any")
    hit = hits["kind"] != abi.HG_HIT_NONE
    differ = np.flatnonzero(hit != (occ["kind"] != abi.HG_HIT_NONE))
    assert differ.size == 0, (name, differ[:8], hits[differ[:8]], occ[differ[:8]])
    assert hit.mean() > 0.3

    def debug_view(mode):
        q = abi.HgParams.from_buffer_copy(params)
        q.halogenDebugMode, q.maxBounces = mode, 0
        return hg_oracle.render(final, q, 1, True)

    # the oracle's pixel after one accumulated frame at FrameCount 3 into a cleared target (tests/test_gpu_query.py)
    w = F(1.0) / F(3.0)
    img, _ = debug_view(2)
    want = F(0.0) * (F(1.0) - w) + ((hits["normal"] + F(1.0)) / F(2.0)).astype(F) * w
    got = img.reshape(-1, 4)[:, :3]
    bad = np.flatnonzero(hit & np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
    assert bad.size == 0, (name, "normal", bad[:8], got[bad[:8]], want[bad[:8]], hits[bad[:8]])
    _, cnt = debug_view(0)
    assert cnt["primary_misses"] == int((~hit).sum()), (name, cnt["primary_misses"], int((~hit).sum()))
