"""Deforming a mesh from its vertices on the device (hg_set_mesh_vertices, hg_deform_mesh*, hg_set_mesh_skin,
hg_skin_mesh*, hg_mesh_vertices_readback; csrc/hg_deform.hip) on tests/refit_cases.py's hazard scene: 3 triangles under a
leaf root, 100 with a 40-triangle leaf-table leaf, the flat plane of 200 with shared vertices, and 500 triangles over 286
shared vertices instanced twice at a non-zero offset (two workgroups with ragged tails in the pack and the skin kernel).

The primary check is tests/test_gpu_refit.py's: after a call the five arrays of the device scene equal, byte for byte,
those of a fresh context that uploaded the caller-side arrays (RayTracingMesh.deform / pose keep them current).  After a
rebuild the record numbers differ from a fresh upload's (tests/test_gpu_rebuild.py has why), so there the comparison is
that file's assert_same_scene."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch  # before the library's first context (tests/test_gpu_query.py has why)

import deform_cases as dc
import hg_oracle
import refit_cases
from halogen import abi, render_pass as rp, scene as hs, scenes
from halogen.render_pass import Camera
from halogen.unity import Transform
from test_gpu_parity import KERNELS, assert_bitwise
from test_gpu_rebuild import COUNTERS, assert_same_scene
from test_gpu_rebuild_sah import roomy

ARRAYS = ("nodes", "leaves", "tris", "normals", "meshes")
GRID = 3  # the grid's mesh index; its second instance is mesh 4
W, H = 64, 36


def state(ctx):
    return {k: ctx.scene_readback(k) for k in ARRAYS}


def fresh_state(packed):
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        return state(ctx)


def assert_same_state(got, want, what):
    for k in ARRAYS:
        assert got[k].size == want[k].size, (what, k, got[k].size, want[k].size)
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {got[k].size} bytes, first at byte {bad[0]}"


def bind_all(ctx, sc):
    for i, m in enumerate(sc.meshes):
        ctx.set_mesh_vertices(i, m.triangles, len(m.vertices))


def dev(a, how):
    """The (n, k) float32 array as deform_mesh takes it: itself, a tensor, or a tensor that starts 4 bytes past a 16-byte
    boundary"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if how == "host":
        return a
    if how == "tensor":
        return torch.from_numpy(a).to("cuda:0")
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def to_numpy(order):
    return order.cpu().numpy() if hasattr(order, "cpu") else order


def hazard_params(packed, frames=1):
    cfg = scenes.CONFIGS["C1"].resized(W, H, frames)
    s = rp.clamp_settings(scenes.settings_for(cfg))
    cam = Camera(Transform((1.5, 0.0, -1.0), (0, 0, 0, 1)), 60.0, W, H)  # the meshes sit at z = 6 .. 10
    return rp.make_params(s, cam, 1, len(packed.spheres), len(packed.meshes), False)


# ---- 1. pack + refit ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "tensor", "tensor_off4"])
def test_gpu_deform_refit_state_equals_a_fresh_upload(gpu, how):
    """The steps of test_gpu_refit_state_equals_a_fresh_upload, from vertices: each mesh in turn, one twice, the instanced
    tree through both instances, then all back to the rest pose"""
    sc = refit_cases.hazard_scene()
    rest = [m.vertices.copy() for m in sc.meshes]
    packed = refit_cases.hazard_packed(sc)
    assert [m.triangle_count for m in sc.meshes] == [3, 100, 200, 500] and len(sc.meshes[GRID].vertices) == 286
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        first = state(ctx)
        bind_all(ctx, sc)
        assert_same_state(state(ctx), first, "binding changes nothing of the scene")
        steps = [(0, refit_cases.noise(rest[0], 0.3)), (1, refit_cases.twist(rest[1], 0.5)),
                 (2, refit_cases.noise(rest[2], 0.2)), (3, refit_cases.twist(rest[3], 0.9, axis=0)),
                 (1, refit_cases.noise(rest[1], 0.05, seed=2)), (4, refit_cases.noise(rest[3], 0.1, seed=3))]
        steps += [(i, rest[i]) for i in range(4)]
        for n, (index, verts) in enumerate(steps):
            mesh = sc.meshes[min(index, 3)]
            mesh.deform(verts)
            assert ctx.deform_mesh(index, dev(mesh.vertices, how), dev(mesh.normals, how)) is None
            assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), f"step {n}: mesh {index}")
        assert_same_state(state(ctx), first, "back at the rest pose")


# ---- 2. the bound list follows every rebuild ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "tensor"])
@pytest.mark.parametrize("trees", ["roomy", "as_built"])
@pytest.mark.parametrize("index", [1, GRID])
def test_gpu_deform_order_tracking(gpu, index, trees, how):
    """deform_mesh(how="sah"), deform_mesh(how="lbvh"), a direct rebuild_mesh and a plain deform_mesh with new vertices
    each time, the index list never touched on the caller's side: after every step the device holds the twin's scene
    (RayTracingMesh.deform with the same arguments) and the returned order is the twin's.

    The leaf size of the "lbvh" step: 4 needs n / 4 - 1 records, which the hazard scene's own trees do not have after an
    SAH rebuild (mesh 1: 24 against 11, the grid: 124 against 75; RayTracingMesh.deform refuses it), so "roomy" uploads
    the mesh under the leaf-size-1 radix tree of its rest pose (n - 1 records) and rebuilds by surface area at node cost
    0.5, which keeps 85 and 409 inner nodes, and "as_built" keeps the scene's trees and the automatic node cost,
    the leaf-table leaf of mesh 1 among them, and rebuilds at leaf size 15.  The last deform of the grid goes through
    its second instance."""
    sc = refit_cases.hazard_scene()
    mesh = sc.meshes[index]
    if trees == "roomy":
        roomy(mesh)
    leaf = 4 if trees == "roomy" else 15
    rest = mesh.vertices.copy()
    through = 4 if index == GRID else index
    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        bind_all(ctx, sc)

        mesh.deform(refit_cases.twist(rest, 0.5), rebuild="sah", node_cost=0.5 if trees == "roomy" else 0.0)
        cost = mesh.rebuild_node_cost
        want = abi.build_blas_lbvh_sah(mesh.rebuild_input, cost)[0]
        got = to_numpy(ctx.deform_mesh(index, dev(mesh.vertices, how), dev(mesh.normals, how), how="sah", node_cost=cost))
        assert got.dtype == np.int32 and np.array_equal(got, want) and not np.array_equal(got, np.arange(len(got)))
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "after how='sah'")

        mesh.deform(refit_cases.twist(rest, 0.8, axis=0), rebuild=True, leaf_size=leaf)
        want = abi.build_blas_lbvh(mesh.rebuild_input, leaf)[0]
        got = to_numpy(ctx.deform_mesh(index, dev(mesh.vertices, how), dev(mesh.normals, how), how="lbvh", leaf_size=leaf))
        assert np.array_equal(got, want) and not np.array_equal(got, np.arange(len(got)))
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "after how='lbvh'")

        mesh.deform(refit_cases.noise(rest, 0.05, seed=4))
        assert ctx.deform_mesh(index, dev(mesh.vertices, how), dev(mesh.normals, how)) is None
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "a plain deform in the rebuilt order")

        # a rebuild from packed triangles, called directly, between two deform_mesh calls
        mesh.deform(refit_cases.twist(rest, -0.6), rebuild=True, leaf_size=15)
        got = ctx.rebuild_mesh(index, mesh.rebuild_input, 15)
        assert not np.array_equal(got, np.arange(len(got)))
        mesh.deform(refit_cases.noise(rest, 0.1, seed=6))
        ctx.deform_mesh(through, dev(mesh.vertices, how), dev(mesh.normals, how))
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "a plain deform after a direct rebuild_mesh")


# ---- 3. skin --------------------------------------------------------------------------------------------------------------------
LIMIT = abi.HG_SKIN_LDS_BONES


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "tensor"])
@pytest.mark.parametrize("n_bones", [1, 4, LIMIT, LIMIT + 1])
def test_gpu_skin_is_the_twins(gpu, n_bones, how):
    """The grid (286 vertices: two workgroups, the second of 30 lanes) under palettes on both sides of the LDS limit: the
    skinned vertices are abi.skin_vertices' bit for bit, the device scene is a fresh upload's after mesh.pose(bones)"""
    sc = refit_cases.hazard_scene()
    mesh = sc.meshes[GRID]
    nv = len(mesh.vertices)
    idx, w = dc.influences(nv, n_bones, seed=n_bones)
    assert idx.max() == n_bones - 1
    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        bind_all(ctx, sc)
        ctx.set_mesh_skin(GRID, mesh.vertices, mesh.normals, idx, w, n_bones)
        mesh.set_skin(idx, w)
        for pose in range(2):
            bones = dc.rigid_palette(n_bones, seed=10 * n_bones + pose)
            assert ctx.skin_mesh(GRID + pose, dev(bones, how)) is None  # (the second pose through the second instance)
            got_p, got_n = ctx.mesh_vertices_readback(GRID, nv)
            want_p, want_n = abi.skin_vertices(mesh.rest_vertices, mesh.rest_normals, idx, w, bones)
            assert np.array_equal(dc.bits(got_p), dc.bits(want_p)), np.argwhere(dc.bits(got_p) != dc.bits(want_p))[:4]
            assert np.array_equal(dc.bits(got_n), dc.bits(want_n)), np.argwhere(dc.bits(got_n) != dc.bits(want_n))[:4]
            assert np.array_equal(dc.bits(want_p), dc.bits(dc.skin_numpy(mesh.rest_vertices, mesh.rest_normals, idx, w, bones)[0]))
            mesh.pose(bones)
            assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), f"{n_bones} bones, pose {pose}")


# ---- 4. render ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def posed():
    """The hazard scene's rest arrays; the grid posed (a refit) and mesh 1 posed with an SAH rebuild on the host; the
    oracle's frame of the twin's arrays.  Built once, shared by the kernels."""
    sc = refit_cases.hazard_scene()
    rest = refit_cases.hazard_packed(sc)
    params = hazard_params(rest)
    skins = {}
    for i, n_bones in ((GRID, 6), (1, 3)):
        m = sc.meshes[i]
        idx, w = dc.influences(len(m.vertices), n_bones, seed=i)
        # (mesh 1 is a soup of unshared vertices under random influences: a mild palette keeps its triangles small
        # enough for an SAH tree within the 15 inner entries of its uploaded tree)
        bones = dc.rigid_palette(n_bones, seed=20 + i, swing=0.3 if i == 1 else 0.5, shift=0.1 if i == 1 else 0.3)
        skins[i] = (m.vertices.copy(), m.normals.copy(), m.triangles.copy(), idx, w, bones)
        m.set_skin(idx, w)
    sc.meshes[GRID].pose(skins[GRID][5])
    sc.meshes[1].pose(skins[1][5], rebuild="sah")
    cost = sc.meshes[1].rebuild_node_cost
    twin = refit_cases.hazard_packed(sc)
    ref, rcnt = hg_oracle.render(twin, params, 1, True)
    ref.setflags(write=False)
    pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    hits = hg_oracle.intersect_batch(twin, hg_oracle.camera_rays(params, 1, pixels))
    seen = np.bincount(hits["object"][hits["kind"] == abi.HG_HIT_MESH], minlength=len(twin.meshes))
    assert seen[1] > 0 and seen[GRID] > 0, seen  # the camera sees both posed meshes
    return rest, params, skins, cost, ref, rcnt


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_gpu_skinned_scene_matches_oracle(gpu, kernel):
    rest, params, skins, cost, ref, rcnt = posed()
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_KERNEL, KERNELS[kernel])
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        for i, (v, n, tris, idx, w, bones) in skins.items():
            ctx.set_mesh_vertices(i, tris, len(v))
            ctx.set_mesh_skin(i, v, n, idx, w, len(bones))
        ctx.skin_mesh(GRID, skins[GRID][5])
        order = ctx.skin_mesh(1, torch.from_numpy(skins[1][5]).to("cuda:0"), how="sah", node_cost=cost)
        assert order.dtype == torch.int32 and sorted(order.cpu().tolist()) == list(range(100))
        ctx.clear_accumulation()
        ctx.set_params(params)
        ctx.render(1, True)
        img = ctx.readback(W, H)
        cnt = ctx.counters()
    assert_bitwise(img, ref, f"posed hazard scene, {kernel}")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])


# ---- 5. degenerate indices ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_deform_degenerate_triangle(gpu):
    """A bound list with a triangle that names one vertex three times (a point: a thin box, padded)"""
    sc = refit_cases.hazard_scene()
    g = sc.meshes[GRID]
    tris = g.triangles.copy()
    tris[7] = tris[7][0]
    sc.meshes[GRID] = hs.RayTracingMesh("grid", g.vertices, g.normals, tris, g.transform)
    mesh = sc.meshes[GRID]
    assert (mesh.triangles[:, 0] == mesh.triangles[:, 1]).sum() == 1
    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        ctx.set_mesh_vertices(GRID, mesh.triangles, len(mesh.vertices))
        mesh.deform(refit_cases.twist(mesh.vertices, 0.7))
        ctx.deform_mesh(GRID, mesh.vertices, mesh.normals)
        assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), "a degenerate triangle")


# ---- 6. refusals and the binding's lifetime ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_deform_refusals_and_lifetime(gpu):
    sc = refit_cases.hazard_scene()
    packed = refit_cases.hazard_packed(sc)
    mesh = sc.meshes[GRID]
    nv = len(mesh.vertices)
    idx, w = dc.influences(nv, 4)
    bones = dc.rigid_palette(4)

    def refused(ctx, call, text, rc=abi.HG_E_INVALID):
        with pytest.raises(abi.HalogenError) as e:
            call()
        assert e.value.rc == rc and text in str(e.value), (e.value.rc, str(e.value))

    with abi.Context(0) as ctx:
        refused(ctx, lambda: ctx.set_mesh_vertices(GRID, mesh.triangles, nv), "hg_upload_scene not called", abi.HG_E_NOSCENE)
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals), "hg_upload_scene not called", abi.HG_E_NOSCENE)
        ctx.upload_scene(packed, generation=3)
        first = state(ctx)
        # no binding yet
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals), "has no vertex binding")
        refused(ctx, lambda: ctx.set_mesh_skin(GRID, mesh.vertices, mesh.normals, idx, w, 4), "has no vertex binding")
        refused(ctx, lambda: ctx.skin_mesh(GRID, bones), "has no vertex binding")
        refused(ctx, lambda: ctx.mesh_vertices_readback(GRID, nv), "has no vertex binding")
        # what a binding refuses
        refused(ctx, lambda: ctx.set_mesh_vertices(GRID, mesh.triangles[:-1], nv), "mesh 3: 499 triangles")
        refused(ctx, lambda: ctx.set_mesh_vertices(9, mesh.triangles, nv), "out of range")
        bad = mesh.triangles.copy()
        bad[123, 1] = nv
        refused(ctx, lambda: ctx.set_mesh_vertices(GRID, bad, nv), f"index {nv} of triangle 123 is outside the {nv} vertices")
        bad[123, 1] = -1
        refused(ctx, lambda: ctx.set_mesh_vertices(GRID, bad, nv), "index -1 of triangle 123")
        refused(ctx, lambda: ctx.set_mesh_vertices(GRID, mesh.triangles, 0), "0 vertices")
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals), "has no vertex binding")
        ctx.set_mesh_vertices(GRID, mesh.triangles, nv)
        # bound: the deform's own refusals, and those of what follows the pack
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices[:-1], mesh.normals[:-1]), f"{nv - 1} vertices, its binding holds {nv}")
        refused(ctx, lambda: ctx.deform_mesh(4, mesh.vertices[:-1], mesh.normals[:-1]), f"{nv - 1} vertices, its binding holds {nv}")
        refused(ctx, lambda: ctx.deform_mesh(1, mesh.vertices, mesh.normals), "mesh 1 has no vertex binding")
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals, how=7), "unknown kind of deform 7")
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals, how="lbvh", leaf_size=16), "leaf_size 16")
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals, how="lbvh", leaf_size=1),
                "capacity", abi.HG_E_UNSUPPORTED)
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals, how="sah", node_cost=-1.0), "node_cost")
        L = abi.lib()
        v = torch.from_numpy(mesh.vertices).to("cuda:0")
        p = C.c_void_p(v.data_ptr())
        assert L.hg_deform_mesh(ctx._h, GRID, None, mesh.normals.ctypes.data, nv, 0, 0, 0.0, None, 0) == abi.HG_E_INVALID
        assert b"null position or normal array" in L.hg_last_error(ctx._h)
        assert L.hg_deform_mesh_device(ctx._h, GRID, p, None, nv, 0, 0, 0.0, None, 0) == abi.HG_E_INVALID
        assert L.hg_deform_mesh_device(ctx._h, GRID, C.c_void_p(v.data_ptr() + 2), p, nv, 0, 0, 0.0, None, 0) == abi.HG_E_INVALID
        assert b"4-byte aligned" in L.hg_last_error(ctx._h)
        # a skin's refusals
        refused(ctx, lambda: ctx.skin_mesh(GRID, bones), "has no skin")
        over = idx.copy()
        over[200, 3] = 4  # = n_bones
        refused(ctx, lambda: ctx.set_mesh_skin(GRID, mesh.vertices, mesh.normals, over, w, 4), "bone index 4 of vertex 200 is not below the 4 bones")
        refused(ctx, lambda: ctx.set_mesh_skin(GRID, mesh.vertices[:-1], mesh.normals[:-1], idx[:-1], w[:-1], 4), "its binding holds")
        refused(ctx, lambda: ctx.skin_mesh(GRID, bones), "has no skin")
        ctx.set_mesh_skin(GRID, mesh.vertices, mesh.normals, idx, w, 4)
        mesh.set_skin(idx, w)  # (the same rest pose)
        refused(ctx, lambda: ctx.mesh_vertices_readback(GRID, nv), "has not been skinned")
        refused(ctx, lambda: ctx.skin_mesh(GRID, dc.rigid_palette(5)), "5 bones, its skin was bound with 4")
        assert L.hg_skin_mesh(ctx._h, GRID, None, 4, 0, 0, 0.0, None, 0) == abi.HG_E_INVALID
        assert b"null bone palette" in L.hg_last_error(ctx._h)
        assert_same_state(state(ctx), first, "after the refusals")
        assert ctx.counters()["scene_uploads"] == 1

        # a vouched upload (the refit's generation, a mesh record moved) keeps the binding and the skin
        mesh.deform(refit_cases.twist(mesh.vertices, 0.4))
        ctx.deform_mesh(GRID, mesh.vertices, mesh.normals, generation=3)
        moved = refit_cases.hazard_packed(sc)
        moved.meshes[1].worldToLocal.m[12] += np.float32(0.05)
        before = ctx.counters()
        ctx.upload_scene(moved, generation=3)
        after = ctx.counters()
        assert after["scene_uploads_vouched"] == before["scene_uploads_vouched"] + 1, after
        mesh.deform(refit_cases.twist(mesh.vertices, -0.2))
        ctx.deform_mesh(4, mesh.vertices, mesh.normals, generation=3)
        ctx.skin_mesh(GRID, bones, generation=3)
        mesh.pose(bones)
        now = refit_cases.hazard_packed(sc)
        now.meshes[1].worldToLocal.m[12] += np.float32(0.05)
        assert_same_state(state(ctx), fresh_state(now), "binding and skin after a vouched upload")
        # a full upload of changed arrays drops the binding
        sc2 = refit_cases.hazard_scene()
        sc2.meshes[2].deform(refit_cases.noise(sc2.meshes[2].vertices, 0.1))
        changed = refit_cases.hazard_packed(sc2)
        ctx.upload_scene(changed)
        assert ctx.counters()["scene_uploads"] - ctx.counters()["scene_uploads_partial"] == 2
        dropped = state(ctx)
        refused(ctx, lambda: ctx.deform_mesh(GRID, mesh.vertices, mesh.normals), "has no vertex binding")
        refused(ctx, lambda: ctx.skin_mesh(GRID, bones), "has no vertex binding")
        assert_same_state(state(ctx), dropped, "after a deform without the dropped binding")
        assert_same_state(dropped, fresh_state(changed), "the full upload")


# ---- 7. the pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_render_pass_vertex_deform_is_the_default_pass(gpu):
    """HalogenRenderPass(vertex_deform=True) against the default pass over one scene whose mesh is deformed, posed,
    rebuilt and deformed again between frames: bit-identical images at every stage, and no second full upload"""
    cfg = scenes.CONFIGS["C1"].resized(40, 32, 3)
    scene, cam = cfg.build_scene(), cfg.camera()
    mesh = scene.meshes[7]
    rest = mesh.vertices.copy()
    idx, w = dc.influences(len(rest), 3, seed=9)
    mesh.set_skin(idx, w)
    passes = [rp.HalogenRenderPass(cfg.settings), rp.HalogenRenderPass(cfg.settings, vertex_deform=True)]
    assert not passes[0].vertex_deform and passes[1].vertex_deform
    for p in passes:
        p.ctx.set_option(abi.HG_OPT_COUNTERS, 1)

    def frames(n, what):
        for p in passes:
            for _ in range(n):
                p.Execute(scene, cam)
        assert_bitwise(passes[1].read_image(), passes[0].read_image(), what)

    frames(2, "the rest pose")
    mesh.deform(refit_cases.twist(rest, 0.7))
    frames(1, "after a deform")
    mesh.pose(dc.rigid_palette(3, seed=1))
    frames(2, "after a pose")
    mesh.deform(refit_cases.twist(rest, 0.3), rebuild="sah")
    frames(1, "after an SAH rebuild")
    mesh.deform(refit_cases.noise(rest, 0.02))  # from the vertices, through the list the device permuted
    frames(3, "after a deform in the rebuilt order")
    for p in passes:
        cnt = p.ctx.counters()
        assert cnt["scene_uploads"] - cnt["scene_uploads_partial"] == 1 and cnt["scene_uploads_vouched"] >= 1, cnt
        p.Dispose()
