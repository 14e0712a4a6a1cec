"""Vertex normals recomputed on the device when a mesh deforms (hg_set_mesh_vertices_opt with HG_BIND_ADJACENCY,
HG_DEFORM_NORMALS in `how` of hg_deform_mesh* / hg_skin_mesh*; the two normal kernels of csrc/hg_deform.hip) on
tests/refit_cases.py's hazard scene (3, 100, 200 and 500 triangles; the grid's 286 vertices and 500 triangles make two
ragged workgroups in both passes) plus a fan of 300 triangles round one vertex as a fifth mesh (one lane's long list).

The check is tests/test_gpu_deform.py's: after a call the five arrays of the device scene equal, byte for byte, those of
a fresh context that uploaded the caller-side arrays, which RayTracingMesh.deform(..., normals="recompute") keeps current
through the host twin; after a rebuild, tests/test_gpu_rebuild.py's assert_same_scene."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch  # before the library's first context (tests/test_gpu_query.py has why)

import deform_cases as dc
import hg_oracle
import normals_cases as nc
import refit_cases
from halogen import abi, render_pass as rp, scenes
from test_gpu_deform import GRID, H, W, assert_same_state, dev, fresh_state, hazard_params, state, to_numpy
from test_gpu_parity import assert_bitwise
from test_gpu_rebuild import COUNTERS, assert_same_scene
from test_gpu_rebuild_sah import roomy

LIMIT = abi.HG_SKIN_LDS_BONES


def bind_all(ctx, sc, adjacency=True):
    for i, m in enumerate(sc.meshes):
        ctx.set_mesh_vertices(i, m.triangles, len(m.vertices), adjacency=adjacency)


# ---- 1. recompute + pack + refit ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "tensor", "tensor_off4"])
def test_gpu_recomputed_normals_state_equals_a_fresh_upload(gpu, how):
    """Each mesh in turn with the flag and no normals, the instanced grid through its second instance"""
    sc = nc.fan_scene()
    rest = [m.vertices.copy() for m in sc.meshes]
    assert [m.triangle_count for m in sc.meshes] == [3, 100, 200, 500, 300]
    assert len(sc.meshes[GRID].vertices) == 286 and len(sc.meshes[nc.FAN].vertices) == 301
    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        first = state(ctx)
        bind_all(ctx, sc)
        assert_same_state(state(ctx), first, "binding with adjacency changes nothing of the scene")
        steps = [(0, refit_cases.noise(rest[0], 0.3)), (1, refit_cases.twist(rest[1], 0.5)),
                 (2, refit_cases.noise(rest[2], 0.2)), (nc.GRID2, refit_cases.twist(rest[3], 0.9, axis=0)),
                 (nc.FAN, refit_cases.noise(rest[nc.FAN], 0.05, seed=4))]
        for n, (index, verts) in enumerate(steps):
            mesh = sc.meshes[GRID if index == nc.GRID2 else index]
            before = mesh.normals.copy()
            mesh.deform(verts, normals="recompute")
            assert not np.array_equal(mesh.normals, before)
            assert ctx.deform_mesh(index, dev(mesh.vertices, how), None, recompute_normals=True) is None
            assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), f"step {n}: mesh {index}")


# ---- 2. the frozen list and the permuted list across rebuilds ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "tensor"])
def test_gpu_recomputed_normals_across_rebuilds(gpu, how):
    """how="sah", how="lbvh", a direct rebuild_mesh and a flagged refit with new positions each time, never rebinding: the
    device sums over the list as it was bound, the twin over the list every rebuild permutes, and the scenes stay equal.
    Then a full upload, a binding of the permuted list, and one more flagged deform.  (The grid under the leaf-size-1
    tree of its rest pose, as tests/test_gpu_deform.py's "roomy" case has it and why.)"""
    sc = nc.fan_scene()
    mesh = roomy(sc.meshes[GRID])
    rest = mesh.vertices.copy()
    bound = mesh.triangles.copy()

    def flagged(index, **kw):
        return ctx.deform_mesh(index, dev(mesh.vertices, how), None, recompute_normals=True, **kw)

    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        bind_all(ctx, sc)

        mesh.deform(refit_cases.twist(rest, 0.5), normals="recompute", rebuild="sah", node_cost=0.5)
        cost = mesh.rebuild_node_cost
        got = to_numpy(flagged(GRID, how="sah", node_cost=cost))
        assert np.array_equal(got, abi.build_blas_lbvh_sah(mesh.rebuild_input, cost)[0])
        assert not np.array_equal(got, np.arange(len(got)))
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "after how='sah'")

        mesh.deform(refit_cases.twist(rest, 0.8, axis=0), normals="recompute", rebuild=True, leaf_size=4)
        got = to_numpy(flagged(GRID, how="lbvh", leaf_size=4))
        assert np.array_equal(got, abi.build_blas_lbvh(mesh.rebuild_input, 4)[0])
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "after how='lbvh'")

        mesh.deform(refit_cases.twist(rest, -0.6), normals="recompute", rebuild=True, leaf_size=15)
        got = ctx.rebuild_mesh(GRID, mesh.rebuild_input, 15)
        assert not np.array_equal(got, np.arange(len(got)))
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "after a direct rebuild_mesh")

        mesh.deform(refit_cases.noise(rest, 0.1, seed=6), normals="recompute")
        assert flagged(nc.GRID2) is None
        assert_same_scene(ctx, refit_cases.hazard_packed(sc), "a flagged refit in the rebuilt order")
        assert not np.array_equal(mesh.triangles, bound)

        ctx.upload_scene(refit_cases.hazard_packed(sc))  # in full: the bindings go
        with pytest.raises(abi.HalogenError, match="has no vertex binding"):
            flagged(GRID)
        ctx.set_mesh_vertices(GRID, mesh.triangles, len(mesh.vertices), adjacency=True)  # the permuted list
        mesh.deform(refit_cases.twist(rest, 0.3), normals="recompute")
        assert flagged(GRID) is None
        assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), "rebound with the permuted list")


# ---- 3. skin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["host", "tensor"])
@pytest.mark.parametrize("n_bones", [LIMIT, LIMIT + 1])
def test_gpu_skin_with_recomputed_normals(gpu, n_bones, how):
    """Palettes on both sides of the skin kernel's LDS limit, one bone scaled non-uniformly (where the skinned normals are
    wrong): the vertices read back are abi.skin_vertices' positions and abi.vertex_normals of those, bit for bit"""
    sc = nc.fan_scene()
    mesh = sc.meshes[GRID]
    nv = len(mesh.vertices)
    idx, w = dc.influences(nv, n_bones, seed=n_bones)
    idx[1::3, 0] = 1  # a third of the vertices under the scaled bone
    bones = dc.rigid_palette(n_bones, seed=3 * n_bones)
    bones[1] = dc.bone(dc.rotation([1, 0, 1], 0.3), (0.1, 0.0, 0.0), (1.0, 2.5, 0.5))
    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        bind_all(ctx, sc)
        ctx.set_mesh_skin(GRID, mesh.vertices, mesh.normals, idx, w, n_bones)
        mesh.set_skin(idx, w)
        assert ctx.skin_mesh(GRID, dev(bones, how), recompute_normals=True) is None
        got_p, got_n = ctx.mesh_vertices_readback(GRID, nv)
        want_p, skinned_n = abi.skin_vertices(mesh.rest_vertices, mesh.rest_normals, idx, w, bones)
        want_n = abi.vertex_normals(want_p, mesh.triangles)
        assert np.array_equal(nc.bits(got_p), nc.bits(want_p)), np.argwhere(nc.bits(got_p) != nc.bits(want_p))[:4]
        assert np.array_equal(nc.bits(got_n), nc.bits(want_n)), np.argwhere(nc.bits(got_n) != nc.bits(want_n))[:4]
        assert not np.array_equal(nc.bits(want_n), nc.bits(skinned_n))
        mesh.pose(bones, normals="recompute")
        assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), f"{n_bones} bones")
        # without the flag the skinned normals are back
        ctx.skin_mesh(GRID, dev(bones, how))
        assert np.array_equal(nc.bits(ctx.mesh_vertices_readback(GRID, nv)[1]), nc.bits(skinned_n))


# ---- 4. render ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def deformed():
    """The scene's rest arrays, the moved vertices of the plane and the grid, and the oracle's frame of the host arrays
    after deform(..., normals="recompute")"""
    sc = nc.fan_scene()
    rest = refit_cases.hazard_packed(sc)
    lists = {i: (sc.meshes[i].triangles.copy(), len(sc.meshes[i].vertices)) for i in (2, GRID)}
    moved = {2: refit_cases.noise(sc.meshes[2].vertices, 0.2), GRID: refit_cases.twist(sc.meshes[GRID].vertices, 0.9, axis=0)}
    for i, v in moved.items():
        sc.meshes[i].deform(v, normals="recompute")
    twin = refit_cases.hazard_packed(sc)
    params = hazard_params(twin)
    ref, rcnt = hg_oracle.render(twin, params, 1, True)
    ref.setflags(write=False)
    assert rcnt["hits"] > 0
    return rest, lists, moved, params, ref, rcnt


@pytest.mark.gpu
def test_gpu_recomputed_normals_image_matches_oracle(gpu):
    rest, lists, moved, params, ref, rcnt = deformed()
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        for i, (tris, nv) in lists.items():
            ctx.set_mesh_vertices(i, tris, nv, adjacency=True)
        ctx.deform_mesh(2, moved[2], None, recompute_normals=True)
        ctx.deform_mesh(GRID, torch.from_numpy(moved[GRID]).to("cuda:0"), None, recompute_normals=True)
        ctx.clear_accumulation()
        ctx.set_params(params)
        ctx.render(1, True)
        img = ctx.readback(W, H)
        cnt = ctx.counters()
    assert_bitwise(img, ref, "the hazard scene after flagged deforms")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_recomputed_normals_refusals(gpu):
    sc = nc.fan_scene()
    mesh = sc.meshes[GRID]
    nv = len(mesh.vertices)
    moved = refit_cases.twist(mesh.vertices, 0.4)

    def refused(call, text, rc=abi.HG_E_INVALID):
        with pytest.raises(abi.HalogenError) as e:
            call()
        assert e.value.rc == rc and text in str(e.value), (e.value.rc, str(e.value))

    with abi.Context(0) as ctx:
        ctx.upload_scene(refit_cases.hazard_packed(sc))
        first = state(ctx)
        L = abi.lib()
        # an unknown bind flag: nothing is bound
        refused(lambda: ctx.set_mesh_vertices(GRID, mesh.triangles, nv, flags=2), "unknown flags")
        refused(lambda: ctx.set_mesh_vertices(GRID, mesh.triangles, nv, flags=abi.HG_BIND_ADJACENCY | 0x80), "unknown flags")
        refused(lambda: ctx.deform_mesh(GRID, moved, None, recompute_normals=True), "has no vertex binding")
        # what hg_set_mesh_vertices refuses, with the flag
        refused(lambda: ctx.set_mesh_vertices(GRID, mesh.triangles[:-1], nv, adjacency=True), "mesh 3: 499 triangles")
        bad = mesh.triangles.copy()
        bad[123, 1] = nv
        refused(lambda: ctx.set_mesh_vertices(GRID, bad, nv, adjacency=True), f"index {nv} of triangle 123")
        # the flag on a binding made without adjacency
        ctx.set_mesh_vertices(GRID, mesh.triangles, nv)
        refused(lambda: ctx.deform_mesh(GRID, moved, None, recompute_normals=True), "hg_set_mesh_vertices_opt")
        refused(lambda: ctx.deform_mesh(GRID, moved, None, how="sah", recompute_normals=True), "hg_set_mesh_vertices_opt")
        t = torch.from_numpy(moved).to("cuda:0")
        refused(lambda: ctx.deform_mesh(GRID, t, None, recompute_normals=True), "hg_set_mesh_vertices_opt")
        idx, w = dc.influences(nv, 4)
        ctx.set_mesh_skin(GRID, mesh.vertices, mesh.normals, idx, w, 4)
        refused(lambda: ctx.skin_mesh(GRID, dc.rigid_palette(4), recompute_normals=True), "hg_set_mesh_vertices_opt")
        # no normals without the flag: today's refusal, on either kind of binding
        refused(lambda: ctx.deform_mesh(GRID, moved, None), "null position or normal array")
        ctx.set_mesh_vertices(GRID, mesh.triangles, nv, adjacency=True)
        refused(lambda: ctx.deform_mesh(GRID, moved, None), "null position or normal array")
        assert L.hg_deform_mesh(ctx._h, GRID, None, None, nv, abi.HG_DEFORM_NORMALS, 0, 0.0, None, 0) == abi.HG_E_INVALID
        assert b"null position array" in L.hg_last_error(ctx._h)
        # the flag is masked before the kind is checked
        refused(lambda: ctx.deform_mesh(GRID, moved, mesh.normals, how=7), "unknown kind of deform 7")
        refused(lambda: ctx.deform_mesh(GRID, moved, None, how=7, recompute_normals=True), "unknown kind of deform 7")
        refused(lambda: ctx.deform_mesh(GRID, moved[:-1], None, recompute_normals=True), f"{nv - 1} vertices, its binding holds {nv}")
        assert L.hg_deform_mesh_device(ctx._h, GRID, C.c_void_p(t.data_ptr() + 2), None, nv, abi.HG_DEFORM_NORMALS, 0, 0.0,
                                       None, 0) == abi.HG_E_INVALID
        assert b"4-byte aligned" in L.hg_last_error(ctx._h)
        # a plain binding after one with adjacency drops the adjacency
        ctx.set_mesh_vertices(GRID, mesh.triangles, nv)
        refused(lambda: ctx.deform_mesh(GRID, moved, None, recompute_normals=True), "hg_set_mesh_vertices_opt")
        assert_same_state(state(ctx), first, "after the refusals")
        # ... and the plain forms work on either binding, the flagged one ignores the normals it is given
        mesh.deform(moved)
        ctx.deform_mesh(GRID, mesh.vertices, mesh.normals)
        assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), "a plain deform on a plain binding")
        ctx.set_mesh_vertices(GRID, mesh.triangles, nv, adjacency=True)
        ctx.deform_mesh(nc.GRID2, mesh.vertices, mesh.normals)
        assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), "a plain deform on an adjacency binding")
        mesh.deform(moved, normals="recompute")
        ctx.deform_mesh(GRID, mesh.vertices, np.full_like(moved, 7), recompute_normals=True)
        assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), "given normals are ignored")


# ---- 6. the pass ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_render_pass_recompute_normals_is_the_default_pass(gpu):
    """HalogenRenderPass(vertex_deform=True, recompute_normals=True) against the default pass over one scene whose mesh is
    deformed with normals="recompute", rebuilt and deformed again between frames: bit-identical images at every stage;
    the recomputing pass sends positions alone for those deforms and positions and normals for a plain one"""
    cfg = scenes.CONFIGS["C1"].resized(40, 32, 3)
    scene, cam = cfg.build_scene(), cfg.camera()
    mesh = scene.meshes[7]
    rest, rest_n = mesh.vertices.copy(), mesh.normals.copy()
    passes = [rp.HalogenRenderPass(cfg.settings), rp.HalogenRenderPass(cfg.settings, vertex_deform=True, recompute_normals=True)]
    assert passes[1].vertex_deform and passes[1].recompute_normals and not passes[0].recompute_normals
    with pytest.raises(ValueError):
        rp.HalogenRenderPass(cfg.settings, recompute_normals=True, context=passes[0].ctx)
    sent = []
    plain = passes[1].ctx.deform_mesh

    def recording(index, positions, normals=None, **kw):
        sent.append((normals is None, bool(kw.get("recompute_normals"))))
        return plain(index, positions, normals, **kw)

    passes[1].ctx.deform_mesh = recording
    for p in passes:
        p.ctx.set_option(abi.HG_OPT_COUNTERS, 1)

    def frames(n, what):
        for p in passes:
            for _ in range(n):
                p.Execute(scene, cam)
        assert_bitwise(passes[1].read_image(), passes[0].read_image(), what)

    frames(2, "the rest pose")
    mesh.deform(refit_cases.twist(rest, 0.7), normals="recompute")
    frames(1, "after a recomputing deform")
    assert sent == [(True, True)]
    mesh.deform(refit_cases.twist(rest, 0.3), normals="recompute", rebuild="sah")
    frames(1, "after an SAH rebuild")
    mesh.deform(refit_cases.noise(rest, 0.02), normals="recompute")
    frames(2, "after a recomputing deform in the rebuilt order")
    assert sent == [(True, True), (True, True)]
    mesh.deform(rest, rest_n)
    frames(2, "after a plain deform")
    assert sent == [(True, True), (True, True), (False, False)]
    for p in passes:
        cnt = p.ctx.counters()
        assert cnt["scene_uploads"] - cnt["scene_uploads_partial"] == 1 and cnt["scene_uploads_vouched"] >= 1, cnt
        p.Dispose()
