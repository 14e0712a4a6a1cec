"""The hand-built scenes of tests/tree_cases.py (the deepest accepted tree, the leaf ladder, ties, extreme transforms;
tests/test_tree_cases.py shows on the CPU that they are what they claim) traced by everything that traverses: the three
megakernels, the render server, the guide kernel, the query kernel, and a refit of the tallest tree.  Every comparison is
with the CPU oracle and bit for bit; queries are compared word for word with hgo_intersect_batch, ties included.

chain62 has stack_depth 64: every lane's spill column (the stack entries beyond the 12 or 16 in LDS) is used down to its
last rows at each of the six places that size and address one."""
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  before the library's first context (tests/test_gpu_query.py has why)

import hg_oracle
import tree_cases as tc
from halogen import abi
from test_gpu_denoise import check_guides_against_queries, stable
from test_gpu_parity import KERNELS, assert_bitwise, gpu_render
from test_gpu_query import blended, words
from test_gpu_refit import assert_same_state, fresh_state, state

F = np.float32
FRAMES = 2
COUNTERS = ("rays", "tri_tests", "aabb_tests", "hits")


@lru_cache(maxsize=None)
def oracle_render(name, frames=FRAMES, debug="None"):
    """The oracle's image and counters of a case, computed once and never modified."""
    c = tc.case(name)
    img, cnt = hg_oracle.render(c.packed, c.params(1, DebugMode=debug), frames, True)
    img.setflags(write=False)
    return img, cnt


# ---- renders -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", tc.CASES)
def test_gpu_tree_case_matches_oracle(gpu, name, kernel):
    c = tc.case(name)
    ref, rcnt = oracle_render(name)
    img, cnt = gpu_render(c.packed, c.params(1), FRAMES, kernel=kernel)
    assert_bitwise(img, ref, f"{name} on {kernel}")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (name, kernel, k, cnt[k], rcnt[k])
    assert (ref[..., :3].max(-1) > 0).mean() > 0.05 and rcnt["hits"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("debug", ["Normal", "Albedo"])
@pytest.mark.parametrize("name", ["ties", "transforms"])
def test_gpu_tree_case_debug_views_match_oracle(gpu, name, debug):
    """The winner of every tie, and the normal under every matrix, as the views show them."""
    c = tc.case(name)
    ref, rcnt = oracle_render(name, 1, debug)
    img, cnt = gpu_render(c.packed, c.params(1, DebugMode=debug), 1)
    assert_bitwise(img, ref, f"{name} {debug}")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (name, debug, k, cnt[k], rcnt[k])


# ---- the render server ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("server", [None, 2], ids=["default", "forced"])
def test_gpu_chain62_through_the_render_server(gpu, server):
    """3 x hg_render(1) (the server's persistent waves, with their own spill buffer) = hg_render(3) = the oracle."""
    c = tc.case("chain62")
    params = c.params(1)
    ref, rcnt = oracle_render("chain62", 3)
    batched, bcnt = gpu_render(c.packed, params, 3)
    assert_bitwise(batched, ref, "hg_render(3)")
    with abi.Context(0) as ctx:
        if server is not None:
            ctx.set_option(abi.HG_OPT_SERVER, server)
        ctx.upload_scene(c.packed)
        ctx.resize(tc.W, tc.H)
        ctx.set_params(params)
        for _ in range(3):
            ctx.render(1, True)
        img = ctx.readback(tc.W, tc.H)
        cnt = ctx.counters()
    assert_bitwise(img, ref, "3 x hg_render(1)")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k] == bcnt[k], (k, cnt[k], rcnt[k], bcnt[k])
    assert cnt["last_kernel"] == abi.HG_KERNEL_MEGA_STREAM
    if server == 2:
        assert cnt["server_launches"] == 1 and cnt["server_frames"] == 3, cnt


# ---- guides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_chain62_guides(gpu):
    """hg_update_guides against the queries and against the oracle's Normal and Albedo views, as
    tests/test_gpu_denoise.py compares them."""
    c = tc.case("chain62")
    params = c.params(3)
    with abi.Context(0) as ctx:
        ctx.upload_scene(c.packed)
        ctx.resize(tc.W, tc.H)
        check_guides_against_queries(ctx, c.packed, params, 3, tc.W, tc.H)  # the very rays frame 3 traces
        g0, g1, hit = check_guides_against_queries(ctx, c.packed, stable(params), 3, tc.W, tc.H)
    for mode, col in (("Normal", (g0[..., :3] + F(1.0)) / F(2.0)), ("Albedo", g1[..., :3])):
        img, _ = hg_oracle.render(c.packed, stable(c.params(3, DebugMode=mode)), 1, True)
        want, got = blended(col), img.reshape(tc.H, tc.W, 4)[..., :3]
        bad = np.argwhere(hit & np.any(got.view(np.uint32) != want.view(np.uint32), axis=2))
        assert bad.size == 0, (mode, bad[:8])


# ---- queries -----------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def query_case(name):
    """The case's camera rays of frame 1 (the oracle's) and its special rays, with the oracle's answers."""
    c = tc.case(name)
    cam = hg_oracle.camera_rays(c.params(1), 1, tc.all_pixels())
    cam_hits = hg_oracle.intersect_batch(c.packed, cam)
    rays = np.concatenate([np.ascontiguousarray(cam).view(F).reshape(-1, 8),
                           tc.special_rays(c, dict(rays=cam, hits=cam_hits))])
    if len(rays) % 64 == 0:  # the last wave of the launch is a partial one
        rays = rays[:-1]
    want = hg_oracle.intersect_batch(c.packed, rays)
    rays.setflags(write=False)
    want.setflags(write=False)
    return cam, rays, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", tc.CASES)
def test_gpu_tree_case_queries_match_oracle(gpu, name):
    c = tc.case(name)
    cam, rays, want = query_case(name)
    assert len(rays) >= 64 * 5 + 1 and len(rays) % 64 != 0
    with abi.Context(0) as ctx:
        ctx.upload_scene(c.packed)
        got_cam = ctx.camera_rays(c.params(1), 1, tc.all_pixels())
        got = ctx.trace_rays(rays, "closest")
        occ = ctx.trace_rays(rays, "any")
    assert np.array_equal(words(got_cam), words(cam)), "hg_camera_rays against hgo_camera_rays"
    hit = want["kind"] != abi.HG_HIT_NONE
    special = np.arange(len(rays)) >= len(cam)
    print(f"{name}: {len(rays)} rays, {int(hit.sum())} hit ({int((hit & special).sum())} of {int(special.sum())} "
          f"special ones)")
    assert (hit & special).sum() >= 50 and (~hit & special).sum() >= 50
    bad = np.flatnonzero(np.any(words(got) != words(want), axis=1))
    assert bad.size == 0, (f"{name}: {bad.size} of {len(rays)} hit records differ ({int((words(got) != words(want)).sum())}"
                           f" words), first ray {bad[0]} {rays[bad[0]]}: got {got[bad[0]]} want {want[bad[0]]}")
    differ = np.flatnonzero((occ["kind"] != abi.HG_HIT_NONE) != hit)
    assert differ.size == 0, (name, "any-hit", differ[:8], rays[differ[:8]])


# ---- refit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_chain62_refit(gpu):
    """hg_refit_mesh on the tallest tree there can be (one launch per height): the device scene equals a fresh upload of
    hg_refit_blas's result, and one frame equals the oracle's."""
    c = tc.case("chain62")
    packed = c.packed
    t0, nt = c.info["chain_tris"]
    n0, nn = c.info["chain_nodes"]
    rng = np.random.default_rng(3)
    tris = tc.tris_np(packed).copy()
    tris[t0:t0 + nt, :9] += rng.normal(0, 0.05, (nt, 9)).astype(F)
    moved_t = (abi.HalogenTriangle * nt).from_buffer_copy(tris[t0:t0 + nt].tobytes())
    moved_n = (abi.BVHEntry * nn).from_buffer_copy(bytes(packed.blas)[32 * n0:32 * (n0 + nn)])
    abi.refit_blas(moved_t, moved_n)
    nodes = tc.bvh_np(packed).copy()
    before = nodes[n0:n0 + nn].copy()
    nodes[n0:n0 + nn] = np.frombuffer(bytes(moved_n), dtype=tc.BVH_DT)
    assert np.array_equal(nodes["indexA"], tc.bvh_np(packed)["indexA"]) and (nodes[n0:n0 + nn] != before).any()
    moved = type(packed)(spheres=packed.spheres, meshes=packed.meshes, materials=packed.materials,
                         triangles=(abi.HalogenTriangle * len(tris)).from_buffer_copy(tris.tobytes()),
                         blas=(abi.BVHEntry * len(nodes)).from_buffer_copy(nodes.tobytes()))
    params = c.params(1)
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        ctx.refit_mesh(c.info["chain_mesh"], moved_t)
        got = state(ctx)
        ctx.resize(tc.W, tc.H)
        ctx.set_params(params)
        ctx.render(1, True)
        img = ctx.readback(tc.W, tc.H)
        cnt = ctx.counters()
    assert_same_state(got, fresh_state(moved), "chain62 refitted")
    ref, rcnt = hg_oracle.render(moved, params, 1, True)
    assert_bitwise(img, ref, "chain62 refitted, 1 frame")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])
