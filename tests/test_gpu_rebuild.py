"""Device rebuild of one mesh's BVH (hg_rebuild_mesh, hg_rebuild_mesh_device; csrc/hg_lbvh.hip) against the host twin
(hg_build_blas_lbvh, tests/test_lbvh.py) and the CPU oracle on the twin's arrays.  The scene is the Cornell box with the
8.7k dragon as its third mesh (a non-zero triangle offset and first record), 64 x 64 pixels, 2 frames.

The twin's arrays come from RayTracingMesh.deform(rebuild=True), which runs hg_build_blas_lbvh and keeps the scene's
pack() current; the device gets the rebuild's own input (the moved triangles in the order before the rebuild).  Record
numbers differ between a rebuilt context and a fresh upload of the twin's arrays (Karras' numbering against the
packer's), so trees are compared by a walk from the root ref: shape, leaf refs, the 24 box floats of every record."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch  # before the library's first context (tests/test_gpu_query.py has why)

import cases
import hg_oracle
import refit_cases
from halogen import abi, render_pass as rp, scene as hs, scenes
from halogen.render_pass import Camera
from halogen.unity import Transform, unity_cube
from test_gpu_parity import GOLD, KERNELS, assert_bitwise

W = H = 64
FRAMES = 2
DI = 2  # the dragon's mesh index
LEAF = 0x80000000
COUNTERS = ("rays", "tri_tests", "aabb_tests", "hits")


def dragon_scene():
    sc = scenes.dragon_cornell(1)
    sc.meshes.insert(DI, sc.meshes.pop())
    return sc


@lru_cache(maxsize=None)
def uniforms():
    cfg = scenes.CONFIGS["C3"].resized(W, H, FRAMES)
    s = rp.clamp_settings(scenes.settings_for(cfg))
    assert not s["UseEnvironmentCubemap"]
    sc = dragon_scene()
    return rp.make_params(s, cfg.camera(), 1, len(sc.spheres), len(sc.meshes), False)


def tris18(tris):
    return np.frombuffer(bytes(tris), dtype=np.float32).reshape(-1, 18).copy()


def on_device(tris):
    return torch.from_numpy(tris18(tris)).to("cuda:0")


def walk(ctx, mesh_index):
    """(root is a leaf, the tree under the mesh's root ref in pre-order): ('leaf', ref) and ('node', the record's 24 box
    floats as bytes, child A is a leaf, child B is a leaf)."""
    rec = ctx.scene_readback("nodes").view(np.uint32).reshape(-1, 16)
    root = int(ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[mesh_index, 16])
    out, stack = [], [root]
    while stack:
        r = stack.pop()
        if r & LEAF:
            out.append(("leaf", r))
            continue
        q = rec[r]
        assert q[11] == 0 and q[15] == 0, (r, q)
        a, b = int(q[3]), int(q[7])
        out.append(("node", q[[0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]].tobytes(), bool(a & LEAF), bool(b & LEAF)))
        stack += [b, a]
        assert len(out) < 1 << 20
    return bool(root & LEAF), out


def assert_same_scene(ctx, packed, what):
    """The context holds the scene a fresh context holds after a full upload of `packed`: triangles and normals byte for
    byte, every mesh's tree by the walk, every mesh record but its root's record number."""
    with abi.Context(0) as fresh:
        fresh.upload_scene(packed)
        for k in ("tris", "normals"):
            got, want = ctx.scene_readback(k), fresh.scene_readback(k)
            assert got.size == want.size and np.array_equal(got, want), \
                f"{what}: {k} differ in {np.count_nonzero(got != want) if got.size == want.size else 'size'}"
        gm = ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)
        wm = fresh.scene_readback("meshes").view(np.uint32).reshape(-1, 36)
        assert gm.shape == wm.shape
        keep = [k for k in range(36) if k != 16]
        assert np.array_equal(gm[:, keep], wm[:, keep]), (what, np.argwhere(gm[:, keep] != wm[:, keep])[:4])
        for mi in range(len(gm)):
            got, want = walk(ctx, mi), walk(fresh, mi)
            assert got[0] == want[0] and len(got[1]) == len(want[1]), (what, mi, len(got[1]), len(want[1]))
            bad = [k for k, (g, w) in enumerate(zip(got[1], want[1])) if g != w]
            assert not bad, f"{what}: mesh {mi}: {len(bad)} of {len(got[1])} tree entries differ, first at {bad[0]}"
        return fresh.counters()


def render(ctx, params, frames=FRAMES):
    ctx.clear_accumulation()
    ctx.set_params(params)
    ctx.render(frames, True)
    return ctx.readback(W, H)


@lru_cache(maxsize=None)
def twisted(leaf_size, frames=FRAMES):
    """The dragon twisted and rebuilt at leaf_size on the host: the rest scene's arrays, the rebuild's input, the twin's
    order, the twin scene's arrays and the oracle's render of them.  Built once, shared."""
    sc = dragon_scene()
    rest = sc.pack()
    assert rest.meshes[DI].triangleBufferOffset > 0 and rest.meshes[DI].accelerationBufferOffset > 0
    dragon = sc.meshes[DI]
    assert dragon.triangle_count == 8712
    dragon.deform(refit_cases.twist(dragon.vertices, 0.5), rebuild=True, leaf_size=leaf_size)
    order, _, _ = abi.build_blas_lbvh(dragon.rebuild_input, dragon.rebuild_leaf)
    assert not np.array_equal(order, np.arange(len(order)))
    twin = sc.pack()
    ref, rcnt = hg_oracle.render(twin, uniforms(), frames, True)
    ref.setflags(write=False)
    return rest, dragon.rebuild_input, dragon.rebuild_leaf, order, twin, ref, rcnt


# ---- 1. the same tree as the twin ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host_pointer", "device_pointer"])
@pytest.mark.parametrize("leaf_size", [4, 15])
def test_gpu_rebuild_is_the_twins_tree(gpu, leaf_size, device):
    rest, moved, L, order, twin, _, _ = twisted(leaf_size)
    assert L == leaf_size
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        first_record = int(ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[DI, 16])
        assert first_record > 0 and not first_record & LEAF
        got = ctx.rebuild_mesh(DI, on_device(moved) if device else moved, leaf_size)
        got = got.cpu().numpy() if device else got
        assert got.dtype == np.int32 and np.array_equal(got, order)
        assert int(ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[DI, 16]) == first_record
        assert_same_scene(ctx, twin, f"dragon rebuilt at L={leaf_size}")


@pytest.mark.gpu
def test_gpu_rebuild_auto_leaf_size(gpu):
    """leaf_size 0 on the dragon picks 4: 2,177 records fit the span of BVHGenerator's tree (leaves of at most 5)."""
    rest, moved, _, order, twin, _, _ = twisted(4)
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        got = ctx.rebuild_mesh(DI, moved, 0)
        assert np.array_equal(got, order)
        assert_same_scene(ctx, twin, "dragon rebuilt at the automatic leaf size")


# ---- 2. image parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_gpu_rebuild_matches_oracle(gpu, kernel):
    rest, moved, L, _, twin, ref, rcnt = twisted(4)
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_KERNEL, KERNELS[kernel])
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        ctx.rebuild_mesh(DI, on_device(moved), L)
        img = render(ctx, uniforms())
        cnt = ctx.counters()
    assert_bitwise(img, ref, f"rebuilt dragon, {kernel}")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (kernel, k, cnt[k], rcnt[k])
    if kernel == "auto":  # 6. the stack depth: the automatic kernel choice is a fresh upload's
        with abi.Context(0) as fresh:
            fresh.upload_scene(twin)
            fresh.resize(W, H)
            assert_bitwise(render(fresh, uniforms()), ref, "the twin's arrays, fresh")
            assert fresh.counters()["last_kernel"] == cnt["last_kernel"] != 0


@pytest.mark.gpu
def test_gpu_rebuild_through_the_render_server(gpu):
    rest, moved, L, _, twin, ref, rcnt = twisted(4, 3)
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_SERVER, 2)
        ctx.set_option(abi.HG_OPT_COALESCE, 32)
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        ctx.clear_accumulation()
        ctx.set_params(uniforms())
        ctx.render(1, True)  # a frame of the rest pose posted to the server: the rebuild stops it
        ctx.rebuild_mesh(DI, on_device(moved), L)
        before = ctx.counters()  # (the rest pose's frame is not the oracle's)
        ctx.clear_accumulation()
        ctx.set_params(uniforms())
        for _ in range(3):
            ctx.render(1, True)
        img = ctx.readback(W, H)
        cnt = ctx.counters()
        assert cnt["server_frames"] > before["server_frames"]
    assert_bitwise(img, ref, "three frames through the render server after a rebuild")
    for k in COUNTERS:
        assert cnt[k] - before[k] == rcnt[k], ("render server", k, cnt[k] - before[k], rcnt[k])


@pytest.mark.gpu
def test_gpu_rebuild_queries_match_oracle(gpu):
    rest, moved, L, order, twin, _, _ = twisted(4)
    pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    cam = hg_oracle.camera_rays(uniforms(), 1, pixels)
    want = hg_oracle.intersect_batch(twin, cam)
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.rebuild_mesh(DI, on_device(moved), L)
        got = ctx.trace_rays(cam, "closest")
    on_dragon = (want["kind"] == abi.HG_HIT_MESH) & (want["object"] == DI)
    assert on_dragon.sum() > 100
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    bad = np.flatnonzero(np.any(g != w, axis=1))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


# ---- 3. sequences ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sequence", ["rebuild_refit", "refit_rebuild", "rebuild_rebuild"])
def test_gpu_rebuild_sequences(gpu, sequence):
    sc = dragon_scene()
    dragon = sc.meshes[DI]
    rest_vertices = dragon.vertices.copy()
    steps = {"rebuild_refit": [(0.5, 4), (0.8, None)], "refit_rebuild": [(0.4, None), (0.7, 4)],
             "rebuild_rebuild": [(0.5, 4), (0.9, 6)]}[sequence]
    with abi.Context(0) as ctx:
        ctx.upload_scene(sc.pack())
        ctx.resize(W, H)
        for n, (strength, leaf_size) in enumerate(steps):
            moved = refit_cases.twist(rest_vertices, strength)
            if leaf_size:
                dragon.deform(moved, rebuild=True, leaf_size=leaf_size)
                ctx.rebuild_mesh(DI, on_device(dragon.rebuild_input), dragon.rebuild_leaf)
            else:
                dragon.deform(moved)  # repacked in the mesh's current order: the last rebuild's
                ctx.refit_mesh(DI, on_device(dragon.packed_triangles))
            twin = sc.pack()
            assert_same_scene(ctx, twin, f"{sequence}, step {n}")
        img = render(ctx, uniforms(), 1)
    with abi.Context(0) as fresh:
        fresh.upload_scene(twin)
        fresh.resize(W, H)
        assert_bitwise(img, render(fresh, uniforms(), 1), f"{sequence}: one frame against a fresh upload")


# ---- 4. edge meshes ---------------------------------------------------------------------------------------------------------------
def edge_scene():
    """tests/refit_cases.py's hazard scene (few, cluster, the flat plane, the grid) plus Unity's cube; hazard_packed adds
    the grid's second instance as the last mesh record."""
    sc = refit_cases.hazard_scene()
    sc.add(hs.RayTracingMesh("cube", *unity_cube(), Transform((3.0, 1.0, 8.0))))
    return sc


def edge_params(packed):
    """C1's settings with a camera in front of the edge scene's meshes (they sit at z = 6 .. 10)."""
    cfg = scenes.CONFIGS["C1"].resized(W, H, 1)
    s = rp.clamp_settings(scenes.settings_for(cfg))
    cam = Camera(Transform((1.5, 0.0, -1.0), (0, 0, 0, 1)), 60.0, W, H)
    return rp.make_params(s, cam, 1, len(packed.spheres), len(packed.meshes), False)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["cube_one_leaf", "identical", "flat_plane", "instances"])
def test_gpu_rebuild_edge_meshes(gpu, what):
    sc = edge_scene()
    packed = refit_cases.hazard_packed(sc)
    index, leaf_size = {"cube_one_leaf": (4, 15), "identical": (1, 0), "flat_plane": (2, 0), "instances": (3, 0)}[what]
    mesh = sc.meshes[index]
    assert packed.meshes[index].triangleBufferOffset > 0
    v = mesh.vertices.copy()
    if what == "identical":  # the unshared vertices of every triangle moved onto one triangle
        v[:] = np.tile(np.float32([[0.25, 0.5, 1.0], [1.25, 0.5, 1.0], [0.25, 1.5, 2.0]]), (len(v) // 3, 1))
    elif what == "instances":
        v = refit_cases.twist(v, 0.9, axis=0)
    params = edge_params(packed)
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        ctx.resize(W, H)
        before = ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36).copy()
        assert not before[index, 16] & LEAF and before[index, 19] == 1  # an inner root, cullable
        mesh.deform(v, rebuild=True, leaf_size=leaf_size)
        K = (mesh.triangle_count + mesh.rebuild_leaf - 1) // mesh.rebuild_leaf
        order = ctx.rebuild_mesh(index, mesh.rebuild_input, mesh.rebuild_leaf)
        assert np.array_equal(order, abi.build_blas_lbvh(mesh.rebuild_input, mesh.rebuild_leaf)[0])
        after = ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36).copy()
        twin = refit_cases.hazard_packed(sc)
        assert_same_scene(ctx, twin, what)
        if what == "cube_one_leaf":
            assert K == 1 and after[index, 16] == (LEAF | 12 << 27 | packed.meshes[index].triangleBufferOffset)
            assert after[index, 19] == 0 and not after[index, 20:].any()  # the root became a leaf: not cullable
        else:
            assert K > 1 and after[index, 19] == 1
        if what == "identical":
            assert np.array_equal(order, np.arange(len(order)))  # every key ties: the caller's order
        if what == "flat_plane":
            assert len(set(tris18(mesh.packed_triangles)[:, [1, 4, 7]].ravel().tolist())) == 1  # flat in y
        if what == "instances":  # both instances' cull boxes moved, each under its own matrix
            last = len(after) - 1
            assert after[last, 16] == after[index, 16] and after[last, 17] == after[index, 17]
            assert (after[index, 20:] != before[index, 20:]).any() and (after[last, 20:] != before[last, 20:]).any()
            assert (after[index, 20:] != after[last, 20:]).any()
        img = render(ctx, params, 1)
        pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
        hits = ctx.trace_rays(ctx.camera_rays(params, 1, pixels), "closest")
    seen = np.bincount(hits["object"][hits["kind"] == abi.HG_HIT_MESH], minlength=len(twin.meshes))
    assert seen[index] > 0, (what, seen)  # the camera sees the rebuilt mesh
    with abi.Context(0) as fresh:
        fresh.upload_scene(twin)
        fresh.resize(W, H)
        assert_bitwise(img, render(fresh, params, 1), f"{what}: one frame against a fresh upload")


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_rebuild_refusals_leave_the_scene(gpu):
    """Every refusal's code; the device scene and the continued accumulation stay as they were."""
    _, params, _, frames, _ = cases.setup("c1_64")
    sc = scenes.cornell_box()
    rest = sc.pack()
    gold = np.load(GOLD / "c1_64.npz")["image"]
    cube = sc.meshes[7]
    tris, n = cube.packed_triangles, len(cube.packed_triangles)
    # capacity, chosen on the CPU: the tree's record span is its inner entries plus at most one pad per pair of inner
    # siblings (hg_pack_geometry), and leaves of one triangle need n - 1 records
    inner = sum(1 for e in cube.bvh if e.triangleCount == 0)
    span_bound = inner + (inner - 1) // 2
    assert inner >= 1 and n - 1 > span_bound, (n, inner)
    assert (n + 5) // 6 - 1 <= inner  # leaf size 6 fits: the refusals below that use it are not the capacity's
    L = abi.lib()
    dev = on_device(tris)
    order = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")

    def refused(ctx, call, rc, text):
        got = call()
        msg = L.hg_last_error(ctx._h).decode()
        assert got == rc and text in msg, (got, msg)

    with abi.Context(0) as ctx:
        refused(ctx, lambda: L.hg_rebuild_mesh(ctx._h, 7, C.cast(tris, C.c_void_p), n, 4, None, 0), abi.HG_E_NOSCENE,
                "hg_upload_scene not called")
        ctx.upload_scene(rest)
        ctx.resize(64, 64)
        ctx.clear_accumulation()
        ctx.set_params(params)
        ctx.render(2, True)
        first = {k: ctx.scene_readback(k) for k in ("nodes", "leaves", "tris", "normals", "meshes")}
        p, d = C.cast(tris, C.c_void_p), C.c_void_p(dev.data_ptr())
        refused(ctx, lambda: L.hg_rebuild_mesh(ctx._h, 7, p, n, 1, None, 0), abi.HG_E_UNSUPPORTED,
                f"{n - 1} records at leaf size 1, the tree's capacity is")
        refused(ctx, lambda: L.hg_rebuild_mesh_device(ctx._h, 7, d, n, 1, None, 0), abi.HG_E_UNSUPPORTED, "capacity")
        refused(ctx, lambda: L.hg_rebuild_mesh(ctx._h, 7, p, n - 1, 4, None, 0), abi.HG_E_INVALID,
                f"mesh 7: {n - 1} triangles")
        refused(ctx, lambda: L.hg_rebuild_mesh_device(ctx._h, 7, d, n - 1, 4, None, 0), abi.HG_E_INVALID,
                f"mesh 7: {n - 1} triangles")
        refused(ctx, lambda: L.hg_rebuild_mesh_device(ctx._h, 7, C.c_void_p(dev.data_ptr() + 2), n, 6, None, 0),
                abi.HG_E_INVALID, "4-byte aligned")
        refused(ctx, lambda: L.hg_rebuild_mesh_device(ctx._h, 7, d, n, 6, C.c_void_p(order.data_ptr() + 1), 0),
                abi.HG_E_INVALID, "4-byte aligned")
        refused(ctx, lambda: L.hg_rebuild_mesh(ctx._h, 7, p, n, 16, None, 0), abi.HG_E_INVALID, "leaf_size 16")
        refused(ctx, lambda: L.hg_rebuild_mesh(ctx._h, 7, None, n, 4, None, 0), abi.HG_E_INVALID, "null triangle array")
        refused(ctx, lambda: L.hg_rebuild_mesh(ctx._h, 99, p, n, 4, None, 0), abi.HG_E_INVALID, "out of range")
        for k, v in first.items():
            assert np.array_equal(ctx.scene_readback(k), v), f"{k} changed by a refused rebuild"
        ctx.render(frames - 2, True)  # the accumulation continues on the scene as it was
        assert_bitwise(ctx.readback(64, 64), gold, "c1_64 continued after refused rebuilds")
        assert ctx.counters()["scene_uploads"] == 1


# ---- 7. the Python layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_render_pass_across_a_rebuild(gpu):
    """Execute across RayTracingMesh.deform(rebuild=True) and a plain deform after it: the pass rebuilds, then refits in
    the new order, with no second full upload, and shows what the oracle renders from the scene's arrays."""
    cfg = scenes.CONFIGS["C1"].resized(40, 32, 3)
    scene, cam = cfg.build_scene(), cfg.camera()
    p1 = rp.HalogenRenderPass(cfg.settings)
    p1.ctx.set_option(abi.HG_OPT_COUNTERS, 1)
    for _ in range(2):
        p1.Execute(scene, cam)
    mesh = scene.meshes[7]
    rest = mesh.vertices.copy()
    n_entries = len(mesh.bvh)
    mesh.deform(refit_cases.twist(rest, 0.7), rebuild=True)
    assert len(mesh.bvh) == n_entries and mesh.rebuild_serial == 1
    assert not np.array_equal(abi.build_blas_lbvh(mesh.rebuild_input, mesh.rebuild_leaf)[0], np.arange(12))
    p1.Execute(scene, cam)
    mesh.deform(refit_cases.twist(rest, 0.3))  # a plain deform: repacked in the rebuild's order, refitted
    for _ in range(3):
        p1.Execute(scene, cam)
    assert p1.getFrameCount() == 4
    a = p1.read_image()
    cnt = p1.ctx.counters()
    assert cnt["scene_uploads"] - cnt["scene_uploads_partial"] == 1 and cnt["scene_uploads_vouched"] >= 1, cnt
    packed = scene.pack()
    params = rp.make_params(p1.s, cam, 1, len(packed.spheres), len(packed.meshes), p1.s["UseEnvironmentCubemap"])
    assert not p1.s["UseEnvironmentCubemap"]
    ref, _ = hg_oracle.render(packed, params, 3, True)
    assert_bitwise(a, ref.reshape(a.shape), "a pass across a rebuild and a refit vs the oracle")
    # rebuilt and deformed again before the pass looks: rebuild from the rebuild's input, then refit
    mesh.deform(refit_cases.twist(rest, 0.5), rebuild=True)
    mesh.deform(refit_cases.twist(rest, 0.6))
    for _ in range(3):
        p1.Execute(scene, cam)
    cnt = p1.ctx.counters()
    assert cnt["scene_uploads"] - cnt["scene_uploads_partial"] == 1, cnt
    ref, _ = hg_oracle.render(scene.pack(), params, 3, True)
    assert_bitwise(p1.read_image(), ref.reshape(a.shape), "rebuild + deform between two frames vs the oracle")
    p1.Dispose()
