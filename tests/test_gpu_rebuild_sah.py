"""Device rebuild of one mesh's BVH with leaves chosen by surface area (hg_rebuild_mesh_sah, hg_rebuild_mesh_sah_device;
csrc/hg_lbvh.hip) against the host twin (hg_build_blas_lbvh_sah, tests/test_lbvh_sah.py) and the CPU oracle on the twin's
arrays.

The twin's arrays come from RayTracingMesh.deform(rebuild="sah"), which runs the twin and keeps the scene's pack()
current; the device gets the rebuild's own input and the node cost the twin used.  A context that was rebuilt is
compared with a fresh context after hg_upload_scene of the twin's arrays: triangles, normals and the leaf table byte for
byte, the mesh records but the root's record number, every tree by tests/test_gpu_rebuild.py's walk from the root (leaf
refs and the 24 box floats of every record: the packer numbers a tree's records in its own pre-order, the rebuild in
Karras' order, so the node array itself differs in record numbers); and the rebuilt tree's record numbers exactly, from
the twin's entry numbering: the inner entry whose children are entries 1 + 2j and 2 + 2j is record (root record) + j.

Test meshes sit behind Unity's cube in a two-mesh scene (a non-zero triangle offset and first record).  A "roomy" mesh
is uploaded with the L = 1 radix tree of its rest pose, n - 1 records, so that a tree at any node cost fits."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch  # before the library's first context (tests/test_gpu_query.py has why)

import hg_oracle
import refit_cases
from halogen import abi, render_pass as rp, scene as hs, scenes
from halogen.render_pass import Camera
from halogen.unity import Transform, unity_cube
from test_gpu_parity import assert_bitwise
from test_gpu_rebuild import COUNTERS, DI, LEAF, assert_same_scene, dragon_scene, on_device, tris18
from test_lbvh_sah import START_COST, case

W, H, FRAMES = 64, 36, 4
MI = 1  # the test mesh's index in case_scene


def corners(tris):
    return tris18(tris)[:, :9].reshape(-1, 3, 3)


def roomy(mesh):
    """The mesh's tree replaced, before the first pack(), by the L = 1 radix tree of its triangles: n - 1 inner entries"""
    order, mesh.packed_triangles, mesh.bvh = abi.build_blas_lbvh(mesh.packed_triangles, 1)
    mesh.triangles = np.ascontiguousarray(mesh.triangles[order])
    mesh.bvh_inner = len(order) - 1
    return mesh


def case_scene(name, room=True):
    """Unity's cube and, behind it in the buffers, the triangles of tests/test_lbvh_sah.py's case `name`"""
    sc = hs.Scene()
    sc.add(hs.RayTracingMesh("cube", *unity_cube(), Transform((-1.5, 0.0, 5.0))))
    mesh = hs.RayTracingMesh(name, *refit_cases._soup(corners(case(name))), Transform((0.5, -0.5, 3.0)))
    sc.add(roomy(mesh) if room else mesh)
    return sc


def case_params(packed, frames=FRAMES):
    cfg = scenes.CONFIGS["C1"].resized(W, H, frames)
    s = rp.clamp_settings(scenes.settings_for(cfg))
    cam = Camera(Transform((0.9, 0.0, 2.2), (0, 0, 0, 1)), 60.0, W, H)  # among the small triangles
    return rp.make_params(s, cam, 1, len(packed.spheres), len(packed.meshes), False)


def records(ctx, mesh_index):
    """The record numbers of the mesh's tree, by a walk from its root ref"""
    rec = ctx.scene_readback("nodes").view(np.uint32).reshape(-1, 16)
    root = int(ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[mesh_index, 16])
    out, stack = [], [root]
    while stack:
        r = stack.pop()
        if not r & LEAF:
            out.append(r)
            stack += [int(rec[r, 3]), int(rec[r, 7])]
    return out


def assert_records_follow_entries(ctx, mesh_index, bvh, what):
    """The rebuilt tree's refs are what the twin's entry numbering says: inner entry e is record root + (indexA(e) - 1) / 2,
    a leaf entry the inline ref of its range; the records are the first ones of the tree's range, contiguous."""
    e = np.frombuffer(bytes(bvh), dtype=np.uint32).reshape(-1, 8)
    m = ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[mesh_index]
    root, toff = int(m[16]), int(m[17])
    rec = ctx.scene_readback("nodes").view(np.uint32).reshape(-1, 16)

    def ref(entry, rec_min):
        a, cnt = int(e[entry, 0]), int(e[entry, 1])
        return (LEAF | cnt << 27 | (toff + a)) if cnt else rec_min + (a - 1) // 2

    if e[0, 1]:
        assert root == ref(0, 0), (what, hex(root))
        return 0
    assert not root & LEAF, what
    n_live = 0
    stack = [0]
    while stack:
        g = stack.pop()
        if e[g, 1]:
            continue
        j = (int(e[g, 0]) - 1) // 2
        n_live += 1
        a = int(e[g, 0])
        assert (int(rec[root + j, 3]), int(rec[root + j, 7])) == (ref(a, root), ref(a + 1, root)), (what, g, j)
        stack += [a, a + 1]
    assert sorted(records(ctx, mesh_index)) == list(range(root, root + n_live)), what
    assert len(e) >= 2 * n_live + 1 and not e[2 * n_live + 1:].any(), f"{what}: entries past the tree are padding"
    return n_live


def assert_twin(ctx, sc_or_packed, mesh_index, mesh, what, leaves=None):
    """leaves: the leaf table the context must hold; None: a fresh upload's.  (A rebuilt tree has inline leaves only, and a
    rebuild of either kind leaves the table as it is: where the uploaded tree had leaves of more than 15 triangles, their
    entries stay behind, unreachable, and a fresh upload of the twin's arrays has none.)"""
    packed = sc_or_packed.pack() if hasattr(sc_or_packed, "pack") else sc_or_packed
    if leaves is None:
        with abi.Context(0) as fresh:
            fresh.upload_scene(packed)
            leaves = fresh.scene_readback("leaves")
    assert np.array_equal(ctx.scene_readback("leaves"), leaves), f"{what}: the leaf table"
    assert_same_scene(ctx, packed, what)
    return assert_records_follow_entries(ctx, mesh_index, mesh.bvh, what)


def render(ctx, params, frames=FRAMES):
    ctx.clear_accumulation()
    ctx.set_params(params)
    ctx.render(frames, True)
    return ctx.readback(W, H)


def moved(mesh, strength=0.5):
    return refit_cases.twist(mesh.vertices, strength)


# ---- 1. device state ------------------------------------------------------------------------------------------------------------
CASES = [("random:1", 2.0), ("random:15", 2.0), ("random:15", 64.0), ("random:16", 2.0), ("random:17", 2.0),
         ("random:257", 2.0), ("random:1000", 0.5), ("random:1000", 2.0), ("identical", 2.0), ("flat:1", 2.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host_pointer", "device_pointer"])
@pytest.mark.parametrize("name,node_cost", CASES)
def test_gpu_sah_rebuild_is_the_twins_tree(gpu, name, node_cost, device):
    sc = case_scene(name)
    mesh = sc.meshes[MI]
    rest = sc.pack()
    assert rest.meshes[MI].triangleBufferOffset == 12 and rest.meshes[MI].accelerationBufferOffset > 0
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        assert min(records(ctx, 0)) == 0 and max(records(ctx, 0)) < min(records(ctx, MI) or [1 << 30])
        cube_before = (ctx.scene_readback("nodes")[:64 * (max(records(ctx, 0)) + 1)].copy(), ctx.scene_readback("tris").copy())
        first_record = int(ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[MI, 16])
        mesh.deform(moved(mesh), rebuild="sah", node_cost=node_cost)
        assert mesh.rebuild_node_cost == node_cost
        want_order = abi.build_blas_lbvh_sah(mesh.rebuild_input, node_cost)[0]
        got = ctx.rebuild_mesh_sah(MI, on_device(mesh.rebuild_input) if device else mesh.rebuild_input, node_cost)
        got = got.cpu().numpy() if device else got
        assert got.dtype == np.int32 and np.array_equal(got, want_order)
        n_live = assert_twin(ctx, sc, MI, mesh, f"{name} at node cost {node_cost}")
        root = int(ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36)[MI, 16])
        assert root == first_record if n_live else root & LEAF
        # the other mesh: its records (the first of the node array) and its triangles are as they were
        nodes, tris = ctx.scene_readback("nodes"), ctx.scene_readback("tris")
        assert np.array_equal(nodes[:len(cube_before[0])], cube_before[0]), "the cube's records"
        per_tri = len(tris) // (12 + mesh.triangle_count)
        assert np.array_equal(tris[:12 * per_tri], cube_before[1][:12 * per_tri]), "the cube's triangles"
    if name == "random:15" and node_cost == 64.0:
        assert n_live == 0, "fifteen triangles under a dear inner node: the root collapses, the tree is one leaf"
    if name == "random:16":
        assert n_live >= 1


@lru_cache(maxsize=None)
def dragon():
    """The Cornell box with the dragon twisted and rebuilt on the host (automatic node cost under the inner entries of
    BVHGenerator's tree): the rest arrays, the rebuild's input, the node cost
    used, the twin's arrays, the dragon's entries, the oracle's image, counters and answers to the camera rays."""
    sc = dragon_scene()
    rest = sc.pack()
    d = sc.meshes[DI]
    d.deform(refit_cases.twist(d.vertices, 0.5), rebuild="sah")
    twin = sc.pack()
    cfg = scenes.CONFIGS["C3"].resized(W, H, FRAMES)
    s = rp.clamp_settings(scenes.settings_for(cfg))
    params = rp.make_params(s, cfg.camera(), 1, len(sc.spheres), len(sc.meshes), False)
    ref, rcnt = hg_oracle.render(twin, params, FRAMES, True)
    ref.setflags(write=False)
    pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    cam = hg_oracle.camera_rays(params, 1, pixels)
    return rest, d.rebuild_input, d.rebuild_node_cost, twin, d, params, ref, rcnt, cam, hg_oracle.intersect_batch(twin, cam)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host_pointer", "device_pointer"])
def test_gpu_sah_rebuild_dragon(gpu, device):
    """The 8.7k dragon: device state, a 4-frame image and its counters, closest-hit queries, all against the twin"""
    rest, inp, node_cost, twin, d, params, ref, rcnt, cam, want = dragon()
    assert node_cost >= START_COST  # (automatic, under the inner entries of BVHGenerator's tree)
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        table = ctx.scene_readback("leaves")  # (BVHGenerator's tree of the dragon has leaves of up to 30 triangles)
        assert len(table) > 8
        # (the node cost the twin used: the device's capacity, the span of the uploaded records with the packer's pads,
        # is no smaller than the twin's limit, so its own ladder could stop a rung earlier; test_gpu_sah_rebuild_ladder)
        order = ctx.rebuild_mesh_sah(DI, on_device(inp) if device else inp, node_cost)
        order = order.cpu().numpy() if device else order
        assert np.array_equal(order, abi.build_blas_lbvh_sah(inp, node_cost)[0])
        n_live = assert_twin(ctx, twin, DI, d, "dragon", leaves=table)
        assert n_live == d.bvh_inner > 1000
        img = render(ctx, params)
        cnt = ctx.counters()
        got = ctx.trace_rays(cam, "closest")
    assert_bitwise(img, ref, "rebuilt dragon")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])
    on_dragon = (want["kind"] == abi.HG_HIT_MESH) & (want["object"] == DI)
    assert on_dragon.sum() > 50  # (of 2,304 pixels)
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    bad = np.flatnonzero(np.any(g != w, axis=1))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.gpu
def test_gpu_sah_rebuild_image_and_queries_small_mesh(gpu):
    """257 triangles (more than one workgroup of nodes) at node cost 2: image, counters and queries against the oracle"""
    sc = case_scene("random:257")
    mesh = sc.meshes[MI]
    rest = sc.pack()
    params = case_params(rest)
    mesh.deform(moved(mesh), rebuild="sah", node_cost=2.0)
    twin = sc.pack()
    ref, rcnt = hg_oracle.render(twin, params, FRAMES, True)
    pixels = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    cam = hg_oracle.camera_rays(params, 1, pixels)
    want = hg_oracle.intersect_batch(twin, cam)
    assert ((want["kind"] == abi.HG_HIT_MESH) & (want["object"] == MI)).sum() > 20, "the camera sees the mesh"
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        ctx.rebuild_mesh_sah(MI, on_device(mesh.rebuild_input), 2.0)
        img = render(ctx, params)
        cnt = ctx.counters()
        got = ctx.trace_rays(cam, "closest")
    assert_bitwise(img, ref, "257 triangles rebuilt")
    for k in COUNTERS:
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])
    g = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    w = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    assert np.array_equal(g, w)


# ---- 2. instances ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_sah_rebuild_instances(gpu):
    """tests/refit_cases.py's grid, instanced twice (two mesh records sharing both offsets): both cull boxes follow"""
    sc = refit_cases.hazard_scene()
    packed = refit_cases.hazard_packed(sc)
    index, last = 3, len(packed.meshes) - 1
    mesh = sc.meshes[index]
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        before = ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36).copy()
        mesh.deform(refit_cases.twist(mesh.vertices, 0.9, axis=0), rebuild="sah")
        order = ctx.rebuild_mesh_sah(index, mesh.rebuild_input, mesh.rebuild_node_cost)
        assert np.array_equal(order, abi.build_blas_lbvh_sah(mesh.rebuild_input, mesh.rebuild_node_cost)[0])
        twin = refit_cases.hazard_packed(sc)
        assert_twin(ctx, twin, index, mesh, "instanced grid")
        after = ctx.scene_readback("meshes").view(np.uint32).reshape(-1, 36).copy()
    assert after[last, 16] == after[index, 16] and after[last, 17] == after[index, 17]
    assert (after[index, 20:] != before[index, 20:]).any() and (after[last, 20:] != before[last, 20:]).any()
    assert (after[index, 20:] != after[last, 20:]).any()
    others = [k for k in range(len(after)) if k not in (index, last)]
    assert np.array_equal(after[others], before[others])


# ---- 3. sequences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sequence", ["sah_refit", "sah_fixed_sah"])
def test_gpu_sah_rebuild_sequences(gpu, sequence):
    """Each state equal to its twin's: an SAH rebuild, then a refit with moved triangles in the new order; an SAH
    rebuild, a fixed-leaf-size rebuild and an SAH rebuild again within the one capacity of the uploaded tree."""
    sc = dragon_scene()
    d = sc.meshes[DI]
    rest_vertices = d.vertices.copy()
    steps = {"sah_refit": [(0.5, "sah"), (0.8, None)], "sah_fixed_sah": [(0.5, "sah"), (0.7, 6), (0.9, "sah")]}[sequence]
    with abi.Context(0) as ctx:
        ctx.upload_scene(sc.pack())
        ctx.resize(W, H)
        for n, (strength, how) in enumerate(steps):
            v = refit_cases.twist(rest_vertices, strength)
            if how == "sah":
                d.deform(v, rebuild="sah")
                ctx.rebuild_mesh_sah(DI, on_device(d.rebuild_input), d.rebuild_node_cost)
            elif how:
                d.deform(v, rebuild=True, leaf_size=how)
                ctx.rebuild_mesh(DI, on_device(d.rebuild_input), d.rebuild_leaf)
            else:
                d.deform(v)  # repacked in the mesh's current order: the rebuild's
                ctx.refit_mesh(DI, on_device(d.packed_triangles))
            twin = sc.pack()
            assert_same_scene(ctx, twin, f"{sequence}, step {n}")
            if how == "sah":
                assert_records_follow_entries(ctx, DI, d.bvh, f"{sequence}, step {n}")
        params = dragon()[5]
        img = render(ctx, params, 1)
    with abi.Context(0) as fresh:
        fresh.upload_scene(twin)
        fresh.resize(W, H)
        assert_bitwise(img, render(fresh, params, 1), f"{sequence}: one frame against a fresh upload")


# ---- 4. the ladder and the refusals ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_sah_rebuild_ladder(gpu):
    """1000 triangles uploaded under their own SAH tree at twice the start cost, M records: the capacity, the span of those
    records with the packer's pads (fewer than M / 2), does not hold the tree at the start cost (more than 1.5 M records),
    so the automatic rebuild moves exactly one rung, as the twin does under the same limit.  The triangles stay where they
    are: a rebuild builds the whole tree all the same."""
    sc = case_scene("random:1000")
    mesh = sc.meshes[MI]
    mesh.deform(mesh.vertices, rebuild="sah", node_cost=2 * START_COST)
    m1 = mesh.bvh_inner
    mesh.bvh = (abi.BVHEntry * (2 * m1 + 1)).from_buffer_copy(bytes(mesh.bvh)[:32 * (2 * m1 + 1)])  # no padding entries
    m0 = (len(abi.build_blas_lbvh_sah(mesh.packed_triangles, START_COST)[2]) - 1) // 2
    assert 2 * m0 > 3 * m1 > 0, (m0, m1)
    with abi.Context(0) as ctx:
        ctx.upload_scene(sc.pack())
        recs = records(ctx, MI)
        capacity = max(recs) - min(recs) + 1
        assert m1 <= capacity < m0, (m1, capacity, m0)
        mesh.deform(mesh.vertices, rebuild="sah")  # (automatic, under the m1 inner entries of its tree)
        used = abi.build_blas_lbvh_sah(mesh.rebuild_input, 0.0, capacity)[3]
        assert used == mesh.rebuild_node_cost == 2 * START_COST, (used, mesh.rebuild_node_cost, capacity)
        ctx.rebuild_mesh_sah(MI, mesh.rebuild_input, 0.0)
        assert_twin(ctx, sc, MI, mesh, "one rung up the ladder")


@pytest.mark.gpu
def test_gpu_sah_rebuild_refusals_leave_the_scene(gpu):
    """Every refusal's code; the device scene and the continued accumulation stay as they were"""
    sc = case_scene("random:1000", room=False)
    mesh = sc.meshes[MI]
    # a third mesh whose uploaded tree is one leaf of 17 triangles: no record, so no rung of the ladder fits
    leaf17 = hs.RayTracingMesh("leaf17", *refit_cases._soup(corners(case("random:17"))), Transform((2.0, 0.5, 4.0)))
    leaf17.bvh = (abi.BVHEntry * 1)(abi.BVHEntry(0, 17))
    abi.refit_blas(leaf17.packed_triangles, leaf17.bvh)
    leaf17.bvh_inner = 0
    sc.add(leaf17)
    rest = sc.pack()
    params = case_params(rest)
    tris, n = mesh.packed_triangles, mesh.triangle_count
    L = abi.lib()
    dev = on_device(tris)
    order = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")

    def refused(ctx, call, rc, text):
        got = call()
        msg = L.hg_last_error(ctx._h).decode()
        assert got == rc and text in msg, (got, msg)

    with abi.Context(0) as fresh:
        fresh.upload_scene(rest)
        fresh.resize(W, H)
        want = render(fresh, params, FRAMES)
    with abi.Context(0) as ctx:
        p, d = C.cast(tris, C.c_void_p), C.c_void_p(dev.data_ptr())
        refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, MI, p, n, 2.0, None, 0), abi.HG_E_NOSCENE,
                "hg_upload_scene not called")
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        ctx.clear_accumulation()
        ctx.set_params(params)
        ctx.render(2, True)
        first = {k: ctx.scene_readback(k) for k in ("nodes", "leaves", "tris", "normals", "meshes")}
        nan, inf = float("nan"), float("inf")
        # (999 records at node cost 0.5; BVHGenerator's tree has 285 inner entries and at most 142 pads between them)
        refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, MI, p, n, 0.5, None, 0), abi.HG_E_UNSUPPORTED,
                "records at node cost 0.5, the tree's capacity is")
        refused(ctx, lambda: L.hg_rebuild_mesh_sah_device(ctx._h, MI, d, n, 0.5, None, 0), abi.HG_E_UNSUPPORTED,
                "capacity")
        t17 = leaf17.packed_triangles
        refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, 2, C.cast(t17, C.c_void_p), 17, 0.0, None, 0),
                abi.HG_E_UNSUPPORTED, "the last of the ladder")
        for bad in (-1.0, nan, inf):
            refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, MI, p, n, bad, None, 0), abi.HG_E_INVALID, "node_cost")
            refused(ctx, lambda: L.hg_rebuild_mesh_sah_device(ctx._h, MI, d, n, bad, None, 0), abi.HG_E_INVALID, "node_cost")
        refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, MI, p, n - 1, 0.0, None, 0), abi.HG_E_INVALID,
                f"mesh {MI}: {n - 1} triangles")
        refused(ctx, lambda: L.hg_rebuild_mesh_sah_device(ctx._h, MI, C.c_void_p(dev.data_ptr() + 2), n, 0.0, None, 0),
                abi.HG_E_INVALID, "4-byte aligned")
        refused(ctx, lambda: L.hg_rebuild_mesh_sah_device(ctx._h, MI, d, n, 0.0, C.c_void_p(order.data_ptr() + 1), 0),
                abi.HG_E_INVALID, "4-byte aligned")
        refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, MI, None, n, 0.0, None, 0), abi.HG_E_INVALID, "null triangle array")
        refused(ctx, lambda: L.hg_rebuild_mesh_sah(ctx._h, 99, p, n, 0.0, None, 0), abi.HG_E_INVALID, "out of range")
        for k, v in first.items():
            assert np.array_equal(ctx.scene_readback(k), v), f"{k} changed by a refused rebuild"
        ctx.render(FRAMES - 2, True)  # the accumulation continues on the scene as it was
        assert_bitwise(ctx.readback(W, H), want, "continued after refused rebuilds")
        assert ctx.counters()["scene_uploads"] == 1


# ---- 5. the Python layers ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_render_pass_across_a_sah_rebuild(gpu):
    """Execute across RayTracingMesh.deform(rebuild="sah") and a plain deform after it: the pass rebuilds on the device at
    the node cost the twin used, then refits in the new order, with no second full upload, and shows what the oracle
    renders from the scene's arrays (the twin's)."""
    cfg = scenes.CONFIGS["C3"].resized(40, 32, 3)
    scene, cam = scenes.dragon_cornell(1), cfg.camera()
    index = max(range(len(scene.meshes)), key=lambda k: scene.meshes[k].triangle_count)
    mesh = scene.meshes[index]
    assert mesh.triangle_count == 8712
    p1 = rp.HalogenRenderPass(cfg.settings)
    p1.ctx.set_option(abi.HG_OPT_COUNTERS, 1)
    for _ in range(2):
        p1.Execute(scene, cam)
    rest = mesh.vertices.copy()
    n_entries = len(mesh.bvh)
    mesh.deform(refit_cases.twist(rest, 0.7), rebuild="sah")
    assert len(mesh.bvh) == n_entries and mesh.rebuild_serial == 1 and mesh.rebuild_node_cost >= START_COST
    p1.Execute(scene, cam)
    assert p1.ctx.counters()["scene_uploads"] - p1.ctx.counters()["scene_uploads_partial"] == 1
    mesh.deform(refit_cases.twist(rest, 0.3))  # a plain deform: repacked in the rebuild's order, refitted
    for _ in range(3):
        p1.Execute(scene, cam)
    a = p1.read_image()
    cnt = p1.ctx.counters()
    assert cnt["scene_uploads"] - cnt["scene_uploads_partial"] == 1 and cnt["scene_uploads_vouched"] >= 1, cnt
    packed = scene.pack()
    params = rp.make_params(p1.s, cam, 1, len(packed.spheres), len(packed.meshes), p1.s["UseEnvironmentCubemap"])
    assert not p1.s["UseEnvironmentCubemap"]
    ref, _ = hg_oracle.render(packed, params, 3, True)
    assert_bitwise(a, ref.reshape(a.shape), "a pass across an SAH rebuild and a refit vs the oracle")
    with abi.Context(0) as fresh:  # the same image as a fresh upload of the twin's arrays
        fresh.upload_scene(packed)
        fresh.resize(40, 32)
        fresh.clear_accumulation()
        fresh.set_params(params)
        fresh.render(3, True)
        assert_bitwise(a, fresh.readback(40, 32).reshape(a.shape), "the pass vs a fresh upload of the twin's arrays")
    p1.Dispose()
