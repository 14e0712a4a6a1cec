"""Device refit of a deforming mesh (hg_refit_mesh, hg_refit_mesh_device, hg_scene_readback).  The primary check is
state equality: after a refit the five arrays of the device scene equal, byte for byte, those of a fresh context that
uploaded the deformed triangles with the host twin's boxes (hg_refit_blas).  Then images and work counters against the
CPU oracle's render of the caller-side arrays, the upload bookkeeping after a refit, refusals, and the render pass."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library's first context (tests/test_gpu_query.py has why)

import cases
import hg_oracle
import refit_cases
from halogen import abi, render_pass as rp, scenes
from halogen.scene import PackedScene
from test_gpu_parity import GOLD, KERNELS, assert_bitwise

ARRAYS = ("nodes", "leaves", "tris", "normals", "meshes")


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


def tris18(mesh):
    return np.frombuffer(bytes(mesh.packed_triangles), dtype=np.float32).reshape(-1, 18).copy()


def refit(ctx, index, mesh, device, generation=0):
    if device:
        ctx.refit_mesh(index, torch.from_numpy(tris18(mesh)).to("cuda:0"), generation)
    else:
        ctx.refit_mesh(index, mesh.packed_triangles, generation)


def _copy(packed):
    arrays = {}
    for k in ("spheres", "meshes", "materials", "triangles", "blas"):
        a = getattr(packed, k)
        b = (type(a)._type_ * len(a))()
        C.memmove(b, a, C.sizeof(a))
        arrays[k] = b
    return PackedScene(**arrays)


# ---- state equality ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host_pointer", "device_pointer"])
def test_gpu_refit_state_equals_a_fresh_upload(gpu, device):
    """The hazard scene (tests/refit_cases.py): each mesh refitted in turn, one refitted twice, then all back to the
    rest pose; after every refit the device equals a fresh upload of the caller's arrays."""
    sc = refit_cases.hazard_scene()
    rest = [m.vertices.copy() for m in sc.meshes]
    packed = refit_cases.hazard_packed(sc)
    assert len(packed.meshes) == 5 and packed.meshes[4].triangleBufferOffset == packed.meshes[3].triangleBufferOffset > 0
    assert packed.blas[packed.meshes[0].accelerationBufferOffset].triangleCount == 3  # a leaf root
    assert max(e.triangleCount for e in packed.blas) >= 40                            # a leaf-table leaf, a long loop
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        first = state(ctx)
        assert_same_state(first, fresh_state(packed), "two uploads")
        records = first["nodes"].reshape(-1, 64)
        assert (~records.any(axis=1)).sum() >= 1, "the hazard scene must hold a zero pad record"
        leaves = first["leaves"].view(np.uint32).reshape(-1, 2)
        assert (leaves[:, 1] >= 40).any()
        steps = [(0, refit_cases.noise(rest[0], 0.3)), (1, refit_cases.twist(rest[1], 0.5)),
                 (2, refit_cases.noise(rest[2], 0.2)),           # the flat plane made bumpy: the pads go
                 (3, refit_cases.twist(rest[3], 0.9, axis=0)),   # the instanced tree, through its first instance
                 (1, refit_cases.noise(rest[1], 0.05, seed=2)),  # a second refit of the same mesh
                 (4, refit_cases.noise(rest[3], 0.1, seed=3))]   # ... and through its second instance
        steps += [(i, rest[i]) for i in range(4)]                # back to the rest pose: the pads come back
        for n, (index, verts) in enumerate(steps):
            mesh = sc.meshes[min(index, 3)]
            mesh.deform(verts)
            refit(ctx, index, mesh, device)
            assert_same_state(state(ctx), fresh_state(refit_cases.hazard_packed(sc)), f"step {n}: mesh {index}")
        assert_same_state(state(ctx), first, "back at the rest pose")


@pytest.mark.gpu
def test_gpu_refit_deep_tree_and_leaf_table(gpu):
    """dragon10 (871,200 triangles, a 32-level tree, hundreds of long leaves): state equality, and one frame against
    the fresh upload's."""
    packed, params, cube, _, acc = cases.setup("dragon10_64x36")
    W, H = int(params.screenParameters.x), int(params.screenParameters.y)
    sc = scenes.dragon_cornell(10)
    di = len(sc.meshes) - 1
    dragon = sc.meshes[di]
    with abi.Context(0) as ctx:
        ctx.upload_scene(sc.pack())
        dragon.deform(refit_cases.twist(dragon.vertices, 0.7))
        moved = sc.pack()
        ctx.refit_mesh(di, dragon.packed_triangles)
        got = state(ctx)
        ctx.resize(W, H)
        ctx.set_params(params)
        ctx.render(1, acc)
        img = ctx.readback(W, H)
    with abi.Context(0) as ctx:
        ctx.upload_scene(moved)
        want = state(ctx)
        ctx.resize(W, H)
        ctx.set_params(params)
        ctx.render(1, acc)
        ref = ctx.readback(W, H)
    leaves = want["leaves"].view(np.uint32).reshape(-1, 2)
    assert len(leaves) > 100 and (leaves[:, 1] > 15).all()
    assert_same_state(got, want, "dragon10 twisted")
    assert_bitwise(img, ref, "dragon10 twisted, 1 frame")


# ---- image and counters against the oracle ---------------------------------------------------------------------------------
DEFORM = {"twist": lambda v: refit_cases.twist(v, 0.5), "noise": lambda v: refit_cases.noise(v, 0.03)}
_oracle = {}


def deformed_case(name, how):
    """The case's scene with its deformable meshes moved (the dragon; the Cornell box's interior cubes), the uniforms,
    and the oracle's render of the caller-side arrays: built once, shared by the kernels."""
    if (name, how) not in _oracle:
        _, params, cube, frames, acc = cases.setup(name)
        sc = scenes.dragon_cornell(1) if name.startswith("dragon") else scenes.cornell_box()
        rest = sc.pack()
        todo = [len(sc.meshes) - 1] if name.startswith("dragon") else [6, 7, 8]
        for i in todo:
            sc.meshes[i].deform(DEFORM[how](sc.meshes[i].vertices))
        moved = sc.pack()
        ref, rcnt = hg_oracle.render(moved, params, frames, acc, cubemap=cube)
        ref.setflags(write=False)
        _oracle[name, how] = (rest, sc, todo, params, frames, acc, ref, rcnt)
    return _oracle[name, how]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("how", sorted(DEFORM))
@pytest.mark.parametrize("name", ["dragon1_64x36", "c1_64", "c1_32_boxtests"])
def test_gpu_refit_matches_oracle(gpu, name, how, kernel):
    """The image and the work counters after a refit are the oracle's for the deformed triangles and the host twin's
    boxes (the box-test view and aabb_tests are what see a loose or a tight box)."""
    rest, sc, todo, params, frames, acc, ref, rcnt = deformed_case(name, how)
    W, H = int(params.screenParameters.x), int(params.screenParameters.y)
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_KERNEL, KERNELS[kernel])
        ctx.upload_scene(rest)
        ctx.resize(W, H)
        for i in todo:
            ctx.refit_mesh(i, sc.meshes[i].packed_triangles)
        ctx.set_params(params)
        ctx.render(frames, acc)
        img = ctx.readback(W, H)
        cnt = ctx.counters()
    assert_bitwise(img, ref, f"{name} {how} {kernel}")
    for k in ("rays", "tri_tests", "aabb_tests", "hits"):
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------------
def _c1():
    _, params, cube, frames, acc = cases.setup("c1_64")
    sc = scenes.cornell_box()
    return sc, sc.pack(), params, frames


def _render(ctx, params, frames, W=64, H=64):
    ctx.clear_accumulation()
    ctx.set_params(params)
    ctx.render(frames, True)
    return ctx.readback(W, H)


@pytest.mark.gpu
def test_gpu_refit_then_uploads(gpu):
    """After a refit: a vouched upload with one moved object is partial and equals a fresh full upload of the same
    arrays; an unvouched upload of the original arrays is a full upload, and the image is the original golden."""
    sc, rest, params, frames = _c1()
    gold = np.load(GOLD / "c1_64.npz")["image"]
    with abi.Context(0) as ctx:
        ctx.upload_scene(rest, generation=3)
        ctx.resize(64, 64)
        sc.meshes[7].deform(refit_cases.twist(sc.meshes[7].vertices, 0.8))
        ctx.refit_mesh(7, sc.meshes[7].packed_triangles, generation=3)
        moved = sc.pack()
        moved.meshes[6].worldToLocal.m[12] += np.float32(0.05)
        moved.meshes[7].worldToLocal.m[13] += np.float32(0.02)  # the refitted mesh moves too: its kept root boxes
        before = ctx.counters()
        ctx.upload_scene(moved, generation=3)
        after = ctx.counters()
        assert after["scene_uploads_partial"] == before["scene_uploads_partial"] + 1, after
        assert after["scene_uploads_vouched"] == before["scene_uploads_vouched"] + 1, after
        assert_same_state(state(ctx), fresh_state(moved), "vouched partial upload after a refit")
        img = _render(ctx, params, frames)
        ctx.upload_scene(_copy(moved), generation=3)  # vouched, nothing changed: skipped
        assert ctx.counters()["scene_uploads_skipped"] == after["scene_uploads_skipped"] + 1
        with abi.Context(0) as other:
            other.upload_scene(moved)
            other.resize(64, 64)
            want = _render(other, params, frames)
        assert_bitwise(img, want, "vouched partial upload after a refit vs a fresh full upload")
        ctx.upload_scene(rest)  # unvouched, and equal to the retained (stale) copies: must not be skipped
        last = ctx.counters()
        assert last["scene_uploads_skipped"] == after["scene_uploads_skipped"] + 1, last
        assert last["scene_uploads_partial"] == after["scene_uploads_partial"], last
        assert last["scene_uploads"] == after["scene_uploads"] + 1, last
        assert_bitwise(_render(ctx, params, frames), gold, "the original arrays after a refit")
        ctx.upload_scene(rest)  # a full upload cleared the mark: now it is skipped again
        assert ctx.counters()["scene_uploads_skipped"] == last["scene_uploads_skipped"] + 1


@pytest.mark.gpu
@pytest.mark.parametrize("server", [0, 2], ids=["held_frames", "render_server"])
def test_gpu_refit_between_frames(gpu, server):
    """A refit between held (coalesced) frames, and with the render server engaged: the frames before it and the frames
    after it are those of separate contexts."""
    sc, rest, params, frames = _c1()
    sc.meshes[8].deform(refit_cases.noise(sc.meshes[8].vertices, 0.05))
    moved = sc.pack()
    want = []
    for packed in (rest, moved):
        with abi.Context(0) as ctx:
            ctx.upload_scene(packed)
            ctx.resize(64, 64)
            want.append(_render(ctx, params, 3))
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_SERVER, server)
        ctx.set_option(abi.HG_OPT_COALESCE, 32)
        ctx.upload_scene(rest)
        ctx.resize(64, 64)
        ctx.clear_accumulation()
        ctx.set_params(params)
        for _ in range(3):
            ctx.render(1, True)  # held, or posted to the server
        ctx.refit_mesh(8, sc.meshes[8].packed_triangles)  # launches the held frames, stops the server, then refits
        before = ctx.readback(64, 64)
        ctx.clear_accumulation()
        ctx.set_params(params)
        for _ in range(3):
            ctx.render(1, True)
        after = ctx.readback(64, 64)
        if server:
            assert ctx.counters()["server_frames"] > 0
    assert_bitwise(before, want[0], "the frames before the refit")
    assert_bitwise(after, want[1], "the frames after the refit")


@pytest.mark.gpu
def test_gpu_refit_refusals_leave_the_scene(gpu):
    """Every refusal's code and text; the scene and the image stay as they were."""
    sc, rest, params, frames = _c1()
    gold = np.load(GOLD / "c1_64.npz")["image"]
    tris = sc.meshes[7].packed_triangles
    n = len(tris)
    L = abi.lib()

    def refused(ctx, call, rc, text):
        got = call()
        msg = L.hg_last_error(ctx._h).decode()
        assert got == rc and msg == text, (got, msg)

    with abi.Context(0) as ctx:
        refused(ctx, lambda: L.hg_refit_mesh(ctx._h, 0, C.cast(tris, C.c_void_p), n, 0), abi.HG_E_NOSCENE,
                "hg_refit_mesh: hg_upload_scene not called")
        with pytest.raises(abi.HalogenError) as e:
            ctx.scene_readback("nodes")
        assert e.value.rc == abi.HG_E_NOSCENE
        ctx.upload_scene(rest)
        ctx.resize(64, 64)
        ctx.clear_accumulation()
        ctx.set_params(params)
        ctx.render(2, True)
        first = state(ctx)
        p = C.cast(tris, C.c_void_p)
        for index in (-1, len(rest.meshes)):
            refused(ctx, lambda: L.hg_refit_mesh(ctx._h, index, p, n, 0), abi.HG_E_INVALID,
                    f"hg_refit_mesh: mesh_index {index} out of range ({len(rest.meshes)} meshes)")
        refused(ctx, lambda: L.hg_refit_mesh(ctx._h, 7, None, n, 0), abi.HG_E_INVALID,
                "hg_refit_mesh: null triangle array")
        refused(ctx, lambda: L.hg_refit_mesh_device(ctx._h, 7, None, n, 0), abi.HG_E_INVALID,
                "hg_refit_mesh: null triangle array")
        refused(ctx, lambda: L.hg_refit_mesh(ctx._h, 7, p, n - 1, 0), abi.HG_E_INVALID,
                f"hg_refit_mesh: mesh 7: {n - 1} triangles, its tree's leaves reach {n}")
        toff = rest.meshes[8].triangleBufferOffset
        refused(ctx, lambda: L.hg_refit_mesh(ctx._h, 8, p, n + 1, 0), abi.HG_E_INVALID,
                f"hg_refit_mesh: mesh 8: triangles {toff} + {n + 1} past the scene's {len(rest.triangles)}")
        refused(ctx, lambda: L.hg_refit_mesh(ctx._h, 6, p, n + 1, 0), abi.HG_E_UNSUPPORTED,
                "hg_refit_mesh: mesh 6 shares triangles with mesh 7, which has another tree")
        with pytest.raises(abi.HalogenError) as e:
            ctx.scene_readback(9)
        assert e.value.rc == abi.HG_E_INVALID and str(e.value).endswith("hg_scene_readback: unknown array 9")
        assert_same_state(state(ctx), first, "after the refusals")
        ctx.render(frames - 2, True)  # the accumulation continues on the scene as it was
        assert_bitwise(ctx.readback(64, 64), gold, "c1_64 continued after refused refits")
        assert ctx.counters()["scene_uploads"] == 1
    # two trees over the same triangles: the second mesh record names another tree (a copy of the first mesh's entries)
    shared = _copy(rest)
    n0 = rest.meshes[1].accelerationBufferOffset  # mesh 0's entries are [0, n0)
    blas = (abi.BVHEntry * (len(rest.blas) + n0))(*list(rest.blas), *list(rest.blas)[:n0])
    shared.blas = blas
    shared.meshes[1].accelerationBufferOffset = len(rest.blas)
    shared.meshes[1].triangleBufferOffset = 0
    with abi.Context(0) as ctx:
        ctx.upload_scene(shared)
        t0 = sc.meshes[0].packed_triangles
        refused(ctx, lambda: L.hg_refit_mesh(ctx._h, 0, C.cast(t0, C.c_void_p), len(t0), 0), abi.HG_E_UNSUPPORTED,
                "hg_refit_mesh: mesh 0 shares triangles with mesh 1, which has another tree")


# ---- the pass ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_render_pass_across_a_deform(gpu):
    """Execute across RayTracingMesh.deform: the pass clears the accumulation, refits the deformed mesh under its
    generation (no full upload) and shows what a fresh pass on the deformed scene shows."""
    cfg = scenes.CONFIGS["C1"].resized(40, 32, 3)
    scene, cam = cfg.build_scene(), cfg.camera()
    p1 = rp.HalogenRenderPass(cfg.settings)
    p1.ctx.set_option(abi.HG_OPT_COUNTERS, 1)
    for _ in range(2):
        p1.Execute(scene, cam)
    scene.meshes[7].deform(refit_cases.twist(scene.meshes[7].vertices, 0.7))
    for _ in range(3):
        p1.Execute(scene, cam)
    assert p1.getFrameCount() == 4
    a = p1.read_image()
    cnt = p1.ctx.counters()
    # the deform cost no second full upload: one full upload, then vouched partial ones (the mesh records' bounds moved)
    assert cnt["scene_uploads"] - cnt["scene_uploads_partial"] == 1 and cnt["scene_uploads_vouched"] >= 1, cnt
    p2 = rp.HalogenRenderPass(cfg.settings)
    for _ in range(3):
        p2.Execute(scene, cam)
    assert_bitwise(a, p2.read_image(), "a pass across a deform vs a fresh pass")
    for p in (p1, p2):
        p.Dispose()
