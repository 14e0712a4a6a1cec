"""GPU parity for every home of the material table.

The regenerating and streaming kernels keep a copy of the material table (80 B per material) in the wave's LDS when
csrc/hg_layout.h hg_wave_lds_plan finds room: at 1 sample per pixel a table of at most 9 materials (720 of 768 B) lies
in the three sample-sum rows, which no lane touches then; a larger table, or any table at more samples (the rows are
live), goes behind the mesh records while the kernel's LDS budget allows; otherwise the kernels read the table from
global memory, as the lockstep kernel always does.  The benchmark scenes have 4 and 7 materials at 1 sample, so only
the first home is exercised there.  Here every kernel runs every home against the live CPU oracle, bit for bit and
with equal work counters: the Cornell box (7 materials) with extra cubes of distinct diffuse, metallic and dielectric
materials for 9, 10 and 107 materials, the nested glass scene framed on the glass (dielectric priorities and the
medium stack), 3 samples per pixel, and the render server across a partial upload that changes one material."""
import dataclasses

import numpy as np
import pytest

import hg_oracle
from halogen import abi, render_pass as rp, scenes
from halogen.scene import HalogenMaterial, RayTracingMesh
from halogen.unity import Transform, euler_to_quat, unity_cube

from test_gpu_parity import KERNELS, assert_bitwise, gpu_render

W, H, FRAMES = 48, 32, 3


def _extra_material(i: int, tint: float = 0.0) -> HalogenMaterial:
    """Material i of the extra cubes: all distinct, in turn diffuse, metallic and glossy, absorbing glass of priority
    0-3."""
    c = (0.15 + 0.007 * i + tint, 0.9 - 0.006 * i, 0.35 + 0.004 * i, 1.0)
    if i % 3 == 0:
        return HalogenMaterial.default(c)
    if i % 3 == 1:
        return HalogenMaterial(color=c, metallic=0.6, roughness=0.1 + 0.005 * i)
    return HalogenMaterial(color=c[:3] + (0.1,), roughness=0.03, metallic=0.02, subsurfaceColor=(0.6, 0.9, 1.0, 1.0),
                           indexOfRefraction=1.3 + 0.002 * i, absorption=0.3, dielectricPriority=i % 4)


def _cornell_with_materials(n_materials: int, tint: float = 0.0):
    """The C1 Cornell box (7 materials) plus one small cube per further material, on a grid inside the box."""
    sc = scenes.cornell_box()
    root = Transform(scenes.CORNELL_ROOT)
    v, n, t = unity_cube()
    n_extra = n_materials - 7
    side = max(1, int(np.ceil(np.sqrt(n_extra))))
    size = min(0.5, 2.4 / side)
    for i in range(n_extra):
        gx, gy = i % side, i // side
        pos = (-2.0 + 4.0 * (gx + 0.5) / side, -2.0 + 3.5 * (gy + 0.5) / side, 14.6)
        q = (0.0, float(np.sin(0.1 * i)), 0.0, float(np.cos(0.1 * i)))
        sc.add(RayTracingMesh(f"Material cube {i}", v, n, t, Transform(pos, q, (size, size, size), root),
                              _extra_material(i, tint if i == 0 else 0.0)))
    packed = sc.pack()
    assert len(packed.materials) == n_materials
    return packed


def _cornell_params(packed, spp=1, first_frame=1):
    cfg = scenes.CONFIGS["C1"]
    settings = dataclasses.replace(scenes.settings_for(cfg), SamplesPerPixel=spp)
    s = rp.clamp_settings(settings)
    return rp.make_params(s, scenes.cornell_camera(W, H), first_frame, len(packed.spheres), len(packed.meshes), False)


def _glass_case():
    """C5's nested glass, the camera moved in until the glass cube fills the view."""
    cfg = scenes.CONFIGS["C5"].resized(W, H, FRAMES)
    settings = scenes.settings_for(cfg)
    s = rp.clamp_settings(settings)
    packed = scenes.nested_glass().pack()
    cube = settings.environmentCubemap if s["UseEnvironmentCubemap"] else None
    cam = scenes.Camera(Transform((0.0, 1.5, -3.0), euler_to_quat(10, 0, 0)), 60.0, W, H)
    return packed, rp.make_params(s, cam, 1, len(packed.spheres), len(packed.meshes), cube is not None), cube


def _build(case):
    if case == "glass":
        return _glass_case()
    n_materials, spp = {"fit9": (9, 1), "one_more10": (10, 1), "global107": (107, 1), "spp3": (9, 3)}[case]
    packed = _cornell_with_materials(n_materials)
    return packed, _cornell_params(packed, spp), None


CASES = ["fit9", "one_more10", "global107", "glass", "spp3"]
_refs = {}


def _reference(case):
    """The case's inputs and the oracle's image and counters, computed once for the four kernels."""
    if case not in _refs:
        packed, params, cube = _build(case)
        ref, rcnt = hg_oracle.render(packed, params, FRAMES, True, cubemap=cube)
        ref.setflags(write=False)
        _refs[case] = (packed, params, cube, ref, rcnt)
    return _refs[case]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("case", CASES)
def test_gpu_material_homes_match_oracle(gpu, case, kernel):
    packed, params, cube, ref, rcnt = _reference(case)
    assert rcnt["hits"] > 0.3 * rcnt["paths"], "the objects are not in view: not a parity check"
    img, cnt = gpu_render(packed, params, FRAMES, True, cube, kernel=kernel)
    assert_bitwise(img, ref, f"{case}: {len(packed.materials)} materials, kernel {kernel}")
    for k in ("rays", "tri_tests", "aabb_tests", "hits"):
        assert cnt[k] == rcnt[k], (k, cnt[k], rcnt[k])


@pytest.mark.gpu
def test_gpu_server_partial_upload_changes_a_material(gpu):
    """The render server's waves copy the table once per lifetime.  One-frame calls through the server, a partial
    upload (same geometry) that changes one material's colour, more calls: the image is the oracle's, rendered the
    same way, so the waves that traced the later frames read the new table."""
    a = _cornell_with_materials(9)
    b = _cornell_with_materials(9, tint=0.5)
    assert bytes(a.materials) != bytes(b.materials) and bytes(a.triangles) == bytes(b.triangles)
    params = _cornell_params(a)
    ref, rcnt = hg_oracle.render(a, params, FRAMES, True)
    ref, rcnt2 = hg_oracle.render(b, _cornell_params(b, first_frame=1 + FRAMES), FRAMES, True, acc=ref)
    assert rcnt["hits"] > 0.3 * rcnt["paths"] and rcnt2["hits"] > 0.3 * rcnt2["paths"]
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_SERVER, 2)  # every qualifying call
        ctx.set_option(abi.HG_OPT_COALESCE, 1)
        ctx.upload_scene(a)
        ctx.resize(W, H)
        ctx.set_params(params)
        for _ in range(FRAMES):
            ctx.render(1, True)
        ctx.upload_scene(b)
        for _ in range(FRAMES):
            ctx.render(1, True)
        img = ctx.readback(W, H)
        cnt = ctx.counters()
    assert_bitwise(img, ref, "server across a material upload")
    assert cnt["scene_uploads_partial"] == 1, cnt
    assert cnt["server_launches"] >= 2 and cnt["server_frames"] == 2 * FRAMES, cnt
    for k in ("rays", "tri_tests", "aabb_tests", "hits"):
        assert cnt[k] == rcnt[k] + rcnt2[k], (k, cnt[k], rcnt[k], rcnt2[k])
