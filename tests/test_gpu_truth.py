"""The kernels against float64 geometry and closed forms (tests/truth.py).

Every other GPU test compares a kernel with the CPU oracle bit for bit, which cannot see a mistake the two share.  Here
the device building blocks (the test-only probe, tests/devprobe.py), the ray query (hg_trace_rays) and the render
kernels run the inputs of tests/test_truth.py through the same checks the oracle passes there: a float64 linear solve,
slab intervals and quadratic; a search over every triangle without a hierarchy; the definition of a net; the laws of
reflection and refraction and the moments of a cosine-weighted hemisphere; images whose pixels are known in closed form.
The inputs, the check functions, the bounds (with the constants they were measured at) and the tests of what each check
leaves out are in tests/test_truth.py; nothing here reads the oracle's results."""
import numpy as np
import pytest

import devprobe
import test_truth as T
from halogen import abi

F = np.float32


# ----------------------------------------------------------------------------------------------------------------------
# 1. intersection building blocks
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flat", [False, True], ids=["branchy", "flat"])
def test_gpu_tri_accept_against_float64(gpu, flat):
    """hgd::tri_accept<false / true> on the 2e5 elements of test_truth.tri_inputs(): the residual |o + t d - v0 - U e1 -
    V e2| of every accepted (t, U, V) within K 2^-24 mag / (c s), K = 8; accept and front (the sign of n . -d with the
    reference's winding, HC:317-318, 350) equal to the float64 decision on every decided element.
    Measured maximum of |R| c s / (2^-24 mag): numpy float32 stand-in 1.84, oracle 1.84."""
    out = devprobe.run(devprobe.TRI_FLAT if flat else devprobe.TRI, T.tri_probe_inputs(T.tri_inputs()))
    T.check_tri(out, f"device tri_accept<{str(flat).lower()}>")


@pytest.mark.gpu
def test_gpu_ray_aabb_against_float64(gpu):
    """hgd::ray_aabb against the float64 slab intervals on the 1e5 elements of test_truth.box_inputs(): hit or miss, the
    entry distance (the box test returns tMin, HC:258) within 4 ulp of max(|t|, |o| |inv|_inf), flat boxes never hit."""
    T.check_box(devprobe.run(devprobe.AABB, T.box_inputs()[0]).view(F), "device ray_aabb")


@pytest.mark.gpu
def test_gpu_isect_spheres_against_float64(gpu):
    """hgd::isect_spheres over one sphere against the float64 quadratic with the reference's root choice (a = 1; from
    inside, the far root; accepted above 1e-4: HC:266-303, 369) on the 1e5 elements of test_truth.sphere_inputs(): | |o + t
    d - c| - r | within K 2^-24 (|o - c| + |t| + r) / sqrt(1 - (b / r)^2), K = 22, for b <= 0.999 r, and the accepted
    reference wherever the float64 answer is decided.
    Measured maximum of the ratio: numpy float32 stand-in 7.06, oracle 7.06."""
    T.check_sphere(devprobe.run(devprobe.SPHERES, T.sphere_inputs()["x"]), "device isect_spheres")


# ----------------------------------------------------------------------------------------------------------------------
# 2. closest hit over instanced meshes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_trace_rays_against_float64(gpu):
    """hg_trace_rays (the world-to-local transform, the cull table, the BVH, the traversal, the leaf tests and
    resolve_mesh) against the hierarchy-free float64 search of test_truth.closest_truth(): 5,376 rays over the dragon, a
    rotated cube scaled (0.5, 1, 2), a mirrored plane and two spheres.  What is judged, and the traits followed (the
    local winding's orientation, the normal as row vector times worldToLocal): test_oracle_closest_against_float64.  The
    any-hit query must report a hit for exactly the rays the closest query hits."""
    packed, _ = T.closest_scene()
    rays = T.closest_rays()
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        hits = ctx.trace_rays(rays, "closest")
        occ = ctx.trace_rays(rays, "any")
    T.check_closest(hits, "device closest hit")
    assert np.array_equal(occ["kind"] != 0, hits["kind"] != 0)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the sampler is a net
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", T.NET_M)
def test_gpu_sampler_is_a_net(gpu, m):
    """hgd::Sampler::get1 / get2 for 32 (pixel, offset, id) triples over the frame blocks [0, 2^m) and [5 2^m, 6 2^m): get1
    puts exactly one sample in every interval of length 2^-m, get2's samples form a (0, m, 2)-net.  Exact comparisons of
    the float32 samples against k / 2^m, no tolerance; a sample exactly on a grid line (float(u32) / 2^32 rounds up to
    it, HR:258) may count for either neighbouring cell (test_inputs_net_floats)."""
    for block in T.NET_BLOCKS:
        t = T.net_tuples(m, block)
        g1 = devprobe.run(devprobe.GET1, t).view(F).reshape(32, -1)
        g2 = devprobe.run(devprobe.GET2, t).view(F).reshape(32, -1, 2)
        assert g1.min() >= 0 and g1.max() <= 1 and g2.min() >= 0 and g2.max() <= 1
        T.check_net_floats(g1, g2, m, f"device sampler block {block}")


@pytest.mark.gpu
@pytest.mark.parametrize("block", T.NET_BLOCKS)
def test_gpu_sampler_dimensions_are_decorrelated(gpu, block):
    """hgd::Sampler::get2 in two dimensions of the same pixel over 1024 consecutive frames: the index shuffle (HR:219)
    makes the pairs of first components fill the 4 x 4 cells of the unit square like independent samples (every count
    within 6 standard deviations of 64); without it 12 of the 16 cells stay empty."""
    a, b = T.pad_tuples(block)
    xa = devprobe.run(devprobe.GET2, a).view(F)[:, 0].reshape(32, -1)
    xb = devprobe.run(devprobe.GET2, b).view(F)[:, 0].reshape(32, -1)
    T.check_dimensions_decorrelated(xa, xb, f"device sampler dimensions, block {block}")


# ----------------------------------------------------------------------------------------------------------------------
# 4. scattering against optics
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_reflect_is_a_mirror(gpu):
    """hgd::reflect: unit length, r . n = -(i . n), r - i parallel to n, each within 8 float32 eps."""
    T.check_reflect(devprobe.run(devprobe.REFLECT, T.reflect_elements(T.optics_inputs())).view(F), "device reflect")


@pytest.mark.gpu
def test_gpu_refract_obeys_snell(gpu):
    """hgd::refract_tir: the TIR flag equals the float64 decision away from the critical angle; otherwise a unit
    direction in the plane of incidence, on the far side, with n1 sin theta1 = n2 sin theta2 within 1e-5 relative
    (grazing incidence left out); on TIR the mirror direction (HC:557-572)."""
    T.check_refract(devprobe.run(devprobe.REFRACT, T.refract_elements(T.optics_inputs())), "device refract")


@pytest.mark.gpu
def test_gpu_schlick_against_float64(gpu):
    """hgd::schlick_adjusted: inside [lo, hi]; lo + R0 (hi - lo) at normal incidence; hi beyond the critical angle;
    non-decreasing along 64 sweeps of 256 angles; within 1e-5 of the float64 formula away from the threshold."""
    val = devprobe.run(devprobe.SCHLICK, T.schlick_elements(T.optics_inputs())).view(F)
    sweep = devprobe.run(devprobe.SCHLICK, T.schlick_sweeps()).view(F)
    T.check_schlick(val, sweep, "device schlick")


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(T.DIFFUSE_NORMALS)))
def test_gpu_diffuse_scatter_is_cosine_weighted(gpu, k):
    """hgd::evaluate_hit's outgoing direction for a purely diffuse material over frames 1 .. 16384 of one pixel: unit, in
    the normal's hemisphere, the moments of a cosine-weighted hemisphere within 4 / sqrt(N) = 0.031; the next ray starts
    at pos + normal * 1e-4 (HC:710)."""
    out = devprobe.run_tables(devprobe.EVALUATE_HIT, T.diffuse_elements(k), materials=T.diffuse_material())
    T.check_diffuse(out, k, "device diffuse scatter")


# ----------------------------------------------------------------------------------------------------------------------
# 5. closed-form images
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["auto", "mega", "regen", "stream"])
@pytest.mark.parametrize("name", sorted(T.IMAGE_CASES))
def test_gpu_closed_form_image(gpu, name, kernel):
    """A convex diffuse object (or nothing) under a constant sky, 16 x 16, 256 accumulated frames, through the C-ABI on
    every kernel form: every pixel and channel within 2 L / N + N 2^-24 (E + L) of E + rho L; alpha 1, everything finite;
    the empty scene L within 4 ulp.  The derivation: test_oracle_closed_form_image."""
    from test_gpu_parity import gpu_render
    packed, params, cube, _, tol = T.image_case(name)
    img, cnt = gpu_render(packed, params, T.IMG_FRAMES, True, cube, kernel=kernel)
    assert cnt["paths"] == T.IMG_W * T.IMG_H * T.IMG_FRAMES
    assert cnt["primary_misses"] == (cnt["paths"] if tol is None else 0)
    T.check_image(img, name, f"device image ({kernel})")


@pytest.mark.gpu
def test_gpu_cube_faces(gpu):
    """hgd::sample_sky picks the face of the D3D table for 600 directions inside the faces of a cubemap whose faces
    are painted apart."""
    d = T.face_directions()
    x = np.concatenate([d.view(np.uint32), np.zeros((len(d), 1), np.uint32)], axis=1)  # direction, level 0
    T.check_faces(devprobe.run_tables(devprobe.SKY, x, cubemap=T.face_sky()).view(F), "device cube faces")
