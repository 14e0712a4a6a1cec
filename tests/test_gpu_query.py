"""Ray queries over the uploaded scene (hg_trace_rays, hg_trace_rays_device, hg_camera_rays; csrc/hg_query.hip).

1. Chain to the oracle: the camera rays of every pixel, traced by the closest query, must name the normal, the
   material and the misses the oracle's debug views and primary-miss counter show for the same frame, bit for bit.
2. Distance, primitive, barycentrics: one identity-transform mesh of random triangles against the oracle's triangle
   test over every (ray, triangle) pair, for unbounded rays and for rays with a finite t_max around their hits.
3. Any-hit equals "closest reports a hit" on every ray of 1 and 2 (asserted where those rays are traced).
4. Wave edges and chunking, 5. the device-pointer form, 6. no side effects on renders, counters and tiling, 7. errors,
8. the pass helpers pick / autofocus.

The oracle renders one accumulated frame at FrameCount 3 into a cleared target, so its pixel is the frame's colour c
after the accumulation blend 0 * (1 - w) + c * w with w = 1 / 3 (AccumulationShader.shader:33, oracle render_job); the
expected pixel below is that expression in numpy float32 over c = (normal + 1) / 2 or the material's albedo.

The reference data of 2 is built from the oracle alone and its non-vacuity conditions are CPU tests of this file."""
import ctypes as C
from dataclasses import replace
from functools import lru_cache

import numpy as np
import pytest
import torch  # before the library's first context: a torch wheel that brings its own HIP runtime finds no device once
              # the system's runtime has opened it (torch first, the library binds to the runtime already loaded)

import cases
import hg_oracle
from halogen import abi, render_pass as rp, scenes
from halogen.scene import RayTracingMesh, Scene
from halogen.unity import Transform

F = np.float32
INF = F(np.inf)
EPS = F(0.0001)
ORACLE_CASES = ["c1_64", "c1_32_aperture", "glass_64x36", "dragon10_64x36"]


def words(a):
    """Records as rows of uint32 words."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


def copy_params(p, **kw):
    q = abi.HgParams.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def all_pixels(W, H):
    return np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)  # row-major


def closest_and_any(ctx, rays):
    """The closest query's hits; the any-hit query on the same rays must report a hit for exactly the same rays."""
    hits = ctx.trace_rays(rays, "closest")
    occ = ctx.trace_rays(rays, "any")
    differ = np.flatnonzero((hits["kind"] != 0) != (occ["kind"] != 0))
    assert differ.size == 0, (differ[:8], hits[differ[:8]], occ[differ[:8]])
    return hits


def blended(c):
    """The oracle's pixel after one accumulated frame at FrameCount 3 into a cleared target."""
    w = F(1.0) / F(3.0)
    return F(0.0) * (F(1.0) - w) + c.astype(F) * w


# ----------------------------------------------------------------------------------------------------------------------
# 1. chain to the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_gpu_query_chain_to_oracle(gpu, name):
    packed, params, cube, _, _ = cases.setup(name, first_frame=3)
    params = copy_params(params, samplesPerPixel=1)
    W, H = int(params.screenParameters.x), int(params.screenParameters.y)
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        rays = ctx.camera_rays(params, 3, all_pixels(W, H))
        assert np.all(rays["t_max"] == INF) and np.all(rays["flags"] == 0)
        hits = closest_and_any(ctx, rays)
    hit = hits["kind"] != abi.HG_HIT_NONE
    print(f"{name}: {int(hit.sum())} of {W * H} camera rays hit "
          f"({int((hits['kind'] == abi.HG_HIT_SPHERE).sum())} spheres)")
    assert hit.any() and np.all(hits["t"][~hit] == INF)
    assert np.all(words(hits)[~hit, 1:] == 0)
    # normals: debug view 2
    img, _ = hg_oracle.render(packed, copy_params(params, halogenDebugMode=2, maxBounces=0), 1, True, cubemap=cube)
    want = blended((hits["normal"] + F(1.0)) / F(2.0))
    got = img.reshape(-1, 4)[:, :3]
    bad = np.flatnonzero(hit & np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
    assert bad.size == 0, (name, "normal", bad[:8], got[bad[:8]], want[bad[:8]], hits[bad[:8]])
    # materials: debug view 1
    img, _ = hg_oracle.render(packed, copy_params(params, halogenDebugMode=1, maxBounces=0), 1, True, cubemap=cube)
    albedo = np.array([[m.albedo.x, m.albedo.y, m.albedo.z] for m in packed.materials], F)
    want = blended(albedo[np.minimum(hits["material"], len(albedo) - 1)])
    got = img.reshape(-1, 4)[:, :3]
    bad = np.flatnonzero(hit & np.any(got.view(np.uint32) != want.view(np.uint32), axis=1))
    assert bad.size == 0, (name, "albedo", bad[:8], got[bad[:8]], want[bad[:8]], hits[bad[:8]])
    # misses: the path tracer's primary-miss counter
    _, cnt = hg_oracle.render(packed, copy_params(params, halogenDebugMode=0, maxBounces=0), 1, True, cubemap=cube)
    assert cnt["primary_misses"] == int((~hit).sum()), (name, cnt["primary_misses"], int((~hit).sum()))


# ----------------------------------------------------------------------------------------------------------------------
# 2. distance, primitive, barycentrics against the oracle's triangle test
# ----------------------------------------------------------------------------------------------------------------------
N_TRIS, N_RAYS = 500, 4096


def _oracle_tri(rays7, tris18):
    out = np.empty((len(rays7), 5), np.uint32)
    fn = hg_oracle.lib().hgo_tri_accept_batch
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    fn(rays7.ctypes.data, tris18.ctypes.data, out.ctypes.data, len(rays7))
    return out


def _brute_force(o, d, t_max, tris):
    """Per ray, over every triangle with closest = t_max: the accepted t (INF where not accepted), u, v, front."""
    n, m = len(o), len(tris)
    t = np.empty((n, m), F)
    u, v = np.empty((n, m), F), np.empty((n, m), F)
    front = np.empty((n, m), bool)
    for at in range(0, n, 256):
        k = min(256, n - at)
        r7 = np.empty((k, m, 7), F)
        r7[:, :, 0:3], r7[:, :, 3:6], r7[:, :, 6] = o[at:at + k, None], d[at:at + k, None], t_max[at:at + k, None]
        out = _oracle_tri(r7.reshape(-1, 7), np.ascontiguousarray(np.broadcast_to(tris, (k, m, 18))).reshape(-1, 18))
        out = out.reshape(k, m, 5)
        acc = out[:, :, 0] != 0
        t[at:at + k] = np.where(acc, out[:, :, 1].view(F), INF)
        u[at:at + k], v[at:at + k], front[at:at + k] = out[:, :, 2].view(F), out[:, :, 3].view(F), out[:, :, 4] != 0
    return t, u, v, front


@lru_cache(maxsize=1)
def tri_case():
    """One identity-transform mesh of seeded random triangles, seeded unit rays (half unbounded, half with a finite
    t_max around the hit an unbounded ray finds) and the oracle's answer for each."""
    rng = np.random.default_rng(20240607)
    centre = rng.uniform(-1.0, 1.0, (N_TRIS, 1, 3))
    verts = (centre + 0.35 * rng.standard_normal((N_TRIS, 3, 3))).reshape(-1, 3).astype(F)
    normals = rng.standard_normal((N_TRIS * 3, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F)
    mesh = RayTracingMesh("random triangles", verts, normals, np.arange(N_TRIS * 3, dtype=np.int32).reshape(-1, 3),
                          Transform())
    scene = Scene()
    scene.add(mesh)
    packed = scene.pack()
    tris = np.frombuffer(bytes(packed.triangles), F).reshape(-1, 18)  # the reordered triangle list
    o = rng.standard_normal((N_RAYS, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.8, 0.8, (N_RAYS, 3)) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o, d = o.astype(F), d.astype(F)
    t_max = np.full(N_RAYS, INF, F)
    t0 = _brute_force(o, d, t_max, tris)[0].min(axis=1)
    half = N_RAYS // 2
    # finite t_max around the expected hit: well short, within the 1e-4 rules on both sides, exactly on it, well beyond
    scale = rng.choice(np.array([0.5, 0.99995, 0.99999, 1.0, 1.00001, 1.00005, 1.0002, 2.0]), N_RAYS - half)
    base = np.where(np.isfinite(t0[half:]), t0[half:], F(4.0))
    t_max[half:] = (base.astype(np.float64) * scale).astype(F)
    t, u, v, front = _brute_force(o, d, t_max, tris)
    tmin = t.min(axis=1)
    first = t.argmin(axis=1)
    hit = tmin < (t_max - EPS)  # float32: a mesh hit is accepted only below seed - 1e-4f
    rays = np.zeros((N_RAYS, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = o, t_max, d
    return {"packed": packed, "rays": rays, "t_max": t_max, "t": t, "u": u, "v": v, "front": front, "tmin": tmin,
            "first": first, "hit": hit, "tied": np.isfinite(tmin) & ((t == tmin[:, None]).sum(axis=1) > 1)}


def test_tri_case_is_not_vacuous(built):
    """On the oracle's data alone: the mesh-local ray is the world ray, most rays hit, finite t_max both cuts hits off
    and keeps them, the 1e-4 band is populated, and ties in t stay under 1 % of the rays."""
    c = tri_case()
    w2l = np.array(c["packed"].meshes[0].worldToLocal.m[:], F).reshape(4, 4)
    assert np.array_equal(w2l.view(np.uint32), np.eye(4, dtype=F).view(np.uint32))
    half = N_RAYS // 2
    hit, t_max, tmin = c["hit"], c["t_max"], c["tmin"]
    assert hit[:half].sum() > half // 2
    fin = slice(half, None)
    accepted = np.isfinite(tmin[fin])
    assert hit[fin].sum() > 200 and (~accepted).sum() > 200
    assert (accepted & ~hit[fin]).sum() > 20  # accepted below t_max, refused by seed - 1e-4f
    assert c["tied"].sum() < N_RAYS // 100


def check_tri_hits(hits, c, idx=None):
    """hits against tri_case()'s reference (for rays idx of it)."""
    idx = np.arange(N_RAYS) if idx is None else idx
    hit, first = c["hit"][idx], c["first"][idx]
    kind = hits["kind"]
    bad = np.flatnonzero((kind == abi.HG_HIT_MESH) != hit)
    assert bad.size == 0 and np.all(kind[~hit] == abi.HG_HIT_NONE), (bad[:8], hits[bad[:8]], c["tmin"][idx][bad[:8]])
    assert np.all(hits["t"][~hit] == INF) and np.all(words(hits)[~hit, 1:] == 0)
    h = np.flatnonzero(hit)
    assert np.array_equal(hits["t"][h].view(np.uint32), c["tmin"][idx][h].view(np.uint32))
    assert np.all(hits["object"][h] == 0) and np.all(hits["material"][h] == 0)
    unique = h[~c["tied"][idx][h]]
    assert np.array_equal(hits["primitive"][unique], first[unique].astype(np.uint32))
    for k in h:  # u, v, orientation: those of the named triangle, which must be one of minimal t
        r, p = idx[k], int(hits["primitive"][k])
        assert c["t"][r, p] == c["tmin"][r], (k, p)
        assert hits["u"][k].view(np.uint32) == c["u"][r, p].view(np.uint32), (k, p)
        assert hits["v"][k].view(np.uint32) == c["v"][r, p].view(np.uint32), (k, p)
        assert hits["orientation"][k] == (F(1.0) if c["front"][r, p] else F(-1.0)), (k, p)


@lru_cache(maxsize=1)
def tri_plain_hits():
    """The plain run of tri_case()'s rays (shared, never modified)."""
    c = tri_case()
    with abi.Context(0) as ctx:
        ctx.upload_scene(c["packed"])
        hits = closest_and_any(ctx, c["rays"])
    hits.setflags(write=False)
    return hits


@pytest.mark.gpu
def test_gpu_query_distance_primitive_barycentrics(gpu):
    c = tri_case()
    hits = tri_plain_hits()
    print(f"random triangles: {int(c['hit'].sum())} of {N_RAYS} rays hit, {int(c['tied'].sum())} with tied minima")
    check_tri_hits(hits, c)
    structured = np.zeros(N_RAYS, abi.RAY_DTYPE)  # the structured form of the same rays: the same bytes out
    structured["origin"], structured["t_max"], structured["direction"] = c["rays"][:, :3], c["rays"][:, 3], c["rays"][:, 4:7]
    with abi.Context(0) as ctx:
        ctx.upload_scene(c["packed"])
        assert np.array_equal(words(ctx.trace_rays(structured)), words(hits))


# ----------------------------------------------------------------------------------------------------------------------
# 4. wave edges and chunking, 5. device form
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_query_wave_edges_and_chunks(gpu):
    c = tri_case()
    plain = words(tri_plain_hits())
    with abi.Context(0) as ctx:
        ctx.upload_scene(c["packed"])
        for n in (0, 1, 63, 64, 65, (1 << 20) + 65):
            idx = np.arange(n) % N_RAYS
            hits = ctx.trace_rays(c["rays"][idx])
            assert hits.shape == (n,)
            assert np.array_equal(words(hits), plain[idx]) if n else True, n
            if n in (63, 65):
                occ = ctx.trace_rays(c["rays"][idx], "any")
                assert np.array_equal(occ["kind"] != 0, hits["kind"] != 0), n


@pytest.mark.gpu
def test_gpu_query_device_form(gpu):
    c = tri_case()
    plain = words(tri_plain_hits())
    with abi.Context(0) as ctx:
        ctx.upload_scene(c["packed"])
        for n in (N_RAYS, 65):
            d_rays = torch.from_numpy(c["rays"][:n].copy()).to("cuda:0")
            d_hits = ctx.trace_rays(d_rays)
            assert d_hits.is_cuda and tuple(d_hits.shape) == (n, 12) and d_hits.dtype == torch.float32
            assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), plain[:n]), n
        d_occ = ctx.trace_rays(d_rays, "any").cpu().numpy().view(np.uint32)
        assert np.array_equal(d_occ[:, 1] != 0, plain[:65, 1] != 0)
        assert ctx.trace_rays(torch.empty((0, 8), dtype=torch.float32, device="cuda:0")).shape == (0, 12)


# ----------------------------------------------------------------------------------------------------------------------
# 6. no side effects
# ----------------------------------------------------------------------------------------------------------------------
def _c1_ctx(server, tiling=None):
    packed, params, cube, _, _ = cases.setup("c1_64")
    W, H = int(params.screenParameters.x), int(params.screenParameters.y)
    ctx = abi.Context(0)
    if server is not None:
        ctx.set_option(abi.HG_OPT_SERVER, server)
    ctx.upload_scene(packed)
    ctx.resize(W, H)
    if tiling:
        ctx.set_tiling(*tiling)
    ctx.set_params(params)
    return ctx, params, W, H


@pytest.mark.gpu
@pytest.mark.parametrize("server", [None, 0], ids=["default", "server_off"])
def test_gpu_query_has_no_side_effects(gpu, server):
    keys = ("paths", "rays", "tri_tests", "aabb_tests")
    ctx, params, W, H = _c1_ctx(server)
    with ctx:
        ctx.render(8, True)
        want = ctx.readback(W, H)
        want_cnt = ctx.counters()
    ctx, params, W, H = _c1_ctx(server)
    with ctx:
        ctx.render(4, True)
        rays = ctx.camera_rays(params, 1, all_pixels(W, H))
        hits = ctx.trace_rays(rays)
        ctx.render(4, True)
        got = ctx.readback(W, H)
        cnt = ctx.counters()
    assert len(hits) == 4096 and (hits["kind"] != 0).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert {k: cnt[k] for k in keys} == {k: want_cnt[k] for k in keys}
    ctx, params, W, H = _c1_ctx(server, tiling=(1, 3))  # a tiled context answers for the whole scene
    with ctx:
        ctx.render(1, True)
        tiled = ctx.trace_rays(rays)
        assert np.array_equal(words(ctx.camera_rays(params, 1, all_pixels(W, H))), words(rays))
    assert np.array_equal(words(tiled), words(hits))


# ----------------------------------------------------------------------------------------------------------------------
# 7. errors
# ----------------------------------------------------------------------------------------------------------------------
def _rc(ctx, fn, *args):
    rc = fn(ctx._h, *args)
    return rc, abi.lib().hg_last_error(ctx._h).decode()


@pytest.mark.gpu
def test_gpu_query_errors(gpu):
    L = abi.lib()
    c = tri_case()
    good = np.ascontiguousarray(c["rays"][:8])
    out = np.zeros(8, abi.RAY_HIT_DTYPE)
    P = lambda a: C.c_void_p(a.ctypes.data)
    with abi.Context(0) as ctx:
        assert _rc(ctx, L.hg_trace_rays, P(good), 8, 0, P(out))[0] == abi.HG_E_NOSCENE
        assert _rc(ctx, L.hg_trace_rays_device, P(good), 8, 0, P(out))[0] == abi.HG_E_NOSCENE
        assert _rc(ctx, L.hg_trace_rays, None, 0, 0, None)[0] == abi.HG_OK  # n == 0: nothing to do, scene or not
        # hg_camera_rays needs no scene
        packed, params, _, _, _ = cases.setup("c1_64")
        assert len(ctx.camera_rays(params, 1, [(0, 0), (63, 63)])) == 2
        for bad_px in [(64, 0), (0, 64), (-1, 0), (0, -1)]:
            with pytest.raises(abi.HalogenError) as e:
                ctx.camera_rays(params, 1, [(1, 1), bad_px])
            assert e.value.rc == abi.HG_E_INVALID and "pixel 1" in str(e.value)
        px = np.zeros((1, 2), np.int32)
        ray = np.zeros(1, abi.RAY_DTYPE)
        assert _rc(ctx, L.hg_camera_rays, None, 1, P(px), 1, P(ray))[0] == abi.HG_E_INVALID
        assert _rc(ctx, L.hg_camera_rays, C.byref(params), 1, None, 1, P(ray))[0] == abi.HG_E_INVALID
        assert _rc(ctx, L.hg_camera_rays, C.byref(params), 1, P(px), 1, None)[0] == abi.HG_E_INVALID
        ctx.upload_scene(c["packed"])
        launches = ctx.counters()["launches"]
        assert _rc(ctx, L.hg_trace_rays, None, 8, 0, P(out))[0] == abi.HG_E_INVALID
        assert _rc(ctx, L.hg_trace_rays, P(good), 8, 0, None)[0] == abi.HG_E_INVALID
        assert _rc(ctx, L.hg_trace_rays_device, None, 8, 0, P(out))[0] == abi.HG_E_INVALID
        assert _rc(ctx, L.hg_trace_rays, P(good), -1, 0, P(out))[0] == abi.HG_E_INVALID
        for mode in (2, -1):
            assert _rc(ctx, L.hg_trace_rays, P(good), 8, mode, P(out))[0] == abi.HG_E_INVALID
            assert _rc(ctx, L.hg_trace_rays_device, P(good), 8, mode, P(out))[0] == abi.HG_E_INVALID
        for col, value, what in [(1, np.nan, "origin"), (0, np.inf, "origin"), (5, np.nan, "direction"),
                                 (6, -np.inf, "direction"), (3, np.nan, "t_max")]:
            bad = good.copy()
            bad[5, col] = value
            bad[7, col] = value
            out[:] = 0
            rc, msg = _rc(ctx, L.hg_trace_rays, P(bad), 8, 0, P(out))
            assert rc == abi.HG_E_INVALID and "ray 5" in msg and what in msg, (col, rc, msg)
            assert not words(out).any()  # nothing was traced
        bad = good.copy()
        bad[2, 4:7] = 0.0
        rc, msg = _rc(ctx, L.hg_trace_rays, P(bad), 8, 0, P(out))
        assert rc == abi.HG_E_INVALID and "ray 2" in msg and "zero direction" in msg
        # infinite t_max of either sign is a valid ray: -inf hits nothing
        neg = good.copy()
        neg[:, 3] = -np.inf
        assert np.all(ctx.trace_rays(neg)["kind"] == 0) and np.all(ctx.trace_rays(neg, "any")["kind"] == 0)
        assert ctx.counters()["launches"] == launches


# ----------------------------------------------------------------------------------------------------------------------
# 8. pass helpers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pick_and_autofocus(gpu):
    scene = scenes.cornell_box()
    camera = scenes.cornell_camera(64, 64)
    settings = replace(scenes.settings_for(scenes.CONFIGS["C1"]))  # a copy: autofocus writes the settings it is given
    tall = next(i for i, m in enumerate(scene.meshes) if m.name == "Cube")  # the 1.5 x 2.5 x 1.5 box
    p = rp.HalogenRenderPass(settings)
    try:
        p.Execute(scene, camera, 1)
        # the pinhole centre rays of every pixel, straight through the query
        params = rp.make_params(p.s, camera, p.FrameCount, len(scene.spheres), len(scene.meshes), False)
        params.filterRadius, params.focalConeAngle = 0.0, 0.0
        hits = p.ctx.trace_rays(p.ctx.camera_rays(params, p.FrameCount, all_pixels(64, 64))).reshape(64, 64)
        on_box = np.argwhere((hits["kind"] == abi.HG_HIT_MESH) & (hits["object"] == tall))
        # the box stands in the left half of the box's floor: its pixels lie left of the image centre
        assert len(on_box) > 40 and on_box[:, 1].mean() < 32
        y, x = (int(v) for v in on_box[len(on_box) // 2])
        kind, obj, t, rec = p.pick(x, y)
        assert kind == "mesh" and obj is scene.meshes[tall] and obj.name == "Cube"
        assert F(t).view(np.uint32) == hits[y, x]["t"].view(np.uint32)
        assert np.array_equal(words(np.asarray(rec).reshape(1)), words(np.asarray(hits[y, x]).reshape(1)))
        sph = np.argwhere(hits["kind"] == abi.HG_HIT_SPHERE)
        assert len(sph) and p.pick(int(sph[0][1]), int(sph[0][0]))[0] == "sphere"
        # the open front: a corner pixel sees past the box
        assert hits[0, 0]["kind"] == abi.HG_HIT_NONE and p.pick(0, 0) is None
        before = p.settings.FocalPlaneDistance
        assert p.autofocus(0, 0) is None and p.settings.FocalPlaneDistance == before
        frames = p.getFrameCount()
        assert frames == 2
        assert p.autofocus(x, y) == t and p.settings.FocalPlaneDistance == t and p.s["FocalPlaneDistance"] == t
        assert p.getFrameCount() == 1  # the lens changed: the accumulation restarts
        p.Execute(scene, camera, 1)
        assert scenes.CONFIGS["C1"].settings.FocalPlaneDistance == before  # the shared configuration is untouched
    finally:
        p.Dispose()
