"""Denoised display on the device (hg_update_guides, hg_readback_guides, hg_readback_begin_denoised; csrc/hg_denoise.hip).

1. Guides: bit for bit what camera_rays + trace_rays("closest") give for the same parameters and frame, and, with the
   stable rays, the oracle's debug views 2 and 1 (the blended expression of test_gpu_query.py); staleness.
2. Filter: the denoised readback equals hg_denoise_host of the plain readback and the guides, bit for bit (the host
   twin is held to the contract's numpy restatement by test_denoise.py), in every format and readback mode.
3. No side effects; plain and denoised readbacks interleaved.  4. Per-frame display beside the render server.
5. Quality: at 1 and 16 frames the denoised image is closer to the 2,048-frame render than the undenoised one.
6. Errors.  7. The pass refreshes the guides once per camera move."""
import ctypes as C
from dataclasses import replace
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  before the library's first context: both then share one HIP runtime (see test_gpu_query.py)

import cases
import denoise_ref as ref
import hg_oracle
from halogen import abi, render_pass as rp, scenes
from halogen.unity import Transform
from test_gpu_query import ORACLE_CASES, all_pixels, blended, copy_params
from test_gpu_server import _ctx, _sized

F = np.float32
INF = F(np.inf)
RGBA32F, RGBA16F, R11 = abi.HG_DISPLAY_RGBA32F, abi.HG_DISPLAY_RGBA16F, abi.HG_DISPLAY_R11G11B10F


def stable(params):
    """The parameters of guides that do not change from frame to frame: no jitter, no aperture."""
    return copy_params(params, filterRadius=0.0, focalConeAngle=0.0)


def rule(n_frames, iterations=3):
    """The pass's rule (render_pass.DenoiseSettings)."""
    return ref.params(iterations, 8.0 / np.sqrt(n_frames), 0.3, 0.0, 1)


def denoised(ctx, W, H, p, fmt=RGBA32F):
    ctx.readback_begin(fmt, denoise=p)
    return ctx.readback_end(W, H)


# ----------------------------------------------------------------------------------------------------------------------
# 1. guides
# ----------------------------------------------------------------------------------------------------------------------
def check_guides_against_queries(ctx, packed, params, frame, W, H):
    ctx.update_guides(params, frame)
    g0, g1 = ctx.guides()
    hits = ctx.trace_rays(ctx.camera_rays(params, frame, all_pixels(W, H))).reshape(H, W)
    hit = hits["kind"] != abi.HG_HIT_NONE
    assert hit.any() and (~hit).any()
    assert ref.same_bits(g0[..., :3], hits["normal"]) and ref.same_bits(g0[..., 3], hits["t"])
    assert np.all(g0[~hit] == np.array([0, 0, 0, INF], F))
    assert np.array_equal(g1[..., 3], hits["kind"].astype(F))
    albedo = np.array([[m.albedo.x, m.albedo.y, m.albedo.z] for m in packed.materials], F)
    want = np.where(hit[..., None], albedo[np.minimum(hits["material"], len(albedo) - 1)], F(1.0))
    assert ref.same_bits(g1[..., :3], want)
    return g0, g1, hit


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_gpu_guides_equal_the_queries_and_the_oracle(gpu, name):
    packed, params, cube, _, _ = cases.setup(name, first_frame=3)
    params = copy_params(params, samplesPerPixel=1)
    W, H = int(params.screenParameters.x), int(params.screenParameters.y)
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        ctx.resize(W, H)
        check_guides_against_queries(ctx, packed, params, 3, W, H)  # the very rays frame 3 traces: jitter, lens
        g0, g1, hit = check_guides_against_queries(ctx, packed, stable(params), 3, W, H)
        s1 = ctx.update_guides(stable(params), 1) or ctx.guides()
        assert ref.same_bits(s1[0], g0) and ref.same_bits(s1[1], g1)  # stable: the frame does not matter
    print(f"{name}: {int(hit.sum())} of {W * H} pixels hit")
    for mode, c in ((2, (g0[..., :3] + F(1.0)) / F(2.0)), (1, g1[..., :3])):
        img, _ = hg_oracle.render(packed, copy_params(stable(params), halogenDebugMode=mode, maxBounces=0), 1, True,
                                  cubemap=cube)
        want, got = blended(c), img.reshape(H, W, 4)[..., :3]
        bad = np.argwhere(hit & np.any(got.view(np.uint32) != want.view(np.uint32), axis=2))
        assert bad.size == 0, (name, mode, bad[:8])


@pytest.mark.gpu
def test_gpu_guides_odd_size_tiling_and_staleness(gpu):
    packed, params, _ = _sized("C1", 37, 23)
    other = cases.setup("glass_64x36")[0]
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        ctx.resize(37, 23)
        g0, g1, _ = check_guides_against_queries(ctx, packed, params, 5, 37, 23)
        ctx.set_tiling(1, 3)  # a tiled context computes the guides of the whole image
        ctx.update_guides(params, 5)
        t0, t1 = ctx.guides()
        assert ref.same_bits(t0, g0) and ref.same_bits(t1, g1)
        ctx.set_tiling(0, 1)
        ctx.update_guides(params, 5)
        ctx.upload_scene(packed)  # skipped: the guides stay
        assert ctx.counters()["scene_uploads_skipped"] == 1
        assert ref.same_bits(ctx.guides()[0], g0)
        ctx.resize(37, 24)
        with pytest.raises(abi.HalogenError) as e:
            ctx.guides()
        assert e.value.rc == abi.HG_E_INVALID and "hg_update_guides" in str(e.value)
        with pytest.raises(abi.HalogenError) as e:
            ctx.readback_begin(RGBA32F, denoise=rule(1))
        assert e.value.rc == abi.HG_E_INVALID and "hg_update_guides" in str(e.value)
        ctx.resize(37, 23)
        ctx.update_guides(params, 5)
        assert ref.same_bits(ctx.guides()[0], g0)
        ctx.upload_scene(other)  # rebuilt: stale
        with pytest.raises(abi.HalogenError) as e:
            ctx.guides()
        assert e.value.rc == abi.HG_E_INVALID


# ----------------------------------------------------------------------------------------------------------------------
# 2. the filter against the host twin
# ----------------------------------------------------------------------------------------------------------------------
SIGMAS = [(5.6, 0.3, 0.0), (0.0, 0.0, 0.0), (5.6, 0.0, 0.5), (0.5, 0.3, 0.2)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(37, 23), (64, 36), (200, 120)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_filter_equals_host_twin(gpu, size):
    """200x120 is larger than any one wave's block of pixels in both directions, and iteration 4's taps (step 16) cross
    block borders; 37x23 is no multiple of any block and narrower than two steps from iteration 4 on."""
    W, H = size
    packed, params, _ = _sized("C1", W, H)
    ctx, _, _ = _ctx(packed, params, server=0)
    with ctx:
        ctx.render(2, True)
        plain = ctx.readback(W, H)
        ctx.update_guides(stable(params), 1)
        g0, g1 = ctx.guides()
        assert np.isinf(g0[..., 3]).any() and (g1[..., 3] == 1).any()
        for iterations in (1, 2, 3, 4, 5):
            for demodulate in (0, 1):
                for sig in SIGMAS:
                    p = ref.params(iterations, *sig, demodulate)
                    got = denoised(ctx, W, H, p)
                    want = abi.denoise_host(plain, g0, g1, p)
                    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                    assert bad.size == 0, (size, iterations, demodulate, sig, len(bad), bad[:4])
        p = rule(2, 5)
        want = abi.denoise_host(plain, g0, g1, p)
        assert not ref.same_bits(want, plain)
        for stream in (0, 1, 2):  # HG_OPT_READBACK_STREAM: context stream, side stream, zero copy
            ctx.set_option(abi.HG_OPT_READBACK_STREAM, stream)
            for fmt in (RGBA32F, RGBA16F, R11):
                got = denoised(ctx, W, H, p, fmt)
                packed_want = abi.pack_display(want, fmt)
                assert got.dtype == packed_want.dtype and got.shape == packed_want.shape
                assert np.array_equal(got.view(np.uint8), packed_want.view(np.uint8)), (size, stream, fmt)
        assert ref.same_bits(ctx.readback(W, H), plain)  # never writes the accumulator


# ----------------------------------------------------------------------------------------------------------------------
# 3. no side effects, interleaving
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("server", [None, 0], ids=["default", "server_off"])
def test_gpu_denoised_readback_has_no_side_effects(gpu, server):
    keys = ("paths", "rays", "tri_tests", "aabb_tests", "hits", "launches")
    packed, params, cube, _, _ = cases.setup("c1_64")
    W = H = 64

    def make():
        ctx = abi.Context(0)
        if server is not None:
            ctx.set_option(abi.HG_OPT_SERVER, server)
        ctx.upload_scene(packed)
        ctx.resize(W, H)
        ctx.set_params(params)
        return ctx

    with make() as ctx:
        ctx.render(8, True)
        want8 = ctx.readback(W, H)
        want_cnt = ctx.counters()
    with make() as ctx:
        ctx.update_guides(stable(params), 1)
        g0, g1 = ctx.guides()
        ctx.render(4, True)
        plain4 = ctx.readback(W, H)
        cnt4 = ctx.counters()
        p, q = rule(4), ref.params(2, 1.0, 0.0, 0.4, 0)
        dp, dq = abi.denoise_host(plain4, g0, g1, p), abi.denoise_host(plain4, g0, g1, q)
        # plain and denoised begins interleaved at depth 2 come back in begin order
        for order in (("plain", p), (p, "plain"), (p, q), (q, p)):
            for what in order:
                ctx.readback_begin(RGBA32F, denoise=None if what == "plain" else what)
            for what in order:
                got = ctx.readback_end(W, H)
                want = plain4 if what == "plain" else dp if what is p else dq
                assert ref.same_bits(got, want), [w if w == "plain" else w.iterations for w in order]
        with pytest.raises(abi.HalogenError):  # a third begin at depth 2
            for _ in range(3):
                ctx.readback_begin(RGBA32F, denoise=p)
        assert ref.same_bits(ctx.readback_end(W, H), dp) and ref.same_bits(ctx.readback_end(W, H), dp)
        assert ref.same_bits(ctx.readback(W, H), plain4)
        cnt = ctx.counters()
        assert {k: cnt[k] for k in keys} == {k: cnt4[k] for k in keys}
        ctx.render(4, True)
        assert ref.same_bits(ctx.readback(W, H), want8)
        cnt = ctx.counters()
        assert {k: cnt[k] for k in keys[:5]} == {k: want_cnt[k] for k in keys[:5]}


# ----------------------------------------------------------------------------------------------------------------------
# 4. the per-frame display beside the render server
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_per_frame_denoised_display_keeps_the_server(gpu):
    packed, params, cube, _, _ = cases.setup("c1_64")
    W = H = 64
    frames = 8
    ref_ctx, _, _ = _ctx(packed, params, cube, server=0)
    with ref_ctx:
        ref_ctx.update_guides(stable(params), 1)
        g0, g1 = ref_ctx.guides()
        plain = []
        for _ in range(frames):
            ref_ctx.render(1, True)
            plain.append(ref_ctx.readback(W, H))
    launches = {}
    for kind in ("denoised", "plain"):
        ctx, _, _ = _ctx(packed, params, cube, server=2)
        with ctx:
            ctx.update_guides(stable(params), 1)  # before the loop: it stops a server
            for k in range(frames):
                ctx.render(1, True)
                if kind == "plain":
                    ctx.readback_begin(RGBA32F)
                    assert ref.same_bits(ctx.readback_end(W, H), plain[k]), k
                else:
                    got = denoised(ctx, W, H, rule(k + 1))
                    assert ref.same_bits(got, abi.denoise_host(plain[k], g0, g1, rule(k + 1))), k
            cnt = ctx.counters()
            launches[kind] = cnt["server_launches"]
            assert cnt["server_frames"] >= 1 and cnt["frames_lost"] == 0, cnt
    print(f"server lifetimes: {launches}")
    assert launches["plain"] >= 1 and launches["denoised"] == launches["plain"], launches


# ----------------------------------------------------------------------------------------------------------------------
# 5. quality
# ----------------------------------------------------------------------------------------------------------------------
def rms(a, b):
    d = np.clip(a[..., :3], 0, 4).astype(np.float64) - np.clip(b[..., :3], 0, 4)
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1_64", "glass_64x36", "dragon10_64x36"])
def test_gpu_denoised_preview_is_closer_to_the_converged_image(gpu, name):
    """The pass's rule (3 iterations, sigma_normal 0.3, depth off, sigma_color 8 / sqrt(N), demodulated) at N = 1 and
    16 against the library's own 2,048-frame render of the same parameters: a condition, not a measured threshold (the
    numpy restatement alone meets it with ratios 0.28-0.61 on the oracle's renders)."""
    packed, params, cube, _, _ = cases.setup(name)
    W, H = int(params.screenParameters.x), int(params.screenParameters.y)
    ctx, _, _ = _ctx(packed, params, cube, server=0, coalesce=32)
    with ctx:
        ctx.update_guides(stable(params), 1)
        out = {}
        ctx.render(1, True)
        out[1] = (ctx.readback(W, H), denoised(ctx, W, H, rule(1)))
        ctx.render(15, True)
        out[16] = (ctx.readback(W, H), denoised(ctx, W, H, rule(16)))
        ctx.render(2048 - 16, True)
        converged = ctx.readback(W, H)
    for n, (noisy, den) in out.items():
        e_noisy, e_den = rms(noisy, converged), rms(den, converged)
        print(f"{name} N={n}: rms noisy {e_noisy:.4f}, denoised {e_den:.4f}, ratio {e_den / e_noisy:.2f}")
        assert e_den < e_noisy, (name, n, e_den, e_noisy)


# ----------------------------------------------------------------------------------------------------------------------
# 6. errors
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_denoise_errors(gpu):
    L = abi.lib()
    packed, params, cube, _, _ = cases.setup("c1_64")
    good = rule(1)
    rc_of = lambda ctx, fn, *a: (fn(ctx._h, *a), L.hg_last_error(ctx._h).decode())
    with abi.Context(0) as ctx:
        assert rc_of(ctx, L.hg_update_guides, C.byref(params), 1)[0] == abi.HG_E_NOSCENE
        ctx.upload_scene(packed)
        assert rc_of(ctx, L.hg_update_guides, C.byref(params), 1)[0] == abi.HG_E_NOTARGET
        assert rc_of(ctx, L.hg_readback_begin_denoised, RGBA32F, C.byref(good))[0] == abi.HG_E_NOTARGET
        assert rc_of(ctx, L.hg_readback_guides, None, None, 0)[0] == abi.HG_E_NOTARGET
        ctx.resize(64, 64)
        ctx.set_params(params)
        rc, msg = rc_of(ctx, L.hg_readback_begin_denoised, RGBA32F, C.byref(good))
        assert rc == abi.HG_E_INVALID and "hg_update_guides" in msg  # no guides yet
        assert rc_of(ctx, L.hg_update_guides, None, 1)[0] == abi.HG_E_INVALID
        wrong = copy_params(params)
        wrong.screenParameters.x = 32.0
        assert rc_of(ctx, L.hg_update_guides, C.byref(wrong), 1)[0] == abi.HG_E_INVALID
        ctx.update_guides(params, 1)
        small = np.zeros(64 * 64 * 4 - 1, F)
        fp = small.ctypes.data_as(C.POINTER(C.c_float))
        assert rc_of(ctx, L.hg_readback_guides, fp, None, small.size)[0] == abi.HG_E_INVALID
        assert rc_of(ctx, L.hg_readback_guides, None, None, 64 * 64 * 4)[0] == abi.HG_OK  # either may be NULL
        assert rc_of(ctx, L.hg_readback_begin_denoised, RGBA32F, None)[0] == abi.HG_E_INVALID
        assert rc_of(ctx, L.hg_readback_begin_denoised, 3, C.byref(good))[0] == abi.HG_E_INVALID
        for bad in (ref.params(0), ref.params(7), ref.params(1, np.nan), ref.params(1, 0, 2e4), ref.params(1, 0, 0, 1e-5),
                    ref.params(1, flags=1), ref.params(1, demodulate=2)):
            assert rc_of(ctx, L.hg_readback_begin_denoised, RGBA32F, C.byref(bad))[0] == abi.HG_E_INVALID
        with pytest.raises(abi.HalogenError):
            ctx.readback_end(64, 64)  # nothing was begun by the refused calls
        ctx.set_tiling(0, 2)
        ctx.update_guides(params, 1)  # the guides of the whole image
        rc, msg = rc_of(ctx, L.hg_readback_begin_denoised, RGBA32F, C.byref(good))
        assert rc == abi.HG_E_UNSUPPORTED, msg


# ----------------------------------------------------------------------------------------------------------------------
# 7. the pass
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_pass_refreshes_guides_once_per_camera_move(gpu):
    scene = scenes.cornell_box()
    camera = scenes.cornell_camera(64, 64)
    settings = replace(scenes.settings_for(scenes.CONFIGS["C1"]))
    p = rp.HalogenRenderPass(settings)
    calls = []
    inner = p.ctx.update_guides
    p.ctx.update_guides = lambda params, frame: (calls.append((params.filterRadius, params.focalConeAngle, frame)),
                                                 inner(params, frame))[1]
    try:
        den = rp.DenoiseSettings()
        p.set_display(RGBA32F, 0, denoise=den)
        for k in range(1, 4):
            p.Execute(scene, camera, 1)
            shown = p.display()
            assert len(calls) == 1, calls
            g0, g1 = p.ctx.guides()
            want = abi.denoise_host(p.read_image(), g0, g1, rule(k))
            assert ref.same_bits(shown, want), k
        assert calls == [(0.0, 0.0, 1)]
        t = camera.transform
        moved = rp.Camera(Transform((t.position[0] + 0.05, t.position[1], t.position[2]), tuple(t.rotation)),
                          camera.fieldOfView, 64, 64)
        for k in range(1, 3):
            p.Execute(scene, moved, 1)
            shown = p.display()
            assert len(calls) == 2, calls
        m0, _ = p.ctx.guides()
        assert not ref.same_bits(m0, g0)
        assert ref.same_bits(shown, abi.denoise_host(p.read_image(), *p.ctx.guides(), rule(2)))
        p.set_display(RGBA32F, 0)  # off again: the plain image
        p.Execute(scene, moved, 1)
        assert ref.same_bits(p.display(), p.read_image()) and len(calls) == 2
    finally:
        p.Dispose()
