"""The display denoiser on the host (hg_denoise_host, csrc/hg_host_denoise.cpp over csrc/hg_atrous.h): the edge-avoiding
a-trous filter of include/halogen_abi.h against its numpy float32 restatement (tests/denoise_ref.py), bit for bit; exact
properties of the contract; rejected parameters; the filter under AddressSanitizer + UBSan as a stand-alone program.

The device path is held to hg_denoise_host by tests/test_gpu_denoise.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_ref as ref
from halogen import abi
from host_programs import run_sanitizer_program

F = np.float32
W, H = 37, 23  # not a multiple of 8, and narrower than 2 * step from iteration 4 on: every border case occurs


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
def test_host_filter_equals_restatement(built, iterations, demodulate):
    rgba, g0, g1 = ref.random_case(W, H, 100 + iterations)
    for sc, sn, sz in itertools.product((0.0, 40.0), (0.0, 0.6), (-1.0, 0.5)):
        p = ref.params(iterations, sc, sn, sz, demodulate)
        got = abi.denoise_host(rgba, g0, g1, p)
        want = ref.restate(rgba, g0, g1, p)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, ((sc, sn, sz), len(bad), bad[:4], got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
        assert np.isfinite(got).all()
    # the terms do something on this data: each one on alone differs from all off
    off = abi.denoise_host(rgba, g0, g1, ref.params(iterations, 0, 0, 0, demodulate))
    for k, s in enumerate((40.0, 0.6, 0.5)):
        sig = [0.0, 0.0, 0.0]
        sig[k] = s
        assert not ref.same_bits(abi.denoise_host(rgba, g0, g1, ref.params(iterations, *sig, demodulate)), off), k


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (7, 1), (9, 5)])
def test_host_filter_small_images(built, size):
    w, h = size
    rgba, g0, g1 = ref.random_case(w, h, 7)
    for iterations in (1, 3, 6):
        p = ref.params(iterations, 3.0, 0.5, 0.5, 1)
        assert ref.same_bits(abi.denoise_host(rgba, g0, g1, p), ref.restate(rgba, g0, g1, p)), (size, iterations)


def test_impulse_gives_the_kernel_weights(built):
    """All terms off, one iteration, a unit impulse away from the border: the output at each tap is h exactly (dyadic
    weights that sum to 1, so every sum and the division are exact)."""
    rgba = np.zeros((H, W, 4), F)
    rgba[..., 3] = 0.5
    rgba[11, 18, :3] = (1.0, 2.0, 4.0)
    g0 = np.zeros((H, W, 4), F)
    g0[..., 1] = 1.0
    g0[..., 3] = 2.0
    g1 = np.ones((H, W, 4), F)
    got = abi.denoise_host(rgba, g0, g1, ref.params(1, 0, 0, 0, 0))
    want = np.zeros((H, W, 4), F)
    want[..., 3] = 0.5
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            h = ref.K[abs(dy)] * ref.K[abs(dx)]
            want[11 + dy, 18 + dx, :3] = h * np.array([1.0, 2.0, 4.0], F)
    assert ref.same_bits(got, want)
    assert want[..., 0].sum() == 1.0
    g0[...] = (0, 0, 0, np.inf)  # every pixel a miss: two misses are equal
    assert ref.same_bits(abi.denoise_host(rgba, g0, g1, ref.params(1, 0, 0.3, 0.5, 0)), want)


def test_constant_colour_stays_constant(built):
    """One iteration over a constant colour: within 52 * 2^-24 relative (25 products and two 25-term sums of positive
    numbers, each rounded once, and the division), whatever the guides weigh."""
    _, g0, g1 = ref.random_case(W, H, 3)
    rgba = np.empty((H, W, 4), F)
    rgba[...] = (0.7, 13.1, 1e-3, 1.0)
    for sig in [(0, 0, 0), (5.0, 0.3, 0.5), (0, 0.3, 0)]:
        got = abi.denoise_host(rgba, g0, g1, ref.params(1, *sig, 0))
        rel = np.abs(got.astype(np.float64) - rgba) / rgba
        print(f"sigmas {sig}: max relative deviation {rel.max() * 2 ** 24:.2f} * 2^-24")
        assert rel.max() <= 52 * 2.0 ** -24, (sig, rel.max() * 2 ** 24)
        assert ref.same_bits(got[..., 3], rgba[..., 3])


def test_orthogonal_half_planes_do_not_mix(built):
    """Two half-planes with orthogonal normals and sigma_normal 0.05: |dn|^2 * r = 800, below which hg_expf is exactly
    0, so one half's colours cannot reach the other half's output."""
    rng = np.random.default_rng(5)
    rgba = np.ones((H, W, 4), F)
    rgba[..., :3] = rng.random((H, W, 3)) * 3
    g0 = np.zeros((H, W, 4), F)
    g0[:, :19, 0] = 1.0
    g0[:, 19:, 1] = 1.0
    g0[..., 3] = 2.0
    g1 = np.ones((H, W, 4), F)
    g1[..., :3] = rng.random((H, W, 3))
    other = rgba.copy()
    other[:, 19:, :3] = rng.random((H, W - 19, 3)) * 50
    for demodulate in (0, 1):
        p = ref.params(4, 2.0, 0.05, 0.5, demodulate)
        a, b = abi.denoise_host(rgba, g0, g1, p), abi.denoise_host(other, g0, g1, p)
        assert ref.same_bits(a[:, :19], b[:, :19])
        assert not ref.same_bits(a[:, 19:], b[:, 19:])
        assert not ref.same_bits(a[:, :19], rgba[:, :19])  # (the left half was filtered)


def test_rejected_parameters(built):
    rgba, g0, g1 = ref.random_case(5, 4, 1)
    out = np.empty_like(rgba)
    fp = C.POINTER(C.c_float)
    L = abi.lib()

    def rc(p, w=5, h=4, a=rgba, b=g0, c=g1, o=out):
        ptr = lambda x: None if x is None else x.ctypes.data_as(fp)
        return L.hg_denoise_host(ptr(a), ptr(b), ptr(c), w, h, None if p is None else C.byref(p), ptr(o))

    assert rc(ref.params(3, 1.0, 0.3, 0.5, 1)) == abi.HG_OK
    assert rc(ref.params(6, 1e-4, 1e4, -np.inf, 0)) == abi.HG_OK
    bad = [ref.params(0), ref.params(7), ref.params(-1), ref.params(1, flags=1), ref.params(1, demodulate=2),
           ref.params(1, demodulate=-1)]
    for k in range(3):
        for s in (np.nan, 0.99e-4, 1.01e4, np.inf, 1e-30):
            sig = [1.0, 1.0, 1.0]
            sig[k] = s
            bad.append(ref.params(1, *sig))
    for p in bad:
        assert rc(p) == abi.HG_E_INVALID, (p.iterations, p.sigma_color, p.sigma_normal, p.sigma_depth, p.demodulate,
                                           p.flags)
        with pytest.raises(abi.HalogenError) as e:
            abi.denoise_host(rgba, g0, g1, p)
        assert e.value.rc == abi.HG_E_INVALID
    good = ref.params(1)
    assert rc(None) == abi.HG_E_INVALID
    assert rc(good, w=0) == abi.HG_E_INVALID and rc(good, h=-1) == abi.HG_E_INVALID
    for k in "abco":
        assert rc(good, **{k: None}) == abi.HG_E_INVALID, k


def test_host_filter_under_asan_ubsan():
    """hg_denoise_host as a stand-alone program built with -fsanitize=address,undefined from the host sources: 1x1, 1x7,
    7x1 and 37x23 images in exactly sized buffers, every term on and off, 1..6 iterations."""
    out = run_sanitizer_program("asan_denoise", 11)
    for size in ("1x1", "1x7", "7x1", "37x23"):
        assert f"{size}: 6 iteration counts x 16 settings, finite" in out, out
    assert "bad parameters rejected" in out
