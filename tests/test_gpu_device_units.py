"""The device building blocks, one at a time, against the CPU oracle's own functions.

Every other GPU correctness check compares rendered images, which exercises these functions only at the arguments a few
hundred thousand paths happen to produce.  Here the test-only probe library (csrc/hg_devprobe.hip, tests/devprobe.py)
evaluates the product's device functions themselves — hg_fmath.h, hgd::rcp_exact, hgd::Sampler, hgd::ray_aabb,
hgd::tri_accept<false/true>, hgd::isect_spheres — on inputs chosen to break them, and the results must equal the
oracle's (oracle/hg_oracle.c: hgo_fmath and the hgo_*_batch exports, which call the oracle's static functions) bit for
bit: uint32 views compared for equality, the sign of zero included; an element also passes when both sides are NaN
(x86 and gfx950 generate different default NaN patterns).

The input generators and the conditions that keep each input class from being vacuous (checked on the oracle's output
alone) run in CPU tests of this file (test_inputs_*), so they are verified without a GPU; the GPU tests reuse the same
generators.  The display packing test feeds the device untile/pack kernel the host packer's edge values through
hg_set_accumulation."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import cases
import devprobe
import hg_oracle
import test_display_pack
from halogen import abi

INF = np.float32(np.inf)
FN_NAMES = {0: "sin", 1: "cos", 2: "acos", 3: "tan", 4: "log", 5: "exp", 6: "round", 7: "rnorm", 8: "asin",
            9: "sincos.sin", 10: "sincos.cos", 11: "acos_fused"}
# the domains the path uses: tests/test_fmath.py FNS; [0, 2 pi] for the fused sincos; the rest chosen here (round:
# every float with a fraction; rnorm: test_rnorm_is_ieee's range; acos_fused: acos's)
FN_DOMAINS = {0: (0.0, 7.0), 1: (0.0, 7.0), 2: (-1.0, 1.0), 3: (0.0, 1.5), 4: (1e-3, 600.0), 5: (-80.0, 5.0),
              6: (-8388608.0, 8388608.0), 7: (1e-6, 1e6), 8: (-1.0, 1.0), 9: (0.0, 2 * np.pi), 10: (0.0, 2 * np.pi),
              11: (-1.0, 1.0)}
# hg_reduce_quadrant_ casts |x| * 4/pi to int: defined only for |x| <= 1e9 (include/hg_fmath.h); Inf and NaN stay in
TRIG_FNS = (0, 1, 3, 9, 10)


# ----------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------
def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


def ulp_steps(x, ks):
    """x (finite, non-zero float32) moved by k units in the last place of its magnitude, for every k in ks: (len(x) *
    len(ks),)."""
    b = u32(f32(x)).astype(np.int64)
    return from_bits((b[:, None] + np.asarray(ks, np.int64)[None, :]).ravel().astype(np.uint32))


def neighbours(x):
    return ulp_steps(f32(x).ravel(), (-1, 0, 1))


def _oracle(name, argtypes):
    fn = getattr(hg_oracle.lib(), name)
    fn.restype = None
    fn.argtypes = argtypes
    return fn


def oracle_fmath(fn, x):
    x = f32(x)
    y = np.empty_like(x)
    _oracle("hgo_fmath", [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64])(fn, x.ctypes.data, y.ctypes.data, x.size)
    return y


def oracle_rcp(x):
    x = f32(x)
    y = np.empty_like(x)
    _oracle("hgo_rcp_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, y.ctypes.data, x.size)
    return y


def oracle_pcg(v):
    v = np.ascontiguousarray(v, np.uint32)
    out = np.empty_like(v)
    _oracle("hgo_pcg_hash_batch", [C.c_void_p, C.c_void_p, C.c_int64])(v.ctypes.data, out.ctypes.data, v.size)
    return out


def oracle_sampler(tuples):
    t = np.ascontiguousarray(tuples, np.uint32)
    n = len(t)
    g1, g2 = np.empty(n, np.float32), np.empty((n, 2), np.float32)
    _oracle("hgo_sampler_batch", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64])(
        t.ctypes.data, g1.ctypes.data, g2.ctypes.data, n)
    return g1, g2


def oracle_aabb(x):
    x = f32(x)
    out = np.empty(len(x), np.float32)
    _oracle("hgo_aabb_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_tri(rays, tris):
    rays, tris = f32(rays), f32(tris)
    assert rays.shape[1] == 7 and tris.shape == (len(rays), 18)
    out = np.empty((len(rays), 5), np.uint32)
    _oracle("hgo_tri_accept_batch", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64])(
        rays.ctypes.data, tris.ctypes.data, out.ctypes.data, len(rays))
    return out


def oracle_spheres(x):
    x = f32(x)
    assert x.shape[1] == 20
    out = np.empty((len(x), 2), np.uint32)
    _oracle("hgo_sphere_accept_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, out.ctypes.data, len(x))
    return out


def assert_same_bits(got, want, inputs, what):
    """got / want: uint32, (n,) or (n, k).  Equal words, or NaN on both sides."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    both_nan = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
    bad = (got != want) & ~both_nan
    if bad.ndim > 1:
        bad = bad.any(axis=1)
    n_bad = int(bad.sum())
    print(f"{what}: {len(got)} inputs compared, {n_bad} differ")
    if n_bad:
        idx = np.nonzero(bad)[0][:5]
        inp = np.asarray(inputs).reshape(len(got), -1)
        rows = [f"  in {[hex(int(v)) for v in u32(inp[i])]} ({inp[i].tolist()}) device "
                f"{[hex(int(v)) for v in np.atleast_1d(got[i])]} oracle {[hex(int(v)) for v in np.atleast_1d(want[i])]}"
                for i in idx]
        pytest.fail(f"{what}: {n_bad} of {len(got)} inputs differ from the oracle; first {len(idx)}:\n" + "\n".join(rows))


def unit(v):
    v = f32(v)
    return f32(v / np.sqrt((v * v).sum(-1, keepdims=True), dtype=np.float32))


def split(n, shares):
    """Class name -> slice of range(n), sizes in proportion to the fixed shares (which sum to 1)."""
    assert abs(sum(s for _, s in shares) - 1.0) < 1e-9
    out, at = {}, 0
    for k, (name, s) in enumerate(shares):
        m = n - at if k == len(shares) - 1 else int(round(n * s))
        out[name] = slice(at, at + m)
        at += m
    return out


# ----------------------------------------------------------------------------------------------------------------------
# fmath
# ----------------------------------------------------------------------------------------------------------------------
def strided_bits(lo, hi, n):
    """n float32 values whose bit patterns are evenly strided over [lo, hi] (both signs when lo < 0 <= hi)."""
    lo, hi = np.float32(lo), np.float32(hi)
    if lo < 0 <= hi:
        neg = np.linspace(0x80000000, int(u32(np.array([lo]))[0]), n // 2).astype(np.uint32)
        pos = np.linspace(0, int(u32(np.array([hi]))[0]), n - n // 2).astype(np.uint32)
        return from_bits(np.concatenate([neg, pos]))
    a, b = sorted((int(u32(np.array([lo]))[0]), int(u32(np.array([hi]))[0])))
    return from_bits(np.linspace(a, b, n).astype(np.uint32))


@lru_cache(maxsize=1)
def fmath_edges():
    e = [from_bits([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                    0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F7FFFFF, 0xFF7FFFFF])]
    k = np.arange(0, 65)
    quarter = np.concatenate([f32(k * (np.pi / 4)), f32(k) * np.float32(np.pi / 4)])
    quarter = quarter[quarter != 0]
    e += [neighbours(quarter), -neighbours(quarter)]
    base = f32([1.0, 0.5, 1e-4])
    e += [ulp_steps(base, range(-4, 5)), -ulp_steps(base, range(-4, 5))]
    m = int(u32(f32([0.70710678]))[0]) & 0x7FFFFF  # log's mantissa split, under every exponent (denormals included)
    ex = np.arange(0, 255, dtype=np.uint32)[:, None] << 23
    e += [from_bits((ex | (np.uint32(m) + np.arange(-2, 3)).astype(np.uint32)[None, :]).ravel())]
    e += [from_bits(np.linspace(1, 0x7FFFFF, 4096).astype(np.uint32)), from_bits(1 << np.arange(0, 23))]  # denormals
    e += [ulp_steps(f32([88.72283905206835, -103.278929903431851103, 88.0, -87.33655]), range(-4, 5)),
          strided_bits(-103.3, -87.3, 1 << 16),  # exp's denormal results
          neighbours(f32(np.arange(-150, 130)[1:] * np.log(2.0))[np.arange(-150, 130)[1:] != 0])]
    half = f32(np.arange(-8, 9) + 0.5)
    e += [neighbours(half), neighbours(-half), f32([8388607.0, 8388608.0, 8388609.0, -8388607.0, -8388608.0, -8388609.0,
                                                    8388607.5, -8388607.5, 4194303.5, -4194303.5, 0.49999997, -0.49999997])]
    return f32(np.concatenate([f32(a).ravel() for a in e]))


@lru_cache(maxsize=1)
def fmath_random():
    return from_bits(np.random.default_rng(2024).integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32))


def fmath_inputs(fn):
    x = np.concatenate([strided_bits(*FN_DOMAINS[fn], 1 << 20), fmath_random(), fmath_edges()])
    if fn in TRIG_FNS:
        x = x[~(np.abs(x) > np.float32(1e9)) | np.isinf(x)]
    return f32(x)


def test_inputs_fmath(built):
    """The fmath input sets hold what they are meant to: the domain sweep, the whole-range random patterns and the edge
    list (special values, denormals, octant boundaries, exp's denormal-result band), and the oracle's results show that
    the edge cases are reached (denormal exp results, NaN / Inf results, both log branches)."""
    edges = fmath_edges()
    assert 60000 < edges.size < 200000
    for special in (0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F800000, 0xFF800000, 0x7FC00000):
        assert (u32(edges) == special).any(), hex(special)
    for fn in sorted(FN_NAMES):
        x = fmath_inputs(fn)
        lo, hi = FN_DOMAINS[fn]
        # (|x| > 1e9 is 38 % of the random bit patterns)
        assert x.size >= ((1 << 20) + (1 << 19) if fn in TRIG_FNS else 1 << 21), (fn, x.size)
        assert ((x >= lo) & (x <= hi)).sum() >= 1 << 20, fn
        if fn in TRIG_FNS:
            assert np.isinf(x).any() and np.isnan(x).any() and np.nanmax(np.abs(x[np.isfinite(x)])) <= 1e9
        else:
            assert np.nanmax(np.abs(x[np.isfinite(x)])) > 1e38
    y = oracle_fmath(5, fmath_inputs(5))
    denorm = (y != 0) & (np.abs(y) < np.float32(1.1754944e-38))
    assert denorm.sum() >= 1 << 15 and (y == INF).any() and (y == 0).any() and np.isnan(y).any()
    x = fmath_inputs(4)
    y = oracle_fmath(4, x)
    assert (np.isfinite(y) & (u32(x) < 0x00800000) & (x > 0)).sum() >= 4096, "log of denormals"
    assert (y == -INF).sum() >= 2 and np.isnan(y).any()


@pytest.mark.gpu
@pytest.mark.parametrize("fn", sorted(FN_NAMES), ids=lambda fn: FN_NAMES[fn].replace(".", "_"))
def test_gpu_fmath_matches_host(gpu, fn):
    """include/hg_fmath.h compiled for gfx950 returns the bits of its host compilation (hgo_fmath) on ~2^21 inputs per
    function: the path's domain, random patterns over all of float32 and the edge list; sin / cos / tan / sincos only
    where |x| <= 1e9 (the header's stated domain), Inf and NaN included."""
    x = fmath_inputs(fn)
    assert_same_bits(devprobe.run(fn, x), u32(oracle_fmath(fn, x)), x, f"hg_fmath {FN_NAMES[fn]}")


def oracle_fmath2(fn, x):
    x = f32(x)
    y = np.empty(len(x), np.float32)
    _oracle("hgo_fmath2", [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64])(fn, x.ctypes.data, y.ctypes.data, len(x))
    return y


@lru_cache(maxsize=1)
def minmax_pairs():
    """Every pairing of the special values (zeros, denormals, infinities, quiet and signalling NaNs of both signs), random
    bit patterns, and random equal pairs."""
    sp = from_bits([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                    0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                    0x7F800001, 0xFFA00000])
    a, b = np.meshgrid(sp, sp, indexing="ij")
    rnd = fmath_random()[:1 << 18].reshape(-1, 2)
    eq = np.repeat(fmath_random()[1 << 18:(1 << 18) + 4096], 2).reshape(-1, 2)
    mixed = np.stack([np.tile(sp, 256), fmath_random()[-len(sp) * 256:]], axis=1)
    return np.ascontiguousarray(np.concatenate([np.stack([a.ravel(), b.ravel()], 1), rnd, eq, mixed, mixed[:, ::-1]]),
                                np.float32)


def test_inputs_minmax(built):
    """hg_fminf / hg_fmaxf on the host: minimumNumber / maximumNumber (a NaN operand, quiet or signalling, is dropped),
    with -0 below +0 whichever operand comes first."""
    x = minmax_pairs()
    lo, hi = oracle_fmath2(12, x), oracle_fmath2(13, x)
    a, b = x[:, 0], x[:, 1]
    with np.errstate(invalid="ignore"):
        want_lo = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.minimum(a, b)))
        want_hi = np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.maximum(a, b)))
    zeros = (x[:, 0] == 0) & (x[:, 1] == 0)
    mixed = zeros & (u32(x[:, 0]) != u32(x[:, 1]))
    assert mixed.sum() >= 2 and np.isnan(x).any(1).sum() >= 100 and np.isnan(x).all(1).sum() >= 16
    assert np.array_equal(np.isnan(lo), np.isnan(x).all(1)) and np.array_equal(np.isnan(hi), np.isnan(x).all(1))
    ok = ~np.isnan(lo) & ~zeros
    assert np.array_equal(u32(lo[ok]), u32(want_lo[ok])) and np.array_equal(u32(hi[ok]), u32(want_hi[ok]))
    assert (u32(lo[mixed]) == 0x80000000).all() and (u32(hi[mixed]) == 0).all()
    same = zeros & ~mixed
    assert np.array_equal(u32(lo[same]), u32(x[same, 0])) and np.array_equal(u32(hi[same]), u32(x[same, 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("fn", [devprobe.FMIN, devprobe.FMAX], ids=["fmin", "fmax"])
def test_gpu_minmax_matches_host(gpu, fn):
    """hg_fminf / hg_fmaxf: the device compilation (v_min_f32 / v_max_f32) returns the bits of the header's compare /
    select definition, the sign of a zero result included."""
    x = minmax_pairs()
    assert_same_bits(devprobe.run(fn, x), u32(oracle_fmath2(fn, x)), x, f"hg_fmath {'fmin' if fn == devprobe.FMIN else 'fmax'}")


# ----------------------------------------------------------------------------------------------------------------------
# rcp_exact
# ----------------------------------------------------------------------------------------------------------------------
def rcp_inputs():
    mant = np.unique(np.concatenate([np.linspace(0, 0x7FFFFF, 1 << 15).astype(np.uint32),
                                     np.array([0, 0x7FFFFF], np.uint32)]))
    ex = np.array([0, 1, 2, 252, 253, 254, 255], np.uint32)
    sign = np.array([0, 0x80000000], np.uint32)
    return from_bits((sign[:, None, None] | (ex[None, :, None] << 23) | mant[None, None, :]).ravel())


def test_inputs_rcp():
    x = rcp_inputs()
    assert x.size == 2 * 7 * (1 << 15)
    ex = (u32(x) >> 23) & 0xFF
    for e in (0, 1, 2, 252, 253, 254, 255):  # the fallback exponents and the fast path's first and last
        assert (ex == e).sum() == 2 * (1 << 15)
    assert (x == 0).sum() == 2 and np.isinf(x).sum() == 2 and np.isnan(x).any()


@pytest.mark.gpu
def test_gpu_rcp_exact_is_ieee_division(gpu):
    """hgd::rcp_exact itself (not a restatement) equals float32(1) / x on the exponents where its fast path begins and
    ends (2, 252) and on every fallback exponent (0, 1, 253, 254, 255: zeros, denormals, huge values, Inf, NaN)."""
    x = rcp_inputs()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        want = f32(np.float32(1.0) / x)
    assert_same_bits(devprobe.run(devprobe.RCP, x), u32(want), x, "rcp_exact")


# ----------------------------------------------------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------------------------------------------------
BOUNCE_INC = 5


def sampler_frames():
    edge = [v for k in range(12, 33) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v != (1 << 32) + 1]
    rnd = np.random.default_rng(31).integers(0, 1 << 32, 1 << 18, dtype=np.uint64)
    # 2^32 itself is FrameCount 0 as the kernel's uint sees it
    return (np.concatenate([np.arange(4096, dtype=np.uint64), np.array(edge, np.uint64), rnd]) & 0xFFFFFFFF).astype(np.uint32)


def sampler_pixels():
    idx = np.concatenate([np.arange(64 * 36), np.arange(1920), 1079 * 1920 + np.arange(1920)]).astype(np.uint32)
    return oracle_pcg(idx)


def _draw_tuples(rng, n, frames, pixels):
    t = np.empty((n, 4), np.uint32)
    t[:, 0] = frames[rng.integers(0, len(frames), n)]
    t[:, 1] = pixels[rng.integers(0, len(pixels), n)]
    t[:, 2] = BOUNCE_INC * rng.integers(0, 301, n)
    t[:, 3] = rng.integers(0, 5, n)
    return t


@lru_cache(maxsize=1)
def sampler_tuples():
    """~2^20 (frame, pixel, offset, id) tuples: every frame of the set at least once, the rest drawn with a seeded
    generator; then widened, with further draws from the same sets, by every tuple among them whose get1 is exactly 0.0f
    or 1.0f in the oracle (float(u32) rounds up to 2^32 for the top 128 values: about one draw in 3e7)."""
    frames, pixels = sampler_frames(), sampler_pixels()
    rng = np.random.default_rng(77)
    t = _draw_tuples(rng, 1 << 20, frames, pixels)
    t[:len(frames), 0] = frames
    t[rng.permutation(len(t))[:len(pixels)], 1] = pixels
    g1, _ = oracle_sampler(t)
    extra = []
    for _ in range(256):
        if ((g1 == 0) | (g1 == 1)).any() or extra:
            break
        w = _draw_tuples(rng, 1 << 22, frames, pixels)
        gw, _ = oracle_sampler(w)
        hit = (gw == 0) | (gw == 1)
        if hit.any():
            extra.append(w[hit])
    return np.ascontiguousarray(np.concatenate([t] + extra))


def test_inputs_sampler(built):
    t = sampler_tuples()
    frames = sampler_frames()
    assert (1 << 20) <= len(t) < (1 << 20) + 64
    assert np.isin(frames, t[:, 0]).all() and np.isin(np.arange(4096), t[:, 0]).all()
    for v in (0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x80000001, 1279, 1280):
        assert (t[:, 0] == v).any(), v
    assert set(np.unique(t[:, 3])) == {0, 1, 2, 3, 4} and t[:, 2].max() == BOUNCE_INC * 300 and t[:, 2].min() == 0
    assert np.isin(sampler_pixels(), t[:, 1]).all() and len(np.unique(t[:, 1])) > 4000
    g1, g2 = oracle_sampler(t)
    assert ((g1 == 0) | (g1 == 1)).any(), "no get1 result where the float(u32) rounding shows"
    assert g1.min() >= 0 and g1.max() <= 1 and 0.45 < g1.mean() < 0.55 and 0.45 < g2.mean() < 0.55


@pytest.mark.gpu
def test_gpu_sampler_matches_oracle(gpu):
    """hgd::pcg_hash and hgd::Sampler::get1 / get2 (the closed-form Sobol) against the oracle's table-driven sampler:
    index = frame, dimension = offset + id, seed = pixel; frames up to 2^32 - 1, far beyond any rendered image's."""
    v = np.concatenate([np.arange(1 << 16, dtype=np.uint32), fmath_random().view(np.uint32)[:1 << 18],
                        np.array([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF], np.uint32)])
    assert_same_bits(devprobe.run(devprobe.PCG, v), oracle_pcg(v), v, "pcg_hash")
    t = sampler_tuples()
    g1, g2 = oracle_sampler(t)
    d1 = devprobe.run(devprobe.GET1, t)
    assert ((d1.view(np.float32) == 0) | (d1.view(np.float32) == 1)).any()
    assert_same_bits(d1, u32(g1), t, "Sampler::get1")
    assert_same_bits(devprobe.run(devprobe.GET2, t), u32(g2), t, "Sampler::get2")


# ----------------------------------------------------------------------------------------------------------------------
# ray_aabb
# ----------------------------------------------------------------------------------------------------------------------
N_AABB = 1 << 20
AABB_SHARES = [("random", 0.30), ("zero_dir", 0.15), ("on_plane", 0.15), ("inside", 0.10), ("behind", 0.10),
               ("flat", 0.10), ("huge", 0.10)]


def _boxes(rng, n):
    c, h = rng.uniform(-10, 10, (n, 3)), 10.0 ** rng.uniform(-2, 1, (n, 3))
    return f32(c - h), f32(c + h)


def _aimed(rng, A, B, o, aim):
    """Directions from o: towards a point of the box where aim, random elsewhere; a random length."""
    n = len(A)
    p = A + (B - A) * f32(rng.uniform(0, 1, (n, 3)))
    d = np.where(aim[:, None], p - o, rng.normal(0, 1, (n, 3)))
    return f32(unit(d) * f32(10.0 ** rng.uniform(-2, 2, (n, 1))))


def _zero_axes(rng, n, at_least_one=True):
    m = rng.random((n, 3)) < 0.5
    if at_least_one:
        m[np.arange(n), rng.integers(0, 3, n)] = True
    return m


def _signed_zero(rng, shape):
    return from_bits(np.where(rng.random(shape) < 0.5, 0x80000000, 0).astype(np.uint32))


@lru_cache(maxsize=1)
def aabb_cases():
    """(inputs (n, 12): A, B, o, inv; directions (n, 3); class -> slice).  inv is the oracle's own 1 / d."""
    rng = np.random.default_rng(404)
    cls = split(N_AABB, AABB_SHARES)
    A, B, o, d = (np.empty((N_AABB, 3), np.float32) for _ in range(4))

    def base(s, aim_share=0.5):
        n = s.stop - s.start
        A[s], B[s] = _boxes(rng, n)
        o[s] = f32(rng.uniform(-30, 30, (n, 3)))
        d[s] = _aimed(rng, A[s], B[s], o[s], rng.random(n) < aim_share)
        return n

    base(cls["random"])
    s = cls["zero_dir"]
    n = base(s)
    z = _zero_axes(rng, n)
    inside_slab = (rng.random(n) < 0.5)[:, None] & z  # half: the origin within the box's extent along the zeroed axes
    o[s] = np.where(inside_slab, A[s] + (B[s] - A[s]) * f32(rng.uniform(0, 1, (n, 3))), o[s])
    d[s] = np.where(z, _signed_zero(rng, (n, 3)), d[s])
    s = cls["on_plane"]
    n = base(s)
    z = _zero_axes(rng, n, at_least_one=False) | ((rng.random(n) < 0.7)[:, None] & _zero_axes(rng, n))
    on = np.where((rng.random(n) < 0.6)[:, None] & z.any(1)[:, None], z, _zero_axes(rng, n))  # 0 * inf where on & z
    inside_slab = ((rng.random(n) < 0.5)[:, None] & z & ~on) | (rng.random(n) < 0.25)[:, None]  # a quarter: in the box
    o[s] = np.where(inside_slab, A[s] + (B[s] - A[s]) * f32(rng.uniform(0.05, 0.95, (n, 3))), o[s])
    o[s] = np.where(on, np.where(rng.random((n, 3)) < 0.5, A[s], B[s]), o[s])
    d[s] = np.where(z, _signed_zero(rng, (n, 3)), d[s])
    s = cls["inside"]
    n = base(s, 0.0)
    o[s] = f32(A[s] + (B[s] - A[s]) * f32(rng.uniform(0.05, 0.95, (n, 3))))
    s = cls["behind"]
    base(s, 1.0)
    d[s] = -d[s]
    s = cls["flat"]
    n = base(s, 1.0)
    flat = _zero_axes(rng, n)
    B[s] = np.where(flat, A[s], B[s])
    kind = rng.integers(0, 3, n)[:, None]  # 0: aimed from outside; 1: the origin in the flat plane; 2: and d = 0 there
    d[s] = _aimed(rng, A[s], B[s], o[s], np.ones(n, bool))
    o[s] = np.where(flat & (kind >= 1), A[s], o[s])
    d[s] = np.where(flat & (kind == 2), _signed_zero(rng, (n, 3)), d[s])
    s = cls["huge"]
    n = s.stop - s.start
    big = lambda: f32(np.sign(rng.normal(size=(n, 3))) * 10.0 ** rng.uniform(18, 30, (n, 3)))
    p, q = big(), big()
    A[s], B[s], o[s] = np.minimum(p, q), np.maximum(p, q), big()
    with np.errstate(over="ignore", invalid="ignore"):
        aim = f32(A[s] * np.float32(0.5) + B[s] * np.float32(0.5)) - o[s]
        aim = f32(aim / np.abs(aim).max(1, keepdims=True))
    d[s] = np.where((rng.random(n) < 0.5)[:, None], aim, rng.normal(0, 1, (n, 3))) * f32(10.0 ** rng.uniform(-20, 20, (n, 1)))
    inv = oracle_rcp(d.ravel()).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([A, B, o, inv], axis=1), np.float32), d, cls


def test_inputs_aabb(built):
    """Each ray_aabb input class does what its name says, judged by the oracle's results."""
    x, d, cls = aabb_cases()
    t = oracle_aabb(x)
    A, B, o, inv = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12]
    with np.errstate(over="ignore", invalid="ignore"):
        t1, t2 = (A - o) * inv, (B - o) * inv
    has_nan = np.isnan(t1).any(1) | np.isnan(t2).any(1)
    overflow = np.isinf(t1).any(1) | np.isinf(t2).any(1)
    hit = np.isfinite(t)
    for name, s in cls.items():
        assert s.stop - s.start >= 1000, name
    assert 0.25 <= hit[cls["random"]].mean() <= 0.9
    s = cls["zero_dir"]
    assert np.isinf(inv[s]).any(1).all() and min(hit[s].sum(), (~hit[s]).sum()) >= 1000
    for k in (1, 2, 3):
        assert (np.isinf(inv[s]).sum(1) == k).sum() >= 1000, k
    assert (u32(inv[s]) == 0xFF800000).sum() >= 1000 and (u32(inv[s]) == 0x7F800000).sum() >= 1000
    s = cls["on_plane"]
    # (a NaN from 0 * Inf drops out of fminf / fmaxf and leaves the other plane's +-Inf: such a ray misses unless the
    # box is flat there, which the flat class covers)
    assert has_nan[s].sum() >= 1000 and min((hit & ~has_nan)[s].sum(), (~hit & has_nan)[s].sum()) >= 1000
    assert ((t == 0) & ~has_nan)[s].sum() >= 1000, "entry distance exactly 0: the sign of zero counts"
    assert (u32(t) == 0x80000000).sum() >= 100 and (u32(t) == 0).sum() >= 100
    assert hit[cls["inside"]].mean() >= 0.9 and (t[cls["inside"]] <= 0).mean() >= 0.9
    assert (~hit[cls["behind"]]).mean() >= 0.9
    s = cls["flat"]
    assert ((A[s] == B[s]).any(1)).all() and hit[s].sum() >= 1000 and (has_nan & hit)[s].sum() >= 1000
    s = cls["huge"]
    assert overflow[s].sum() >= 1000 and min(hit[s].sum(), (~hit[s]).sum()) >= 1000


@pytest.mark.gpu
def test_gpu_ray_aabb_matches_oracle(gpu):
    """hgd::ray_aabb against the oracle's on 2^20 cases: +-0 direction components (inv = +-Inf), origins on box planes (0 *
    Inf = NaN operands, entry distances of exactly +-0), flat boxes, overflowing products.  (With the C library's fminf /
    fmaxf in the oracle, 199 on_plane cases differed in the sign of a zero entry distance, e.g. A = (4.8537803,
    -3.8105218, -6.6392694), B = (8.932475, -3.7058723, -4.126132), o = (4.8537803, -3.7777355, -4.126132), inv =
    (110.54224, 1093.8691, -58.12669): +0 on the device, -0 from glibc's fmaxf(+0, -0); hg_fminf / hg_fmaxf of
    include/hg_fmath.h now define the operation for both sides.)"""
    x, d, cls = aabb_cases()
    want = u32(oracle_aabb(x))
    got = devprobe.run(devprobe.AABB, x)
    for name, s in cls.items():
        assert_same_bits(got[s], want[s], x[s], f"ray_aabb [{name}]")


# ----------------------------------------------------------------------------------------------------------------------
# tri_accept
# ----------------------------------------------------------------------------------------------------------------------
N_TRI = 1 << 19
TRI_SHARES = [("random", 0.25), ("lattice_edge", 0.15), ("det_threshold", 0.15), ("t_threshold", 0.10),
              ("best_t", 0.10), ("degenerate", 0.10), ("back_face", 0.15)]
ULPS = np.arange(-4, 5)


def pack_triangles(pa, pb, pc):
    """HalogenTriangle records ((n, 18) float32) through the product's exported hg_pack_triangles."""
    n = len(pa)
    V = np.ascontiguousarray(np.stack([pa, pb, pc], axis=1).reshape(-1, 3), np.float32)
    N = np.zeros_like(V)
    idx = np.arange(3 * n, dtype=np.int32)
    out = np.empty((n, 18), np.float32)
    rc = abi.lib().hg_pack_triangles(V.ctypes.data, N.ctypes.data, 3 * n, idx.ctypes.data, n, out.ctypes.data)
    assert rc == 0, rc
    return out


def device_tri_inputs(rays, tris):
    """(lo, ld, best_t, v0, e1, e2): the 36-B device record is v0 and the fp32 edges, as hg_upload_scene forms them."""
    v0, v1, v2 = tris[:, 0:3], tris[:, 3:6], tris[:, 6:9]
    return np.ascontiguousarray(np.concatenate([rays, v0, f32(v1 - v0), f32(v2 - v0)], axis=1), np.float32)


def _axis_case(rng, n):
    """Triangles v0, v0 + (a, 0, 0), v0 + (0, b, 0) (a, b powers of two, v0.z = 0) under rays along -z: det = -dz a b, U
    = tx / a, V = ty / b, t = -tz / dz, each exact; (v0, a, b, u, v) with the hit (u, v) well inside."""
    v0 = np.concatenate([f32(rng.integers(-64, 65, (n, 2)) / 8.0), np.zeros((n, 1), np.float32)], axis=1)
    a, b = (f32(2.0 ** rng.integers(-2, 3, n)) for _ in range(2))
    u, v = f32(rng.integers(1, 4, n) / 8.0), f32(rng.integers(1, 4, n) / 8.0)
    return v0, a, b, u, v


@lru_cache(maxsize=1)
def tri_cases():
    """(rays (n, 7): o, d, best_t; HalogenTriangle records (n, 18); class -> slice)."""
    rng = np.random.default_rng(909)
    cls = split(N_TRI, TRI_SHARES)
    pa, pb, pc, o, d = (np.zeros((N_TRI, 3), np.float32) for _ in range(5))
    best = np.full(N_TRI, INF, np.float32)

    def random_hits(s, aim_share):
        n = s.stop - s.start
        pa[s], pb[s], pc[s] = (f32(rng.uniform(-5, 5, (n, 3))) for _ in range(3))
        o[s] = f32(rng.uniform(-20, 20, (n, 3)))
        w = rng.dirichlet((1, 1, 1), n)
        p = pa[s] * w[:, :1] + pb[s] * w[:, 1:2] + pc[s] * w[:, 2:]
        aim = rng.random(n) < aim_share
        dd = np.where(aim[:, None], p - o[s], rng.normal(0, 1, (n, 3)))
        d[s] = f32(unit(dd) * f32(10.0 ** rng.uniform(-1, 1, (n, 1))))
        return n

    s = cls["random"]
    n = random_hits(s, 0.5)
    best[s] = np.where(rng.random(n) < 0.5, INF, f32(10.0 ** rng.uniform(-1, 2.5, n)))

    s = cls["lattice_edge"]  # even integer vertices: vertices and edge midpoints are lattice points, all arithmetic exact
    n = s.stop - s.start
    pa[s], pb[s], pc[s] = (f32(2 * rng.integers(-4, 5, (n, 3))) for _ in range(3))
    spot = rng.integers(0, 6, n)[:, None]  # A, B, C, mid AB, mid BC, mid CA
    p = np.select([spot == 0, spot == 1, spot == 2, spot == 3, spot == 4],
                  [pa[s], pb[s], pc[s], (pa[s] + pb[s]) / 2, (pb[s] + pc[s]) / 2], (pc[s] + pa[s]) / 2)
    o[s] = f32(rng.integers(-12, 13, (n, 3)))
    d[s] = f32(p - o[s])  # t = 1

    s = cls["det_threshold"]
    n = s.stop - s.start
    v0, a, b, u, v = _axis_case(rng, n)
    kind = rng.integers(0, 11, n)  # 0..8: |det| = 1e-8 moved by -4..4 ulp; 9, 10: det = +-0
    mag = ulp_steps(f32([1e-8]), ULPS)[np.minimum(kind, 8)]
    det = np.where(kind >= 9, np.float32(0), mag) * np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1))
    dz = f32(-det / (a * b))  # exact: a, b powers of two
    pa[s], pb[s], pc[s] = v0, v0 + np.stack([a, 0 * a, 0 * a], 1), v0 + np.stack([0 * b, b, 0 * b], 1)
    tz = f32(rng.uniform(0.25, 2.0, n)) * np.abs(dz) * np.where(dz < 0, 1, -1)  # t = -tz / dz in (0.25, 2)
    tz = np.where(det == 0, np.float32(1e-8), tz)
    o[s] = v0 + np.stack([u * a, v * b, f32(tz)], 1)
    d[s] = np.stack([0 * dz, 0 * dz, dz], 1)

    s = cls["t_threshold"]
    n = s.stop - s.start
    v0, a, b, u, v = _axis_case(rng, n)
    pa[s], pb[s], pc[s] = v0, v0 + np.stack([a, 0 * a, 0 * a], 1), v0 + np.stack([0 * b, b, 0 * b], 1)
    tt = ulp_steps(f32([1e-4]), ULPS)[rng.integers(0, 9, n)]
    dz = f32(-(2.0 ** rng.integers(-1, 2, n)))  # t = -tz / dz: exact scalings of the threshold neighbours ...
    o[s] = v0 + np.stack([u * a, v * b, f32(-tt * dz)], 1)
    d[s] = np.stack([0 * dz, 0 * dz, f32(dz / (a * b)) * a * b], 1)
    flip = rng.random(n) < 0.5  # ... seen from either side of the triangle (det > 0 / < 0): swap e1 and e2
    pb[s], pc[s] = np.where(flip[:, None], pc[s], pb[s]), np.where(flip[:, None], pb[s], pc[s])

    s = cls["best_t"]
    n = random_hits(s, 1.0)
    t_hit = oracle_tri(np.concatenate([o[s], d[s], best[s, None]], 1), pack_triangles(pa[s], pb[s], pc[s]))[:, 1]
    t_hit = t_hit.view(np.float32)
    kind = rng.integers(0, 4, n)  # the hit's own t, its two neighbours, +Inf
    near = ulp_steps(np.where(np.isfinite(t_hit) & (t_hit > 0), t_hit, np.float32(1)), (-1, 0, 1)).reshape(n, 3)
    best[s] = np.where(kind == 3, INF, near[np.arange(n), np.minimum(kind, 2)])

    s = cls["degenerate"]
    n = random_hits(s, 1.0)
    kind = rng.integers(0, 4, n)[:, None]  # B = A; C = A; C on line AB (exactly, on a lattice); C = B
    lat = f32(rng.integers(-8, 9, (n, 3)))
    pa[s] = np.where(kind == 2, lat, pa[s])
    pb[s] = np.where(kind == 0, pa[s], np.where(kind == 2, lat + f32(rng.integers(-3, 4, (n, 3))), pb[s]))
    pc[s] = np.where(kind == 1, pa[s], np.where(kind == 2, pa[s] + 3 * (pb[s] - pa[s]), np.where(kind == 3, pb[s], pc[s])))

    s = cls["back_face"]
    n = random_hits(s, 1.0)
    tris = pack_triangles(pa[s], pb[s], pc[s])
    front = oracle_tri(np.concatenate([o[s], d[s], best[s, None]], 1), tris)[:, 4] == 1
    pb[s], pc[s] = np.where(front[:, None], pc[s], pb[s]), np.where(front[:, None], pb[s], pc[s])

    rays = np.ascontiguousarray(np.concatenate([o, d, best[:, None]], axis=1), np.float32)
    return rays, pack_triangles(pa, pb, pc), cls


def test_inputs_tri(built):
    """Each tri_accept input class reaches its edge, judged by the oracle's results."""
    rays, tris, cls = tri_cases()
    r = oracle_tri(rays, tris)
    acc, t, U, V, front = r[:, 0] == 1, r[:, 1].view(np.float32), r[:, 2].view(np.float32), r[:, 3].view(np.float32), r[:, 4] == 1
    for name, s in cls.items():
        assert s.stop - s.start >= 1000, name
    s = cls["random"]
    assert acc[s].mean() >= 0.25 * 0.5 and min(acc[s].sum(), (~acc[s]).sum()) >= 1000
    assert (np.isfinite(t[s]) & ~acc[s]).sum() >= 1000, "hits rejected by best_t"
    s = cls["lattice_edge"]
    on_edge = np.isfinite(t[s]) & ((U[s] == 0) | (V[s] == 0) | (U[s] + V[s] == 1))
    assert (np.isfinite(t[s]) & ((U[s] == 0) | (U[s] + V[s] == 1))).sum() >= 100 and on_edge.sum() >= 1000
    assert (np.isfinite(t[s]) & (U[s] == 0) & (V[s] == 0)).sum() >= 100, "vertex hits"
    s = cls["det_threshold"]  # by construction U, V, t and best_t accept: a rejection is the determinant test's
    assert min(acc[s].sum(), (~acc[s]).sum()) >= 1000 and min((acc & front)[s].sum(), (acc & ~front)[s].sum()) >= 1000
    s = cls["t_threshold"]
    assert min(acc[s].sum(), (~acc[s]).sum()) >= 1000 and np.isfinite(t[s]).all()
    assert (np.abs(u32(t[s]).astype(np.int64) - int(u32(f32([1e-4]))[0])) <= 4).all()
    assert min((acc & front)[s].sum(), (acc & ~front)[s].sum()) >= 1000
    s = cls["best_t"]
    assert min(acc[s].sum(), (~acc[s]).sum()) >= 1000 and (np.isfinite(t[s]) & (t[s] == rays[s, 6])).sum() >= 1000
    assert (~acc[cls["degenerate"]]).mean() >= 0.9
    s = cls["back_face"]
    assert (acc & ~front)[s].mean() >= 0.25


@pytest.mark.gpu
@pytest.mark.parametrize("flat", [False, True], ids=["branchy", "flat"])
def test_gpu_tri_accept_matches_oracle(gpu, flat):
    """hgd::tri_accept<false / true> on records built with hg_pack_triangles against the oracle's triangle test plus the
    mesh loop's accept rule (HC:416): the accept flag everywhere; t, U, V and the facing where the oracle accepts."""
    rays, tris, cls = tri_cases()
    x = device_tri_inputs(rays, tris)
    want = oracle_tri(rays, tris)
    got = devprobe.run(devprobe.TRI_FLAT if flat else devprobe.TRI, x)
    rejected = want[:, 0] == 0
    got, want = got.copy(), want.copy()
    got[rejected, 1:] = 0  # compare only the flag where the oracle rejects
    want[rejected, 1:] = 0
    for name, s in cls.items():
        assert_same_bits(got[s], want[s], x[s], f"tri_accept<{str(flat).lower()}> [{name}]")


# ----------------------------------------------------------------------------------------------------------------------
# isect_spheres, one sphere
# ----------------------------------------------------------------------------------------------------------------------
N_SPH = 1 << 19
SPH_SHARES = [("outside", 0.30), ("inside", 0.15), ("surface", 0.15), ("tangent", 0.15), ("hd_threshold", 0.15),
              ("box_at_far", 0.10)]
HD_BITS = int(u32(f32([1e-4]))[0])


def _np_hd(o, d, c, r):
    """sphere_intersection's front root in numpy float32 (the same IEEE operations), for choosing inputs."""
    sh = f32(o - c)
    dot = lambda p, q: f32(f32(p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2])
    bq = f32(np.float32(2) * dot(sh, d))
    cq = f32(dot(sh, sh) - r * r)
    disc = f32(bq * bq - np.float32(4) * cq)
    with np.errstate(invalid="ignore"):
        return f32((-bq - np.sqrt(disc)) / np.float32(2)), disc


@lru_cache(maxsize=1)
def sphere_cases():
    """(inputs (n, 20): o, d, closest, far, (centre, radius), (cornerA, 0), (cornerB, 0); class -> slice)."""
    rng = np.random.default_rng(1212)
    cls = split(N_SPH, SPH_SHARES)
    n_all = N_SPH
    c = f32(rng.uniform(-10, 10, (n_all, 3)))
    r = f32(10.0 ** rng.uniform(-1, 1, n_all))
    o, d = np.zeros((n_all, 3), np.float32), np.zeros((n_all, 3), np.float32)
    closest = np.full(n_all, INF, np.float32)
    far = np.full(n_all, 1000.0, np.float32)

    def aimed(s, share):
        n = s.stop - s.start
        p = c[s] + unit(rng.normal(0, 1, (n, 3))) * (r[s] * f32(rng.uniform(0, 0.95, n)))[:, None]
        dd = np.where((rng.random(n) < share)[:, None], p - o[s], rng.normal(0, 1, (n, 3)))
        d[s] = unit(dd)

    s = cls["outside"]
    n = s.stop - s.start
    o[s] = c[s] + unit(rng.normal(0, 1, (n, 3))) * (r[s] * f32(rng.uniform(1.05, 6, n)))[:, None]
    aimed(s, 0.5)
    closest[s] = np.where(rng.random(n) < 0.5, INF, f32(10.0 ** rng.uniform(-1, 2, n)))
    s = cls["inside"]
    n = s.stop - s.start
    o[s] = c[s] + unit(rng.normal(0, 1, (n, 3))) * (r[s] * f32(rng.uniform(0, 0.95, n)))[:, None]
    aimed(s, 0.0)
    s = cls["surface"]
    n = s.stop - s.start
    o[s] = f32(c[s] + unit(rng.normal(0, 1, (n, 3))) * r[s, None])
    aimed(s, 0.5)

    s = cls["tangent"]  # centre 0, ray along an axis at lateral offset r (+- ulps): disc = 0 exactly for lattice values
    n = s.stop - s.start
    c[s] = 0
    lattice = rng.random(n) < 0.5
    r[s] = np.where(lattice, f32(rng.integers(1, 17, n)), r[s])
    L = np.where(lattice, f32(rng.integers(1, 17, n)), f32(rng.uniform(1, 16, n)))
    off = ulp_steps(r[s], ULPS).reshape(n, 9)[np.arange(n), rng.integers(0, 9, n)]
    ax = rng.integers(0, 3, n)
    sgn = np.where(rng.random(n) < 0.5, np.float32(-1), np.float32(1))
    oo, dd = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    oo[np.arange(n), ax] = -L * sgn
    oo[np.arange(n), (ax + 1) % 3] = off
    dd[np.arange(n), ax] = sgn
    o[s], d[s] = oo, dd

    s = cls["hd_threshold"]  # tiny spheres, so that the root's ulp is that of 1e-4: candidates kept by their root
    n = s.stop - s.start
    m = 8 * n
    rr = f32(2.0 ** rng.integers(-14, -10, m))
    h = ulp_steps(f32([1e-4]), np.arange(-64, 65))[rng.integers(0, 129, m)]
    ax, sgn = rng.integers(0, 3, m), np.where(rng.random(m) < 0.5, np.float32(-1), np.float32(1))
    cc = f32(rng.integers(-4, 5, (m, 3)) * 0)  # centre 0: the origin's coordinates keep their last places
    oo, dd = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
    oo[np.arange(m), ax] = -f32(rr + h) * sgn
    dd[np.arange(m), ax] = sgn
    hd, _ = _np_hd(oo, dd, cc, rr)
    dist = np.abs(u32(hd).astype(np.int64) - HD_BITS)
    order = np.argsort(dist, kind="stable")[:n]
    order = order[rng.permutation(n)]
    c[s], r[s], o[s], d[s] = cc[order], rr[order], oo[order], dd[order]

    s = cls["box_at_far"]
    n = s.stop - s.start
    o[s] = c[s] + unit(rng.normal(0, 1, (n, 3))) * (r[s] * f32(rng.uniform(2.5, 6, n)))[:, None]
    aimed(s, 1.0)

    pad = np.ones(n_all, np.float32)
    pad[cls["tangent"]] = 2  # (a tangent ray grazes the tight box too, whose test would decide first)
    A, B = f32(c - (r * pad)[:, None]), f32(c + (r * pad)[:, None])
    s = cls["box_at_far"]
    n = s.stop - s.start
    inv = oracle_rcp(d[s].ravel()).reshape(-1, 3)
    entry = oracle_aabb(np.concatenate([A[s], B[s], o[s], inv], 1))
    ok = np.isfinite(entry) & (entry > 0)
    step = ulp_steps(np.where(ok, entry, np.float32(1)), (-1, 0, 1)).reshape(n, 3)
    far[s] = np.where(ok, step[np.arange(n), rng.integers(0, 3, n)], far[s])
    z = np.zeros((n_all, 1), np.float32)
    x = np.concatenate([o, d, closest[:, None], far[:, None], c, r[:, None], A, z, B, z], axis=1)
    return np.ascontiguousarray(x, np.float32), cls


def test_inputs_spheres(built):
    """Each isect_spheres input class reaches its edge, judged by the oracle's results."""
    x, cls = sphere_cases()
    r = oracle_spheres(x)
    acc, back, t = r[:, 0] != 0xFFFFFFFF, r[:, 0] == 0x80000000, r[:, 1].view(np.float32)
    for name, s in cls.items():
        assert s.stop - s.start >= 1000, name
    assert (acc & ~back)[cls["outside"]].mean() >= 0.25 * 0.5 and (~acc)[cls["outside"]].sum() >= 1000
    assert (acc & back)[cls["inside"]].mean() >= 0.9
    s = cls["surface"]
    # (from the surface the front root is ~0: below 1e-4 and rejected, or negative and the back root is taken)
    assert min((acc & back)[s].sum(), (~acc)[s].sum()) >= 1000
    s = cls["tangent"]
    hd, disc = _np_hd(x[s, 0:3], x[s, 3:6], x[s, 8:11], x[s, 11])
    assert (disc == 0).sum() >= 1000 and min(acc[s].sum(), (~acc)[s].sum()) >= 1000
    assert np.array_equal(acc[s], disc >= 0), "an axis ray's acceptance is the discriminant's sign"
    s = cls["hd_threshold"]
    hd, disc = _np_hd(x[s, 0:3], x[s, 3:6], x[s, 8:11], x[s, 11])
    assert (np.abs(u32(hd).astype(np.int64) - HD_BITS) <= 4).sum() >= 1000
    assert min(acc[s].sum(), (~acc)[s].sum()) >= 1000
    assert np.array_equal(u32(t[s][acc[s]]), u32(hd[acc[s]])), "the numpy restatement that chose the inputs"
    s = cls["box_at_far"]
    assert min(acc[s].sum(), (~acc)[s].sum()) >= 1000


@pytest.mark.gpu
def test_gpu_isect_spheres_matches_oracle(gpu):
    """hgd::isect_spheres over a one-sphere HgKernelParams against the oracle's sphere loop (HC:357-376): the accepted
    sphere reference (index | back-face bit, or none) and the closest distance afterwards."""
    x, cls = sphere_cases()
    want = oracle_spheres(x)
    got = devprobe.run(devprobe.SPHERES, x)
    for name, s in cls.items():
        assert_same_bits(got[s], want[s], x[s], f"isect_spheres [{name}]")


# ----------------------------------------------------------------------------------------------------------------------
# display packing on the device (the product library, no probe)
# ----------------------------------------------------------------------------------------------------------------------
PACK_W, PACK_H = 61, 37  # partial edge tiles in both directions


def display_images():
    """sample_values() as (k, 37, 61, 4) images: pixel i holds values i .. i + 3, so every value appears in each of the
    four channels; the last image is padded by wrapping around."""
    v = test_display_pack.sample_values()
    px = np.stack([np.roll(v, -k) for k in range(4)], axis=1)
    per = PACK_W * PACK_H
    k = -(-len(px) // per)
    px = np.concatenate([px, px[:k * per - len(px)]])
    return np.ascontiguousarray(px.reshape(k, PACK_H, PACK_W, 4), np.float32), v


def test_inputs_display():
    imgs, v = display_images()
    assert imgs.shape[1:] == (PACK_H, PACK_W, 4) and PACK_W % 8 and PACK_H % 8
    want = np.sort(u32(v))
    for ch in range(4):
        assert np.array_equal(np.unique(u32(imgs[..., ch])), np.unique(want)), ch
    assert np.isnan(v).any() and np.isinf(v).any() and (v < 0).any() and (u32(v) == 0x80000000).any()


@pytest.mark.gpu
def test_gpu_display_packing_edge_values(gpu):
    """The device untile / pack kernel (hg_untile_image with hg_pack.h) on the host packer's edge values — NaN, +-Inf,
    negatives, denormals, overflow thresholds, every tie — loaded with hg_set_accumulation into a 61x37 target: every
    display format's readback equals hg_pack_display of the same array, bit for bit."""
    imgs, _ = display_images()
    packed, params, cube, frames, acc = cases.setup("c1_64")
    total = 0
    with abi.Context(0) as ctx:
        ctx.upload_scene(packed)
        ctx.resize(PACK_W, PACK_H)
        params.screenParameters.x, params.screenParameters.y = PACK_W, PACK_H
        ctx.set_params(params)
        for k, img in enumerate(imgs):
            ctx.set_accumulation(img, 2)
            for fmt in (abi.HG_DISPLAY_RGBA32F, abi.HG_DISPLAY_RGBA16F, abi.HG_DISPLAY_R11G11B10F):
                ctx.readback_begin(fmt)
                got = ctx.readback_end(PACK_W, PACK_H)
                want = abi.pack_display(img, fmt)
                assert got.shape == want.shape and got.dtype == want.dtype, (fmt, got.shape, want.shape)
                gb, wb = (a.view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize]) for a in (got, want))
                bad = np.argwhere(gb != wb)
                total += gb.size
                assert bad.size == 0, (f"image {k} format {fmt}: {len(bad)} values differ from the host packing; first "
                                       f"{[(i.tolist(), hex(int(gb[tuple(i)])), hex(int(wb[tuple(i)]))) for i in bad[:5]]}")
    print(f"display packing: {total} packed values compared, 0 differ")
