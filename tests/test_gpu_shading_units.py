"""The shading half of the device building blocks, one at a time, against the CPU oracle's own functions.

tests/test_gpu_device_units.py covers the intersection half of hg_device.h (hg_dev_isect.h, hg_dev_trav.h); this file covers what a path does after the
hit, with the same probe library (csrc/hg_devprobe.hip fn 50-58, tests/devprobe.py) and the same criterion: sample_sky
with cube_adjacent, sky_level, lambert, reflect, schlick_adjusted, refract_tir, medium_push / medium_pop (the device's
eight bytes of a uint64_t against the oracle's array of structs), evaluate_hit with material_brdf, and
inv_blackman_harris are evaluated on inputs chosen to break them, and every output word must equal the oracle's
(oracle/hg_oracle.c hgo_sky_batch ... hgo_evaluate_hit_batch, which call the oracle's static functions): uint32 views
compared for equality, NaN on both sides equal.  No tolerance anywhere: each of these functions is IEEE fp32 in one fixed
operation order on both sides (-ffp-contract=off).

As in test_gpu_device_units, the seeded input generators and the conditions that keep each input class from being
vacuous (judged on the oracle's output alone) run in CPU tests (test_inputs_*); the GPU tests reuse the generators.

The mutation list the inputs were checked against (each built into a scratch copy of the oracle and compared with the
unmutated one through these exports, on these inputs).  Changing output words: `>=` in refract_tir's and in
schlick_adjusted's threshold, `<=` in the push's search loop, `>=` in its first comparison, the pop removing the last
match, the corner average over the wrong three texels, pr0 >= albedo.w, the absorption taken from hm.  Changing nothing,
for no input can show them: orient >= 0 for orient > 0 (orientations are +-1), and (v + size) / 2 for (v + size - 1) / 2
in cube_adjacent: there v has the parity of size - 1 and |v| < size (v = +-size takes the other branch), so v + size is
odd and positive and C's truncating division gives the same texel."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import devprobe
import hg_oracle
from halogen import abi
from halogen.envmap import Cubemap
from test_gpu_device_units import (assert_same_bits, f32, from_bits, oracle_sampler, sampler_tuples, split, strided_bits,
                                   u32, ulp_steps, unit)

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
TINY = np.float32(1.1754944e-38)  # the smallest normal float32
ONE_BITS = 0x3F800000
ID_JITTER, ID_PROPERTY = 1, 3
IORS = f32([1.0, 1.0003, 1.33, 1.5, 2.4])


# ----------------------------------------------------------------------------------------------------------------------
# helpers and the oracle's batch exports
# ----------------------------------------------------------------------------------------------------------------------
def _fn(name, argtypes, L=None):
    fn = getattr(L if L is not None else hg_oracle.lib(), name)
    fn.restype = None
    fn.argtypes = argtypes
    return fn


def words(*cols):
    """Columns of float32 / int32 / uint32 arrays ((n,) or (n, k)) side by side as the (n, total) uint32 words of an
    element array."""
    out = []
    for c in cols:
        c = np.asarray(c)
        c = c.astype(np.float32) if c.dtype.kind == "f" else c
        assert c.dtype.itemsize == 4, c.dtype
        out.append(np.ascontiguousarray(c).view(np.uint32).reshape(len(c), -1))
    return np.ascontiguousarray(np.concatenate(out, axis=1))


def nudge(x, rng, r=2):
    """Each element of x (finite, non-zero) moved by a random -r..r units in the last place of its magnitude."""
    x = f32(x)
    return from_bits((u32(x).astype(np.int64) + rng.integers(-r, r + 1, x.shape)).astype(np.uint32)).reshape(x.shape)


def bit_distance(x, bits):
    return np.abs(u32(f32(x)).astype(np.int64) - bits)


def signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, np.float32(-1), np.float32(1))


def axis_vectors(rng, n):
    v = np.zeros((n, 3), np.float32)
    v[np.arange(n), rng.integers(0, 3, n)] = signs(rng, n)
    return v


def oracle_sky(cube, x, L=None):
    """(rgb (n, 3) float32, info (n, 4) int32: face, corner texel or -1, texels off the face, their mask)."""
    x = np.ascontiguousarray(x, np.uint32)
    scene = hg_oracle.HgoScene()
    tex = np.ascontiguousarray(cube.texels, np.float32)
    scene.cube_texels, scene.cube_face_size, scene.cube_mips = tex.ctypes.data, cube.face_size, cube.n_mips
    rgb, info = np.empty((len(x), 3), np.float32), np.empty((len(x), 4), np.int32)
    _fn("hgo_sky_batch", [C.c_void_p] * 4 + [C.c_int64], L)(C.addressof(scene), x.ctypes.data, rgb.ctypes.data,
                                                            info.ctypes.data, len(x))
    return rgb, info


def oracle_sky_level(x, L=None):
    x = np.ascontiguousarray(x, np.uint32)
    out = np.empty(len(x), np.int32)
    _fn("hgo_sky_level_batch", [C.c_void_p, C.c_void_p, C.c_int64], L)(x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_scatter(fn, x, L=None):
    """fn 0 lambert_scatter(n, rv), 1 specular_scatter(i, n)."""
    x = f32(x)
    out = np.empty((len(x), 3), np.float32)
    _fn("hgo_scatter_batch", [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64], L)(fn, x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_schlick(x, L=None):
    x = f32(x)
    out = np.empty(len(x), np.float32)
    _fn("hgo_schlick_batch", [C.c_void_p, C.c_void_p, C.c_int64], L)(x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_refract(x, L=None):
    x = f32(x)
    out = np.empty((len(x), 4), np.uint32)
    _fn("hgo_refract_batch", [C.c_void_p, C.c_void_p, C.c_int64], L)(x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_medium_ops(mats, x, L=None):
    """The stack after each of the 16 ops: (n, 16, 9) uint32 (sp, 8 ids)."""
    x = np.ascontiguousarray(x, np.uint32)
    out = np.empty((len(x), 16, 9), np.uint32)
    _fn("hgo_medium_ops_batch", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64], L)(
        C.addressof(mats), x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_evaluate_hit(mats, x, L=None):
    x = np.ascontiguousarray(x, np.uint32)
    out = np.empty((len(x), 19), np.uint32)
    _fn("hgo_evaluate_hit_batch", [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64], L)(
        C.addressof(mats), len(mats), x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_inv_bh(x, L=None):
    x = f32(x)
    out = np.empty(len(x), np.float32)
    _fn("hgo_inverted_blackman_harris_batch", [C.c_void_p, C.c_void_p, C.c_int64], L)(x.ctypes.data, out.ctypes.data, len(x))
    return out


def compare_classes(got, want, x, cls, what):
    for name, s in cls.items():
        assert_same_bits(got[s], want[s], x[s], f"{what} [{name}]")


# ----------------------------------------------------------------------------------------------------------------------
# sample_sky with cube_adjacent
# ----------------------------------------------------------------------------------------------------------------------
# (face size, mips).  hg_upload_cubemap accepts any positive face size (mip m is max(1, size >> m) texels wide), so 12 is
# the face size that is no power of two: mips of 12, 6, 3 and 1.
SKY_CUBES = {"1x1": (1, 1), "2x2": (2, 2), "8x4": (8, 4), "32x6": (32, 6), "12x4": (12, 4)}
N_SKY = 1 << 18
SKY_SHARES = [("random", 0.20), ("corner", 0.20), ("edge", 0.20), ("axis", 0.05), ("texel_grid", 0.20), ("scaled", 0.15)]
# the direction with face coordinates (sc, tc) on face f: the inverse of sample_sky's face selection
FACE_DIR = {0: lambda sc, tc, o: (o, -tc, -sc), 1: lambda sc, tc, o: (-o, -tc, sc), 2: lambda sc, tc, o: (sc, o, tc),
            3: lambda sc, tc, o: (sc, -o, -tc), 4: lambda sc, tc, o: (sc, -tc, o), 5: lambda sc, tc, o: (-sc, -tc, -o)}


@lru_cache(maxsize=None)
def sky_cube(size, mips):
    """Random positive texels, distinct per texel, so that a wrong texel shows in the result."""
    n = sum(6 * max(1, size >> m) ** 2 for m in range(mips))
    rng = np.random.default_rng(1000 * size + mips)
    return Cubemap(size, mips, f32(rng.permutation(np.linspace(0.05, 4.0, n * 4))))  # (steps of > 200 ulp: distinct)


def mip_size(cube, level):
    return np.maximum(1, cube.face_size >> np.clip(level, 0, cube.n_mips - 1))


@lru_cache(maxsize=None)
def sky_cases(name):
    """(elements (n, 4) words: direction, level; class -> slice).  The zero vector and NaN or infinite components are
    excluded: sc / ma is NaN there and the oracle's (int) conversion of it is undefined in C; the kernel only ever passes
    a normalised direction."""
    size, mips = SKY_CUBES[name]
    cube = sky_cube(size, mips)
    rng = np.random.default_rng(5150 + size)
    cls = split(N_SKY, SKY_SHARES)
    d = np.zeros((N_SKY, 3), np.float32)
    # half of the levels over -3..70 (most of them clamped from above), half around the mips that exist
    level = np.where(rng.random(N_SKY) < 0.5, rng.integers(-3, 71, N_SKY), rng.integers(-3, mips + 3, N_SKY)).astype(np.int32)

    s = cls["random"]
    n = s.stop - s.start
    d[s] = unit(rng.normal(0, 1, (n, 3)))
    s = cls["corner"]  # (+-1, +-1, +-1), each component moved by -2..2 ulp: exact two- and three-way ties and neighbours
    n = s.stop - s.start
    d[s] = nudge(signs(rng, (n, 3)), rng)
    s = cls["edge"]  # two components at +-1 (moved likewise), the third free
    n = s.stop - s.start
    e = nudge(signs(rng, (n, 3)), rng)
    e[np.arange(n), rng.integers(0, 3, n)] = f32(rng.uniform(-1, 1, n))
    d[s] = e
    s = cls["axis"]  # the other two components +-0 of both signs
    n = s.stop - s.start
    a = from_bits(np.where(rng.random((n, 3)) < 0.5, 0x80000000, 0).astype(np.uint32)).reshape(n, 3).copy()
    a[np.arange(n), rng.integers(0, 3, n)] = signs(rng, n) * f32(10.0 ** rng.uniform(-3, 3, n))
    d[s] = a
    s = cls["texel_grid"]  # through texel centres and texel boundaries of the mip the element asks for: fx, fy 0 and 0.5
    n = s.stop - s.start
    lv = rng.integers(0, mips, n).astype(np.int32)
    sz = mip_size(cube, lv)
    level[s] = lv

    def grid(k):
        twice = 2 * rng.integers(0, sz + 1) - (rng.random(n) < 0.5)  # 2 k: a boundary k / size; 2 k + 1: a centre
        return f32(np.clip(twice, 0, 2 * sz) / sz.astype(np.float64) - 1.0)  # (2 s - 1 with s = twice / (2 size))

    sc, tc, one = grid(0), grid(1), np.ones(n, np.float32)
    face = rng.integers(0, 6, n)
    g = np.zeros((n, 3), np.float32)
    for f in range(6):
        m = face == f
        g[m] = np.stack(FACE_DIR[f](sc, tc, one), axis=1)[m]
    d[s] = g * f32(2.0 ** rng.integers(-3, 4, n))[:, None]  # exact scalings: sc / ma keeps its value
    s = cls["scaled"]  # the classes above times 1e-30 and 1e30
    n = s.stop - s.start
    src = rng.integers(0, s.start, n)
    d[s] = f32(d[src] * np.where(rng.random(n) < 0.5, np.float32(1e-30), np.float32(1e30))[:, None])
    level[s] = level[src]
    assert np.isfinite(d).all() and (d != 0).any(1).all()
    return words(d, level), cls


def sky_edge_of(info):
    """Per element: the face edge (0 left, 1 right, 2 top, 3 bottom) its footprint crosses without a corner texel, -1
    for any other footprint."""
    mask = info[:, 3]
    plain = (info[:, 1] < 0) & ((info[:, 2] == 1) | (info[:, 2] == 2))
    edge = np.select([mask == 0b0101, mask == 0b1010, mask == 0b0011, mask == 0b1100], [0, 1, 2, 3], -1)
    assert (edge[plain] >= 0).all(), "a footprint with one or two texels off the face and no corner crosses one edge"
    return np.where(plain, edge, -1)


def test_inputs_sky(built):
    """Every sky class reaches its edge on every cubemap, judged by what the oracle reports of its footprints."""
    tot_corner = tot_edge = 0
    pair_corner, pair_edge = np.zeros((6, 4), np.int64), np.zeros((6, 4), np.int64)
    for name, (size, mips) in SKY_CUBES.items():
        cube = sky_cube(size, mips)
        assert len(np.unique(cube.texels)) == cube.texels.size and cube.texels.min() > 0, "distinct positive texels"
        x, cls = sky_cases(name)
        d, level = x[:, :3].view(np.float32), x[:, 3].view(np.int32)
        rgb, info = oracle_sky(cube, x)
        assert np.isfinite(rgb).all() and (rgb > 0).all()
        for k, s in cls.items():
            assert s.stop - s.start >= 1000, k
        face, corner, edge = info[:, 0], info[:, 1], sky_edge_of(info)
        assert np.bincount(face, minlength=6).min() >= 1000, (name, np.bincount(face, minlength=6))
        assert level.min() == -3 and level.max() == 70
        assert (level < 0).sum() >= 100 and (level > mips - 1).sum() >= 100, "both clamps of the level"
        for m in range(mips):
            assert (np.clip(level, 0, mips - 1) == m).sum() >= 1000, (name, m)
        assert (mip_size(cube, level) == 1).sum() >= 1000, "samples of a size-1 mip"
        tot_corner += int((corner >= 0).sum())
        tot_edge += int((edge >= 0).sum())
        np.add.at(pair_corner, (face[corner >= 0], corner[corner >= 0]), 1)
        np.add.at(pair_edge, (face[edge >= 0], edge[edge >= 0]), 1)
        pc = np.zeros((6, 4), np.int64)
        np.add.at(pc, (face[corner >= 0], corner[corner >= 0]), 1)
        assert (corner >= 0).sum() >= 1000 and pc.min() >= 10, (name, pc)
        if size > 1:  # (a 1-texel face has a corner texel in every footprint)
            pe = np.zeros((6, 4), np.int64)
            np.add.at(pe, (face[edge >= 0], edge[edge >= 0]), 1)
            assert (edge >= 0).sum() >= 1000 and pe.min() >= 10, (name, pe)
        else:
            assert (corner >= 0).all()
        # signed zeros, exact ties of the axis magnitudes, huge and tiny directions
        ad = np.abs(d)
        assert (u32(d[cls["axis"]]) == 0x80000000).sum() >= 1000 and (u32(d[cls["axis"]]) == 0).sum() >= 1000
        s = cls["corner"]
        assert ((ad[s, 0] == ad[s, 1]) & (ad[s, 1] == ad[s, 2])).sum() >= 100, "three-way ties"
        assert ((ad[s, 0] == ad[s, 1]) ^ (ad[s, 1] == ad[s, 2])).sum() >= 1000, "two-way ties"
        assert (ad[cls["scaled"]].max(1) > 1e29).sum() >= 1000 and (ad[cls["scaled"]].max(1) < 1e-29).sum() >= 1000
    assert tot_corner >= 1000 and pair_corner.min() >= 10 and tot_edge >= 1000 and pair_edge.min() >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SKY_CUBES))
def test_gpu_sample_sky_matches_oracle(gpu, name):
    """hgd::sample_sky (face selection, level clamp, the mip table of hg_cube_mip_offsets, cube_adjacent, the corner
    average and the bilinear blend) against hgo_cube_sample on five cubemaps of distinct random texels: all eight corners
    and twelve edges with their ulp neighbours, +-0 components, texel centres and boundaries of every mip, levels -3..70."""
    x, cls = sky_cases(name)
    cube = sky_cube(*SKY_CUBES[name])
    want, _ = oracle_sky(cube, x)
    got = devprobe.run_tables(devprobe.SKY, x, cubemap=cube)
    compare_classes(got, u32(want), x, cls, f"sample_sky {name}")


# ----------------------------------------------------------------------------------------------------------------------
# sky_level
# ----------------------------------------------------------------------------------------------------------------------
SKY_LEVEL_MIPS = [-5, 0, 1, 7, 63, 64, 65, 1000, INT32_MIN, INT32_MAX]


@lru_cache(maxsize=1)
def sky_level_cases():
    """(elements (n, 2) words: default_mip, acc_rough; class -> slice): every default_mip with every acc_rough."""
    rng = np.random.default_rng(64)
    ties = ulp_steps(f32(np.arange(-16, 1057)[np.arange(-16, 1057) != 0] / 16.0), range(-2, 3))  # k / 16 -2..2 ulp
    special = from_bits([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000001, 0x80000001])
    groups = [("random", f32(np.concatenate([rng.normal(0, 3, 400), rng.uniform(0, 9, 400)]))), ("ties", ties),
              ("special", np.concatenate([special, f32([1e30, -1e30, -1.0, -0.03125, -100.0, 3e9, -3e9])]))]
    acc = np.concatenate([g for _, g in groups])
    cls, at = {}, 0
    for name, g in groups:  # elements ordered class by class, each class all mips
        cls[name] = slice(at * len(SKY_LEVEL_MIPS), (at + len(g)) * len(SKY_LEVEL_MIPS))
        at += len(g)
    mip = np.tile(np.array(SKY_LEVEL_MIPS, np.int64).astype(np.int32), len(acc))
    return words(mip, np.repeat(acc, len(SKY_LEVEL_MIPS))), cls


def test_inputs_sky_level(built):
    x, cls = sky_level_cases()
    assert (1 << 15) <= len(x) <= (1 << 16)
    mip, acc = x[:, 0].view(np.int32), x[:, 1].view(np.float32)
    lvl = oracle_sky_level(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lf = f32(mip.astype(np.float32) + acc * np.float32(8))  # before the rounding
    assert lvl.min() == 0 and lvl.max() == 64 and set(np.unique(lvl)) == set(range(65)), "every level occurs"
    assert ((lvl == 0) & (lf < -1)).sum() >= 100 and ((lvl == 64) & (lf > 66)).sum() >= 100, "through the clamps"
    assert (lvl[np.isnan(lf)] == 0).all() and np.isnan(lf).sum() >= 10
    tie = np.isfinite(lf) & (lf - np.floor(np.where(np.isfinite(lf), lf, 0)) == 0.5)
    assert set(np.arange(64) + 0.5) <= set(lf[tie].tolist()), "a rounding tie below every level 1..64"
    inside = tie & (lf > 0) & (lf < 64)
    assert (lvl[inside] == np.rint(lf[inside])).all() and (lvl[inside] % 2 == 0).all(), "ties go to the even level"
    assert np.isinf(acc).any() and (u32(acc) == 0x80000000).any() and (acc < 0).sum() >= 1000


@pytest.mark.gpu
def test_gpu_sky_level_matches_oracle(gpu):
    """hgd::sky_level against the oracle's: the round-half-to-even ties of default_mip + acc_rough * 8, both clamps, NaN, +-Inf
    and default_mip up to INT32_MIN / INT32_MAX."""
    x, cls = sky_level_cases()
    compare_classes(devprobe.run(devprobe.SKY_LEVEL, x), oracle_sky_level(x).view(np.uint32), x, cls, "sky_level")


# ----------------------------------------------------------------------------------------------------------------------
# lambert, reflect, schlick_adjusted, refract_tir
# ----------------------------------------------------------------------------------------------------------------------
def np_dot(a, b):
    """dot3 / hgd::dot in numpy float32: the same three products and two sums, each rounded."""
    a, b = f32(a), f32(b)
    return f32(f32(a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])


def np_refract_product(inc, nrm, n1, n2):
    """refract_tir's n12 * st in numpy float32, for choosing inputs (TIR where it is > 1)."""
    ct = np.minimum(np_dot(-f32(inc), nrm), np.float32(1))
    st = np.sqrt(f32(np.float32(1) - f32(ct * ct)))
    return f32(f32(f32(n1) / f32(n2)) * st)


def np_schlick(n1, n2, nrm, inc, mn, mx):
    """schlick_adjusted in numpy float32: (value, sinT2 (NaN where n1 <= n2), early exit taken)."""
    n1, n2, mn, mx = f32(n1), f32(n2), f32(mn), f32(mx)
    r0 = f32(f32(n1 - n2) / f32(n1 + n2))
    r0 = f32(r0 * r0)
    cosx = -np_dot(nrm, inc)
    n = f32(n1 / n2)
    sin_t2 = f32(f32(n * n) * f32(np.float32(1) - f32(cosx * cosx)))
    dense = n1 > n2
    leave = dense & (sin_t2 > 1)
    with np.errstate(invalid="ignore"):
        cosx = np.where(dense, np.sqrt(f32(np.float32(1) - sin_t2)), cosx)
    x = f32(np.float32(1) - cosx)
    p = f32(np.float32(1) - r0)
    for _ in range(5):
        p = f32(p * x)
    ret = f32(r0 + p)
    val = f32(mn + f32(ret * f32(mx - mn)))
    return np.where(leave, mx, val), np.where(dense, sin_t2, np.float32(np.nan)), leave


def np_lambert_len(n, rv):
    p = f32(f32(rv) + f32(n))
    return np.sqrt(np_dot(p, p))


def threshold_candidates(rng, n, which, pairs):
    """n (inc, nrm, n1, n2) with incidence at the critical angle of the pair, kept by the restated value out of 8 n
    candidates: `which` = "refract": n12 * st closest to 1; "schlick": sinT2 closest to 1."""
    m = 8 * n
    pairs = f32(pairs)
    which_pair = rng.integers(0, len(pairs), m)
    pr = pairs[which_pair]
    n1, n2 = pr[:, 0].copy(), pr[:, 1].copy()
    nrm = np.where((rng.random(m) < 0.5)[:, None], axis_vectors(rng, m), unit(rng.normal(0, 1, (m, 3))))
    nd = nrm.astype(np.float64)
    t = np.cross(nd, rng.normal(0, 1, (m, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    theta = np.arcsin(n2.astype(np.float64) / n1) * (1 + rng.uniform(-1.5e-6, 1.5e-6, m))
    inc = f32(np.sin(theta)[:, None] * t - np.cos(theta)[:, None] * nd)
    val = np_refract_product(inc, nrm, n1, n2) if which == "refract" else np_schlick(n1, n2, nrm, inc, n1, n1)[1]
    # the candidates within +-4 ulp of 1 first, taken in turn from every (pair, distance) group so that no pair and no
    # side of the threshold crowds out another (a pair like 1.0003 / 1 puts every candidate within 1 ulp); then the rest
    sd = u32(f32(val)).astype(np.int64) - ONE_BITS
    key = which_pair * 128 + np.clip(sd, -64, 63) + 64
    order = np.lexsort((rng.random(m), key))
    start = np.concatenate([[0], np.nonzero(np.diff(key[order]))[0] + 1])
    rank = np.arange(m) - np.repeat(start, np.diff(np.concatenate([start, [m]])))
    keep = order[np.lexsort((np.abs(sd[order]), rank, np.abs(sd[order]) > 4))[:n]]
    keep = keep[rng.permutation(n)]
    return inc[keep], nrm[keep], n1[keep], n2[keep]


N_BSDF = 1 << 18
BSDF_SHARES = [("random", 0.20), ("normal_incidence", 0.05), ("grazing", 0.15), ("back_facing", 0.10),
               ("refract_threshold", 0.25), ("schlick_threshold", 0.25)]
DENSE_PAIRS = [(a, b) for a in IORS for b in IORS if a > b]


@lru_cache(maxsize=1)
def bsdf_cases():
    """(incident, normal, n1, n2, min, max; class -> slice): the inputs of reflect, schlick_adjusted and refract_tir."""
    rng = np.random.default_rng(1621)
    cls = split(N_BSDF, BSDF_SHARES)
    inc, nrm = np.zeros((N_BSDF, 3), np.float32), np.zeros((N_BSDF, 3), np.float32)
    n1, n2 = IORS[rng.integers(0, 5, N_BSDF)], IORS[rng.integers(0, 5, N_BSDF)]  # every pair, n1 = n2 included

    def facing(s, back):
        n = s.stop - s.start
        nrm[s], v = unit(rng.normal(0, 1, (n, 3))), unit(rng.normal(0, 1, (n, 3)))
        inc[s] = np.where(((np_dot(v, nrm[s]) > 0) != back)[:, None], -v, v)

    facing(cls["random"], False)
    facing(cls["back_facing"], True)
    s = cls["normal_incidence"]  # d = -n on an axis: cos exactly 1
    n = s.stop - s.start
    nrm[s] = axis_vectors(rng, n)
    inc[s] = -nrm[s]
    s = cls["grazing"]  # dot(d, n) within a few ulp of 0, both signs
    n = s.stop - s.start
    ax = rng.random(n) < 0.5
    na = axis_vectors(rng, n)
    k = np.argmax(np.abs(na), axis=1)
    ia = unit(rng.normal(0, 1, (n, 3)))
    tiny = f32(rng.choice([0.0, 1e-8, 6e-8, 1.2e-7, 1e-6, 1e-30], n)) * signs(rng, n)
    ia[np.arange(n), k] = tiny
    ng = unit(rng.normal(0, 1, (n, 3)))
    ig = f32(np.cross(ng.astype(np.float64), rng.normal(0, 1, (n, 3))))
    nrm[s], inc[s] = np.where(ax[:, None], na, ng), np.where(ax[:, None], ia, unit(ig))
    s = cls["refract_threshold"]
    inc[s], nrm[s], n1[s], n2[s] = threshold_candidates(rng, s.stop - s.start, "refract", DENSE_PAIRS)
    s = cls["schlick_threshold"]
    inc[s], nrm[s], n1[s], n2[s] = threshold_candidates(rng, s.stop - s.start, "schlick", DENSE_PAIRS)
    mn = f32(rng.choice([0.0, 1e-40, 0.02, 0.5, 1.0], N_BSDF))
    mx = np.where(rng.random(N_BSDF) < 0.7, np.float32(1), f32(rng.uniform(0, 2, N_BSDF)))
    return inc, nrm, f32(n1), f32(n2), mn, f32(mx), cls


def schlick_inputs():
    inc, nrm, n1, n2, mn, mx, cls = bsdf_cases()
    return f32(np.concatenate([n1[:, None], n2[:, None], nrm, inc, mn[:, None], mx[:, None]], axis=1)), cls


def refract_inputs():
    inc, nrm, n1, n2, mn, mx, cls = bsdf_cases()
    return f32(np.concatenate([inc, nrm, n1[:, None], n2[:, None]], axis=1)), cls


def reflect_inputs():
    inc, nrm, n1, n2, mn, mx, cls = bsdf_cases()
    return f32(np.concatenate([inc, nrm], axis=1)), cls


N_LAMBERT = 1 << 17
LAMBERT_SHARES = [("random", 0.35), ("axis", 0.10), ("opposite", 0.30), ("axis_threshold", 0.25)]
LEN_EPS = np.float32(1e-8)


@lru_cache(maxsize=1)
def lambert_cases():
    """(elements (n, 6): n, rv; class -> slice)."""
    rng = np.random.default_rng(1760)
    cls = split(N_LAMBERT, LAMBERT_SHARES)
    nrm, rv = np.zeros((N_LAMBERT, 3), np.float32), np.zeros((N_LAMBERT, 3), np.float32)
    s = cls["random"]
    n = s.stop - s.start
    nrm[s], rv[s] = unit(rng.normal(0, 1, (n, 3))), unit(rng.normal(0, 1, (n, 3)))
    s = cls["axis"]
    n = s.stop - s.start
    nrm[s], rv[s] = axis_vectors(rng, n), unit(rng.normal(0, 1, (n, 3)))
    s = cls["opposite"]  # rv = -n exactly (p = 0), or moved by a few ulp per component; some normals nearly on an axis
    n = s.stop - s.start
    v = rng.normal(0, 1, (n, 3)) * np.where(rng.random((n, 3)) < 0.3, 10.0 ** rng.uniform(-9, -3, (n, 3)), 1.0)
    nrm[s] = unit(v)
    moved = nudge(np.where(nrm[s] == 0, np.float32(1e-20), -nrm[s]), rng, 3)
    rv[s] = np.where((rng.random(n) < 0.3)[:, None], -nrm[s], moved)
    s = cls["axis_threshold"]  # axis normals, p = (0, a, 0) with |a| = 1e-8 moved by -4..4 ulp, 5e-9, 2e-8 or 0
    n = s.stop - s.start
    nrm[s] = axis_vectors(rng, n)
    k = (np.argmax(np.abs(nrm[s]), axis=1) + rng.integers(1, 3, n)) % 3
    near = ulp_steps(f32([1e-8]), range(-4, 5))[rng.integers(0, 9, n)]
    a = np.select([rng.random(n) < 0.7, rng.random(n) < 0.4, rng.random(n) < 0.5], [near, np.float32(5e-9), np.float32(2e-8)],
                  np.float32(0)) * signs(rng, n)
    r = -nrm[s]
    r[np.arange(n), k] = a
    rv[s] = r
    return f32(np.concatenate([nrm, rv], axis=1)), cls


def test_inputs_bsdf(built):
    """Every class of the lambert / reflect / schlick_adjusted / refract_tir inputs reaches its edge, and the numpy
    restatements that chose the threshold inputs agree with the oracle on the branch taken."""
    inc, nrm, n1, n2, mn, mx, cls = bsdf_cases()
    for name, s in cls.items():
        assert s.stop - s.start >= 1000, name
    assert {(float(a), float(b)) for a, b in zip(n1, n2)} == {(float(a), float(b)) for a in IORS for b in IORS}
    x, _ = refract_inputs()
    r = oracle_refract(x)
    tir = r[:, 3] == 1
    prod = np_refract_product(inc, nrm, n1, n2)
    assert np.array_equal(tir, prod > 1), "the restatement that chose the refraction inputs"
    s = cls["refract_threshold"]
    near = bit_distance(prod[s], ONE_BITS) <= 4
    assert (near & tir[s]).sum() >= 1000 and (near & ~tir[s]).sum() >= 1000 and near.mean() >= 0.5
    assert (prod[s] == 1).sum() >= 10, "n12 * st == 1.0f exactly"
    assert len({(float(a), float(b)) for a, b in zip(n1[s][near], n2[s][near])}) == len(DENSE_PAIRS)
    cos = np_dot(-inc, nrm)
    assert (cos[cls["normal_incidence"]] == 1).all()
    g = cls["grazing"]
    assert (np.abs(cos[g]) < 1e-6).sum() >= 0.9 * (g.stop - g.start)
    assert (cos[g] > 0).sum() >= 1000 and (cos[g] < 0).sum() >= 1000 and (cos[g] == 0).sum() >= 100
    assert (cos[cls["back_facing"]] < 0).all() and (cos[cls["random"]] >= 0).all()
    assert min(tir.sum(), (~tir).sum()) >= 1000 and np.isfinite(r[:, :3].view(np.float32)[~tir]).all()

    xs, _ = schlick_inputs()
    val, sin_t2, leave = np_schlick(n1, n2, nrm, inc, mn, mx)
    got = oracle_schlick(xs)
    same = (u32(got) == u32(val)) | (np.isnan(got) & np.isnan(val))
    assert same.all(), "the restatement that chose the Schlick inputs"
    s = cls["schlick_threshold"]
    near = bit_distance(sin_t2[s], ONE_BITS) <= 4
    assert (near & leave[s]).sum() >= 1000 and (near & ~leave[s]).sum() >= 1000 and near.mean() >= 0.5
    assert (sin_t2[s] == 1).sum() >= 10, "sinT2 == 1.0f exactly"
    assert (u32(got[leave]) == u32(mx[leave])).all() and leave.sum() >= 1000

    xl, lcls = lambert_cases()
    ln = np_lambert_len(xl[:, :3], xl[:, 3:])
    fallback = ln < LEN_EPS
    out = oracle_scatter(0, xl)
    plain = oracle_scatter(0, np.concatenate([xl[:, :3], np.zeros((len(xl), 3), np.float32)], axis=1))  # lambert(n, 0)
    assert fallback.sum() >= 100 and np.array_equal(u32(out[fallback]), u32(plain[fallback])), "the fallback p = n"
    assert (ln == 0).sum() >= 100, "p = 0"
    s = lcls["axis_threshold"]
    assert (bit_distance(ln[s], int(u32(f32([1e-8]))[0])) <= 4).sum() >= 1000
    assert fallback[s].sum() >= 1000 and (~fallback[s] & (ln[s] < 1e-7)).sum() >= 1000
    assert (~fallback[lcls["opposite"]]).sum() >= 1000 and fallback[lcls["opposite"]].sum() >= 1000
    assert not fallback[lcls["random"]].any()


@pytest.mark.gpu
def test_gpu_lambert_matches_oracle(gpu):
    """hgd::lambert against lambert_scatter: both sides of len(p) < 1e-8 (p = 0 included), where p = n is taken."""
    x, cls = lambert_cases()
    compare_classes(devprobe.run(devprobe.LAMBERT, x), u32(oracle_scatter(0, x)), x, cls, "lambert")


@pytest.mark.gpu
def test_gpu_reflect_matches_oracle(gpu):
    x, cls = reflect_inputs()
    compare_classes(devprobe.run(devprobe.REFLECT, x), u32(oracle_scatter(1, x)), x, cls, "reflect")


@pytest.mark.gpu
def test_gpu_schlick_adjusted_matches_oracle(gpu):
    """hgd::schlick_adjusted against the oracle's: every index pair, normal to grazing and back-facing incidence, and
    sinT2 within +-4 ulp of 1 (the early exit at the threshold)."""
    x, cls = schlick_inputs()
    compare_classes(devprobe.run(devprobe.SCHLICK, x), u32(oracle_schlick(x)), x, cls, "schlick_adjusted")


@pytest.mark.gpu
def test_gpu_refract_tir_matches_oracle(gpu):
    """hgd::refract_tir against the oracle's: the direction and the TIR flag, with n12 * st within +-4 ulp of 1 and
    exactly 1."""
    x, cls = refract_inputs()
    compare_classes(devprobe.run(devprobe.REFRACT, x), oracle_refract(x), x, cls, "refract_tir")


# ----------------------------------------------------------------------------------------------------------------------
# the medium stack
# ----------------------------------------------------------------------------------------------------------------------
BASE_PRIORITIES = [-1, 0, 0, 1, 2, 2, 3, 5, 7, INT32_MAX - 1, 0, 1, 2, 3, -1, 5, 7, 2, 1, 0, -1, 3, 5, INT32_MAX - 1]
ABSORPTIONS = [(0.0, 0.0, 0.0), (0.1, 0.5, 2.0), (1.8, 1.9, 2.0), (0.0, 0.3, 0.0), (10.0, 5.0, 0.02), (0.02, 0.01, 0.005)]
N_MEDIUM_MATS = len(BASE_PRIORITIES)
ABSENT_IDS = [200, 255, 1000, 0x3FFFFFFF]  # ids of no material


@lru_cache(maxsize=4)
def material_table(n=N_MEDIUM_MATS, w_values=()):
    """n materials whose id is their index: priorities -1, 0, 0, 1, 2, 2, 3, 5, 7, INT32_MAX - 1, ... (ties included), ior
    and absorption cycling through IORS and ABSORPTIONS (zero absorption and ior 1 included); the surface fields (for
    evaluate_hit) drawn from albedo.w {0, 1, 0.1} + w_values, metallic {0, a denormal, 0.02, 1}, roughness {0, 0.04, 0.5,
    1}.  The first 24 do not depend on n."""
    rng = np.random.default_rng(2424)
    mats = (abi.PackedHalogenMaterial * n)()
    w_set = [0.0, 1.0, 0.1] + list(w_values)
    w_p = [0.35, 0.1, 0.25] + [0.3 / len(w_values)] * len(w_values) if w_values else [0.5, 0.15, 0.35]
    for i, m in enumerate(mats):
        a, sp, em = rng.uniform(0.1, 1.0, 3), rng.uniform(0.1, 1.0, 3), rng.uniform(0.0, 2.0, 4)
        w, metal, rough = rng.choice(len(w_set), p=w_p), rng.choice([0.0, 1e-40, 0.02, 1.0]), rng.choice([0.0, 0.04, 0.5, 1.0])
        m.materialID = i
        m.albedo = abi.Vec4(a[0], a[1], a[2], np.float32(w_set[w]))
        m.specularAlbedo = abi.Vec4(sp[0], sp[1], sp[2], 1.0)
        m.metallic, m.roughness = metal, rough
        m.emissive = abi.Vec4(*em)
        m.rayMedium.indexOfRefraction = float(IORS[i % 5])
        m.rayMedium.absorption = abi.Vec3(*ABSORPTIONS[(i + i // 5) % 6])
        m.rayMedium.priority = BASE_PRIORITIES[i % N_MEDIUM_MATS]
        m.rayMedium.materialID = i
    return mats


def table_fields(mats):
    prio = np.array([m.rayMedium.priority for m in mats], np.int64)
    ior = f32([m.rayMedium.indexOfRefraction for m in mats])
    absorb = f32([[m.rayMedium.absorption.x, m.rayMedium.absorption.y, m.rayMedium.absorption.z] for m in mats])
    w = f32([m.albedo.w for m in mats])
    return prio, ior, absorb, w


def pack_stack(sp, entries, above):
    """(sp, lo, hi) words of stacks: entries (n, 8) material indices, used below sp; `above` (n, 8) bytes above sp."""
    b = np.where(np.arange(8)[None, :] < sp[:, None], entries, above).astype(np.uint64)
    s = (b << (8 * np.arange(8, dtype=np.uint64))[None, :]).sum(axis=1).astype(np.uint64)
    return np.stack([sp.astype(np.uint32), (s & np.uint64(0xFFFFFFFF)).astype(np.uint32), (s >> np.uint64(32)).astype(np.uint32)], 1)


def stack_bytes(lo, hi):
    """The eight material indices in the bytes of a stack's (lo, hi) words: (n, 8) int64."""
    s = lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))
    return ((s[:, None] >> (8 * np.arange(8, dtype=np.uint64))[None, :]) & np.uint64(0xFF)).astype(np.int64)


def random_above(rng, n):
    """The bytes above sp, which must never be read: zero in one half, random in the other."""
    return np.where((rng.random(n) < 0.5)[:, None], 0, rng.integers(0, 256, (n, 8)))


N_MEDIUM = 1 << 16
MEDIUM_SHARES = [("random_ops", 0.25), ("fill", 0.15), ("ascending", 0.08), ("descending", 0.08), ("tied", 0.09),
                 ("full_distinct", 0.15), ("arbitrary_initial", 0.20)]


@lru_cache(maxsize=1)
def medium_cases():
    """(elements (n, 19) words: sp, stack bytes, 16 ops; class -> slice).  The op lists are built one op at a time on the
    oracle's own states, so a pop can name the top, the bottom, a middle entry, an id present twice or an absent id."""
    rng = np.random.default_rng(808)
    mats = material_table()
    prio, _, _, _ = table_fields(mats)
    nm, N = len(mats), N_MEDIUM
    cls = split(N, MEDIUM_SHARES)
    sp0 = np.zeros(N, np.int64)
    s = cls["arbitrary_initial"]  # not reached by pushes: any order of any materials, sp 0..8
    sp0[s] = rng.integers(0, 9, s.stop - s.start)
    init = pack_stack(sp0, rng.integers(0, nm, (N, 8)), random_above(rng, N))
    init[:s.start, 1:] = 0
    ops = np.zeros((N, 16), np.uint32)
    n_ops = rng.integers(1, 17, N)
    n_ops[cls["fill"]] = 16
    n_ops[cls["full_distinct"]] = rng.integers(10, 17, cls["full_distinct"].stop - cls["full_distinct"].start)
    p_push = np.full(N, 0.6)
    p_push[cls["fill"]] = 0.85
    p_push[cls["arbitrary_initial"]] = 0.5
    # a scripted run of pushes first: ascending / descending priorities, one tied priority, distinct materials to depth 8
    script = np.full((N, 16), -1, np.int64)
    for name in ("ascending", "descending", "tied", "full_distinct"):
        s = cls[name]
        n = s.stop - s.start
        pick = np.argsort(rng.random((n, nm)), axis=1)[:, :10]  # 10 distinct materials each
        if name == "tied":
            tied = [np.nonzero(prio == p)[0] for p in (0, 2, -1, 5)]
            pick = np.stack([t[rng.integers(0, len(t), 10)] for t in (tied[k] for k in rng.integers(0, 4, n))])
        elif name != "full_distinct":
            order = np.argsort(prio[pick], axis=1, kind="stable")
            pick = np.take_along_axis(pick, order if name == "ascending" else order[:, ::-1], axis=1)
        ln = 8 if name == "full_distinct" else rng.integers(2, 11, n)
        script[s, :10] = np.where(np.arange(10)[None, :] < np.broadcast_to(ln, (n,))[:, None], pick, -1)
        n_ops[s] = np.maximum(n_ops[s], np.broadcast_to(ln, (n,)) + 1)
    for k in range(16):
        st = oracle_medium_ops(mats, np.concatenate([init, ops], axis=1))[:, max(k - 1, 0)]  # the stack before op k
        sp, ids = st[:, 0].astype(np.int64), st[:, 1:].astype(np.int64)
        at = lambda pos: ids[np.arange(N), np.clip(pos, 0, 7)]
        on_stack = at(rng.integers(0, np.maximum(sp, 1)))
        push_m = np.where((rng.random(N) < 0.25) & (sp > 0), on_stack, rng.integers(0, nm, N))  # a quarter: already on it
        target = rng.integers(0, 6, N)  # top, bottom, middle, any entry, an absent id, any material's id
        pop_id = np.select([target == 0, target == 1, target == 2, target == 3, target == 4],
                           [at(sp - 1), at(np.zeros(N, np.int64)), at(rng.integers(1, np.maximum(sp - 1, 2))), on_stack,
                            np.array(ABSENT_IDS)[rng.integers(0, len(ABSENT_IDS), N)]], rng.integers(0, nm, N))
        pop_id = np.where((sp == 0) & (target < 4), rng.integers(0, nm, N), pop_id)  # (an empty stack names no entry)
        pop_id &= 0x3FFFFFFF  # (a position above sp reads as 0xFFFFFFFF: an absent id)
        push = rng.random(N) < p_push
        if k == 8:  # a full stack of distinct materials: a dropped push, or the pop of the entry at byte 7
            s = cls["full_distinct"]
            push[s] = rng.random(s.stop - s.start) < 0.4
            pop_id[s] = ids[s, 7]
        op = np.where(push, devprobe.OP_PUSH | push_m, devprobe.OP_POP | pop_id)
        op = np.where(script[:, k] >= 0, devprobe.OP_PUSH | script[:, k], op)
        ops[:, k] = np.where(k < n_ops, op, 0).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([init, ops], axis=1), np.uint32), cls


def medium_transitions(x, out):
    """Per op: (kind, value, sp before, ids before (8), sp after, ids after (8)) from the oracle's states."""
    n = len(x)
    kind, val = (x[:, 3:] >> 30).astype(np.int64), (x[:, 3:] & 0x3FFFFFFF).astype(np.int64)
    sp_init = x[:, 0].astype(np.int64)
    ids_init = np.where(np.arange(8)[None, :] < sp_init[:, None], stack_bytes(x[:, 1], x[:, 2]), 0xFFFFFFFF)  # ids are indices
    first = np.concatenate([sp_init[:, None], ids_init], axis=1)[:, None, :]
    before = np.concatenate([first, out[:, :-1].astype(np.int64)], axis=1)
    after = out.astype(np.int64)
    return kind, val, before[..., 0], before[..., 1:], after[..., 0], after[..., 1:]


def test_inputs_medium(built):
    """The op lists reach every depth, the dropped push, inserts at the bottom, the top and between, pops that remove
    nothing and the pop at byte 7, judged on the oracle's states."""
    x, cls = medium_cases()
    mats = material_table()
    prio, ior, absorb, _ = table_fields(mats)
    assert len(mats) == 24 and [m.rayMedium.materialID for m in mats] == list(range(24))
    for p in (-1, 0, 1, 2, 3, 5, 7, INT32_MAX - 1):
        assert (prio == p).sum() >= (2 if p in (0, 2) else 1), p
    assert (absorb == 0).all(1).any() and (ior == 1).any() and len(np.unique(ior)) == 5
    out = oracle_medium_ops(mats, x)
    kind, val, sp_b, ids_b, sp_a, ids_a = medium_transitions(x, out)
    assert np.array_equal(ids_b[:, 0][x[:, 0] > 0, 0], (x[:, 1] & 0xFF)[x[:, 0] > 0].astype(np.int64)), "the initial stack"
    depth = np.bincount(np.concatenate([sp_b[:, 0], sp_a.ravel()]), minlength=9)
    assert len(depth) == 9 and depth.min() >= 1000, depth
    push, pop = kind == 1, kind == 2
    assert kind.max() <= 2 and val[push].max() < len(mats) and x[:, 0].max() == 8, "what the probe's host check accepts"
    assert (push & (sp_b == 8)).sum() >= 100 and (sp_a[push & (sp_b == 8)] == 8).all(), "a dropped push"
    assert np.array_equal(ids_a[push & (sp_b == 8)], ids_b[push & (sp_b == 8)])
    ins = push & (sp_b > 0) & (sp_b < 8)
    assert (sp_a[ins] == sp_b[ins] + 1).all()
    new = ins & ~(ids_b == val[..., None]).any(-1)  # (a material not yet on the stack: its position is unambiguous)
    differs = ids_a[..., :8] != ids_b
    pos = np.where(differs.any(-1), differs.argmax(-1), 8)
    assert (ids_a[new][np.arange(new.sum()), pos[new]] == val[new]).all()
    assert (new & (pos == 0)).sum() >= 1000 and (new & (pos == sp_b)).sum() >= 1000, "inserts at 0 and at sp"
    assert (new & (pos > 0) & (pos < sp_b)).sum() >= 1000, "inserts strictly between"
    again = ins & (ids_b == val[..., None]).any(-1)
    assert again.sum() >= 1000, "pushes of a material already on the stack"
    assert (pop & (sp_a == sp_b)).sum() >= 1000, "pops that remove nothing"
    assert (pop & (sp_a == sp_b) & (sp_b > 0)).sum() >= 1000 and (pop & (sp_b == 0)).sum() >= 100
    hit = pop & (sp_a == sp_b - 1)
    where = np.where(hit, (ids_b == val[..., None]).argmax(-1), -1)
    assert (hit & (where == 7)).sum() >= 100, "a pop at index 7"
    assert (hit & (where == 0) & (sp_b > 1)).sum() >= 1000 and (hit & (where == sp_b - 1) & (sp_b > 1)).sum() >= 1000
    assert (hit & (where > 0) & (where < sp_b - 1)).sum() >= 1000, "pops of the bottom, the top and a middle entry"
    twice = hit & ((ids_b == val[..., None]).sum(-1) >= 2)
    assert twice.sum() >= 1000, "pops of an id present twice"
    for name in ("ascending", "descending", "tied"):
        s = cls[name]
        pv = np.where(kind[s, :3] == 1, prio[np.clip(val[s, :3], 0, 23)], 0)
        d = np.diff(pv[:, :2], axis=1)[:, 0]
        assert ((d >= 0) if name == "ascending" else (d <= 0) if name == "descending" else (d == 0)).all(), name
    s = cls["arbitrary_initial"]
    above = (x[s, 1].astype(np.uint64) | (x[s, 2].astype(np.uint64) << np.uint64(32))) >> (8 * x[s, 0].astype(np.uint64) % 64)
    full = x[s, 0] == 8
    assert ((above != 0) & ~full).sum() >= 1000 and ((above == 0) & ~full).sum() >= 1000, "bytes above sp: random and zero"
    assert np.bincount(x[s, 0], minlength=9).min() >= 100


@pytest.mark.gpu
def test_gpu_medium_stack_matches_oracle(gpu):
    """hgd::medium_push / medium_pop on the uint64_t byte stack against add_to_medium_stack / pop_from_medium_stack on
    the oracle's array of structs: sp and every entry's id after each of up to 16 ops, over a 24-material table packed
    by hg_pack_spheres_materials; stacks of 8 with dropped pushes, the delete at byte 7, priority ties, duplicates and
    arbitrary initial stacks with random bytes above sp."""
    x, cls = medium_cases()
    mats = material_table()
    want = oracle_medium_ops(mats, x).reshape(len(x), -1)
    got = devprobe.run_tables(devprobe.MEDIUM_OPS, x, materials=mats)
    compare_classes(got, want, x, cls, "medium stack")


# ----------------------------------------------------------------------------------------------------------------------
# evaluate_hit with material_brdf
# ----------------------------------------------------------------------------------------------------------------------
N_EVAL = 1 << 19
N_EVAL_MATS = 192
EVAL_SHARES = [("general", 0.80), ("tir_threshold", 0.12), ("w_equal", 0.08)]
HIT_T = f32([1e-4, 1.0, 50.0, 1e4])
N_W = 12  # tuples whose get2(ID_PROPERTY) first component becomes a material's albedo.w


def property_draws(t3):
    """get2(ID_PROPERTY)'s first component for (frame, pixel, offset) tuples."""
    return oracle_sampler(np.concatenate([t3, np.full((len(t3), 1), ID_PROPERTY, np.uint32)], axis=1))[1][:, 0]


@lru_cache(maxsize=1)
def eval_table():
    tuples = sampler_tuples()[:, :3]
    special = tuples[np.random.default_rng(12).integers(0, len(tuples), N_W)]
    w = property_draws(special)
    return material_table(N_EVAL_MATS, tuple(float(v) for v in w)), special, w


@lru_cache(maxsize=1)
def eval_cases():
    """(elements (n, 21) words; class -> slice)."""
    rng = np.random.default_rng(4711)
    mats, special, w_special = eval_table()
    prio, ior, absorb, w = table_fields(mats)
    nm, N = len(mats), N_EVAL
    cls = split(N, EVAL_SHARES)
    tuples = sampler_tuples()[:, :3]
    tup = tuples[rng.integers(0, len(tuples), N)]
    mat = rng.integers(0, nm, N)
    inc_all, nrm_all = bsdf_cases()[:2]
    pick = rng.integers(0, len(inc_all), N)
    inc, nrm = unit(inc_all[pick]), unit(nrm_all[pick])
    orient = signs(rng, N)
    # the stack: empty, holding the hit material, not holding it, full (with and without it)
    kind = rng.integers(0, 4, N)
    sp = np.select([kind == 0, kind == 3], [0, 8], rng.integers(1, 8, N))
    entries = rng.integers(0, nm, (N, 8))
    entries = np.where((entries == mat[:, None]) & (kind == 2)[:, None], (entries + 1) % nm, entries)
    holds = (kind == 1) | ((kind == 3) & (rng.random(N) < 0.5))
    where = rng.integers(0, np.maximum(sp, 1))
    entries[np.arange(N)[holds], where[holds]] = mat[holds]

    s = cls["tir_threshold"]  # leaving a material into the empty medium at its critical angle: n1 = its ior, n2 = 1
    n = s.stop - s.start
    ti, tn, t1, _ = threshold_candidates(rng, n, "refract", [(a, 1.0) for a in IORS[1:]])
    clear = [np.nonzero((ior == a) & (w == 0))[0] for a in IORS]
    assert all(len(c) for c in clear[1:]), "a refracting material of every ior"
    for a, c in zip(IORS[1:], clear[1:]):
        m = np.nonzero(t1 == a)[0]
        mat[s.start + m] = c[rng.integers(0, len(c), len(m))]
    inc[s], nrm[s], orient[s], sp[s] = ti, tn, -1, 0
    s = cls["w_equal"]  # the tuple whose pr0 is the material's albedo.w: `pr0 > w` at equality
    n = s.stop - s.start
    k = rng.integers(0, N_W, n)
    users = [np.nonzero(u32(w) == u32(w_special[j:j + 1])[0])[0] for j in range(N_W)]
    usable = np.array([j for j in range(N_W) if len(users[j])])
    assert len(usable) >= 4
    k = usable[k % len(usable)]
    tup[s] = special[k]
    mat[s] = [users[j][rng.integers(0, len(users[j]))] for j in k]

    stack = pack_stack(sp, entries, random_above(rng, N))
    t = HIT_T[rng.integers(0, 4, N)]
    pos, org = f32(rng.uniform(-10, 10, (N, 3))), f32(rng.uniform(-10, 10, (N, 3)))
    x = words(tup, stack, org, inc, t, orient, pos, nrm, mat.astype(np.uint32))
    assert x.shape == (N, 21)
    return x, cls


def eval_media(x, mats):
    """(true hit, cur, hm) per element: the material index of the medium evaluate_material_hit calls cur and hm (-1: the
    empty medium), from the element and the oracle's own stack ops."""
    prio, _, _, _ = table_fields(mats)
    n = len(x)
    sp = x[:, 3].astype(np.int64)
    by = stack_bytes(x[:, 4], x[:, 5])
    top = np.where(sp > 0, by[np.arange(n), np.maximum(sp - 1, 0)], -1)
    mat = x[:, 20].astype(np.int64)
    front = x[:, 13].view(np.float32) == 1
    solid = prio[mat] >= 0
    true_hit = ~solid | (sp == 0) | (prio[mat] <= prio[np.maximum(top, 0)])
    ops = np.zeros((n, 16), np.uint32)
    ops[:, 0] = devprobe.OP_POP | mat  # ids are indices
    popped = oracle_medium_ops(mats, np.concatenate([x[:, 3:6], ops], axis=1))[:, 0].astype(np.int64)
    top_popped = np.where(popped[:, 0] > 0, popped[np.arange(n), np.maximum(popped[:, 0], 1)], -1)
    cur = np.where(front, top, np.where(solid & (sp > 0), top, mat))
    hm = np.where(front, mat, np.where(solid, top_popped, top))
    return true_hit, cur, hm


def test_inputs_evaluate_hit(built):
    """The evaluate_hit elements reach every bounce type at each orientation, false hits, TIR, the four cur / hm cases on
    empty and non-empty stacks, the pop after the BRDF, Beer absorption down to denormal and zero, the dropped push and
    pr0 == albedo.w, judged on the oracle's results."""
    x, cls = eval_cases()
    mats, special, w_special = eval_table()
    prio, ior, absorb, w = table_fields(mats)
    assert len(mats) == N_EVAL_MATS < 256
    first = table_fields(material_table())
    assert all(np.array_equal(a[:24], b) for a, b in zip((prio, ior, absorb), first[:3])), "the medium test's table first"
    metal, rough = f32([m.metallic for m in mats]), f32([m.roughness for m in mats])
    assert set(np.unique(metal)) == set(f32([0, 1e-40, 0.02, 1])) and set(np.unique(rough)) == set(f32([0, 0.04, 0.5, 1]))
    assert {0.0, 1.0, float(np.float32(0.1))} <= set(float(v) for v in np.unique(w)) and (prio < 0).sum() >= 10
    out = oracle_evaluate_hit(mats, x)
    att, bt = out[:, 0:3].view(np.float32), out[:, 9]
    sp0, sp1 = x[:, 3].astype(np.int64), out[:, 10].astype(np.int64)
    mat, t = x[:, 20].astype(np.int64), x[:, 12].view(np.float32)
    front = x[:, 13].view(np.float32) == 1
    assert set(np.unique(x[:, 13].view(np.float32))) == {-1.0, 1.0} and set(np.unique(t)) == set(HIT_T)
    true_hit, cur, hm = eval_media(x, mats)
    for o in (front, ~front):
        for b in (0, 1, 2):
            assert (o & true_hit & (bt == b)).sum() >= 1000, (b, "bounce type at each orientation")
    false_hit = ~true_hit
    assert false_hit.sum() >= 1000 and (bt[false_hit] == 2).all()
    assert np.array_equal(out[false_hit, 6:9], x[false_hit, 9:12]), "a false hit keeps the direction"
    for o in (front, ~front):
        for solid in (prio[mat] >= 0, prio[mat] < 0):
            for empty in (sp0 == 0, sp0 > 0):
                assert (o & solid & empty).sum() >= 1000, "cur / hm case (orientation x priority sign x stack)"
    refr = true_hit & (bt == 2)
    n1, n2 = np.where(cur >= 0, ior[np.maximum(cur, 0)], 1), np.where(hm >= 0, ior[np.maximum(hm, 0)], 1)
    d, nrm = x[:, 9:12].view(np.float32), x[:, 17:20].view(np.float32)
    tir = oracle_refract(np.concatenate([d, nrm, f32(n1)[:, None], f32(n2)[:, None]], axis=1))[:, 3] == 1
    assert (refr & tir).sum() >= 1000 and (refr & ~tir).sum() >= 1000, "TIR inside material_brdf"
    s = cls["tir_threshold"]
    prod = np_refract_product(d[s], nrm[s], n1[s], n2[s])
    near = (bit_distance(prod, ONE_BITS) <= 4) & refr[s]
    assert (near & tir[s]).sum() >= 1000 and (near & ~tir[s]).sum() >= 1000 and (cur[s] == mat[s]).all() and (hm[s] < 0).all()
    post_pop = true_hit & front & (bt != 2)
    assert post_pop.sum() >= 1000 and (post_pop & (prio[mat] >= 0) & (sp0 < 8) & (sp1 == sp0)).sum() >= 1000, "the pop after the BRDF"
    absorbing = (cur >= 0) & (absorb[np.maximum(cur, 0)] != 0).any(1)
    assert absorbing.sum() >= 1000 and ((cur >= 0) & ~absorbing).sum() >= 1000 and (cur < 0).sum() >= 1000
    small = ((att == 0) | (np.abs(att) < TINY)).any(1)
    assert (small & absorbing).sum() >= 100 and ((att != 0) & (np.abs(att) < TINY)).any(1).sum() >= 100, "denormal / zero attenuation"
    assert not small[~absorbing].any()
    assert (front & (prio[mat] >= 0) & (sp0 == 8)).sum() >= 100, "a push dropped on a full stack"
    pr0 = property_draws(x[:, 0:3])
    equal = u32(pr0) == u32(w[mat])
    assert (equal & true_hit).sum() >= 1000 and (bt[equal & true_hit] != 2).all(), "pr0 == albedo.w: no refraction"
    held = (np.where(np.arange(8)[None, :] < sp0[:, None], stack_bytes(x[:, 4], x[:, 5]), -1) == mat[:, None]).any(1)
    assert (held & (sp0 == 8)).sum() >= 1000 and (~held & (sp0 == 8)).sum() >= 1000 and (held & (sp0 < 8)).sum() >= 1000
    assert (~held & (sp0 > 0) & (sp0 < 8)).sum() >= 1000


@pytest.mark.gpu
def test_gpu_evaluate_hit_matches_oracle(gpu):
    """hgd::evaluate_hit with material_brdf against evaluate_material_hit: the attenuation, the new ray, the bounce type
    and the whole medium stack afterwards, over a 192-material table (priorities below zero, roughness up to 1, albedo.w
    equal to the sampler's own draws), stacks from empty to full, both orientations, incidence from normal to the TIR
    threshold, and Beer absorption whose hg_expf argument runs from 0 to below -103."""
    x, cls = eval_cases()
    mats, _, _ = eval_table()
    want = oracle_evaluate_hit(mats, x)
    got = devprobe.run_tables(devprobe.EVALUATE_HIT, x, materials=mats)
    compare_classes(got, want, x, cls, "evaluate_hit")


# ----------------------------------------------------------------------------------------------------------------------
# inv_blackman_harris
# ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=1)
def inv_bh_cases():
    t = sampler_tuples()[:1 << 16].copy()
    t[:, 3] = ID_JITTER
    jitter = oracle_sampler(t)[1].ravel()  # every get2(ID_JITTER) value of 2^16 tuples
    edge = np.concatenate([from_bits([0, 1, 2, 0x80000000, 0x80000001, 0x007FFFFF, 0x00800000]),
                           ulp_steps(f32([1.0, 0.5]), range(-2, 3))])
    parts = [("strided", strided_bits(0.0, 1.0, 1 << 20)), ("jitter", jitter), ("edge", edge)]
    cls, at = {}, 0
    for name, p in parts:
        cls[name] = slice(at, at + len(p))
        at += len(p)
    return f32(np.concatenate([p for _, p in parts])), cls


def test_inputs_inv_blackman_harris(built):
    x, cls = inv_bh_cases()
    y = oracle_inv_bh(x)
    assert cls["strided"].stop == 1 << 20 and cls["jitter"].stop - cls["jitter"].start == 1 << 17
    assert (x == 0).any() and (x == 1).any() and (u32(x) == ONE_BITS + 1).any() and (u32(x) == ONE_BITS - 1).any()
    inside = (x >= 0) & (x <= 1)
    assert np.isfinite(y[inside]).all() and inside.sum() >= (1 << 20) + (1 << 17)
    assert abs(float(y[x == 0.5][0])) < 1e-6, "odd about x = 0.5"
    assert y[inside].min() < -0.45 and y[inside].max() > 0.45 and np.all(np.diff(y[cls["strided"]]) >= 0)


@pytest.mark.gpu
def test_gpu_inv_blackman_harris_matches_oracle(gpu):
    """hgd::inv_blackman_harris against hgo_inverted_blackman_harris on 2^20 bit-strided values of [0, 1], every pixel
    jitter draw of 2^16 sampler tuples, and 0, 1 and their neighbours."""
    x, cls = inv_bh_cases()
    compare_classes(devprobe.run(devprobe.INV_BH, x), u32(oracle_inv_bh(x)), x, cls, "inv_blackman_harris")
