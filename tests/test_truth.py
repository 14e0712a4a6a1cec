"""The CPU oracle against float64 geometry and closed forms (tests/truth.py), and the input-quality checks of the cases.

Every other test holds a kernel against the oracle bit for bit; here the oracle itself is held against references that
share nothing with it: a 3 x 3 linear solve, slab intervals, the quadratic, a search over every triangle without a
hierarchy, the definition of a (0, m, 2)-net, Snell's law, the moments of a cosine-weighted hemisphere, and images
whose pixels are known in closed form.  tests/test_gpu_truth.py runs the kernels through the same checks with the same
inputs; the generators, the check functions and the shares each check leaves out live here, and every share has a
test_inputs_* test on the float64 side alone, so that no check can pass by leaving out its cases.

The constants K of the residual bounds are three times what a plain numpy float32 restatement (a stand-in, not the code
under test) measures on the same inputs; the measured maxima, for the stand-in and for the oracle, stand in the
docstrings of the tests that use them.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import hg_oracle
import truth
from halogen import render_pass as rp, scenes
from halogen.envmap import Cubemap
from halogen.scene import HalogenMaterial, RayTracingMesh, RayTracingSphere, Scene, pack_material
from halogen.unity import Transform, euler_to_quat, unity_cube, unity_plane

F = np.float32
INF = F(np.inf)
EPS = float(np.finfo(np.float32).eps)  # 2^-23


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def unit32(v):
    return f32(truth.unit(v))


def _oracle(name, argtypes):
    fn = getattr(hg_oracle.lib(), name)
    fn.restype = None
    fn.argtypes = argtypes
    return fn


def report(what, **figures):
    print(f"{what}: " + ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


# ----------------------------------------------------------------------------------------------------------------------
# 1a. triangle
# ----------------------------------------------------------------------------------------------------------------------
# three times the 2.4 that a numpy float32 Moller-Trumbore measured on 4e5 elements of this distribution when the bound
# was chosen, rounded up (on tri_inputs() itself the stand-in measures 1.84: test_standin_constants)
K_TRI = 8.0
N_TRI = 200_000
UNDECIDED_TRI_CAP = 0.10
BEST_T_FACTORS = np.array([0.5, 0.99995, 0.99999, 1.0, 1.00001, 1.00005, 2.0])


@lru_cache(maxsize=1)
def tri_inputs():
    """dict: o, d, v0, v1, v2, e1, e2 (float32; e = v - v0 in float32, what both sides are given), best_t."""
    rng = np.random.default_rng(8101)
    n = N_TRI
    scale = 10.0 ** rng.uniform(-3, 3, (n, 1))
    v0 = f32(rng.uniform(-1, 1, (n, 3)) * scale)
    v1 = f32(v0 + rng.normal(0, 0.5, (n, 3)) * scale)
    v2 = f32(v0 + rng.normal(0, 0.5, (n, 3)) * scale)
    e1, e2 = f32(v1 - v0), f32(v2 - v0)
    o = f32(3.0 * scale * truth.unit(rng.normal(0, 1, (n, 3))))
    bu, bv = rng.uniform(-0.3, 1.3, (n, 1)), rng.uniform(-0.3, 1.3, (n, 1))
    d = unit32(v0 + bu * e1 + bv * e2 - o)
    t = truth.tri_solve(o, d, v0, e1, e2)[0]
    best = np.full(n, INF, F)
    fin = (rng.random(n) < 0.5) & np.isfinite(t) & (t > 0)
    best[fin] = f32(t * rng.choice(BEST_T_FACTORS, n))[fin]
    return {"o": o, "d": d, "v0": v0, "v1": v1, "v2": v2, "e1": e1, "e2": e2, "best_t": best}


def tri_geometry(c):
    return c["o"], c["d"], c["v0"], c["e1"], c["e2"]


def tri_oracle_inputs(c):
    """(rays (n, 7), HalogenTriangle records (n, 18): the three points, zero normals)."""
    rays = f32(np.concatenate([c["o"], c["d"], c["best_t"][:, None]], axis=1))
    tris = f32(np.concatenate([c["v0"], c["v1"], c["v2"], np.zeros((len(rays), 9), F)], axis=1))
    return rays, tris


def tri_probe_inputs(c):
    """The device probe's element: lo, ld, best_t, v0, e1, e2 (16 floats)."""
    return f32(np.concatenate([c["o"], c["d"], c["best_t"][:, None], c["v0"], c["e1"], c["e2"]], axis=1))


def oracle_tri(c):
    rays, tris = tri_oracle_inputs(c)
    out = np.empty((len(rays), 5), np.uint32)
    _oracle("hgo_tri_accept_batch", [C.c_void_p] * 3 + [C.c_int64])(rays.ctypes.data, tris.ctypes.data, out.ctypes.data, len(rays))
    return out


@lru_cache(maxsize=1)
def tri_truth():
    c = tri_inputs()
    accept, front, decided, t, u, v = truth.tri_decide(K_TRI, *tri_geometry(c), c["best_t"])
    return {"accept": accept, "front": front, "decided": decided, "t": t, "u": u, "v": v}


def tri_ratio(c, out, rows):
    """|R| c s / (2^-24 mag) of the (t, U, V) in out's words 1 .. 3, for the given rows."""
    g = [a[rows] for a in tri_geometry(c)]
    t, u, v = (out[rows, k].view(F) for k in (1, 2, 3))
    return truth.tri_residual(*g, t, u, v) / truth.tri_bound(1.0, *g, t, u, v)


def check_tri(out, what):
    """out: (n, 5) words accept, t, U, V, front of the code under test on tri_inputs().  Returns the largest residual
    ratio."""
    c, ref = tri_inputs(), tri_truth()
    acc, front = out[:, 0] == 1, out[:, 4] == 1
    rows = np.flatnonzero(acc)
    ratio = tri_ratio(c, out, rows)
    dec = ref["decided"]
    wrong = dec & (acc != ref["accept"])
    wrong_front = dec & ref["accept"] & acc & (front != ref["front"])
    report(what, accepted=len(rows), max_residual_ratio=float(ratio.max()), K=K_TRI, decided=int(dec.sum()),
           wrong_accept=int(wrong.sum()), wrong_front=int(wrong_front.sum()))
    assert len(rows) >= N_TRI // 10
    worst = rows[np.argsort(ratio)[-3:]]
    assert ratio.max() <= K_TRI, (what, "residual over the bound", ratio.max(), worst, out[worst])
    assert not wrong.any(), (what, "accept differs from the float64 decision", np.flatnonzero(wrong)[:5],
                             out[np.flatnonzero(wrong)[:5]], ref["t"][wrong][:5], ref["u"][wrong][:5], ref["v"][wrong][:5])
    assert not wrong_front.any(), (what, "front differs from sign(n . -d)", np.flatnonzero(wrong_front)[:5])
    return float(ratio.max())


def np_tri_f32(c):
    """A plain numpy float32 Moller-Trumbore (the stand-in that sets K): words t, U, V as check_tri reads them."""
    o, d, v0, e1, e2 = tri_geometry(c)
    cross = lambda a, b: f32(np.cross(a, b))
    dot = lambda a, b: f32((a * b).sum(-1, dtype=F))
    p = cross(d, e2)
    with np.errstate(all="ignore"):
        inv = F(1) / dot(p, e1)
        s = f32(o - v0)
        q = cross(s, e1)
        t, u, v = dot(e2, q) * inv, dot(s, p) * inv, dot(d, q) * inv
    out = np.zeros((len(o), 5), np.uint32)
    out[:, 1], out[:, 2], out[:, 3] = u32(f32(t)), u32(f32(u)), u32(f32(v))
    return out


def test_inputs_tri_truth():
    """The triangle inputs on the float64 side alone: at most 10 % undecided; hits, misses, both facings, finite best_t
    on both sides of the hit, and scales from 1e-3 to 1e3 among the decided elements."""
    c, ref = tri_inputs(), tri_truth()
    und = 1.0 - ref["decided"].mean()
    dec, acc = ref["decided"], ref["accept"]
    fin = np.isfinite(c["best_t"])
    report("triangle inputs", undecided=float(und), accepted=int((dec & acc).sum()), front=int((dec & acc & ref["front"]).sum()),
           cut_by_best_t=int((dec & fin & ~acc & (ref["t"] > c["best_t"])).sum()))
    assert und <= UNDECIDED_TRI_CAP
    assert (dec & acc).sum() >= N_TRI // 10 and (dec & ~acc).sum() >= N_TRI // 5
    assert min((dec & acc & ref["front"]).sum(), (dec & acc & ~ref["front"]).sum()) >= N_TRI // 20
    assert 0.45 <= fin.mean() <= 0.55
    assert (dec & fin & acc).sum() >= 5000 and (dec & fin & ~acc & (ref["t"] > c["best_t"])).sum() >= 5000
    size = truth.norm(c["e1"])
    for lo, hi in ((0, 1e-2), (1e-2, 1), (1, 1e2), (1e2, np.inf)):
        assert (dec & acc & (size >= lo) & (size < hi)).sum() >= 1000, (lo, hi)
    assert (dec & ~acc & (np.abs(truth.tri_solve(*tri_geometry(c))[3]) < truth.DET_EPS)).sum() >= 100, "parallel by 1e-8"


def test_standin_constants():
    """What sets the constants: the numpy float32 stand-ins on the tests' own inputs.  Triangle: 2.4 on 4e5 elements of
    this distribution when the bound was chosen, measured here on tri_inputs(); sphere: sphere_ratio of np_sphere_f32.
    K is three times the measured value, rounded up: the margin for another operation order, fused multiply-adds and the
    exact reciprocal."""
    c, ref = tri_inputs(), tri_truth()
    rows = np.flatnonzero(ref["decided"] & ref["accept"])
    r_tri = float(tri_ratio(c, np_tri_f32(c), rows).max())
    s = sphere_inputs()
    out = np_sphere_f32(s)
    rows = np.flatnonzero(sphere_judged(s) & (out[:, 0] != 0xFFFFFFFF))
    r_sph = float(sphere_ratio(s, out, rows).max())
    report("stand-ins", triangle=r_tri, K_TRI=K_TRI, sphere=r_sph, K_SPH=K_SPH)
    assert 3.0 * r_tri <= K_TRI and 3.0 * r_sph <= K_SPH


def test_oracle_tri_against_float64(built):
    """hgo_tri_accept_batch (triangle_intersection_doublesided HC:307-355 with the accept rule HC:416) on 2e5 elements:
    the residual |o + t d - v0 - U e1 - V e2| of every accepted (t, U, V) within K 2^-24 mag / (c s), K = 8; accept and
    front equal to the float64 decision on every decided element.  Traits followed: |det| >= 1e-8, t > 1e-4, t < best_t
    (an element is decided only if t also clears best_t - 1e-4, HC:452's rule), front = sign(n . -d).
    Measured maximum of |R| c s / (2^-24 mag) on these inputs: numpy float32 stand-in 1.84, oracle 1.84."""
    check_tri(oracle_tri(tri_inputs()), "oracle triangle")


# ----------------------------------------------------------------------------------------------------------------------
# 1b. box
# ----------------------------------------------------------------------------------------------------------------------
N_BOX = 100_000
BOX_SHARES = [("aimed", 0.30), ("random", 0.10), ("inside", 0.15), ("on_face", 0.15), ("zero_dir", 0.20), ("flat", 0.10)]
UNDECIDED_BOX_CAP = 0.05


def split(n, shares):
    out, at = {}, 0
    for k, (name, s) in enumerate(shares):
        m = n - at if k == len(shares) - 1 else int(round(n * s))
        out[name] = slice(at, at + m)
        at += m
    return out


@lru_cache(maxsize=1)
def box_inputs():
    """(elements (n, 12): A, B, o, inv = 1 / d in float32 (+-inf for +-0); d; class -> slice).  No origin lies on a face
    plane of an axis whose direction component is zero (0 * inf, which the reference's min / max drop, HC:246-258)."""
    rng = np.random.default_rng(8102)
    n = N_BOX
    cls = split(n, BOX_SHARES)
    ctr, half = rng.uniform(-10, 10, (n, 3)), 10.0 ** rng.uniform(-2, 1, (n, 3))
    A, B = f32(ctr - half), f32(ctr + half)
    o = f32(rng.uniform(-30, 30, (n, 3)))
    inside_pt = lambda s, lo=0.02, hi=0.98: f32(A[s] + (B[s] - A[s]) * f32(rng.uniform(lo, hi, (s.stop - s.start, 3))))
    s = cls["inside"]
    o[s] = inside_pt(s)
    s = cls["on_face"]  # one coordinate exactly on a face; the others inside (leaving or entering) or anywhere
    m = s.stop - s.start
    k = rng.integers(0, 3, m)
    o[s] = np.where((rng.random(m) < 0.5)[:, None], inside_pt(s), o[s])
    os_ = o[s].copy()
    os_[np.arange(m), k] = np.where((rng.random(m) < 0.5)[:, None], A[s], B[s])[np.arange(m), k]
    o[s] = os_
    s = cls["flat"]
    m = s.stop - s.start
    flat = rng.random((m, 3)) < 0.4
    flat[np.arange(m), rng.integers(0, 3, m)] = True
    B[s] = np.where(flat, A[s], B[s])
    aim = np.zeros(n, bool)
    aim[cls["aimed"]] = aim[cls["flat"]] = True
    aim[cls["on_face"]] = rng.random(cls["on_face"].stop - cls["on_face"].start) < 0.5
    aim[cls["zero_dir"]] = rng.random(cls["zero_dir"].stop - cls["zero_dir"].start) < 0.5
    target = f32(A + (B - A) * f32(rng.uniform(0, 1, (n, 3))))
    d = np.where(aim[:, None], target.astype(np.float64) - o, rng.normal(0, 1, (n, 3)))
    d = f32(truth.unit(d) * 10.0 ** rng.uniform(-1, 1, (n, 1)))
    s = cls["zero_dir"]  # one or two zero components, either sign of zero; half of those axes with the origin in the slab
    m = s.stop - s.start
    z = rng.random((m, 3)) < 0.4
    z[np.arange(m), rng.integers(0, 3, m)] = True
    full = z.all(1)
    z[np.arange(m)[full], rng.integers(0, 3, int(full.sum()))] = False
    in_slab = z & (rng.random((m, 3)) < 0.6)
    o[s] = np.where(in_slab, inside_pt(s), o[s])
    zero = np.where(rng.random((m, 3)) < 0.5, F(-0.0), F(0.0))
    d[s] = np.where(z, zero, d[s])
    with np.errstate(divide="ignore"):
        inv = f32(F(1) / d)
    return f32(np.concatenate([A, B, o, inv], axis=1)), d, cls


@lru_cache(maxsize=1)
def box_truth():
    x, _, _ = box_inputs()
    hit, entry, exit_ = truth.box_slabs(x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12])
    lower = np.maximum(0.0, entry)
    with np.errstate(invalid="ignore"):
        big = np.maximum(np.abs(entry), np.abs(exit_))
        decided = ~np.isfinite(entry) | ~np.isfinite(exit_) | (np.abs(exit_ - lower) > 4 * truth.ulp32(big))
    flat = (x[:, 0:3] == x[:, 3:6]).any(1)  # a flat axis gives t1 = t2 there, so tMax <= tMin in any arithmetic
    return {"hit": hit, "entry": entry, "exit": exit_, "decided": decided | flat}


def oracle_box(x):
    out = np.empty(len(x), F)
    _oracle("hgo_aabb_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, out.ctypes.data, len(x))
    return out


def check_box(t, what):
    """t: (n,) float32 results of the code under test on box_inputs() (+inf: no hit)."""
    x, _, cls = box_inputs()
    ref = box_truth()
    t = np.asarray(t).view(F) if np.asarray(t).dtype != F else np.asarray(t)
    hit = np.isfinite(t) | (t == -INF)
    wrong = ref["decided"] & (hit != ref["hit"])
    both = hit & ref["hit"] & np.isfinite(ref["entry"])
    inv = np.abs(x[:, 9:12].astype(np.float64))
    inv_max = np.where(np.isfinite(inv), inv, 0).max(1)
    tol = 4 * truth.ulp32(np.maximum(np.abs(ref["entry"]), truth.norm(x[:, 6:9]) * inv_max))
    with np.errstate(invalid="ignore"):
        err = np.abs(t.astype(np.float64) - ref["entry"])
    off = both & ~(err <= tol)
    report(what, hits=int(hit.sum()), wrong=int(wrong.sum()), compared_t=int(both.sum()),
           worst_t_over_tol=float((err[both] / tol[both]).max()))
    assert not np.isnan(t).any()
    assert not wrong.any(), (what, np.flatnonzero(wrong)[:5], x[wrong][:3], t[wrong][:3], ref["entry"][wrong][:3], ref["exit"][wrong][:3])
    assert not off.any(), (what, np.flatnonzero(off)[:5], t[off][:3], ref["entry"][off][:3])
    assert not hit[cls["flat"]].any(), "a box that is flat along an axis is never hit (tMax > tMin, HC:258)"


def test_inputs_box_truth():
    """The box inputs on the float64 side alone: at most 5 % undecided; origins inside (negative entry) and on faces,
    one and two zero direction components of either sign with hits and misses, flat boxes."""
    x, d, cls = box_inputs()
    ref = box_truth()
    A, B, o, inv = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12]
    dec, hit = ref["decided"], ref["hit"]
    report("box inputs", undecided=float(1 - dec.mean()), hit_share=float(hit.mean()))
    assert 1 - dec.mean() <= UNDECIDED_BOX_CAP
    assert not np.isnan(ref["entry"]).any() and not np.isnan(ref["exit"]).any(), "no 0 * inf"
    s = cls["inside"]
    assert hit[s].all() and (ref["entry"][s] < 0).all()
    s = cls["on_face"]
    assert ((o[s] == A[s]) | (o[s] == B[s])).any(1).all() and min((dec & hit)[s].sum(), (dec & ~hit)[s].sum()) >= 1000
    assert ((ref["entry"][s] == 0) & hit[s]).sum() >= 500, "entering through the face the origin lies on"
    s = cls["zero_dir"]
    nz = np.isinf(inv[s]).sum(1)
    assert ((nz == 1).sum() >= 2000) and ((nz == 2).sum() >= 2000) and (nz <= 2).all() and (nz >= 1).all()
    assert (u32(inv[s]) == 0xFF800000).sum() >= 1000 and (u32(inv[s]) == 0x7F800000).sum() >= 1000
    assert min((dec & hit)[s].sum(), (dec & ~hit)[s].sum()) >= 1000
    s = cls["flat"]
    assert (A[s] == B[s]).any(1).all() and not hit[s].any()
    assert (dec & hit)[cls["aimed"]].mean() >= 0.9 and (dec & ~hit)[cls["random"]].sum() >= 1000


def test_oracle_box_against_float64(built):
    """hgo_aabb_batch (ray_AABB_test, HC:244-259) on 1e5 elements against the float64 slab intervals: hit or miss equal
    wherever the float64 exit and max(0, entry) differ by more than 4 float32 ulp of the larger of |entry|, |exit|; on a
    hit the returned value is the ENTRY distance tMin (negative from inside: the trait), within 4 ulp of max(|t|, |o|
    |inv|_inf); flat boxes never hit."""
    check_box(oracle_box(box_inputs()[0]), "oracle box")


# ----------------------------------------------------------------------------------------------------------------------
# 1c. sphere
# ----------------------------------------------------------------------------------------------------------------------
# three times the 7.1 of the numpy float32 stand-in (test_standin_constants), rounded up.  (The form leaves out the factor
# |o - c| / r by which b^2 - 4 c cancels for an origin far outside: origins here lie up to 6 radii out, which is where the
# 7.1 comes from.)
K_SPH = 22.0
N_SPH = 100_000
SPH_SHARES = [("outside", 0.60), ("inside", 0.285), ("surface", 0.10), ("miss", 0.015)]
TANGENT = 0.999
LEFT_OUT_SPH_CAP = 0.02
UNDECIDED_SPH_CAP = 0.15
FAR = F(1e30)


@lru_cache(maxsize=1)
def sphere_inputs():
    """dict o, d (unit), c, r (float32) and `x`, the (n, 20) elements: o, d, closest = inf, far = 1e30, (c, r), the box
    c -+ 1.01 r; class -> slice under `cls`."""
    rng = np.random.default_rng(8103)
    n = N_SPH
    cls = split(n, SPH_SHARES)
    c = f32(rng.uniform(-10, 10, (n, 3)))
    r = f32(10.0 ** rng.uniform(-1, 1, n))
    rad = np.ones(n)
    s = cls["outside"]
    rad[s] = rng.uniform(1.05, 6, s.stop - s.start)
    s = cls["inside"]
    rad[s] = rng.uniform(0, 0.95, s.stop - s.start)
    s = cls["miss"]
    rad[s] = rng.uniform(1.5, 6, s.stop - s.start)
    o = f32(c + truth.unit(rng.normal(0, 1, (n, 3))) * (r * rad)[:, None])
    aim = c + truth.unit(rng.normal(0, 1, (n, 3))) * (r * rng.uniform(0, 0.97, n))[:, None]
    d = aim - o
    s = cls["inside"]
    d[s] = rng.normal(0, 1, (s.stop - s.start, 3))
    s = cls["miss"]
    d[s] = rng.normal(0, 1, (s.stop - s.start, 3))
    d = unit32(d)
    z = np.zeros((n, 1), F)
    pad = f32(r * F(1.01))[:, None]
    x = np.concatenate([o, d, np.full((n, 1), INF), np.full((n, 1), FAR), c, r[:, None], f32(c - pad), z, f32(c + pad), z], axis=1)
    return {"o": o, "d": d, "c": c, "r": r, "x": f32(x), "cls": cls}


def sphere_geometry(s):
    return s["o"], s["d"], s["c"], s["r"]


@lru_cache(maxsize=1)
def sphere_truth():
    s = sphere_inputs()
    t, back, disc, miss = truth.sphere_roots(*sphere_geometry(s))
    b = 2.0 * truth.dot(s["o"].astype(np.float64) - s["c"], s["d"])
    far = np.where(back, t, -b - t)  # the roots add up to -b
    return {"t": t, "back": back, "disc": disc, "far": far, "b_over_r": miss / s["r"].astype(np.float64)}


def sphere_judged(s):
    """The elements whose residual is judged: the ray's line passes the centre within 0.999 r."""
    return sphere_truth()["b_over_r"] <= TANGENT


def sphere_ratio(s, out, rows):
    g = [a[rows] for a in sphere_geometry(s)]
    t = out[rows, 1].view(F)
    return truth.sphere_residual(*g, t) / truth.sphere_bound(1.0, *g, t)


def np_sphere_f32(s):
    """A plain numpy float32 quadratic with the reference's root choice (the stand-in that sets K): words ref, t."""
    o, d, c, r = sphere_geometry(s)
    dot = lambda a, b: f32((a * b).sum(-1, dtype=F))
    sh = f32(o - c)
    b = F(2) * dot(sh, d)
    cq = dot(sh, sh) - r * r
    disc = b * b - F(4) * cq
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
        near, far = (-b - sq) / F(2), (-b + sq) / F(2)
    t = np.where(near < 0, far, near)
    ok = (disc >= 0) & (t > F(0.0001))
    out = np.zeros((len(o), 2), np.uint32)
    out[:, 0] = np.where(ok, np.where(near < 0, 0x80000000, 0), 0xFFFFFFFF)
    out[:, 1] = u32(f32(np.where(ok, t, INF)))
    return out


def oracle_sphere(x):
    out = np.empty((len(x), 2), np.uint32)
    _oracle("hgo_sphere_accept_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, out.ctypes.data, len(x))
    return out


def sphere_decisions(s):
    """(want, decided): want = the reference word (0 front, 0x80000000 back, 0xFFFFFFFF none) of the float64 answer;
    decided where the line passes within 0.999 r and the near root clears 0 and the chosen root clears 1e-4 by the
    residual bound, or where the line clearly misses (beyond 1.001 r)."""
    ref = sphere_truth()
    g = sphere_geometry(s)
    t, back = ref["t"], ref["back"]
    sh =g[0].astype(np.float64) - g[2]
    b = 2.0 * truth.dot(sh, g[1])
    with np.errstate(invalid="ignore"):
        near = (-b - np.sqrt(ref["disc"])) / 2.0
        margin = truth.sphere_bound(K_SPH, *g, t)
        hits_line = ref["b_over_r"] <= TANGENT
        decided = hits_line & (np.abs(near) > margin) & (np.abs(t - truth.HIT_EPS) > margin)
        accept = hits_line & (t > truth.HIT_EPS)
    clear_miss = ref["b_over_r"] >= 2.0 - TANGENT
    want = np.where(accept, np.where(back, 0x80000000, 0), 0xFFFFFFFF).astype(np.uint32)
    return np.where(clear_miss, 0xFFFFFFFF, want).astype(np.uint32), decided | clear_miss


def check_sphere(out, what):
    """out: (n, 2) words (reference, closest t afterwards) of the code under test on sphere_inputs()["x"].  Returns the
    largest residual ratio."""
    s = sphere_inputs()
    acc = out[:, 0] != 0xFFFFFFFF
    rows = np.flatnonzero(acc & sphere_judged(s))
    ratio = sphere_ratio(s, out, rows)
    want, decided = sphere_decisions(s)
    wrong = decided & (out[:, 0] != want)
    report(what, accepted=int(acc.sum()), judged=len(rows), max_residual_ratio=float(ratio.max()), K=K_SPH,
           decided=int(decided.sum()), wrong=int(wrong.sum()))
    assert len(rows) >= N_SPH // 2
    assert ratio.max() <= K_SPH, (what, ratio.max(), rows[np.argsort(ratio)[-3:]])
    assert not wrong.any(), (what, np.flatnonzero(wrong)[:5], out[wrong][:5], want[wrong][:5])
    assert (out[~acc, 1].view(F) == INF).all(), "the closest distance stays where it was"
    k = s["cls"]["surface"]  # the near root is a rounded zero: rejected below 1e-4, or negative and the far root taken
    far_clear = sphere_truth()["far"][k] > 2 * truth.HIT_EPS
    assert np.isin(out[k, 0][far_clear], (0x80000000, 0xFFFFFFFF)).all(), "from the surface inward: never a front hit"
    return float(ratio.max())


def test_inputs_sphere_truth():
    """The sphere inputs on the float64 side alone: at most 2 % with the line beyond 0.999 r (left out of the residual
    check; the clear misses among them still have their decision checked), at most 15 % undecided (the origins on the
    surface, whose near root is a rounded zero: either answer of HC:288 is right there), and outside and inside origins
    decided almost everywhere."""
    s = sphere_inputs()
    ref, cls = sphere_truth(), s["cls"]
    want, decided = sphere_decisions(s)
    left_out = 1.0 - sphere_judged(s).mean()
    report("sphere inputs", left_out=float(left_out), undecided=float(1 - decided.mean()))
    assert left_out <= LEFT_OUT_SPH_CAP and 1 - decided.mean() <= UNDECIDED_SPH_CAP
    assert (decided & (want == 0))[cls["outside"]].mean() >= 0.95
    assert (decided & (want == 0x80000000))[cls["inside"]].mean() >= 0.95
    k = cls["surface"]
    assert (ref["far"][k] > 2 * truth.HIT_EPS).mean() >= 0.9, "aimed inward: the far root is the only hit there can be"
    dist = np.abs(truth.norm(s["o"][k].astype(np.float64) - s["c"][k]) - s["r"][k])
    assert (dist <= 2 * EPS * (truth.norm(s["c"][k]) + s["r"][k])).all(), "on the surface to the rounding of the origin"
    assert (decided & (want == 0xFFFFFFFF)).sum() >= 500, "clear misses"


def test_oracle_sphere_against_float64(built):
    """hgo_sphere_accept_batch (sphere_intersection HC:266-303 in the loop HC:357-376) on 1e5 elements: | |o + t d - c| - r |
    of every accepted t within K 2^-24 (|o - c| + |t| + r) / sqrt(1 - (b / r)^2), K = 22, where the ray's line passes the
    centre within b <= 0.999 r; the accepted reference (front, back or none) equal to the float64 quadratic's with the
    reference's root choice wherever that is decided.  Traits followed: a = 1 (HC:272), from inside the far root with
    orientation -1 (HC:288-292), accepted only above 1e-4 (HC:369).
    Measured maximum of the ratio on these inputs: numpy float32 stand-in 7.06, oracle 7.06."""
    check_sphere(oracle_sphere(sphere_inputs()["x"]), "oracle sphere")


# ----------------------------------------------------------------------------------------------------------------------
# 2. closest hit over instanced meshes against a search over every triangle
# ----------------------------------------------------------------------------------------------------------------------
DISPUTED_CAP = 0.05
EDGE_HUNG_CAP = 0.01
MIN_COS = 0.05
NORMAL_TOL = 1e-5  # about 100 float32 epsilons for a normalised sum of three terms
SCENE_SPHERES = [((-1.3, 0.2, 0.3), 0.5), ((0.3, 0.5, -1.5), 0.4)]
N_OUTER, N_INNER, N_AXIS = 4096, 1024, 256


@lru_cache(maxsize=1)
def closest_scene():
    """The 8,712-triangle dragon at identity, a Unity cube rotated and scaled (0.5, 1, 2), a Unity plane under a mirroring
    transform (scale x < 0) and two analytic spheres.  Returns (packed, meshes): per mesh the float32 matrices as float64
    (row, column), the triangle range in packed.triangles, sign(det localToWorld) and the scale ratio."""
    scene = Scene()
    v, n, t = scenes.dragon_mesh(1)
    scene.add(RayTracingMesh("dragon", v, n, t, Transform()))
    v, n, t = unity_cube()
    scene.add(RayTracingMesh("cube", v, n, t, Transform((1.5, 0.1, 0.2), euler_to_quat(20, 35, 10), (0.5, 1.0, 2.0))))
    v, n, t = unity_plane()
    scene.add(RayTracingMesh("mirrored plane", v, n, t, Transform((0.0, -1.2, 0.0), euler_to_quat(5, 0, 8), (-0.3, 1.0, 0.3))))
    for k, (c, r) in enumerate(SCENE_SPHERES):
        scene.add(RayTracingSphere(f"sphere {k}", Transform(c), r))
    packed = scene.pack()
    meshes = []
    for i, m in enumerate(packed.meshes):
        l2w = np.array(m.localToWorld.m[:], np.float32).reshape(4, 4).T.astype(np.float64)  # m00, m10, m20, m30, m01, ...
        w2l = np.array(m.worldToLocal.m[:], np.float32).reshape(4, 4).T.astype(np.float64)
        sv = np.linalg.svd(l2w[:3, :3], compute_uv=False)
        meshes.append({"l2w": l2w, "w2l": w2l, "first": int(m.triangleBufferOffset), "count": scene.meshes[i].triangle_count,
                       "sign": float(np.sign(np.linalg.det(l2w[:3, :3]))), "ratio": float(sv.max() / sv.min())})
    return packed, meshes


@lru_cache(maxsize=1)
def closest_rays():
    """(n, 8) float32 rays (origin, t_max = inf, unit direction, 0): 4096 from a sphere of radius 6 aimed into the scene,
    1024 from inside the scene's bounds, 256 parallel to an axis with +-0 in the other components."""
    rng = np.random.default_rng(8104)
    lo, hi = np.array([-1.9, -1.3, -2.0]), np.array([2.3, 1.2, 1.9])
    o1 = 6.0 * truth.unit(rng.normal(0, 1, (N_OUTER, 3)))
    d1 = truth.unit(rng.uniform(lo * 0.7, hi * 0.7, (N_OUTER, 3)) - o1)
    o2 = rng.uniform(lo, hi, (N_INNER, 3))
    d2 = truth.unit(rng.normal(0, 1, (N_INNER, 3)))
    ax, sg = rng.integers(0, 3, N_AXIS), np.where(rng.random(N_AXIS) < 0.5, -1.0, 1.0)
    o3 = rng.uniform(lo * 0.6, hi * 0.6, (N_AXIS, 3))
    o3[np.arange(N_AXIS), ax] = -5.0 * sg
    d3 = np.where(rng.random((N_AXIS, 3)) < 0.5, -0.0, 0.0)
    d3[np.arange(N_AXIS), ax] = sg
    rays = np.zeros((N_OUTER + N_INNER + N_AXIS, 8), F)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = np.concatenate([o1, o2, o3]), INF, np.concatenate([d1, d2, d3])
    return rays


@lru_cache(maxsize=1)
def closest_truth():
    """The float64 answer for closest_rays() in closest_scene(): every triangle's float32 local vertices through the
    float64 localToWorld, every ray against every triangle and both spheres, no hierarchy, no cull table."""
    packed, meshes = closest_scene()
    rays = closest_rays().astype(np.float64)
    o, d = rays[:, 0:3], rays[:, 4:7]
    tris = np.frombuffer(bytes(packed.triangles), F).reshape(-1, 18)
    n_t = len(tris)
    v0, e1, e2 = np.empty((n_t, 3)), np.empty((n_t, 3)), np.empty((n_t, 3))
    owner = np.empty(n_t, np.int64)
    for i, m in enumerate(meshes):
        s = slice(m["first"], m["first"] + m["count"])
        v0[s], e1[s], e2[s] = truth.world_triangles(tris[s, 0:3], tris[s, 3:6], tris[s, 6:9], m["l2w"])
        owner[s] = i
    bf = truth.brute_force_closest(o, d, v0, e1, e2)
    R = len(o)
    # the spheres: accepted roots
    ts = np.full((R, len(SCENE_SPHERES)), np.inf)
    back = np.zeros((R, len(SCENE_SPHERES)), bool)
    graze = np.zeros(R, bool)  # a sphere whose hit or miss hangs on a tangent (or on its tight cull box)
    for k, (c, r) in enumerate(SCENE_SPHERES):
        cc, rr = np.broadcast_to(f32(c), (R, 3)), np.full(R, F(r))
        t, b, disc, miss = truth.sphere_roots(o, d, cc, rr)
        ok = (disc >= 0) & (t > truth.HIT_EPS)
        ts[:, k], back[:, k] = np.where(ok, t, np.inf), b
        far_root = np.where(b, t, -2.0 * truth.dot(o - cc, d) - t)
        graze |= (np.abs(miss / r - 1) < 1e-3) & ~(far_root < 0)
    ks = ts.argmin(1)
    t_s = ts[np.arange(R), ks]
    mesh_wins = bf["t1"] < t_s
    t1 = np.minimum(bf["t1"], t_s)
    hit = np.isfinite(t1)
    t2 = np.where(mesh_wins, np.minimum(bf["t2"], t_s), np.minimum(bf["t1"], np.sort(ts, 1)[:, 1]))
    i1 = np.maximum(bf["i1"], 0)
    own = owner[i1]
    sign = np.array([m["sign"] for m in meshes])[own]
    ratio = np.array([m["ratio"] for m in meshes])[own]
    g = (o, d, v0[i1], e1[i1], e2[i1])
    with np.errstate(invalid="ignore", divide="ignore"):
        c_tri, s_tri, _ = truth.tri_conditioning(*g)
        delta = truth.tri_bound(K_TRI, *g, bf["t1"], bf["u"], bf["v"]) * ratio
        du, dv = delta / (truth.norm(e1[i1]) * s_tri), delta / (truth.norm(e2[i1]) * s_tri)
        u, v = bf["u"], bf["v"]
        clear_edges = (u > du) & (v > dv) & (u + v < 1 - du - dv)
    orient_mesh = np.sign(bf["det"]) * sign  # sign(det) on the LOCAL ray: the world winding times sign(det localToWorld)
    w2l = np.stack([m["w2l"] for m in meshes])[own]
    with np.errstate(invalid="ignore"):
        n_mesh = truth.world_normal(tris[i1, 9:12], tris[i1, 12:15], tris[i1, 15:18], np.nan_to_num(u), np.nan_to_num(v),
                                    np.nan_to_num(orient_mesh), w2l)
    # the sphere winner
    cs = f32([c for c, _ in SCENE_SPHERES]).astype(np.float64)[ks]
    rs = f32([r for _, r in SCENE_SPHERES]).astype(np.float64)[ks]
    t_fin = np.where(np.isfinite(t_s), t_s, 0.0)
    orient_s = np.where(back[np.arange(R), ks], -1.0, 1.0)
    n_s = truth.unit(o + t_fin[:, None] * d - cs + 1e-300) * orient_s[:, None]
    delta_s = truth.sphere_bound(K_SPH, o, d, cs, rs, t_fin)
    cos_s = np.abs(truth.dot(n_s, d))
    margin = np.where(mesh_wins, delta, delta_s)
    with np.errstate(invalid="ignore"):
        undisputed = hit & (t2 - t1 >= 2 * truth.HIT_EPS + margin) & (t1 > truth.HIT_EPS + margin) \
            & np.where(mesh_wins, clear_edges & (c_tri >= MIN_COS), (cos_s >= MIN_COS) & ~graze)
    hung = (bf["hit_loose"] != bf["hit_tight"]) | graze  # hit or miss hangs on an edge or a tangent
    # a sphere's normal is (pos - c) / r: the root's error delta / cos along the ray moves pos by as much, and pos itself
    # is rounded at the magnitude |o| + t; a mesh normal is a normalised sum of three terms
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_s = (delta_s / cos_s + 8 * EPS * (truth.norm(o) + t_fin)) / rs
    return {"hit": hit, "mesh": mesh_wins, "t": t1, "object": np.where(mesh_wins, own, ks), "primitive": np.where(mesh_wins, i1, 0),
            "orientation": np.where(mesh_wins, orient_mesh, orient_s), "normal": np.where(mesh_wins[:, None], n_mesh, n_s),
            "undisputed": undisputed, "hung": hung, "margin": margin, "normal_tol": np.where(mesh_wins, NORMAL_TOL, tol_s), "v0": v0, "e1": e1, "e2": e2, "ratio": ratio, "tris": tris, "first": np.array([m["first"] for m in meshes]),
            "w2l": np.stack([m["w2l"] for m in meshes]),
            "any_hit": bf["hit_tight"] | np.isfinite(t_s)}


def check_closest(hits, what):
    """hits: RAY_HIT_DTYPE records of the code under test for closest_rays().  kind: 0 none, 1 mesh, 2 sphere."""
    ref = closest_truth()
    rays = closest_rays().astype(np.float64)
    o, d = rays[:, 0:3], rays[:, 4:7]
    und = ref["undisputed"]
    kind = hits["kind"]
    want_kind = np.where(ref["mesh"], 1, 2)
    t = hits["t"].astype(np.float64)
    bad = {}
    bad["kind"] = und & (kind != want_kind)
    bad["object"] = und & (hits["object"] != ref["object"])
    bad["primitive"] = und & ref["mesh"] & (hits["primitive"] != ref["primitive"])
    bad["orientation"] = und & (np.sign(hits["orientation"]) != ref["orientation"])
    with np.errstate(invalid="ignore"):
        bad["t"] = und & ~(np.abs(t - ref["t"]) <= ref["margin"])
    m = und & ref["mesh"] & (kind == 1)
    i = np.where(m, hits["primitive"].astype(np.int64), 0) % len(ref["v0"])
    u, v = hits["u"].astype(np.float64), hits["v"].astype(np.float64)
    g = (o, d, ref["v0"][i], ref["e1"][i], ref["e2"][i])
    with np.errstate(invalid="ignore", divide="ignore"):
        resid = truth.tri_residual(*g, np.where(m, t, 0), u, v)
        bound = truth.tri_bound(K_TRI, *g, np.where(m, t, 0), u, v) * ref["ratio"]
    bad["position"] = m & ~((resid <= bound) & (u >= 0) & (v >= 0) & (u + v <= 1))
    # a mesh normal: the float64 interpolation at the hit's own (u, v), whose error the position check bounds, so that
    # 1e-5 judges what it was worked out for, the normalised sum of three terms (against the float64 (u, v) the
    # interpolation amplifies the barycentrics' error by |n1 - n0|: up to 2.6e-5 on the dragon's 0.02-sized triangles)
    own = np.searchsorted(ref["first"], i, side="right") - 1
    with np.errstate(invalid="ignore", divide="ignore"):
        n_own = truth.world_normal(ref["tris"][i, 9:12], ref["tris"][i, 12:15], ref["tris"][i, 15:18], u, v,
                                   np.sign(hits["orientation"].astype(np.float64)), ref["w2l"][own])
    want_n = np.where(m[:, None], np.nan_to_num(n_own), ref["normal"])
    err_n = truth.norm(hits["normal"].astype(np.float64) - want_n)
    err_n64 = truth.norm(hits["normal"].astype(np.float64) - ref["normal"])
    bad["normal"] = und & ~(err_n <= ref["normal_tol"])
    judged = ~ref["hung"]
    bad["hit or miss"] = judged & ((kind != 0) != ref["any_hit"])
    report(what, rays=len(rays), undisputed=int(und.sum()), mesh=int((und & ref["mesh"]).sum()),
           worst_mesh_normal=float(err_n[und & ref["mesh"]].max()), at_float64_uv=float(err_n64[und & ref["mesh"]].max()), worst_sphere_normal_over_tol=float((err_n / ref["normal_tol"])[und & ~ref["mesh"]].max()), worst_position_over_bound=float((resid[m] / bound[m]).max()),
           **{f"bad_{k.replace(' ', '_')}": int(b.sum()) for k, b in bad.items()})
    for name, b in bad.items():
        idx = np.flatnonzero(b)[:4]
        assert not b.any(), (what, name, int(b.sum()), idx, hits[idx], ref["t"][idx], ref["object"][idx], ref["primitive"][idx],
                             ref["orientation"][idx], ref["normal"][idx])
    miss = kind == 0
    assert np.all(hits["t"][miss] == INF)


def oracle_closest():
    packed, _ = closest_scene()
    return hg_oracle.intersect_batch(packed, closest_rays())


def test_inputs_closest_truth(built):
    """The closest-hit case on the float64 side alone: at most 5 % of the rays disputed, at most 1 % with a hit or miss
    hanging on an edge or a tangent; undisputed winners on every mesh and sphere, of both orientations on the mirrored
    plane and from inside; unit directions, +-0 components among the axis rays."""
    ref = closest_truth()
    rays = closest_rays()
    _, meshes = closest_scene()
    und = ref["undisputed"]
    disputed = (ref["hit"] & ~und).mean()  # a ray with a float64 winner that is not judged
    report("closest inputs", disputed=float(disputed), hung=float(ref["hung"].mean()), hit=float(ref["hit"].mean()))
    assert disputed <= DISPUTED_CAP and ref["hung"].mean() <= EDGE_HUNG_CAP
    assert np.abs(truth.norm(rays[:, 4:7]) - 1).max() <= 2 * EPS
    z = rays[-N_AXIS:, 4:7]
    assert ((z == 0).sum(1) == 2).all() and (u32(z) == 0x80000000).sum() >= 64 and (u32(z) == 0).sum() >= 64
    assert [m["sign"] for m in meshes] == [1.0, 1.0, -1.0] and meshes[1]["ratio"] > 3.9
    for k in range(3):
        w = und & ref["mesh"] & (ref["object"] == k)
        assert w.sum() >= 150, (k, int(w.sum()))
        assert min((w & (ref["orientation"] > 0)).sum(), (w & (ref["orientation"] < 0)).sum()) >= (20 if k else 5), k
    for k in range(2):
        w = und & ~ref["mesh"] & (ref["object"] == k)
        assert w.sum() >= 100 and (w & (ref["orientation"] < 0)).sum() >= 5, k
    assert (~ref["hit"] & ~ref["hung"]).sum() >= 50, "clear misses"


def test_oracle_closest_against_float64(built):
    """hgo_intersect_batch (get_ray_intersection, HC:357-485: the world-to-local transform, the BVH descent, the leaf
    tests and the hit's resolution) against the hierarchy-free float64 search, on 5,376 rays over the dragon, a scaled
    cube, a mirrored plane and two spheres.  Undisputed rays: kind, object, primitive and the sign of the orientation
    equal; t within the section-1 bound (world magnitudes times the instance's scale ratio); the hit point within that
    bound of o + t d = v0 + u e1 + v e2 on the winner's world triangle with the hit's (u, v) inside it; a mesh normal
    within 1e-5 of the float64 interpolation at that (u, v), carried to world space and normalised, times the
    orientation; a sphere normal within (delta / cos + 8 eps (|o| + t)) / r of (pos - c) / r.
    Measured: worst mesh normal 1.4e-7 (2.6e-5 against the float64 (u, v)), worst position 0.2 of its bound.
    Every ray whose answer does not hang on an edge or a tangent: hit or miss equal.  Traits followed: the orientation
    is the LOCAL winding's (a mirrored instance flips the world winding, HC:350, 392), the normal goes to world space as
    row vector times worldToLocal (HC:467), which is the textbook inverse transpose also under the (0.5, 1, 2) scale."""
    check_closest(oracle_closest(), "oracle closest hit")


# ----------------------------------------------------------------------------------------------------------------------
# 3. the sampler is a net
# ----------------------------------------------------------------------------------------------------------------------
NET_M = (1, 3, 6, 10)
NET_BLOCKS = (0, 5)  # the aligned blocks [0, 2^m) and [5 2^m, 6 2^m) of `frame`
ON_GRID_CAP = 0.001


@lru_cache(maxsize=1)
def net_triples():
    """32 seeded (pixel, offset, id) triples: pixel any uint32, offset a multiple of the bounce increment, id 0 .. 4."""
    rng = np.random.default_rng(8105)
    return np.stack([rng.integers(0, 1 << 32, 32, dtype=np.uint64), 5 * rng.integers(0, 40, 32), rng.integers(0, 5, 32)],
                    axis=1).astype(np.uint32)


def net_tuples(m, block):
    """The probe's (frame, pixel, offset, id) elements of every triple over the block: (32 * 2^m, 4) uint32."""
    tr = net_triples()
    frames = np.arange(block << m, (block + 1) << m, dtype=np.uint32)
    t = np.empty((len(tr), len(frames), 4), np.uint32)
    t[:, :, 0], t[:, :, 1:] = frames[None, :], tr[:, None, :]
    return t.reshape(-1, 4)


def oracle_net_u32(m, block):
    """(get1 (32, 2^m), get2 (32, 2^m, 2)) uint32 of the oracle: index = frame, dimension = offset + id, seed = pixel."""
    L = hg_oracle.lib()
    t = net_tuples(m, block)
    g1, g2 = np.empty(len(t), np.uint32), np.empty((len(t), 2), np.uint32)
    pair = (C.c_uint32 * 2)()
    for k, (frame, pixel, offset, ident) in enumerate(t.tolist()):
        g1[k] = L.hgo_u32_owen_scrambled_sobol(frame, offset + ident, pixel)
        L.hgo_u32_2d_owen_scrambled_sobol(frame, offset + ident, pixel, pair)
        g2[k] = pair[0], pair[1]
    return g1.reshape(32, -1), g2.reshape(32, -1, 2)


def check_net_floats(g1, g2, m, what):
    """g1 (32, 2^m), g2 (32, 2^m, 2): the float32 samples (u32 / 2^32) of a block.  Exact: no tolerance."""
    bad = grid = 0
    for k in range(len(g1)):
        b1, a1 = truth.net_violations_float(g1[k][:, None], m)
        b2, a2 = truth.net_violations_float(g2[k], m)
        bad, grid = bad + b1 + b2, grid + a1 + a2
    assert bad == 0, (what, m, bad)
    return grid


def test_oracle_sampler_is_a_net(built):
    """hgo_u32_owen_scrambled_sobol and hgo_u32_2d_owen_scrambled_sobol (HR:203-228) on their uint32 values, for 32
    triples, m in {1, 3, 6, 10} and the frame blocks [0, 2^m) and [5 2^m, 6 2^m): get1 puts exactly one point in every
    interval of length 2^-m; get2's points form a (0, m, 2)-net, one point in every elementary box 2^-a x 2^-(m - a).  No
    tolerance.  (Owen scrambling keeps both; the index shuffle maps an aligned block onto an aligned block.)"""
    total = 0
    for m in NET_M:
        for block in NET_BLOCKS:
            g1, g2 = oracle_net_u32(m, block)
            for k in range(32):
                assert truth.strata_violations_u32(g1[k], m) == 0, (m, block, k)
                assert truth.net_violations_u32(g2[k], m) == 0, (m, block, k)
                total += 1
    report("oracle sampler", blocks_checked=total)


def test_inputs_net_floats(built):
    """The float form of the check (what the device probe returns) on the oracle's values: float(u32) / 2^32 rounds to 24
    bits (HR:258), so a sample may land exactly on a grid line k / 2^m from just below it; such samples may count for
    either neighbouring cell.  At most 0.1 % of the samples are of that kind, the float check passes on the oracle's
    values, and it is not vacuous: it fails when two samples of a block are swapped between blocks or one is repeated."""
    grid = n = 0
    for m in NET_M:
        for block in NET_BLOCKS:
            g1, g2 = oracle_net_u32(m, block)
            f1, f2 = f32(g1.astype(F) / F(4294967296.0)), f32(g2.astype(F) / F(4294967296.0))
            grid += check_net_floats(f1, f2, m, "oracle floats")
            n += 3 * g1.size
    report("net floats", samples=n, on_grid_lines=grid)
    assert grid <= ON_GRID_CAP * n
    g1, g2 = oracle_net_u32(6, 0)
    f2 = f32(g2.astype(F) / F(4294967296.0))
    broken = f2.copy()
    broken[0, 3] = broken[0, 4]
    assert truth.net_violations_float(broken[0], 6)[0] > 0
    other = f32(oracle_net_u32(6, 5)[1].astype(F) / F(4294967296.0))
    mixed = f2[0].copy()
    mixed[:8] = other[0][:8]
    assert truth.net_violations_float(mixed, 6)[0] > 0
    assert truth.net_violations_float(f32(g1[0].astype(F) / F(4294967296.0))[:, None] * F(0.5), 6)[0] > 0


PAD_M = 10


def pad_tuples(block):
    """net_tuples(10, block) twice: with each triple's id, and with the next id (another dimension of the same pixel)."""
    a = net_tuples(PAD_M, block)
    b = a.copy()
    b[:, 3] = (b[:, 3] + 1) % 5
    return a, b


def check_dimensions_decorrelated(xa, xb, what):
    """xa, xb: (32, 1024) samples in [0, 1], the first components of get2 in two dimensions at the same frames.  The index
    shuffle (HR:219, "shuffles index to decorrelate between dimensions") makes the pairs fill the 4 x 4 cells of the unit
    square like independent samples: every count within 6 standard deviations of 64, i.e. in [18, 110].  Without it both
    are Owen scrambles of the same Sobol point and 12 of the 16 cells stay empty."""
    lo, hi = truth.independent_cell_bound(1 << PAD_M)
    worst = [0, 1 << PAD_M]
    for k in range(len(xa)):
        c = truth.cell_counts(xa[k], xb[k])
        worst = [max(worst[0], int(c.max())), min(worst[1], int(c.min()))]
        assert c.min() >= lo and c.max() <= hi, (what, k, c.reshape(4, 4))
    report(what, largest_cell=worst[0], smallest_cell=worst[1], bound=(round(float(lo), 1), round(float(hi), 1)))


def oracle_get2_x(t):
    L = hg_oracle.lib()
    pair = (C.c_uint32 * 2)()
    out = np.empty(len(t), np.float64)
    for k, (frame, pixel, offset, ident) in enumerate(t.tolist()):
        L.hgo_u32_2d_owen_scrambled_sobol(frame, offset + ident, pixel, pair)
        out[k] = pair[0] / 4294967296.0
    return out.reshape(32, -1)


@pytest.mark.parametrize("block", NET_BLOCKS)
def test_oracle_sampler_dimensions_are_decorrelated(built, block):
    """hgo_u32_2d_owen_scrambled_sobol in two dimensions of the same pixel over 1024 consecutive frames
    (check_dimensions_decorrelated): what the net property cannot see, since the unshuffled Sobol points are a net too."""
    a, b = pad_tuples(block)
    check_dimensions_decorrelated(oracle_get2_x(a), oracle_get2_x(b), f"oracle sampler dimensions, block {block}")


# ----------------------------------------------------------------------------------------------------------------------
# 4. scattering against optics
# ----------------------------------------------------------------------------------------------------------------------
IORS = f32([1.0, 1.0003, 1.33, 1.5, 2.4])
N_OPTICS = 60_000
OPTICS_SHARES = [("random", 0.50), ("normal_incidence", 0.05), ("near_critical", 0.25), ("beyond_critical", 0.10), ("grazing", 0.10)]
CRITICAL_BAND = 1e-5  # "away from the critical angle": |(n1 / n2) sin theta1 - 1| > 1e-5
GRAZING = 1e-3
NEAR_CRITICAL_CAP = 0.05
N_SWEEPS, N_ANGLES = 64, 256


def _incident(n, tangent, theta):
    return unit32(np.sin(theta)[:, None] * tangent - np.cos(theta)[:, None] * n.astype(np.float64))


def _tangent(rng, n):
    return truth.unit(np.cross(n.astype(np.float64), rng.normal(0, 1, (len(n), 3))))


@lru_cache(maxsize=1)
def optics_inputs():
    """dict i, n (unit float32, n facing the ray: cos theta1 = -i . n > 0), n1, n2 (every pair of IORS), lo, hi (lo < hi)."""
    rng = np.random.default_rng(8106)
    N = N_OPTICS
    cls = split(N, OPTICS_SHARES)
    n = unit32(rng.normal(0, 1, (N, 3)))
    axis = np.zeros((N, 3), F)
    axis[np.arange(N), rng.integers(0, 3, N)] = np.where(rng.random(N) < 0.5, -1, 1)
    n = np.where((rng.random(N) < 0.1)[:, None], axis, n)
    n1, n2 = IORS[rng.integers(0, 5, N)], IORS[rng.integers(0, 5, N)]
    theta = np.arccos(rng.uniform(0.02, 1.0, N))
    s = cls["normal_incidence"]
    n[s], theta[s] = axis[s], 0.0
    dense = [(a, b) for a in IORS for b in IORS if a > b]
    for name, lo_f, hi_f in (("near_critical", 1 - 1e-3, 1 + 1e-3), ("beyond_critical", 1.01, None)):
        s = cls[name]
        m = s.stop - s.start
        pair = np.array(dense)[rng.integers(0, len(dense), m)]
        n1[s], n2[s] = pair[:, 0], pair[:, 1]
        crit = np.arcsin(pair[:, 1].astype(np.float64) / pair[:, 0])
        theta[s] = crit * rng.uniform(lo_f, hi_f, m) if hi_f else rng.uniform(np.minimum(crit * lo_f, 1.5), 0.99 * np.pi / 2)
    s = cls["grazing"]
    theta[s] = np.arccos(rng.uniform(2e-3, 2e-2, s.stop - s.start))
    i = _incident(n, _tangent(rng, n), theta)
    i[cls["normal_incidence"]] = -n[cls["normal_incidence"]]
    lo = f32(rng.choice([0.0, 0.02, 0.5], N))
    hi = np.where(rng.random(N) < 0.7, F(1), f32(rng.uniform(0.6, 2.0, N)))
    return {"i": i, "n": n, "n1": f32(n1), "n2": f32(n2), "lo": lo, "hi": f32(hi), "cls": cls}


@lru_cache(maxsize=1)
def schlick_sweeps():
    """64 seeded sweeps of 256 angles 0 .. pi / 2 each, as (64 * 256, 10) schlick elements: n1, n2, normal, incident, lo, hi."""
    rng = np.random.default_rng(8107)
    n = unit32(rng.normal(0, 1, (N_SWEEPS, 3)))
    tg = _tangent(rng, n)
    n1, n2 = IORS[rng.integers(0, 5, N_SWEEPS)], IORS[rng.integers(0, 5, N_SWEEPS)]
    n1[:8], n2[:8] = IORS[[4, 4, 3, 3, 2, 2, 1, 4]], IORS[[0, 3, 0, 2, 0, 1, 0, 2]]  # from the denser side for certain
    lo, hi = f32(rng.choice([0.0, 0.02, 0.5], N_SWEEPS)), f32(rng.choice([1.0, 0.8, 1.5], N_SWEEPS))
    theta = np.linspace(0.0, np.pi / 2, N_ANGLES)
    rep = lambda a: np.repeat(a, N_ANGLES, axis=0)
    inc = _incident(rep(n), rep(tg), np.tile(theta, N_SWEEPS))
    return f32(np.concatenate([rep(n1)[:, None], rep(n2)[:, None], rep(n), inc, rep(lo)[:, None], rep(hi)[:, None]], axis=1))


def reflect_elements(c):
    return f32(np.concatenate([c["i"], c["n"]], axis=1))


def refract_elements(c):
    return f32(np.concatenate([c["i"], c["n"], c["n1"][:, None], c["n2"][:, None]], axis=1))


def schlick_elements(c):
    return f32(np.concatenate([c["n1"][:, None], c["n2"][:, None], c["n"], c["i"], c["lo"][:, None], c["hi"][:, None]], axis=1))


def check_reflect(r, what):
    """r: (n, 3) float32 results for reflect_elements(optics_inputs()).  Inputs are unit to half a float32 ulp per
    component, so |r|^2 = |i|^2 + 4 (i . n)^2 (|n|^2 - 1) is 1 within 5 * 2^-24 before the five roundings of r itself."""
    c = optics_inputs()
    i, n, r = (a.astype(np.float64) for a in (c["i"], c["n"], r))
    length = np.abs(truth.norm(r) - 1).max()
    mirror = np.abs(truth.dot(r, n) + truth.dot(i, n)).max()
    parallel = truth.norm(np.cross(r - i, n)).max()
    report(what, length=float(length / EPS), mirror=float(mirror / EPS), parallel=float(parallel / EPS), unit="float32 eps")
    assert length <= 8 * EPS and mirror <= 8 * EPS and parallel <= 8 * EPS


def refract_split(c):
    """(sin1, product (n1 / n2) sin1, cos1, away from the critical angle, not grazing)."""
    sin1, prod, cos1 = truth.snell(c["i"], c["n"], c["n1"], c["n2"])
    return sin1, prod, cos1, np.abs(prod - 1) > CRITICAL_BAND, np.abs(cos1) >= GRAZING


def check_refract(out, what):
    """out: (n, 4) words direction, tir for refract_elements(optics_inputs()).  Unit length and coplanarity within 16
    float32 eps: the direction is n12 (i + cos n) - sqrt(|1 - lp^2|) n with n12 <= 2.4, whose square scales the inputs'
    half-ulp departures from unit length, plus some ten roundings."""
    c = optics_inputs()
    sin1, prod, cos1, away, steep = refract_split(c)
    tir = out[:, 3] == 1
    wrong = away & (tir != (prod > 1))
    t = out[:, 0:3].view(F).astype(np.float64)
    ok = ~tir & steep & away
    i, n = c["i"].astype(np.float64), c["n"].astype(np.float64)
    length = np.abs(truth.norm(t) - 1)[ok].max()
    oblique = ok & (sin1 > 1e-3)  # the plane of incidence is defined
    coplanar = np.abs(truth.dot(t[oblique], truth.unit(np.cross(i, n)[oblique]))).max()
    far_side = truth.dot(t, n)[ok].max()
    sin2 = truth.norm(np.cross(t, n))
    rel = (np.abs(c["n1"] * sin1 - c["n2"] * sin2) / np.maximum(c["n1"] * sin1, 1e-30))[oblique].max()
    report(what, tir=int(tir.sum()), refracted=int(ok.sum()), wrong_tir=int(wrong.sum()), length_eps=float(length / EPS),
           coplanar_eps=float(coplanar / EPS), far_side=float(far_side), snell_rel=float(rel))
    assert not wrong.any(), (what, np.flatnonzero(wrong)[:5], prod[wrong][:5])
    assert length <= 16 * EPS and coplanar <= 16 * EPS and far_side <= 16 * EPS and rel <= 1e-5
    # total internal reflection returns the mirror direction (HC:563-566)
    m = tir & away
    mirror = i - 2 * truth.dot(i, n)[:, None] * n
    assert truth.norm(t - mirror)[m].max() <= 8 * EPS


SCHLICK_AWAY = 0.9
SCHLICK_LEFT_OUT_CAP = 0.30


def schlick_away(sin_t2):
    """Where the value is held to 1e-5 of the float64 formula: sinT2 <= 0.9 (or beyond the critical angle, where it is
    `hi`).  cosX = sqrt(1 - sinT2) turns sinT2's rounding, about 2 n12^2 2^-24 <= 7e-7, into 7e-7 / (2 sqrt(1 - sinT2)),
    and (1 - cosX)^5 multiplies it by at most 5: 5.5e-6 at sinT2 = 0.9, and past 1e-5 from 0.97 on."""
    return (sin_t2 <= SCHLICK_AWAY) | (sin_t2 > 1 + CRITICAL_BAND)


def check_schlick(val, sweep_val, what):
    """val: (n,) float32 for schlick_elements(optics_inputs()); sweep_val: (64 * 256,) for schlick_sweeps()."""
    c = optics_inputs()
    want, sin_t2 = truth.schlick(c["n1"], c["n2"], c["n"], c["i"], c["lo"], c["hi"])
    v = val.astype(np.float64)
    lo, hi = c["lo"].astype(np.float64), c["hi"].astype(np.float64)
    away = schlick_away(sin_t2)
    s = c["cls"]["normal_incidence"]
    r0 = ((c["n1"].astype(np.float64) - c["n2"]) / (c["n1"].astype(np.float64) + c["n2"])) ** 2
    at_normal = np.abs(v[s] - (lo[s] + r0[s] * (hi[s] - lo[s]))).max()
    beyond = sin_t2 > 1 + CRITICAL_BAND
    err = np.abs(v - want)[away].max()
    report(what, outside_range=int(((v < lo) | (v > hi)).sum()), at_normal=float(at_normal), beyond=int(beyond.sum()), err=float(err))
    assert ((v >= lo) & (v <= hi)).all()
    assert at_normal <= 4 * EPS
    assert beyond.sum() >= 1000 and (val[beyond] == c["hi"][beyond]).all()
    assert err <= 1e-5
    sw = sweep_val.astype(np.float64).reshape(N_SWEEPS, N_ANGLES)
    assert (np.diff(sw, axis=1) >= 0).all(), "non-decreasing in the angle"
    assert (sw[:, -1] > sw[:, 0]).all(), "and it does rise"


def oracle_reflect(x):
    out = np.empty((len(x), 3), F)
    _oracle("hgo_scatter_batch", [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64])(1, x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_refract(x):
    out = np.empty((len(x), 4), np.uint32)
    _oracle("hgo_refract_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, out.ctypes.data, len(x))
    return out


def oracle_schlick(x):
    out = np.empty(len(x), F)
    _oracle("hgo_schlick_batch", [C.c_void_p, C.c_void_p, C.c_int64])(x.ctypes.data, out.ctypes.data, len(x))
    return out


def test_inputs_optics():
    """The optics inputs on the float64 side alone: unit vectors facing the ray, every index pair, at most 5 % inside
    the critical band (left out of the TIR and value checks), refraction and total internal reflection both present away
    from it, near-critical cases on both sides, normal incidence exact."""
    c = optics_inputs()
    sin1, prod, cos1, away, steep = refract_split(c)
    report("optics inputs", in_band=float(1 - away.mean()), tir=int((away & (prod > 1)).sum()), grazing=int((~steep).sum()))
    assert 1 - away.mean() <= NEAR_CRITICAL_CAP
    assert np.abs(truth.norm(c["i"]) - 1).max() <= 2 * EPS and np.abs(truth.norm(c["n"]) - 1).max() <= 2 * EPS
    assert (cos1 > 0).all() and (cos1[c["cls"]["normal_incidence"]] == 1).all()
    assert {(float(a), float(b)) for a, b in zip(c["n1"], c["n2"])} == {(float(a), float(b)) for a in IORS for b in IORS}
    assert (away & (prod > 1)).sum() >= 5000 and (away & (prod <= 1) & steep).sum() >= 20000
    s = c["cls"]["near_critical"]
    near = np.abs(prod[s] - 1) < 2e-3
    assert (near & away[s] & (prod[s] > 1)).sum() >= 3000 and (near & away[s] & (prod[s] < 1)).sum() >= 3000
    assert (c["lo"] < c["hi"]).all()
    _, sin_t2 = truth.schlick(c["n1"], c["n2"], c["n"], c["i"], c["lo"], c["hi"])
    left_out = 1 - schlick_away(sin_t2).mean()  # (the near-critical class, which is there for refract's decision)
    report("schlick inputs", left_out_of_value_check=float(left_out))
    assert left_out <= SCHLICK_LEFT_OUT_CAP and (np.abs(sin_t2 - 1) <= CRITICAL_BAND).mean() <= NEAR_CRITICAL_CAP
    assert ((sin_t2 > 0) & (sin_t2 <= SCHLICK_AWAY)).sum() >= 3000, "from the denser side, below the critical angle"
    sw = schlick_sweeps()
    assert sw.shape == (N_SWEEPS * N_ANGLES, 10) and (sw[::N_ANGLES, 0] > sw[::N_ANGLES, 1]).sum() >= 8


def test_oracle_optics(built):
    """specular_scatter (HC:506), refract (HC:557-572) and schlick_adjusted_specular (HC:519-540) of the oracle against
    optics: the mirror law; Snell's law n1 sin theta1 = n2 sin theta2 within 1e-5 relative, the TIR decision away from the
    critical angle, a unit, coplanar, far-side direction; Schlick inside [lo, hi], lo + R0 (hi - lo) at normal incidence,
    hi beyond the critical angle, non-decreasing along 64 sweeps, within 1e-5 of the float64 formula.  Trait followed: from
    the denser side Schlick uses the transmitted angle's cosine (HC:525-534)."""
    c = optics_inputs()
    check_reflect(oracle_reflect(reflect_elements(c)), "oracle reflect")
    check_refract(oracle_refract(refract_elements(c)), "oracle refract")
    check_schlick(oracle_schlick(schlick_elements(c)), oracle_schlick(schlick_sweeps()), "oracle schlick")


# the diffuse scatter, through evaluate_material_hit
N_DIFFUSE = 16384
DIFFUSE_NORMALS = f32([[0.0, 1.0, 0.0], truth.unit([1.0, 2.0, 3.0]), truth.unit([-0.3, 0.5, -0.8])])
DIFFUSE_ALBEDO = (0.6, 0.5, 0.4, 1.0)
DIFFUSE_POS = f32([1.0, 2.0, 3.0])
MOMENT_TOL = 4.0 / np.sqrt(N_DIFFUSE)  # the plain Monte Carlo bound for a variable of variance at most 1


@lru_cache(maxsize=1)
def diffuse_material():
    """One purely diffuse material: no specular chance (metallic 0), not transmissive (albedo.w = 1), no interface
    tracking, index 1, no absorption."""
    from halogen import abi
    mats = (abi.PackedHalogenMaterial * 1)()
    mats[0] = pack_material(HalogenMaterial(color=DIFFUSE_ALBEDO, metallic=0.0, dielectricPriority=-1), 0)
    return mats


def diffuse_elements(k):
    """evaluate_hit elements (n, 21) for normal k: frames 1 .. 16384 of one pixel at dimension offset 0, an empty medium
    stack, a front hit at DIFFUSE_POS."""
    n = DIFFUSE_NORMALS[k]
    x = np.zeros((N_DIFFUSE, 21), np.uint32)
    x[:, 0] = np.arange(1, N_DIFFUSE + 1)
    x[:, 1] = 0x9E3779B9 + k
    fl = x[:, 6:20].view(F)
    fl[:, 0:3] = DIFFUSE_POS + 2 * n
    fl[:, 3:6] = -n
    fl[:, 6], fl[:, 7] = 2.0, 1.0
    fl[:, 8:11], fl[:, 11:14] = DIFFUSE_POS, n
    return x


def check_diffuse(out, k, what):
    """out: (n, 19) words of evaluate_hit for diffuse_elements(k): attenuation, ray.o, ray.d, bounce type, stack."""
    n = DIFFUSE_NORMALS[k].astype(np.float64)
    att, org, d = (out[:, a:a + 3].view(F).astype(np.float64) for a in (0, 3, 6))
    moments = truth.hemisphere_moments(d, n)
    off = np.abs(moments - truth.COSINE_MOMENTS)
    want_o = DIFFUSE_POS.astype(np.float64) + n * truth.HIT_EPS
    report(what, normal=k, moments=np.round(moments, 4).tolist(), worst=float(off.max()), tol=float(MOMENT_TOL),
           min_cos=float((d @ n).min()))
    assert (out[:, 9] == 0).all() and (out[:, 10] == 0).all(), "a diffuse bounce, the stack empty afterwards"
    assert np.array_equal(out[:, 0:3].view(F), np.broadcast_to(f32(DIFFUSE_ALBEDO[:3]), (len(out), 3)))
    assert np.abs(truth.norm(d) - 1).max() <= 4 * EPS and (d @ n).min() >= 0
    assert off.max() <= MOMENT_TOL, (what, moments)
    assert np.abs(org - want_o).max() <= 2 * truth.ulp32(4.0), "the next ray starts at pos + normal * 1e-4 (HC:710)"


def oracle_evaluate_hit(mats, x):
    out = np.empty((len(x), 19), np.uint32)
    _oracle("hgo_evaluate_hit_batch", [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64])(
        C.addressof(mats), len(mats), x.ctypes.data, out.ctypes.data, len(x))
    return out


@pytest.mark.parametrize("k", range(len(DIFFUSE_NORMALS)))
def test_oracle_diffuse_scatter_is_cosine_weighted(built, k):
    """evaluate_material_hit's outgoing direction for a purely diffuse material (lambertain_scatter of HC:491-501 over
    get_random_unit_vector of the frame's Sobol point) over frames 1 .. 16384 of one pixel: unit, in the normal's
    hemisphere, with the moments of a cosine-weighted hemisphere (E[cos] = 2/3, E[cos^2] = 1/2, E[x] = E[y] = 0, E[x^2] =
    E[y^2] = 1/4) within 4 / sqrt(N) = 0.031; a uniform-hemisphere or unnormalised sampler misses by 0.17."""
    check_diffuse(oracle_evaluate_hit(diffuse_material(), diffuse_elements(k)), k, "oracle diffuse scatter")


def test_hemisphere_moments_tell_samplers_apart():
    """The moment check on the float64 side alone: a uniform hemisphere misses E[cos] by 0.17, a cosine-weighted one
    drawn the textbook way passes."""
    rng = np.random.default_rng(8108)
    n = DIFFUSE_NORMALS[1]
    v = truth.unit(rng.normal(0, 1, (N_DIFFUSE, 3)))
    uniform = np.where((v @ n < 0)[:, None], -v, v)
    assert np.abs(truth.hemisphere_moments(uniform, n) - truth.COSINE_MOMENTS).max() > 0.15
    cosine = truth.unit(v + n.astype(np.float64))
    assert np.abs(truth.hemisphere_moments(cosine, n) - truth.COSINE_MOMENTS).max() <= MOMENT_TOL


# ----------------------------------------------------------------------------------------------------------------------
# 5. closed-form images
# ----------------------------------------------------------------------------------------------------------------------
IMG_W = IMG_H = 16
IMG_FRAMES = 256
SKY_L = 1.0
# name: (shape, albedo, emission E)
IMAGE_CASES = {
    "sphere_grey": ("sphere", (0.5, 0.5, 0.5), 0.0),
    "sphere_coloured": ("sphere", (0.8, 0.4, 0.2), 0.0),
    "sphere_emissive": ("sphere", (0.5, 0.5, 0.5), 0.25),
    "cube_flat": ("cube", (0.5, 0.5, 0.5), 0.0),
    "empty": ("empty", (0.0, 0.0, 0.0), 0.0),
}


@lru_cache(maxsize=1)
def constant_sky():
    """Face size 4, 3 mips, every texel (1, 1, 1, 1)."""
    return Cubemap(4, 3, np.full(6 * (16 + 4 + 1) * 4, SKY_L, np.float32))


@lru_cache(maxsize=8)
def image_case(name):
    """(packed, params, cubemap, expected rgb, tolerance): a 16 x 16 view (60 degrees, filter radius 1) from the origin
    along +z of one convex diffuse object that fills the frame, jitter included, under the constant sky."""
    shape, albedo, E = IMAGE_CASES[name]
    mat = HalogenMaterial(color=albedo + (1.0,), metallic=0.0, dielectricPriority=-1, emissionColor=(1.0, 1.0, 1.0, 1.0),
                          emissionIntensity=E)
    scene = Scene()
    if shape == "sphere":  # from 1.25 radii the sphere spans 53 degrees off the axis; the frame's corner, 39 + 4 of jitter
        scene.add(RayTracingSphere("sphere", Transform((0.0, 0.0, 1.25)), 1.0, mat))
    elif shape == "cube":  # side 4 from 2.7 away: its inscribed sphere spans 48 degrees, the camera is outside
        v, n, t = unity_cube()
        scene.add(RayTracingMesh("cube", v, n, t, Transform((0.0, 0.0, 2.7), euler_to_quat(10, 15, 5), (4.0, 4.0, 4.0)), mat))
    packed = scene.pack()
    cube = constant_sky()
    settings = rp.HalogenSettings(useHDRISky=True, environmentCubemap=cube, FilterRadius=1.0)
    params = rp.make_params(rp.clamp_settings(settings), rp.Camera(Transform(), 60.0, IMG_W, IMG_H), 1, len(packed.spheres),
                            len(packed.meshes), True)
    if shape == "empty":
        return packed, params, cube, np.full(3, SKY_L), None
    return packed, params, cube, truth.closed_form_pixel(E, SKY_L, f32(albedo)), truth.closed_form_tolerance(E, SKY_L, IMG_FRAMES)


def check_image(img, name, what):
    """img: (16, 16, 4) float32 after 256 accumulated frames from FrameCount 1."""
    _, _, _, want, tol = image_case(name)
    rgb = img[..., :3].astype(np.float64)
    err = np.abs(rgb - want).max()
    assert np.isfinite(img).all() and (img[..., 3] == 1).all(), (what, name)
    if tol is None:  # the sky alone: L through the cube lookup and 256 blends
        report(what, case=name, worst_ulp=float(err / truth.ulp32(SKY_L)))
        assert err <= 4 * truth.ulp32(SKY_L), (what, name, err)
        return
    report(what, case=name, want=np.round(want, 4).tolist(), worst=float(err), tol=float(tol),
           mean_error=float(np.abs(rgb.mean((0, 1)) - want).max()))
    assert err <= tol, (what, name, err, tol, np.argwhere(np.abs(rgb - want) > tol)[:4])


@pytest.mark.parametrize("name", sorted(IMAGE_CASES))
def test_oracle_closed_form_image(built, name):
    """hg_oracle.render of a convex diffuse object under a constant sky: every path is hit, scatter outward, leave to
    the sky; Russian roulette at the hit survives with probability max(albedo) and rescales by 1 / max(albedo)
    (HC:929-935), so a pixel's mean is E + L (rho_c / rho_max) m / N with m the frames whose roulette sample is <=
    rho_max, and |m - rho_max N| <= 2 over frames 1 .. N by the sampler's 1-D stratification.  Every pixel and channel
    within 2 L / N + N 2^-24 (E + L) = 0.0078 of E + rho_c L; a missing rescale, a stray pi or a stray cosine is off by
    0.25 or more.  From the scene alone: every camera ray of every frame hits the object (primary_misses == 0).  The
    empty scene: every pixel is L within 4 ulp."""
    packed, params, cube, want, tol = image_case(name)
    img, cnt = hg_oracle.render(packed, params, IMG_FRAMES, True, cubemap=cube)
    assert cnt["paths"] == IMG_W * IMG_H * IMG_FRAMES
    if tol is None:
        assert cnt["primary_misses"] == cnt["paths"] and cnt["hits"] == 0
    else:
        assert cnt["primary_misses"] == 0, "the object does not fill the frame"
        assert cnt["rays"] <= 2 * cnt["paths"] and cnt["hits"] == cnt["paths"], "a scattered ray hit the convex object again"
    check_image(img, name, "oracle image")


# ----------------------------------------------------------------------------------------------------------------------
# the D3D cube-face table
# ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=1)
def face_sky():
    """Face size 4, 1 mip, face f painted (f + 1, 10 (f + 1), 100 (f + 1)): a lookup names its face."""
    tex = np.zeros((6, 4, 4, 4), np.float32)
    for f in range(6):
        tex[f, :, :, :3] = (f + 1.0, 10.0 * (f + 1), 100.0 * (f + 1))
        tex[f, :, :, 3] = 1.0
    return Cubemap(4, 1, tex.reshape(-1))


@lru_cache(maxsize=1)
def face_directions():
    """600 directions well inside a face (|s|, |t| <= 0.7: bilinear taps stay on the face), any length."""
    rng = np.random.default_rng(8109)
    d = rng.normal(0, 1, (4000, 3))
    face, s, t = truth.cube_face(d)
    keep = (np.abs(s) <= 0.7) & (np.abs(t) <= 0.7)
    return f32(d[keep][:600] * 10.0 ** rng.uniform(-2, 2, (int(keep.sum()), 1))[:600])


def check_faces(rgb, what):
    face = truth.cube_face(face_directions())[0]
    want = np.stack([face + 1.0, 10.0 * (face + 1), 100.0 * (face + 1)], axis=1)
    assert np.array_equal(rgb.astype(np.float64), want), (what, np.flatnonzero((rgb != want).any(1))[:5])


def test_oracle_cube_faces(built):
    """The oracle's cubemap lookup picks the face of the D3D table (largest |component|; +X -X +Y -Y +Z -Z) for 600
    directions inside the faces; the seams and the filtering stay oracle-checked only."""
    d = face_directions()
    assert len(d) == 600 and set(truth.cube_face(d)[0].tolist()) == set(range(6))
    check_faces(np.stack([hg_oracle.cube_sample(face_sky(), v, 0) for v in d]), "oracle cube faces")
