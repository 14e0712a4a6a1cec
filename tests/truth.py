"""Float64 references written from the mathematics, in numpy only (no oracle, no halogen.abi): what tests/test_truth.py
holds the CPU oracle against and tests/test_gpu_truth.py the kernels.

Every function takes the float32 inputs the code under test was given (converted to float64, exactly) and answers in
float64.  Where the reference (HC = Assets/Scripts/Halogen Shaders/HalgoenCompute.compute, HR = HalogenRandom.hlsl)
deliberately departs from the textbook, the function follows the reference's text and says so with the line:

  * a triangle hit needs |det| >= 1e-8, 0 <= U <= 1, V >= 0, U + V <= 1, t > 0 (HC:321-345), then t > 1e-4 and
    t < closest (HC:416); a mesh hit replaces the sphere pass's only below closest - 1e-4 (HC:452);
  * `front` is sign(det) with det = dot(cross(d, v0v2), v0v1) = n . (-d), n = v0v1 x v0v2 (HC:317-318, 350), taken on
    the mesh-LOCAL ray: under a mirroring instance the world-space winding has the other sign;
  * a sphere's root is the near one, or the far one when the near one is negative ("from inside, the far root",
    HC:284-292), with a = 1 whatever |d| is (HC:272), accepted when 1e-4 < t < closest (HC:369);
  * the box test returns tMin, which is negative from inside, and hits only when tMax > max(0, tMin) (HC:258): a box
    that is flat along an axis is never hit;
  * a mesh normal is the interpolated vertex normal times the orientation, carried to world space as the ROW vector
    times worldToLocal, i.e. by the inverse transpose of localToWorld, then normalised (HC:463-467): the textbook rule,
    also under non-uniform and mirroring scales;
  * lambertain_scatter falls back to the normal when |n + rv| < 1e-8 (HC:494), and the next ray starts at
    pos + normal * 1e-4 (HC:710);
  * float(u32) / 4294967296.0f rounds the top 128 values up to exactly 1.0f (HR:258).
"""
import numpy as np

F64 = np.float64
EPS32 = 2.0 ** -24  # half a float32 unit in the last place of 1: the unit roundoff
HIT_EPS = F64(np.float32(0.0001))  # hitDistanceEpsilon as the float32 the shader holds
DET_EPS = F64(np.float32(0.00000001))


def f64(x):
    return np.asarray(x, dtype=F64)


def norm(v):
    return np.sqrt((f64(v) ** 2).sum(-1))


def unit(v):
    v = f64(v)
    return v / norm(v)[..., None]


def dot(a, b):
    return (f64(a) * f64(b)).sum(-1)


def ulp32(x):
    """The float32 unit in the last place at magnitude |x| (float64 in, float64 out; the smallest normal's below it)."""
    x = np.maximum(np.abs(f64(x)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23)


# ----------------------------------------------------------------------------------------------------------------------
# ray - triangle: the 3 x 3 linear system  o + t d = v0 + u e1 + v e2
# ----------------------------------------------------------------------------------------------------------------------
def tri_solve(o, d, v0, e1, e2):
    """Elementwise (n, 3) inputs -> (t, u, v, det): the solution of [-d e1 e2] (t, u, v)^T = o - v0 by numpy's LU solve,
    and det = n . (-d) with n = e1 x e2 (the reference's determinant, HC:317-318).  A singular system gives NaN."""
    o, d, v0, e1, e2 = (f64(a) for a in (o, d, v0, e1, e2))
    M = np.stack([-d, e1, e2], axis=-1)
    det = -dot(np.cross(e1, e2), d)
    ok = np.abs(np.linalg.det(M)) > 0
    M = np.where(ok[:, None, None], M, np.eye(3))
    x = np.linalg.solve(M, (o - v0)[..., None])[..., 0]
    x = np.where(ok[:, None], x, np.nan)
    return x[:, 0], x[:, 1], x[:, 2], det


def tri_conditioning(o, d, v0, e1, e2):
    """(c, s, mag0): c = |n^ . d|, s = |e1 x e2| / (|e1| |e2|), and the magnitudes |o| + |v0| of the residual bound."""
    n = np.cross(f64(e1), f64(e2))
    ln = norm(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.abs(dot(n, d)) / (ln * norm(d))
        s = ln / (norm(e1) * norm(e2))
    return c, s, norm(o) + norm(v0)


def tri_bound(K, o, d, v0, e1, e2, t, u, v):
    """K 2^-24 mag / (c s), mag = |o| + |v0| + |t| + |u| |e1| + |v| |e2|: the bound on the residual
    |o + t d - v0 - u e1 - v e2| of a float32 solution (t, u, v)."""
    c, s, mag0 = tri_conditioning(o, d, v0, e1, e2)
    mag = mag0 + np.abs(t) * norm(d) + np.abs(u) * norm(e1) + np.abs(v) * norm(e2)
    with np.errstate(invalid="ignore", divide="ignore"):
        return K * EPS32 * mag / (c * s)


def tri_residual(o, d, v0, e1, e2, t, u, v):
    o, d, v0, e1, e2, t, u, v = (f64(a) for a in (o, d, v0, e1, e2, t, u, v))
    return norm(o + t[:, None] * d - v0 - u[:, None] * e1 - v[:, None] * e2)


def tri_decide(K, o, d, v0, e1, e2, best_t):
    """The float64 decision of the mesh loop's accept rule for one triangle per ray.

    Returns (accept, front, decided, t, u, v).  decided: the float64 (t, u, v, 1 - u - v, det) clear every acceptance
    threshold (det against +-1e-8, u and v against 0, u against 1, u + v against 1, t against 0, 1e-4, best_t and best_t -
    1e-4) by more than the float32 solution's margin, on either side: delta = tri_bound in t, delta / (|e| s) in the
    barycentrics, K 2^-24 |d| |e1| |e2| in det."""
    t, u, v, det = tri_solve(o, d, v0, e1, e2)
    best_t = f64(best_t)
    c, s, _ = tri_conditioning(o, d, v0, e1, e2)
    delta = tri_bound(K, o, d, v0, e1, e2, t, u, v)
    l1, l2 = norm(e1), norm(e2)
    with np.errstate(invalid="ignore", divide="ignore"):
        du, dv = delta / (l1 * s), delta / (l2 * s)
        ddet = K * EPS32 * norm(d) * l1 * l2
        det_in = np.abs(det) >= DET_EPS
        inside = (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1)
        accept = det_in & inside & (t > 0) & (t > HIT_EPS) & (t < best_t)
        clear_det = np.abs(np.abs(det) - DET_EPS) > ddet
        clear_uv = (np.abs(u) > du) & (np.abs(u - 1) > du) & (np.abs(v) > dv) & (np.abs(u + v - 1) > du + dv)
        clear_t = (np.abs(t) > delta) & (np.abs(t - HIT_EPS) > delta)
        fin = np.isfinite(best_t)
        clear_t &= ~fin | ((np.abs(t - best_t) > delta) & (np.abs(t - (best_t - HIT_EPS)) > delta))
        # a rejection that is itself clear decides the element whatever the later thresholds say: a clearly parallel
        # ray, a clearly outside point, a hit clearly behind the origin or clearly beyond best_t
        sure_out = clear_det & ((~det_in) | (u < -du) | (u > 1 + du) | (v < -dv) | (u + v > 1 + du + dv)
                                | (t < HIT_EPS - delta) | (fin & (t > best_t + delta)))
        decided = np.isfinite(delta) & ((clear_det & clear_uv & clear_t) | sure_out)
    return accept, det > 0, decided, t, u, v


# ----------------------------------------------------------------------------------------------------------------------
# ray - box: slab intervals
# ----------------------------------------------------------------------------------------------------------------------
def box_slabs(A, B, o, inv):
    """(hit, entry, exit): per axis the interval between (A - o) inv and (B - o) inv, inv = 1 / d as given (+-inf for a
    zero component: the slab is everything or nothing); entry the largest lower end, exit the smallest upper end; a hit
    when exit > max(0, entry), and the value returned on a hit is entry (HC:244-259).  A 0 * inf is NaN (no element of
    the tests has one)."""
    A, B, o, inv = (f64(a) for a in (A, B, o, inv))
    with np.errstate(invalid="ignore", over="ignore"):
        t1, t2 = (A - o) * inv, (B - o) * inv
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    entry, exit_ = lo.max(-1), hi.min(-1)
    return exit_ > np.maximum(0.0, entry), entry, exit_


# ----------------------------------------------------------------------------------------------------------------------
# ray - sphere: the quadratic with a = 1
# ----------------------------------------------------------------------------------------------------------------------
def sphere_roots(o, d, c, r):
    """(t, back, disc, miss): t^2 + b t + cq = 0 with b = 2 (o - c) . d, cq = |o - c|^2 - r^2 (a = 1, HC:272); t the near
    root, or the far one (back = True) when the near one is negative; NaN when disc < 0.  miss: the distance of the
    ray's line from the centre."""
    o, d, c, r = (f64(a) for a in (o, d, c, r))
    sh = o - c
    b = 2.0 * dot(sh, d)
    cq = dot(sh, sh) - r * r
    disc = b * b - 4.0 * cq
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
        near, far = (-b - sq) / 2.0, (-b + sq) / 2.0
    back = near < 0
    du = unit(d)
    miss = norm(sh - dot(sh, du)[:, None] * du)
    return np.where(back, far, near), back, disc, miss


def sphere_bound(K, o, d, c, r, t):
    """K 2^-24 (|o - c| + |t| + r) / sqrt(1 - (b / r)^2), b the miss distance: the bound on | |o + t d - c| - r |."""
    _, _, _, miss = sphere_roots(o, d, c, r)
    with np.errstate(invalid="ignore", divide="ignore"):
        return K * EPS32 * (norm(f64(o) - f64(c)) + np.abs(f64(t)) + f64(r)) / np.sqrt(1.0 - (miss / f64(r)) ** 2)


def sphere_residual(o, d, c, r, t):
    return np.abs(norm(f64(o) + f64(t)[:, None] * f64(d) - f64(c)) - f64(r))


# ----------------------------------------------------------------------------------------------------------------------
# closest hit over every triangle and sphere, no hierarchy
# ----------------------------------------------------------------------------------------------------------------------
def brute_force_closest(o, d, v0, e1, e2, slack=1e-3, chunk=256):
    """For rays (R, 3) against triangles (T, 3): per ray the two smallest accepted t and their triangles, and the
    winner's (u, v, det).  The system of tri_solve by Cramer's rule, written as matrix products over (ray, triangle):
    det = -d . n, t = (o - v0) . n / det, u = (e2 . (o x d) - d . (e2 x v0)) / det, v = (-e1 . (o x d) - d . (v0 x e1)) /
    det.  Accepted: |det| >= 1e-8, 0 <= u <= 1, v >= 0, u + v <= 1, t > 1e-4 (HC:321-345, 416).  Returns a dict of (R,)
    arrays: t1, i1, u, v, det, t2 (inf / -1 where there is none), and hit_loose / hit_tight: whether any triangle grown /
    shrunk by `slack` in its barycentrics is hit (where the two differ, a hit or miss hangs on an edge)."""
    o, d, v0, e1, e2 = (f64(a) for a in (o, d, v0, e1, e2))
    n = np.cross(e1, e2)
    v0n = dot(v0, n)
    e2xv0, v0xe1 = np.cross(e2, v0), np.cross(v0, e1)
    R = len(o)
    out = {k: np.full(R, np.inf) for k in ("t1", "t2")}
    out.update({k: np.full(R, np.nan) for k in ("u", "v", "det")})
    out["i1"] = np.full(R, -1, np.int64)
    out["hit_loose"], out["hit_tight"] = np.zeros(R, bool), np.zeros(R, bool)
    for at in range(0, R, chunk):
        oo, dd = o[at:at + chunk], d[at:at + chunk]
        oxd = np.cross(oo, dd)
        det = -(dd @ n.T)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = (oo @ n.T - v0n[None, :]) / det
            u = (oxd @ e2.T - dd @ e2xv0.T) / det
            v = (-(oxd @ e1.T) - dd @ v0xe1.T) / det
        ok = (np.abs(det) >= DET_EPS) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t > HIT_EPS)
        k = len(oo)
        front_of = (np.abs(det) >= DET_EPS) & (t > HIT_EPS)
        for name, g in (("hit_loose", -slack), ("hit_tight", slack)):
            out[name][at:at + k] = (front_of & (u >= g) & (v >= g) & (u + v <= 1 - g)).any(1)
        t = np.where(ok, t, np.inf)
        rows = np.arange(k)
        i1 = t.argmin(1)
        t1 = t[rows, i1]
        hit = np.isfinite(t1)
        out["t1"][at:at + k] = t1
        out["i1"][at:at + k] = np.where(hit, i1, -1)
        for name, a in (("u", u), ("v", v), ("det", det)):
            out[name][at:at + k] = np.where(hit, a[rows, i1], np.nan)
        t[rows, i1] = np.inf
        out["t2"][at:at + k] = t.min(1)
    return out


def world_triangles(v0, v1, v2, local_to_world):
    """Float32 local vertices through the float64 4 x 4 localToWorld (row r, column c): (v0, e1, e2) in world space."""
    M = f64(local_to_world)
    w = [f64(p) @ M[:3, :3].T + M[:3, 3] for p in (v0, v1, v2)]
    return w[0], w[1] - w[0], w[2] - w[0]


def world_normal(n0, n1, n2, u, v, orientation, world_to_local):
    """normalize(mul(float4(n, 0), worldToLocal).xyz) with n = (n0 + (n1 - n0) u + (n2 - n0) v) * orientation: the row
    vector times the matrix, i.e. worldToLocal^T n (HC:463-467)."""
    n = f64(n0) + (f64(n1) - f64(n0)) * f64(u)[:, None] + (f64(n2) - f64(n0)) * f64(v)[:, None]
    n = n * f64(orientation)[:, None]
    W = f64(world_to_local)[..., :3, :3]
    return unit(np.einsum("...j,...jk->...k", n, W))


# ----------------------------------------------------------------------------------------------------------------------
# the sampler as a net: exact integer checks
# ----------------------------------------------------------------------------------------------------------------------
def strata_violations_u32(x, m):
    """x: (2^m,) uint32 points.  The number of intervals [k, k + 1) 2^-m that do not hold exactly one point."""
    k = np.asarray(x, np.uint64) >> np.uint64(32 - m)
    return int((np.bincount(k.astype(np.int64), minlength=1 << m) != 1).sum())


def net_violations_u32(xy, m):
    """xy: (2^m, 2) uint32 points.  Over a = 0 .. m, the number of elementary boxes 2^-a x 2^-(m - a) that do not hold
    exactly one point: 0 for a (0, m, 2)-net."""
    x, y = np.asarray(xy[:, 0], np.uint64), np.asarray(xy[:, 1], np.uint64)
    bad = 0
    for a in range(m + 1):
        kx = (x >> np.uint64(32 - a)) if a else np.zeros_like(x)
        ky = (y >> np.uint64(32 - (m - a))) if m - a else np.zeros_like(y)
        box = (kx << np.uint64(m - a)) | ky
        bad += int((np.bincount(box.astype(np.int64), minlength=1 << m) != 1).sum())
    return bad


def _cells(f, bits):
    """Float32 samples f in [0, 1] against the grid k / 2^bits, exactly (f 2^bits is exact in float64): the cell floor(f
    2^bits), and whether f sits exactly on a grid line k > 0.  Such a value is what float(u32) / 2^32 gives for the u32
    values just below the line as well (HR:258 rounds to 24 bits; 1.0f is the line 2^bits): its cell is k - 1 or k."""
    if bits == 0:  # one cell: [0, 1] with its end
        return np.zeros(len(f), np.int64), np.zeros(len(f), bool)
    s = f64(f) * float(1 << bits)
    k = np.floor(s)
    return k.astype(np.int64), (s == k) & (k > 0)


def net_violations_float(xy, m):
    """net_violations_u32 for the float32 samples of the same points ((2^m, 1) for the 1-D check: only a = m is then
    counted).  Points on no grid line must sit in distinct boxes; every point on a grid line must have an otherwise
    empty box among the two (four) it may have come from, and there must be as many such points as empty boxes.
    Returns (violations, points on grid lines)."""
    xy = np.asarray(xy, np.float32).reshape(len(xy), -1)
    one_d = xy.shape[1] == 1
    bad = amb_total = 0
    for a in ([m] if one_d else range(m + 1)):
        kx, ax = _cells(xy[:, 0], a)
        ky, ay = _cells(xy[:, 1], m - a) if not one_d else (np.zeros(len(xy), np.int64), np.zeros(len(xy), bool))
        amb = ax | ay
        amb_total += int(amb.sum())
        sure = ~amb
        inside = (kx < (1 << a)) & (ky < (1 << (m - a)))
        bad += int((sure & ~inside).sum())
        count = np.bincount(((kx << (m - a)) | ky)[sure & inside], minlength=1 << m)
        bad += int((count > 1).sum())
        empty = count == 0
        if int(empty.sum()) != int(amb.sum()):
            bad += 1
        for i in np.flatnonzero(amb):
            cand = [(x, y) for x in ((kx[i] - 1, kx[i]) if ax[i] else (kx[i],)) for y in ((ky[i] - 1, ky[i]) if ay[i] else (ky[i],))
                    if 0 <= x < (1 << a) and 0 <= y < (1 << (m - a))]
            bad += 0 if any(empty[(x << (m - a)) | y] for x, y in cand) else 1
    return bad, amb_total


def cell_counts(x, y, bits=2):
    """Samples x, y in [0, 1] (float): the counts of the 2^bits x 2^bits equal cells of the unit square."""
    n = 1 << bits
    kx = np.minimum((f64(x) * n).astype(np.int64), n - 1)
    ky = np.minimum((f64(y) * n).astype(np.int64), n - 1)
    return np.bincount(kx * n + ky, minlength=n * n)


def independent_cell_bound(n_points, bits=2, sigmas=6.0):
    """(lo, hi) for a cell's count under independent uniform samples: the binomial mean -+ 6 standard deviations."""
    p = 1.0 / (1 << (2 * bits))
    sd = np.sqrt(n_points * p * (1 - p))
    return n_points * p - sigmas * sd, n_points * p + sigmas * sd


# ----------------------------------------------------------------------------------------------------------------------
# optics
# ----------------------------------------------------------------------------------------------------------------------
def snell(i, n, n1, n2):
    """(sin theta1, (n1 / n2) sin theta1, cos theta1) for incident i onto the normal n (facing the ray: cos = -i . n)."""
    i, n = unit(i), unit(n)
    cos1 = -dot(i, n)
    sin1 = norm(np.cross(i, n))
    return sin1, f64(n1) / f64(n2) * sin1, cos1


def schlick(n1, n2, n, i, lo, hi):
    """Schlick's approximation as the reference adjusts it (HC:519-540): R0 = ((n1 - n2) / (n1 + n2))^2; from the denser
    side the cosine of the TRANSMITTED angle is used and beyond the critical angle the answer is `hi`; the result
    interpolates lo .. hi.  Returns (value, sinT2) with sinT2 = (n1 / n2)^2 sin^2 theta1 (0 where n1 <= n2)."""
    n1, n2, lo, hi = (f64(a) for a in (n1, n2, lo, hi))
    r0 = ((n1 - n2) / (n1 + n2)) ** 2
    cos_x = -dot(n, i)
    dense = n1 > n2
    sin_t2 = np.where(dense, (n1 / n2) ** 2 * (1.0 - cos_x * cos_x), 0.0)
    with np.errstate(invalid="ignore"):
        cos_x = np.where(dense, np.sqrt(np.maximum(1.0 - sin_t2, 0.0)), cos_x)
    ret = r0 + (1.0 - r0) * (1.0 - cos_x) ** 5
    return np.where(sin_t2 > 1.0, hi, lo + ret * (hi - lo)), sin_t2


def hemisphere_moments(d, n):
    """Moments of unit directions d about the normal n, in an orthonormal frame (x, y, n): E[cos], E[cos^2], E[x], E[y],
    E[x^2], E[y^2].  A cosine-weighted hemisphere has 2/3, 1/2, 0, 0, 1/4, 1/4."""
    d, n = f64(d), unit(f64(n))
    a = np.eye(3)[np.argmin(np.abs(n))]
    x = unit(np.cross(n, a))
    y = np.cross(n, x)
    c, px, py = d @ n, d @ x, d @ y
    return np.array([c.mean(), (c * c).mean(), px.mean(), py.mean(), (px * px).mean(), (py * py).mean()])


COSINE_MOMENTS = np.array([2.0 / 3.0, 0.5, 0.0, 0.0, 0.25, 0.25])


# ----------------------------------------------------------------------------------------------------------------------
# the D3D cube-face table
# ----------------------------------------------------------------------------------------------------------------------
def cube_face(d):
    """Direction -> (face, s, t): the face of the largest |component| (+X -X +Y -Y +Z -Z = 0 .. 5) and the D3D face
    coordinates in [-1, 1] (sc / |ma|, tc / |ma|): +X (-z, -y), -X (z, -y), +Y (x, z), -Y (x, -z), +Z (x, -y), -Z (-x,
    -y)."""
    d = f64(d)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax = np.argmax(np.abs(d), axis=-1)
    neg = np.take_along_axis(d, ax[..., None], -1)[..., 0] < 0
    face = 2 * ax + neg
    ma = np.abs(np.take_along_axis(d, ax[..., None], -1)[..., 0])
    sc = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)
    tc = np.select([face == 2, face == 3], [z, -z], -y)
    return face, sc / ma, tc / ma


# ----------------------------------------------------------------------------------------------------------------------
# closed-form images
# ----------------------------------------------------------------------------------------------------------------------
def closed_form_pixel(E, L, albedo):
    """A convex diffuse emitter (emission E, albedo rho) under a constant sky L, every path hit - scatter - sky, Russian
    roulette surviving with probability max(rho) and rescaling by 1 / max(rho) (HC:929-935): E + rho L per channel."""
    return f64(E) + f64(albedo) * f64(L)


def closed_form_tolerance(E, L, N):
    """2 L / N for the roulette's stratified count (|m - rho_max N| <= 2 over frames 1 .. N) plus N 2^-24 (E + L) for the
    progressive blend's roundings."""
    return 2.0 * L / N + N * EPS32 * (E + L)
