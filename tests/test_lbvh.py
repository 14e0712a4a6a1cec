"""hg_build_blas_lbvh, the host twin of the device rebuild, against an independent numpy restatement of the contract
in csrc/hg_lbvh.h (key points, grid, Morton codes, the stable order, leaves of L, Karras' radix tree by the textbook
binary searches) and csrc/hg_refit.h (the boxes, tests/test_refit.py's restatement); what the pipeline makes of the
result (hg_refit_blas, hg_pack_geometry through tests/test_scene_pack.py's driver); the edge inputs, each with an
assertion that the input is the edge it claims to be; the host sanitizer program (make asan_lbvh).  The device build is
tests/test_gpu_rebuild.py's."""
import ctypes as C

import numpy as np
import pytest

import lbvh_cases
from halogen import abi
from halogen.scene import PackedScene
from host_programs import run_sanitizer_program
from test_refit import BVH_DT, as_np, assert_same_nodes, refit_native, refit_numpy, tris_np
from test_scene_pack import driver, mesh as mesh_record, parse, write_scene  # noqa: F401 (driver: a fixture)

f32, u32 = np.float32, np.uint32
LEAF_SIZES = (1, 4, 15)


# ---- the contract, restated -------------------------------------------------------------------------------------------------
def key_points(t18):
    corners = t18[:, :9].reshape(-1, 3, 3)
    with np.errstate(over="ignore"):
        return (corners.min(axis=1) + corners.max(axis=1)).astype(f32)


def cells(p):
    """(n, 3) uint32 cells, and the unclamped products (for the tests that look at the clamp)."""
    pmin, pmax = p.min(axis=0), p.max(axis=0)
    with np.errstate(all="ignore"):
        ext = (pmax - pmin).astype(f32)
        ok = np.isfinite(ext) & (ext > 0)
        scale = (f32(1024.0) / ext).astype(f32)
        raw = ((p - pmin).astype(f32) * scale).astype(f32)
        v = np.where(np.isnan(raw), f32(1023.0), np.minimum(raw, f32(1023.0)))
        return np.where(ok, v, f32(0.0)).astype(u32), np.where(ok, raw, f32(0.0)), ext


def morton(cell):
    code = np.zeros(len(cell), u32)
    for b in range(10):
        for axis in range(3):
            code |= ((cell[:, axis] >> u32(b)) & u32(1)) << u32(3 * b + 2 - axis)
    return code


def clz32(x):
    return 32 - int(x).bit_length()


def karras(keys):
    """Children of every internal node of the K keys: [(('leaf' | 'node', index), (..., index))], Karras 2012 fig. 4."""
    K = len(keys)
    keys = [int(k) for k in keys]

    def delta(i, j):
        if j < 0 or j >= K:
            return -1
        return clz32(keys[i] ^ keys[j]) if keys[i] != keys[j] else 32 + clz32(i ^ j)

    out = []
    for i in range(K - 1):
        d = 1 if delta(i, i + 1) > delta(i, i - 1) else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        l, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (l + t) * d) > dmin:
                l += t
            t //= 2
        j = i + l * d
        dnode = delta(i, j)
        s, t = 0, l
        while True:
            t = (t + 1) // 2
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t == 1:
                break
        g = i + s * d + min(d, 0)
        out.append((("leaf" if min(i, j) == g else "node", g), ("leaf" if max(i, j) == g + 1 else "node", g + 1)))
    return out


def lbvh_numpy(t18, L):
    """order, sorted codes and the BVH_DT tree of the contract."""
    n = len(t18)
    cell, _, _ = cells(key_points(t18))
    code = morton(cell)
    order = np.argsort(code, kind="stable").astype(np.int32)
    sorted_codes = code[order]
    K = (n + L - 1) // L
    nodes = np.zeros(2 * K - 1, BVH_DT)

    def put(entry, child):
        kind, j = child
        if kind == "leaf":
            nodes["indexA"][entry], nodes["count"][entry] = j * L, min(L, n - j * L)
        else:
            nodes["indexA"][entry], nodes["count"][entry] = 1 + 2 * j, 0

    put(0, ("leaf", 0) if K == 1 else ("node", 0))
    for i, (a, b) in enumerate(karras(sorted_codes[::L])):
        put(1 + 2 * i, a)
        put(2 + 2 * i, b)
    return order, sorted_codes, refit_numpy(t18[order], nodes)


def depth_and_leaves(nodes):
    """The deepest entry's depth and the (first, count) of every leaf, by a walk from the root."""
    deepest, leaves, seen, stack = 0, [], set(), [(0, 0)]
    while stack:
        g, d = stack.pop()
        assert g not in seen and d <= 62, (g, d)
        seen.add(g)
        deepest = max(deepest, d)
        a, cnt = int(nodes["indexA"][g]), int(nodes["count"][g])
        if cnt:
            leaves.append((a, cnt))
        else:
            stack += [(a + 1, d + 1), (a, d + 1)]
    assert len(seen) == len(nodes), "every entry is reached"
    return deepest, leaves


def check(tris, L, what):
    """Everything that holds for every input: the twin equals the restatement, the partition, the depth bound, the
    identity under hg_refit_blas.  Returns (order, sorted codes, native nodes, depth)."""
    t18 = tris_np(tris)
    n = len(t18)
    order, out, nodes = abi.build_blas_lbvh(tris, L)
    got = as_np(nodes)
    want_order, codes, want = lbvh_numpy(t18, L)
    assert np.array_equal(order, want_order), what
    assert tris_np(out).tobytes() == t18[want_order].tobytes(), what
    assert_same_nodes(got, want, what)
    K = (n + L - 1) // L
    assert len(got) == 2 * K - 1, what
    depth, leaves = depth_and_leaves(got)
    leaves.sort()
    assert [a for a, _ in leaves] == [j * L for j in range(K)], what       # every triangle in exactly one leaf
    assert all(c == L for _, c in leaves[:-1]) and leaves[-1][1] == n - (K - 1) * L, what
    assert sorted(order.tolist()) == list(range(n)), what
    assert depth <= 30 + (K - 1).bit_length(), (what, depth, K)
    assert_same_nodes(refit_native(tris_np(out), got), got, what + ": hg_refit_blas is the identity")
    return order, codes, got, depth


# ---- meshes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LEAF_SIZES)
@pytest.mark.parametrize("kind", ["plane", "cube", "dragon"])
def test_twin_equals_the_restatement(kind, L):
    tris = lbvh_cases.mesh_triangles(kind)
    assert len(tris) == {"plane": 200, "cube": 12, "dragon": 8712}[kind]
    _, codes, _, _ = check(tris, L, f"{kind} L={L}")
    if kind == "dragon":
        assert len(np.unique(codes)) > 1000  # a grid that resolves the mesh, not a handful of cells


@pytest.mark.parametrize("L", LEAF_SIZES)
@pytest.mark.parametrize("kind", ["plane", "cube", "dragon"])
def test_upload_validation_accepts_the_tree(driver, kind, L):
    """hg_pack_geometry (hg_upload_scene's validation and layout) takes the twin's arrays as they are."""
    tris = lbvh_cases.mesh_triangles(kind)
    _, out, nodes = abi.build_blas_lbvh(tris, L)
    packed = PackedScene(spheres=(abi.HalogenSphere * 0)(), meshes=(abi.HalogenMeshData * 1)(mesh_record(0, 0)),
                         materials=(abi.PackedHalogenMaterial * 1)(), triangles=out, blas=nodes)
    r = parse(driver("pack", write_scene(driver, packed)))
    K = (len(tris) + L - 1) // L
    depth, _ = depth_and_leaves(as_np(nodes))
    assert r["walk"] == "ok" and int(r["inner"]) == K - 1 and int(r["inline"]) == K and int(r["table"]) == 0, r
    assert int(r["max_depth"]) == depth, (r, depth)


def test_refusals():
    tris = lbvh_cases.mesh_triangles("cube")
    L = abi.lib()
    order = np.zeros(12, np.int32)
    out, nodes = (abi.HalogenTriangle * 12)(), (abi.BVHEntry * 23)()
    p = lambda a: C.cast(a, C.c_void_p)  # noqa: E731
    call = lambda n, leaf, cap: L.hg_build_blas_lbvh(p(tris), n, leaf, order.ctypes.data, p(out), p(nodes), cap)  # noqa: E731
    assert call(12, 1, 23) == 23
    assert call(12, 1, 22) == -24  # the count, negated minus one
    assert call(0, 1, 23) == abi.HG_E_INVALID and call(12, 0, 23) == abi.HG_E_INVALID
    assert call(12, 16, 23) == abi.HG_E_INVALID and call(-1, 4, 23) == abi.HG_E_INVALID
    assert L.hg_build_blas_lbvh(None, 12, 4, order.ctypes.data, p(out), p(nodes), 23) == abi.HG_E_INVALID


# ---- edge inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LEAF_SIZES)
def test_smallest_counts(L):
    for n in sorted({1, 2, L, L + 1}):
        tris = lbvh_cases.random_triangles(n, seed=n)
        _, _, got, depth = check(tris, L, f"n={n} L={L}")
        K = (n + L - 1) // L
        assert len(got) == 2 * K - 1
        if n <= L:  # one leaf: the root is that leaf, no internal node
            assert K == 1 and (got["indexA"][0], got["count"][0]) == (0, n) and depth == 0
        else:
            assert got["count"][0] == 0 and got["indexA"][0] == 1 and depth >= 1
    n = L + 1
    assert (n + L - 1) // L == 2  # L + 1 triangles: two leaves, the last one short (or both of one triangle at L = 1)


@pytest.mark.parametrize("L", LEAF_SIZES)
def test_all_triangles_identical(L):
    """Every key ties: the tree is the index-balanced one (delta = 32 + clz(i ^ j)), whose depth is bits(K - 1)."""
    n = 100
    tris = lbvh_cases.identical_triangles(n)
    order, codes, got, depth = check(tris, L, f"identical L={L}")
    assert len(np.unique(codes)) == 1, "every key must tie"
    assert np.array_equal(order, np.arange(n)), "ties keep the caller's order"
    K = (n + L - 1) // L
    assert depth == (K - 1).bit_length() and (K == 1 or depth >= 3), (depth, K)
    if K > 1:  # the root splits the index range at its highest differing bit
        first_right = 1 << ((K - 1).bit_length() - 1)
        _, leaves = depth_and_leaves(got)
        # child A of the root covers leaves [0, first_right): walk it
        sub = got.copy()
        a = int(got["indexA"][0])
        stack, firsts = [a], []
        while stack:
            g = stack.pop()
            if sub["count"][g]:
                firsts.append(int(sub["indexA"][g]) // L)
            else:
                stack += [int(sub["indexA"][g]), int(sub["indexA"][g]) + 1]
        assert sorted(firsts) == list(range(first_right)), (sorted(firsts), first_right)


@pytest.mark.parametrize("flat_axes", [(1,), (0, 2), (0, 1, 2)], ids=["one_axis", "two_axes", "three_axes"])
def test_flat_meshes(flat_axes):
    tris = lbvh_cases.flat_triangles(60, flat_axes)
    p = key_points(tris_np(tris))
    cell, _, ext = cells(p)
    for axis in range(3):
        if axis in flat_axes:
            assert ext[axis] == 0 and not cell[:, axis].any(), "a flat axis: extent zero, every cell 0"
        else:
            assert ext[axis] > 0 and len(np.unique(cell[:, axis])) > 10
    for L in LEAF_SIZES:
        _, codes, _, _ = check(tris, L, f"flat {flat_axes} L={L}")
        if len(flat_axes) == 3:
            assert not codes.any()


@pytest.mark.parametrize("what", ["tiny", "huge", "denormal", "overflow"])
def test_extreme_extents(what):
    tris = lbvh_cases.extreme_triangles(what)
    p = key_points(tris_np(tris))
    cell, raw, ext = cells(p)
    tiny = np.finfo(f32).tiny
    if what == "tiny":
        assert (ext > tiny).all() and (ext < 1e-29).all() and len(np.unique(morton(cell))) > 20
    elif what == "huge":
        assert (ext > 1e29).all() and np.isfinite(ext).all() and len(np.unique(morton(cell))) > 20
    elif what == "denormal":
        # the scale is +Inf on every axis: a positive difference gives +Inf, the point at pmin gives 0 * Inf = NaN; both
        # end in cell 1023
        assert (ext > 0).all() and (ext < tiny).all()
        assert np.isnan(raw).any() and np.isinf(raw).any() and (cell == 1023).all()
    else:
        assert np.isinf(p).any() and not np.isfinite(ext).any() and not cell.any()  # sums that overflowed: cell 0
    for L in LEAF_SIZES:
        check(tris, L, f"{what} L={L}")


def test_key_points_one_ulp_apart():
    tris = lbvh_cases.ulp_triangles()
    p = key_points(tris_np(tris))
    a, b = p[3, 0], p[4, 0]
    assert a != b and np.nextafter(a, f32(np.inf)) == b, "the two key points differ by one ulp in x"
    assert np.array_equal(p[3, 1:], p[4, 1:])
    for L in LEAF_SIZES:
        check(tris, L, f"ulp L={L}")


def test_key_point_at_pmax_is_cell_1023():
    tris = lbvh_cases.random_triangles(50, seed=9)
    p = key_points(tris_np(tris))
    cell, raw, _ = cells(p)
    for axis in range(3):
        top = int(np.argmax(p[:, axis]))
        assert raw[top, axis] >= 1024.0, "unclamped, the point at pmax would land in cell 1024"
        assert cell[top, axis] == 1023 and cell[:, axis].max() == 1023
    for L in LEAF_SIZES:
        check(tris, L, f"pmax L={L}")


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------
def test_asan_lbvh_program():
    """host/asan_lbvh.cpp under AddressSanitizer + UBSan: hg_build_blas_lbvh on the input classes above (make
    asan_lbvh; a stand-alone program, host code only)."""
    assert "asan_lbvh ok" in run_sanitizer_program("asan_lbvh")
