"""The host side of recomputed vertex normals: hg_vertex_normals (the twin of a deform with HG_DEFORM_NORMALS,
csrc/hg_normals.h) against a numpy restatement of the contract, bit for bit; that the order of the triangles does not
matter; refusals; RayTracingMesh.deform / pose with normals="recompute"; the constants the Python layer mirrors; the host
sanitizer program (make asan_normals).  The entry points that need a context are tests/test_gpu_normals.py's."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import deform_cases as dc
import normals_cases as nc
import refit_cases
from halogen import abi
from host_programs import run_sanitizer_program

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


def grid():
    m = refit_cases.hazard_scene().meshes[3]
    return m.vertices.copy(), m.triangles.copy()


def twin_cases():
    out = {}
    for m in refit_cases.hazard_scene().meshes:
        out[m.name] = (m.vertices.copy(), m.triangles.copy())
    out["fan of 300"] = nc.fan()
    gv, gi = grid()
    # unreferenced vertices: one in the middle (its triangles renamed to a neighbour), two appended, one of them the last
    idx = gi.copy()
    idx[idx == 140] = 141
    out["unreferenced vertices"] = (np.concatenate([gv, f32([[1, 2, 3], [4, 5, 6]])]), idx)
    idx = gi.copy()
    idx[7] = idx[7][0]
    out["one vertex three times"] = (gv, idx)
    idx = gi.copy()
    idx[3] = (0, 0, 1)                      # two corners on one vertex
    idx[10] = idx[11] = idx[499] = idx[12]  # one triangle four times, apart in the list
    idx[20] = (5, 6, 7)
    v = gv.copy()
    v[5:8] = [[0, 0.125, 1.0], [0, 0.25, 1.25], [0, 0.375, 1.5]]  # ... collinear, exactly
    out["collinear and duplicated"] = (v, idx)
    out["grid * 1e-3"] = ((gv * f32(1e-3)).astype(f32), gi)
    out["grid * 1e3"] = ((gv * f32(1e3)).astype(f32), gi)
    out["grid + 1e6"] = ((gv + f32(1e6)).astype(f32), gi)
    return out


CASES = twin_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_vertex_normals_equals_the_numpy_contract_bit_for_bit(built, name):
    v, idx = CASES[name]
    got = abi.vertex_normals(v, idx)
    want = nc.normals_numpy(v, idx)
    assert got.shape == v.shape and got.dtype == f32 and np.isfinite(got).all()
    bad = np.argwhere(nc.bits(got) != nc.bits(want))
    assert bad.size == 0, (name, len(bad), bad[:4], got[bad[0][0]], want[bad[0][0]])
    val = nc.valences(idx, len(v))
    assert not got[val == 0].any(), "an unreferenced vertex has the normal (0, 0, 0)"
    lengths = np.linalg.norm(got.astype(np.float64), axis=1)
    assert (np.abs(lengths[lengths > 0] - 1) < 4 * 2.0 ** -23).all()
    if name == "fan of 300":
        assert len(v) == 301 and val[0] == 300 and got[0, 1] > 0.9
    if name == "unreferenced vertices":
        assert list(np.flatnonzero(val == 0)) == [140, len(v) - 2, len(v) - 1]
    if name == "collinear and duplicated":
        e1, e2 = v[6] - v[5], v[7] - v[5]
        assert not np.cross(e1.astype(np.float64), e2.astype(np.float64)).any()


def test_vertex_normals_do_not_depend_on_the_order_of_the_triangles(built):
    for name in ("grid", "cluster", "fan of 300", "collinear and duplicated"):
        v, idx = CASES[name]
        first = abi.vertex_normals(v, idx)
        for seed in range(4):
            perm = np.random.default_rng(seed).permutation(len(idx))
            assert np.array_equal(nc.bits(abi.vertex_normals(v, idx[perm])), nc.bits(first)), (name, seed)
    # ... while a sum in list order would: the restatement without its sort differs on some permutation of the fan
    v, idx = CASES["fan of 300"]
    f = np.cross(v[idx[:, 1]] - v[idx[:, 0]], v[idx[:, 2]] - v[idx[:, 0]]).astype(f32)
    sums = set()
    for seed in range(4):
        s = f32([0, 0, 0])
        for t in np.random.default_rng(seed).permutation(len(idx)):
            s = s + f[t]
        sums.add(s.tobytes())
    assert len(sums) > 1, "the fan's sum is sensitive to its order, so the test above can fail"


def test_flat_plane_normals_are_exactly_the_axis(built):
    """The hazard scene's plane lies in XZ (halogen.unity.unity_plane: normal +Y), so the components that are exactly 0
    on it are x and z, and y > 0; the same plane turned into XY (a cyclic permutation of the coordinates, which is a
    rotation) has x and y exactly 0 and z > 0."""
    v, idx = CASES["plane"]
    assert nc.valences(idx, len(v)).min() > 0 and not v[:, 1].any()
    n = abi.vertex_normals(v, idx)
    assert (nc.bits(n[:, 0]) == 0).all() and (nc.bits(n[:, 2]) == 0).all() and (n[:, 1] > 0).all()
    n = abi.vertex_normals(np.roll(v, 1, axis=1), idx)
    assert (nc.bits(n[:, 0]) == 0).all() and (nc.bits(n[:, 1]) == 0).all() and (n[:, 2] > 0).all()
    assert np.abs(n[:, 2] - 1).max() <= 2.0 ** -23


def test_vertex_normals_refusals_write_nothing(built):
    v, idx = grid()
    L = abi.lib()
    out = np.full_like(v, 7)
    good = [v.ctypes.data, len(v), idx.ctypes.data, len(idx), out.ctypes.data]

    def call(**changed):
        a = list(good)
        for k, x in changed.items():
            a[int(k[1:])] = x
        return L.hg_vertex_normals(*a)

    assert call(a0=None) == abi.HG_E_INVALID and call(a2=None) == abi.HG_E_INVALID and call(a4=None) == abi.HG_E_INVALID
    assert call(a1=0) == abi.HG_E_INVALID and call(a1=-1) == abi.HG_E_INVALID
    assert call(a3=0) == abi.HG_E_INVALID and call(a3=-1) == abi.HG_E_INVALID
    assert call(a1=len(v) - 1) == abi.HG_E_INVALID, "the last vertex is named: an index outside [0, n_vertices)"
    for wrong in (len(v), -1, 2 ** 31 - 1, -2 ** 31):
        bad = idx.copy()
        bad[321, 2] = wrong
        assert call(a2=bad.ctypes.data) == abi.HG_E_INVALID, wrong
    assert (out == 7).all(), "nothing is written on a refusal"
    assert call() == abi.HG_OK and not (out == 7).any()
    for args in ((v[:0], idx), (v, idx[:0])):
        with pytest.raises(abi.HalogenError) as e:
            abi.vertex_normals(*args)
        assert e.value.rc == abi.HG_E_INVALID


def packed_of(mesh, v, n):
    out = (abi.HalogenTriangle * len(mesh.triangles))()
    rc = abi.lib().hg_pack_triangles(v.ctypes.data, n.ctypes.data, len(v), mesh.triangles.ctypes.data, len(mesh.triangles),
                                     C.cast(out, C.c_void_p))
    assert rc == 0
    return out


def test_deform_recompute_keeps_the_host_arrays_current(built):
    """deform(v, normals="recompute") = deform(v, the twin's normals): triangles and boxes byte for byte (so
    hg_refit_blas has run), also after an SAH rebuild has permuted the list, and through pose()"""
    a = refit_cases.hazard_scene().meshes[3]
    b = refit_cases.hazard_scene().meshes[3]
    rest = a.vertices.copy()
    assert not a.normals_recomputed
    v = refit_cases.twist(rest, 0.9, axis=0)
    a.deform(v, normals="recompute")
    n = abi.vertex_normals(v, a.triangles)
    assert a.normals_recomputed and np.array_equal(nc.bits(a.normals), nc.bits(n)) and not np.array_equal(n, b.normals)
    assert bytes(a.packed_triangles) == bytes(packed_of(a, v, n))
    b.deform(v, n)
    assert bytes(a.packed_triangles) == bytes(b.packed_triangles) and bytes(a.bvh) == bytes(b.bvh)
    before = a.triangles.copy()
    v = refit_cases.twist(rest, 0.5)
    a.deform(v, normals="recompute", rebuild="sah")
    assert not np.array_equal(a.triangles, before) and a.rebuild_serial == 1
    n = abi.vertex_normals(v, before)  # (the list in either order: the same normals)
    assert np.array_equal(nc.bits(a.normals), nc.bits(n))
    b.deform(v, n, rebuild="sah")
    assert bytes(a.packed_triangles) == bytes(b.packed_triangles) and bytes(a.bvh) == bytes(b.bvh)
    v = refit_cases.noise(rest, 0.05, seed=3)
    a.deform(v, normals="recompute")  # a second recompute, over the permuted list
    n = abi.vertex_normals(v, before)
    assert bytes(a.packed_triangles) == bytes(packed_of(a, v, n))
    b.deform(v, n)
    assert bytes(a.packed_triangles) == bytes(b.packed_triangles) and bytes(a.bvh) == bytes(b.bvh)
    a.deform(rest)
    assert not a.normals_recomputed and a.deform_serial == 4
    with pytest.raises(ValueError):
        a.deform(rest, normals="smooth")
    # pose: the skinned positions, the recomputed normals
    idx, w = dc.influences(len(rest), 3, seed=2)
    a.set_skin(idx, w)
    bones = dc.rigid_palette(3, seed=4)
    bones[1] = dc.bone(dc.rotation([1, 0, 1], 0.3), (0.1, 0, 0), (1.0, 2.5, 0.5))  # scaled non-uniformly
    rest_v, rest_n = a.vertices.copy(), a.normals.copy()
    a.pose(bones, normals="recompute")
    sv, sn = abi.skin_vertices(rest_v, rest_n, idx, w, bones)
    n = abi.vertex_normals(sv, a.triangles)
    assert a.normals_recomputed and np.array_equal(a.vertices, sv) and np.array_equal(nc.bits(a.normals), nc.bits(n))
    assert not np.array_equal(n, sn)
    with pytest.raises(ValueError):
        a.pose(bones, normals="smooth")


def test_python_constants_match_the_sources(built):
    header = (ROOT / "include" / "halogen_abi.h").read_text()
    assert int(re.search(r"\bHG_DEFORM_NORMALS = (0x[0-9a-fA-F]+)", header).group(1), 16) == abi.HG_DEFORM_NORMALS == 0x100
    assert int(re.search(r"\bHG_BIND_ADJACENCY = (\d+)", header).group(1)) == abi.HG_BIND_ADJACENCY == 1
    assert not abi.HG_DEFORM_NORMALS & max(abi.DEFORM_KINDS.values())
    cs = (ROOT / "bindings" / "csharp" / "HalogenNative.cs").read_text()
    assert "HG_DEFORM_NORMALS = 0x100" in cs and "HG_BIND_ADJACENCY = 1" in cs
    assert "hg_set_mesh_vertices_opt" in cs and "hg_vertex_normals" in cs


def test_asan_normals_program():
    """host/asan_normals.cpp under AddressSanitizer + UBSan: the adjacency builder, the shared arithmetic and
    hg_vertex_normals on random and adversarial lists (make asan_normals; a stand-alone program, host code only)."""
    assert "asan_normals ok" in run_sanitizer_program("asan_normals")
