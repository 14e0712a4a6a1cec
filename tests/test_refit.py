"""Refit of a mesh's BVH for deforming geometry, the host side (no GPU): hg_refit_blas against the builders' own boxes
and against a numpy float32 restatement of the contract (csrc/hg_refit.h); the refit plan of a packed scene and the
upload decision after a refit (csrc/hg_refit_plan.h, csrc/hg_scene_pack.h), compiled with g++ into a small driver as
tests/test_scene_pack.py does; the host sanitizer program (make asan_refit).  The entry points that need a context
(hg_refit_mesh's refusals among them) are tests/test_gpu_refit.py's."""
import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from halogen import abi, scene as hs, scenes
from halogen.unity import Transform, unity_cube, unity_plane
from host_programs import run_sanitizer_program

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "halogen-pathtracer_amd"
f32, u32 = np.float32, np.uint32
BVH_DT = np.dtype([("indexA", "<u4"), ("count", "<u4"), ("lo", "<f4", 3), ("hi", "<f4", 3)])
EPS = f32(0.00001)


# ---- the contract, restated in numpy float32 ---------------------------------------------------------------------------
def raw_box(points):
    """Per component min / max of (n, 3) float32 points with the sign of zero pinned: -0 < +0."""
    lo, hi = points.min(axis=0), points.max(axis=0)
    zero, neg = points == 0, np.signbit(points)
    lo = np.where((lo == 0) & (zero & neg).any(axis=0), f32(-0.0), np.where(lo == 0, f32(0.0), lo))
    hi = np.where((hi == 0) & (zero & ~neg).any(axis=0), f32(0.0), np.where(hi == 0, f32(-0.0), hi))
    return lo.astype(f32), hi.astype(f32)


def round_trip(lo, hi):
    extents = (hi - lo) * f32(0.5)
    center = lo + extents
    return center - extents, center + extents, extents * f32(2.0)


def stored_box(lo, hi, pad):
    mn, mx, size = round_trip(lo, hi)
    if pad and (size < EPS).any():
        mn, mx, _ = round_trip(mn, mx + EPS * f32(1.0))
    return mn, mx


def refit_numpy(tris18, bvh):
    """The contract over a BVH_DT array (root at 0) and (n, 18) float32 triangles; returns the refitted copy."""
    out = bvh.copy()
    raw = {}
    stack = [0]
    while stack:
        g = stack[-1]
        a, cnt = int(bvh["indexA"][g]), int(bvh["count"][g])
        if cnt:
            raw[g] = raw_box(tris18[a:a + cnt, :9].reshape(-1, 3))
            stack.pop()
        elif a in raw and a + 1 in raw:
            (la, ha), (lb, hb) = raw[a], raw[a + 1]
            raw[g] = raw_box(np.stack([la, ha, lb, hb]))
            stack.pop()
        else:
            stack += [a + 1, a]
    for g, (lo, hi) in raw.items():
        out["lo"][g], out["hi"][g] = stored_box(lo, hi, g != 0)
    # the root's exception: a root that already is the padded stored box of its triangles stays (a builder that pads it)
    plo, phi = stored_box(*raw[0], True)
    if bvh["lo"][0].tobytes() == plo.astype(f32).tobytes() and bvh["hi"][0].tobytes() == phi.astype(f32).tobytes():
        out["lo"][0], out["hi"][0] = plo, phi
    return out


def as_np(bvh):
    return np.frombuffer(bytes(bvh), dtype=BVH_DT).copy()


def tris_np(packed_triangles):
    return np.frombuffer(bytes(packed_triangles), dtype=f32).reshape(-1, 18).copy()


def refit_native(tris18, bvh_np):
    nodes = (abi.BVHEntry * len(bvh_np)).from_buffer_copy(bvh_np.tobytes())
    t = (abi.HalogenTriangle * len(tris18)).from_buffer_copy(np.ascontiguousarray(tris18, f32).tobytes())
    abi.refit_blas(t, nodes)
    return as_np(nodes)


def assert_same_nodes(got, want, what):
    bad = np.flatnonzero(got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1))
    assert bad.size == 0, f"{what}: {len(set(bad // 32))} of {len(got)} entries differ, first {got[bad[0] // 32]} " \
                          f"want {want[bad[0] // 32]}"


def _mesh(kind, builder):
    prev = hs.set_blas_builder(builder)
    try:
        v, n, t = {"plane": unity_plane, "cube": unity_cube, "dragon": lambda: scenes.dragon_mesh(1)}[kind]()
        return hs.RayTracingMesh(kind, v, n, t, Transform((0, 0, 0)))
    finally:
        hs.set_blas_builder(prev)


@pytest.fixture(scope="module")
def meshes():
    return {(k, b): _mesh(k, b) for k in ("plane", "cube", "dragon") for b in hs.BLAS_BUILDERS}


# ---- hg_refit_blas ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", hs.BLAS_BUILDERS)
@pytest.mark.parametrize("kind", ["cornell", "plane", "cube", "dragon"])
def test_unchanged_triangles_return_the_builders_boxes(meshes, kind, builder):
    """The contract is BVHGenerator's arithmetic: a refit of the builder's own output changes no byte of it.  (The two
    builders differ in one box: hg_build_blas_sah pads the root of a flat mesh, BVHGenerator's root is mesh.bounds; a
    root that already is the padded box of its triangles is kept, csrc/hg_refit.h.)"""
    if kind == "cornell":
        prev = hs.set_blas_builder(builder)
        try:
            todo = scenes.cornell_box().meshes
        finally:
            hs.set_blas_builder(prev)
    else:
        todo = [meshes[kind, builder]]
    for m in todo:
        want = as_np(m.bvh)
        got = refit_native(tris_np(m.packed_triangles), want)
        assert_same_nodes(got, want, f"{m.name} ({builder})")


@pytest.mark.parametrize("kind", ["cornell", "plane", "cube", "dragon"])
def test_unchanged_triangles_return_the_sequential_builders_boxes(meshes, kind):
    """The same for hg_build_blas, the sequential builder (RayTracingMesh builds with hg_build_blas_mt)."""
    from halogen.unity import mesh_bounds_min_max
    L = abi.lib()
    fp = C.POINTER(C.c_float)
    todo = scenes.cornell_box().meshes if kind == "cornell" else [meshes[kind, "reference"]]
    for m in todo:
        idx = m.triangles.copy()  # (already permuted: the build permutes it again, the mesh is the same)
        mn, mx = (np.ascontiguousarray(a, dtype=f32) for a in mesh_bounds_min_max(m.vertices))
        cap = 2 * len(idx) + 2
        nodes = (abi.BVHEntry * cap)()
        n = L.hg_build_blas(m.vertices.ctypes.data, len(m.vertices), idx.ctypes.data, len(idx), mn.ctypes.data_as(fp),
                            mx.ctypes.data_as(fp), m.max_hierarchy_depth, C.cast(nodes, C.c_void_p), cap)
        assert n > 0
        tris = (abi.HalogenTriangle * len(idx))()
        assert L.hg_pack_triangles(m.vertices.ctypes.data, m.normals.ctypes.data, len(m.vertices), idx.ctypes.data,
                                   len(idx), C.cast(tris, C.c_void_p)) == 0
        want = as_np(nodes)[:n]
        assert_same_nodes(refit_native(tris_np(tris), want), want, f"{m.name} (hg_build_blas)")


@pytest.mark.parametrize("builder", hs.BLAS_BUILDERS)
@pytest.mark.parametrize("kind", ["plane", "cube", "dragon"])
def test_random_deformations_match_the_numpy_contract(meshes, kind, builder):
    m = meshes[kind, builder]
    rng = np.random.default_rng(7)
    bvh, t = as_np(m.bvh), tris_np(m.packed_triangles)
    for scale in (1e-3, 0.3):
        d = t.copy()
        d[:, :9] += rng.normal(0, scale, d[:, :9].shape).astype(f32)
        assert_same_nodes(refit_native(d, bvh), refit_numpy(d, bvh), f"{kind} ({builder}) noise {scale}")


def test_pad_flips_both_ways(meshes):
    """A flat mesh made bumpy loses the thin-box pad, a bumpy one flattened gains it; the root never has it."""
    m = meshes["plane", "reference"]
    bvh, flat = as_np(m.bvh), tris_np(m.packed_triangles)
    rng = np.random.default_rng(3)
    bumpy = flat.copy()
    bumpy[:, 1:9:3] += rng.uniform(0.01, 1.0, (len(flat), 3)).astype(f32)
    b = refit_native(bumpy, bvh)
    assert_same_nodes(b, refit_numpy(bumpy, bvh), "flat -> bumpy")
    assert ((b["hi"][:, 1] - b["lo"][:, 1]) > 1e-3).all()
    again = refit_native(flat, b)  # from the bumpy tree back to the flat triangles
    assert_same_nodes(again, refit_numpy(flat, bvh), "bumpy -> flat")
    assert_same_nodes(again, bvh, "bumpy -> flat vs the builder")
    thick = again["hi"][:, 1] - again["lo"][:, 1]
    assert thick[0] == 0 and (thick[1:] > 0).all() and (thick[1:] < 2e-5).all()


def test_a_padded_root_is_kept_only_while_it_is_current(meshes):
    """The SAH builder pads the root of a flat mesh.  While that root is the padded box of the triangles it is kept
    (a refit of a current tree is the identity); once the triangles moved, the root is the contract's: no pad."""
    m = meshes["plane", "sah"]
    bvh, flat = as_np(m.bvh), tris_np(m.packed_triangles)
    assert bvh["hi"][0, 1] > bvh["lo"][0, 1]  # this builder padded the root
    lifted = flat.copy()
    lifted[:, 1:9:3] += f32(0.75)  # still flat, elsewhere
    got = refit_native(lifted, bvh)
    assert_same_nodes(got, refit_numpy(lifted, bvh), "lifted")
    assert got["lo"][0, 1] == got["hi"][0, 1] == f32(0.75) and (got["hi"][1:, 1] > got["lo"][1:, 1]).all()
    assert_same_nodes(refit_native(lifted, got), got, "refitting twice")


@pytest.mark.parametrize("order", ["plus_first", "minus_first"])
def test_signed_zero_extremes(order):
    """A mesh whose largest x occurs as +0.0 and as -0.0, in both orders: the twin and the restatement agree, and the
    order of the two zeros changes nothing."""
    rng = np.random.default_rng(11)
    n = 24
    v = -rng.uniform(0.1, 3.0, (3 * n, 3)).astype(f32)
    zeros = (f32(0.0), f32(-0.0)) if order == "plus_first" else (f32(-0.0), f32(0.0))
    for k in range(0, n, 2):  # pairs of neighbouring triangles touch x = 0 with either sign
        v[3 * k, 0], v[3 * (k + 1), 0] = zeros
        v[3 * k, 1:] = v[3 * (k + 1), 1:]
    t = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    m = hs.RayTracingMesh("zeros", v, np.tile(f32([0, 1, 0]), (3 * n, 1)), t, Transform((0, 0, 0)))
    bvh, tri = as_np(m.bvh), tris_np(m.packed_triangles)
    assert len(bvh) > 3 and (np.signbit(tri[:, 0:9:3][tri[:, 0:9:3] == 0])).any() and \
        (~np.signbit(tri[:, 0:9:3][tri[:, 0:9:3] == 0])).any()
    got = refit_native(tri, bvh)
    assert_same_nodes(got, refit_numpy(tri, bvh), order)
    assert_same_nodes(got, bvh, f"{order} vs the builder")
    flipped = tri.copy()
    x = flipped[:, 0:9:3]
    x[x == 0] = -x[x == 0]
    assert_same_nodes(refit_native(flipped, bvh), got, f"{order}, the zeros' signs swapped")


def test_refit_blas_writes_reachable_entries_only_and_refuses_bad_trees(meshes):
    m = meshes["cube", "reference"]
    bvh, tri = as_np(m.bvh), tris_np(m.packed_triangles)
    extra = np.concatenate([bvh, np.zeros(2, BVH_DT)])
    extra["lo"][-2:], extra["hi"][-2:] = 7.0, 9.0  # two entries no ref reaches
    moved = tri.copy()
    moved[:, :9] *= f32(1.5)
    got = refit_native(moved, extra)
    assert got[-2:].tobytes() == extra[-2:].tobytes() and got["indexA"].tolist() == extra["indexA"].tolist() and \
        got["count"].tolist() == extra["count"].tolist()

    def rc_of(nodes_np, n_tris=len(tri), null_tris=False):
        nodes = (abi.BVHEntry * len(nodes_np)).from_buffer_copy(nodes_np.tobytes())
        t = (abi.HalogenTriangle * len(tri)).from_buffer_copy(tri.tobytes())
        rc = abi.lib().hg_refit_blas(None if null_tris else C.cast(t, C.c_void_p), n_tris, C.cast(nodes, C.c_void_p),
                                     len(nodes_np))
        return rc, as_np(nodes)

    leaf = int(np.flatnonzero(bvh["count"] > 0)[0])
    inner = int(np.flatnonzero(bvh["count"] == 0)[-1])
    cases = []
    bad = bvh.copy(); bad["indexA"][leaf] = len(tri); cases.append((bad, abi.HG_E_INVALID))       # leaf out of range
    bad = bvh.copy(); bad["indexA"][inner] = len(bvh) - 1; cases.append((bad, abi.HG_E_INVALID))  # child B out of range
    bad = bvh.copy(); bad["indexA"][inner] = 0; cases.append((bad, abi.HG_E_UNSUPPORTED))         # a cycle through the root
    for nodes_np, want in cases:
        rc, after = rc_of(nodes_np)
        assert rc == want and after.tobytes() == nodes_np.tobytes()  # refused before anything is written
    assert rc_of(bvh, n_tris=len(tri) - 1)[0] == abi.HG_E_INVALID
    assert rc_of(bvh, null_tris=True)[0] == abi.HG_E_INVALID
    assert abi.lib().hg_refit_blas(None, 0, None, 0) == abi.HG_E_INVALID
    chain = np.zeros(2 * 64 + 1, BVH_DT)  # a 64-deep chain: inner entry 2k has children 2k + 1 (a leaf) and 2k + 2
    for k in range(64):
        chain[2 * k] = (2 * k + 1, 0, 0, 0)
        chain[2 * k + 1] = (0, 1, 0, 0)
    chain[128] = (0, 1, 0, 0)
    assert rc_of(chain)[0] == abi.HG_E_UNSUPPORTED
    with pytest.raises(abi.HalogenError) as e:
        abi.refit_blas((abi.HalogenTriangle * 1)(), (abi.BVHEntry * 1)(abi.BVHEntry(5, 1)))
    assert e.value.rc == abi.HG_E_INVALID


def test_deform_keeps_pack_current(meshes):
    """RayTracingMesh.deform: packed_triangles follow the permuted index list, bvh is the host refit, the cache token
    stays and the deform serial advances."""
    v, n, t = scenes.dragon_mesh(1)
    m = hs.RayTracingMesh("d", v, n, t, Transform((0, 0, 0)))
    token, topo = m.cache_token, as_np(m.bvh)[["indexA", "count"]].copy()
    ang = v[:, 1:2] * f32(0.8)
    twisted = np.concatenate([v[:, 0:1] * np.cos(ang) - v[:, 2:3] * np.sin(ang), v[:, 1:2],
                              v[:, 0:1] * np.sin(ang) + v[:, 2:3] * np.cos(ang)], axis=1).astype(f32)
    m.deform(twisted)
    assert m.cache_token == token and m.deform_serial == 1
    tri = tris_np(m.packed_triangles)
    assert np.array_equal(tri[:, :9].reshape(-1, 3, 3), twisted[m.triangles])
    after = as_np(m.bvh)
    assert np.array_equal(after[["indexA", "count"]], topo)
    assert_same_nodes(after, refit_numpy(tri, after), "deform")
    with pytest.raises(ValueError):
        m.deform(twisted[:-1])


# ---- the plan and the upload decision: csrc/hg_refit_plan.h, csrc/hg_scene_pack.h under g++ ------------------------------
DRIVER = r"""
#include "scene_pack_check.h"
// plan <scene>: packs the scene, plans every mesh's tree and checks the plans against a walk of the records
// decide <retained> <incoming> <stale> <last_gen> <gen>: hg_upload_decide_refit with <retained> as the last upload
static int plan(const char* path) {
    HgSceneFile f;
    if (!f.read(path)) return 2;
    HgScenePack p;
    HgPackError err;
    const HgSceneIn in = f.in();
    if (hg_pack_spheres_materials(in, p, err) || hg_pack_geometry(in, p, err)) { std::printf("rejected %s\n", err.text.c_str()); return 0; }
    HgPackStats st;
    const std::string s = hg_check_pack(in, p, st);
    if (!s.empty()) { std::printf("badpack %s\n", s.c_str()); return 0; }
    const size_t n_rec = p.rec.size() / 4;
    std::vector<uint32_t> refs(2 * n_rec), leaves(2 * p.leaf.size());
    for (size_t r = 0; r < n_rec; ++r) {
        std::memcpy(&refs[2 * r], &p.rec[4 * r].w, 4);
        std::memcpy(&refs[2 * r + 1], &p.rec[4 * r + 1].w, 4);
    }
    std::memcpy(leaves.data(), p.leaf.data(), leaves.size() * 4);
    std::vector<int> seen(n_rec, 0);
    std::vector<uint32_t> height(n_rec, 0);
    size_t planned = 0, levels = 0, strict = 0;
    for (size_t mi = 0; mi < p.dm.size(); ++mi) {
        bool first = true;  // instances share a tree: plan it once
        for (size_t mj = 0; mj < mi; ++mj) first = first && p.dm[mj].root_ref != p.dm[mi].root_ref;
        HgRefitPlan pl;
        if (!hg_refit_plan(refs.data(), n_rec, leaves.data(), p.leaf.size(), p.dm[mi].root_ref, p.dm[mi].tri_offset, pl)) {
            std::printf("noplan mesh %zu\n", mi);
            return 0;
        }
        std::printf("mesh %zu records=%zu levels=%zu extent=%u min=%u span=%u\n", mi, pl.records.size(),
                    pl.level_off.empty() ? size_t(0) : pl.level_off.size() - 1, pl.extent, pl.rec_min, pl.rec_span);
        if (!first) continue;
        levels = std::max(levels, pl.level_off.empty() ? size_t(0) : pl.level_off.size() - 1);
        for (size_t h = 1; h < pl.level_off.size(); ++h)
            for (uint32_t i = pl.level_off[h - 1]; i < pl.level_off[h]; ++i) {
                const uint32_t r = pl.records[i];
                if (r < pl.rec_min || r - pl.rec_min >= pl.rec_span) { std::printf("span\n"); return 0; }
                seen[r]++;
                height[r] = uint32_t(h);
                planned++;
            }
        for (uint32_t r : pl.records) {
            uint32_t top = 0;
            for (int k = 0; k < 2; ++k) {
                const uint32_t c = refs[2 * size_t(r) + k];
                if (c & HG_LEAF_BIT) continue;
                if (height[c] == 0 || height[c] >= height[r]) { std::printf("height of %u under %u\n", c, r); return 0; }
                top = std::max(top, height[c]);
                strict++;
            }
            if (height[r] != top + 1) { std::printf("height of %u is not 1 + its children's\n", r); return 0; }
        }
    }
    size_t once = 0, pads = 0;
    const float4 z[4] = {f4(0, 0, 0, 0), f4(0, 0, 0, 0), f4(0, 0, 0, 0), f4(0, 0, 0, 0)};
    for (size_t r = 0; r < n_rec; ++r) {
        const bool pad = !std::memcmp(&p.rec[4 * r], z, sizeof z);
        if (seen[r] > 1 || (seen[r] == 1) == pad) { std::printf("record %zu seen %d pad %d\n", r, seen[r], int(pad)); return 0; }
        once += seen[r];
        pads += pad;
    }
    std::printf("ok planned=%zu once=%zu inner=%zu pads=%zu stat_pads=%zu levels=%zu inner_children=%zu\n", planned, once,
                st.inner, pads, st.pads + (st.inner == 0 ? 1 : 0), levels, strict);
    return 0;
}

static int decide(char** a) {
    HgSceneFile last, next;
    if (!last.read(a[0]) || !next.read(a[1])) return 2;
    const HgSceneIn li = last.in();
    std::vector<uint8_t> copy[5];
    for (int k = 0; k < 5; ++k) copy_bytes(copy[k], li.src(k), li.bytes(k));
    const HgUploadDecision d = hg_upload_decide_refit(true, std::atoi(a[2]) != 0, copy, std::strtoull(a[3], nullptr, 10),
                                                      size_t(li.n_meshes), li.n_tris, li.n_nodes, next.in(),
                                                      std::strtoull(a[4], nullptr, 10));
    const char* kind[3] = {"skip", "partial", "full"};
    std::printf("%s vouched=%d\n", kind[d.kind], int(d.vouched));
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "plan")) return plan(argv[2]);
    if (argc == 7 && !std::strcmp(argv[1], "decide")) return decide(argv + 2);
    return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("refit")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                    f"-I{PKG / 'csrc'}", f"-I{PKG / 'host'}", str(d / "driver.cpp"), "-o", str(exe), "-lpthread"],
                   check=True)

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.returncode, r.stdout, r.stderr)
        return r.stdout.strip().splitlines()

    run.dir = d
    return run


_files = [0]


def write_scene(run, packed) -> Path:
    _files[0] += 1
    path = run.dir / f"scene{_files[0]}.bin"
    arrays = [packed.spheres, packed.meshes, packed.materials, packed.triangles, packed.blas]
    path.write_bytes(struct.pack("<5i", *map(len, arrays)) + b"".join(bytes(a) for a in arrays))
    return path


def _copy(packed):
    out = {}
    for k in ("spheres", "meshes", "materials", "triangles", "blas"):
        a = getattr(packed, k)
        b = (type(a)._type_ * len(a))()
        C.memmove(b, a, C.sizeof(a))
        out[k] = b
    return hs.PackedScene(**out)


def hazard_scene():
    """The synthetic scene of tests/test_gpu_refit.py: a leaf root, a 40-triangle leaf beside spread triangles, a flat
    10 x 10 plane, two instances of one 500-triangle tree at a non-zero triangle offset."""
    import refit_cases
    return refit_cases.hazard_packed(refit_cases.hazard_scene())


def test_plan_covers_every_record_once(driver):
    import cases
    for name, packed in (("hazards", hazard_scene()), ("cornell", cases._scene("cornell", 10)),
                         ("dragon1", cases._scene("dragon", 1))):
        out = driver("plan", write_scene(driver, packed))
        assert out[-1].startswith("ok "), (name, out)
        v = dict(kv.split("=") for kv in out[-1].split()[1:])
        assert v["planned"] == v["once"] == v["inner"] and v["pads"] == v["stat_pads"], (name, out[-1])
        assert int(v["levels"]) >= 1 and int(v["inner_children"]) > 0, (name, out[-1])
        if name == "hazards":
            assert int(v["pads"]) >= 1, "the hazard scene must hold a pad record"
            per_mesh = [dict(kv.split("=") for kv in line.split()[2:]) for line in out[:-1]]
            assert per_mesh[0]["records"] == "0" and per_mesh[0]["extent"] == "3"      # the leaf root
            assert per_mesh[3] == per_mesh[4] and per_mesh[3]["extent"] == "500"       # the two instances


def test_upload_decision_after_a_refit(driver):
    """After a refit the retained triangles and BVH entries are stale: only a vouched upload may skip or be partial."""
    import cases
    base = cases._scene("cornell", 10)
    a = write_scene(driver, base)
    moved = _copy(base)
    moved.meshes[0].worldToLocal.m[12] += 0.05
    deformed = _copy(base)  # the caller's arrays after a deformation: other triangles and boxes, same sizes
    deformed.triangles[0].pointA.x += 0.25
    deformed.blas[1].boundingCornerB.x += 0.25
    deformed_moved = _copy(deformed)
    deformed_moved.meshes[0].worldToLocal.m[12] += 0.05
    fewer = _copy(base)
    fewer.triangles = (abi.HalogenTriangle * (len(base.triangles) - 1))(*list(base.triangles)[:-1])
    more_nodes = _copy(base)
    more_nodes.blas = (abi.BVHEntry * (len(base.blas) + 1))(*list(base.blas), abi.BVHEntry())
    offset = _copy(base)
    offset.meshes[1].triangleBufferOffset += 1
    acc = _copy(base)
    acc.meshes[1].accelerationBufferOffset += 1
    table = [
        # incoming, stale, last_gen, gen -> kind, vouched
        (deformed, 1, 5, 5, "skip", 1),             # vouched, small tables unchanged
        (deformed_moved, 1, 5, 5, "partial", 1),    # vouched, an object moved
        (base, 1, 5, 5, "skip", 1),                 # vouched is trusted: the geometry is not looked at
        (base, 1, 5, 6, "full", 0),                 # unvouched: another generation, even with the retained arrays
        (deformed, 1, 5, 6, "full", 0),
        (moved, 1, 5, 6, "full", 0),
        (base, 1, 5, 0, "full", 0),                 # generation 0 never vouches
        (base, 1, 0, 0, "full", 0),
        (deformed_moved, 1, 0, 0, "full", 0),
        (fewer, 1, 5, 5, "full", 0),                # size changed under the refit's generation
        (more_nodes, 1, 5, 5, "full", 0),
        (offset, 1, 5, 5, "full", 0),               # an offset changed
        (acc, 1, 5, 5, "full", 0),
        # not stale: hg_upload_decide's rows are unchanged
        (base, 0, 5, 6, "skip", 0),
        (base, 0, 5, 5, "skip", 1),
        (moved, 0, 5, 6, "partial", 0),
        (deformed, 0, 5, 6, "full", 0),
        (deformed, 0, 5, 5, "skip", 1),
    ]
    for incoming, stale, last_gen, gen, kind, vouched in table:
        out = driver("decide", a, write_scene(driver, incoming), stale, last_gen, gen)[-1]
        assert out == f"{kind} vouched={vouched}", (stale, last_gen, gen, out, kind)
        if stale and not vouched:
            assert out.startswith("full")  # no row skips or goes partial unvouched after a refit


def test_asan_refit_program():
    """host/asan_refit.cpp under AddressSanitizer + UBSan: hg_refit_blas, the plan and the decision on adversarial
    input (make asan_refit; a stand-alone program, host code only)."""
    assert "asan_refit ok" in run_sanitizer_program("asan_refit")
