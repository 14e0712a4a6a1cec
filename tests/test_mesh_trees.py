"""The host bookkeeping of the mesh updates (refit, rebuild, deform, skin), csrc/hg_mesh_trees.h, with no GPU: compiled
with g++ into a small driver as tests/test_refit.py and tests/test_scene_pack.py do.  The driver packs a scene, resets
the bookkeeping from the pack and applies the operations given on its command line as the device path applies them
(hg_refit.hip update_mesh), the host twins hg_build_blas_lbvh / hg_build_blas_lbvh_sah standing in for the device build
(host/mesh_trees_check.h has the checks it makes after every adopted rebuild).  One line per operation:
    ok refit ... | ok rebuild records=.. leaves=.. rec_min=.. capacity=.. depth=.. root_leaf=.. | refused <code> <text> | bad <what>
followed by same=1 if the bookkeeping and the mesh table compare equal to what they were before the operation.

"ok rebuild" means that HgTreesHarness::rebuild (host/mesh_trees_check.h, shared with host/asan_mesh_trees.cpp) found,
after adopt(), all of: every instance of the tree carries the new root, which is the slot's first record, or one inline
leaf for no records; the slot recorded for the tree is the one the check handed out (a rebuild does not change it); the
plan lies under the tree's new key, its extent is the triangle count, it plans exactly the twin's records and every one
of them inside the slot; the walk of rec_refs from the new root meets the twin's entries one for one, the same leaves
in the same order, covering every triangle once; the returned stack depth is hg_pack_geometry's for the scene with the
twin's triangles and entries in the mesh's place.  Anything else is a "bad" line, which no test below accepts.  The
expected texts are the entry points' own (tests/test_gpu_refit.py, test_gpu_rebuild.py, test_gpu_rebuild_sah.py and
test_gpu_deform.py assert them on the device)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import refit_cases
from halogen import abi, scene as hs, scenes
from halogen.unity import Transform
from host_programs import run_sanitizer_program
from test_refit import write_scene

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "halogen-pathtracer_amd"

DRIVER = r"""
#include "scene_pack_check.h"
#include "mesh_trees_check.h"
// <scene> <op>...: refit:M:N[:null] lbvh:M:N:LEAF[:null] sah:M:N:COST[:null] cycle:M range:M noscene upload
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    HgSceneFile f;
    if (!f.read(argv[1])) return 2;
    HgTreesHarness h;
    h.spheres = f.spheres; h.meshes = f.meshes; h.materials = f.materials; h.tris = f.tris; h.blas = f.blas;
    const std::string up = h.upload();
    if (!up.empty()) { std::printf("rejected %s\n", up.c_str()); return 0; }
    for (const HgDevMesh& m : h.dm) (void)h.trees.plan_of(m);  // every plan cached: a refusal then changes nothing
    for (int a = 2; a < argc; ++a) {
        std::vector<std::string> w(1);
        for (const char* p = argv[a]; *p; ++p) { if (*p == ':') w.emplace_back(); else w.back() += *p; }
        w.resize(5);
        const HgTreesHarness::Snapshot before = h.snapshot();
        const int32_t mesh = std::atoi(w[1].c_str()), n = std::atoi(w[2].c_str());
        std::string out;
        if (w[0] == "noscene") { h.has_scene = false; out = "ok noscene"; }
        else if (w[0] == "upload") {  // a full upload of the caller's arrays as they are now
            const std::string again = h.upload();
            for (const HgDevMesh& m : h.dm) (void)h.trees.plan_of(m);
            out = again.empty() ? "ok upload" : "bad " + again;
        }
        else if (w[0] == "refit") out = h.refit(mesh, w[3] != "null", n);
        else if (w[0] == "lbvh") out = h.rebuild(mesh, w[4] != "null", n, HG_DEFORM_REBUILD, std::atoi(w[3].c_str()), 0.0f);
        else if (w[0] == "sah") out = h.rebuild(mesh, w[4] != "null", n, HG_DEFORM_REBUILD_SAH, 0, std::strtof(w[3].c_str(), nullptr));
        else if (w[0] == "cycle" || w[0] == "range") out = h.adopt_bad(mesh, w[0]);
        else return 2;
        std::printf("%s same=%d\n", out.c_str(), int(h.same_as(before)));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("mesh_trees")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", f"-I{ROOT / 'include'}",
                    f"-I{PKG / 'csrc'}", f"-I{PKG / 'host'}", str(d / "driver.cpp"),
                    *map(str, sorted((PKG / "csrc").glob("hg_host_*.cpp"))), "-o", str(exe), "-lpthread"], check=True)

    def run(*args):
        r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.returncode, r.stdout, r.stderr)
        return r.stdout.strip().splitlines()

    run.dir = d
    return run


def counts(packed):
    """Triangles per mesh record: to the next larger offset, or the scene's end"""
    offs = [m.triangleBufferOffset for m in packed.meshes]
    return [min([o for o in offs if o > s] + [len(packed.triangles)]) - s for s in offs]


def roomy(mesh):
    """tests/test_gpu_rebuild_sah.py's: the mesh under the L = 1 radix tree of its triangles, n - 1 inner entries"""
    order, mesh.packed_triangles, mesh.bvh = abi.build_blas_lbvh(mesh.packed_triangles, 1)
    mesh.triangles = np.ascontiguousarray(mesh.triangles[order])
    mesh.bvh_inner = len(order) - 1
    return mesh


@pytest.fixture(scope="module")
def files(driver):
    """The scene files, written once: the hazard scene as built, with roomy trees for meshes 1 and the grid, with a
    17-triangle single-leaf mesh added; the cornell box"""
    out = {"hazard": write_scene(driver, refit_cases.hazard_packed(refit_cases.hazard_scene()))}
    sc = refit_cases.hazard_scene()
    roomy(sc.meshes[1])
    roomy(sc.meshes[3])
    out["roomy"] = write_scene(driver, refit_cases.hazard_packed(sc))
    sc = refit_cases.hazard_scene()
    rng = np.random.default_rng(17)
    soup = rng.uniform(-0.2, 0.2, (17, 3, 3)) + rng.uniform(-2, 2, (17, 1, 3))
    leaf17 = hs.RayTracingMesh("leaf17", *refit_cases._soup(soup), Transform((2.0, 0.5, 4.0)))
    leaf17.bvh = (abi.BVHEntry * 1)(abi.BVHEntry(0, 17))
    abi.refit_blas(leaf17.packed_triangles, leaf17.bvh)
    leaf17.bvh_inner = 0
    sc.add(leaf17)
    out["leaf17"] = write_scene(driver, refit_cases.hazard_packed(sc))
    cornell = scenes.cornell_box().pack()
    out["cornell"] = write_scene(driver, cornell)
    out["cornell_counts"] = counts(cornell)
    out["cornell_packed"] = cornell
    return out


def fields(line):
    return {k: v for k, v in (kv.split("=") for kv in line.split() if "=" in kv)}


def rebuilt(line):
    assert line.startswith("ok rebuild "), line
    return {k: int(v) for k, v in fields(line).items()}


GRID, TWIN = 3, 4  # the hazard scene's grid of 500 triangles and its second instance
E = {k: getattr(abi, k) for k in ("HG_E_INVALID", "HG_E_UNSUPPORTED", "HG_E_NOSCENE")}


def refused(line, code, text):
    assert line == f"refused {E[code]} {text} same=1", line


# ---- sequences: every adopted rebuild passes the harness's checks (walk = the twin's tree, extent, records inside the
# slot, both instances' root, the slot kept, a full upload's stack depth) ---------------------------------------------------
def test_sah_then_lbvh4_then_refit(driver, files):
    """The sequence the order-tracking GPU test was reshaped around: a rebuild by surface area, a linear BVH at leaf size
    4, a refit.  The device keeps the slot of the first upload (the grid: 143 records, mesh 1: 16), so on the hazard
    scene's own trees it takes the sequence for the grid (124 records) and refuses leaf size 4 for mesh 1 (24 against
    16).  What that test met is the caller's side, which it compares the device against: RayTracingMesh.deform plays a
    full upload of its own arrays, and an upload lays the records out for the tree it is given, so after the rebuild by
    surface area the capacity is that tree's span (include/halogen_abi.h).  With that upload in between the bookkeeping
    refuses as the twin does.  Under the leaf-size-1 upload that tests/test_gpu_deform.py uses, all three steps pass on
    both meshes, the refit through the second instance."""
    out = driver(files["hazard"], f"sah:{GRID}:500:0", f"lbvh:{GRID}:500:4", f"refit:{TWIN}:500", "sah:1:100:0",
                 "lbvh:1:100:4", "refit:1:100")
    a, b = rebuilt(out[0]), rebuilt(out[1])
    assert (a["rec_min"], a["capacity"]) == (b["rec_min"], b["capacity"]) == (64, 143)
    assert a["records"] <= 143 and (b["records"], b["leaves"]) == (124, 125)
    assert out[2] == "ok refit instances=2 extent=500 same=1"
    assert rebuilt(out[3])["capacity"] == 16
    refused(out[4], "HG_E_UNSUPPORTED", "hg_rebuild_mesh: mesh 1: 24 records at leaf size 4, the tree's capacity is 16")
    assert out[5] == "ok refit instances=1 extent=100 same=1"
    for mesh, n, need in ((GRID, 500, 124), (1, 100, 24)):
        out = driver(files["hazard"], f"sah:{mesh}:{n}:0", "upload", f"lbvh:{mesh}:{n}:4", f"lbvh:{mesh}:{n}:15")
        kept = rebuilt(out[0])["records"]
        assert out[1] == "ok upload same=0"
        m = re.fullmatch(rf"refused {E['HG_E_UNSUPPORTED']} hg_rebuild_mesh: mesh {mesh}: {need} records at leaf size 4, the "
                         r"tree's capacity is (\d+) same=1", out[2])
        assert m and kept <= int(m.group(1)) < need, out[2]  # (the span: the records and the pads between sibling pairs)
        assert rebuilt(out[3])["capacity"] == int(m.group(1))
    out = driver(files["roomy"], f"sah:{GRID}:500:0.5", f"lbvh:{GRID}:500:4", f"refit:{TWIN}:500", "sah:1:100:0.5",
                 "lbvh:1:100:4", "refit:1:100")
    a, b = rebuilt(out[0]), rebuilt(out[1])
    assert a["capacity"] == b["capacity"] >= 499 and a["rec_min"] == b["rec_min"] and 143 < a["records"] <= 499
    assert b["records"] == 124 and b["leaves"] == 125 and out[2] == "ok refit instances=2 extent=500 same=1"
    assert rebuilt(out[3])["capacity"] >= 99 and 16 < rebuilt(out[3])["records"] <= 99 and rebuilt(out[4])["records"] == 24
    assert out[5] == "ok refit instances=1 extent=100 same=1"


def test_lbvh_sah_lbvh_within_the_first_uploads_capacity(driver, files):
    out = driver(files["hazard"], f"lbvh:{GRID}:500:0", f"sah:{TWIN}:500:0", f"lbvh:{GRID}:500:15", f"refit:{TWIN}:500",
                 "lbvh:1:100:0", "sah:1:100:0", "lbvh:1:100:9", "lbvh:2:200:0", "sah:2:200:0")
    steps = [rebuilt(line) for line in out[:3]]
    assert {(s["rec_min"], s["capacity"]) for s in steps} == {(64, 143)}
    assert steps[0]["records"] == 124 and steps[0]["leaves"] == 125  # leaf size 4 fits the 143 records
    assert steps[1]["records"] <= 143 and steps[2]["records"] == 33
    assert out[3] == "ok refit instances=2 extent=500 same=1"
    for line in out[4:]:
        assert rebuilt(line)["records"] <= rebuilt(line)["capacity"]
    # mesh 1's 16 records: leaf size 6 is the smallest from 4 that fits (K - 1 = 16)
    assert rebuilt(out[4])["records"] == 16 and rebuilt(out[6])["records"] == 11


def test_rebuild_to_no_records_and_back(driver, files):
    """Cornell's mesh 7 (a cube, 12 triangles, one record): one leaf of 12 needs no record and the root becomes an inline
    leaf; leaf size 6 then needs the record again, from the slot the first upload gave"""
    assert files["cornell_counts"][7] == 12
    out = driver(files["cornell"], "lbvh:7:12:15", "refit:7:12", "lbvh:7:12:6", "refit:7:12", "sah:7:12:0", "lbvh:7:12:6",
                 "sah:7:12:0.01", "refit:7:12")
    zero, one = rebuilt(out[0]), rebuilt(out[2])
    assert zero["records"] == 0 and zero["root_leaf"] == 1 and zero["capacity"] == 1
    assert one["records"] == 1 and one["root_leaf"] == 0 and (one["rec_min"], one["capacity"]) == (zero["rec_min"], 1)
    assert out[1] == out[3] == out[7] == "ok refit instances=1 extent=12 same=1"
    assert rebuilt(out[4])["root_leaf"] == 1 and rebuilt(out[5])["records"] == 1
    refused(out[6], "HG_E_UNSUPPORTED", "hg_rebuild_mesh_sah: mesh 7: 5 records at node cost 0.01, the tree's capacity is 1")
    # the hazard scene's leaf root (3 triangles, no slot): a rebuild keeps it a leaf
    out = driver(files["hazard"], "lbvh:0:3:0", "sah:0:3:0", "refit:0:3")
    assert rebuilt(out[0])["capacity"] == 0 and rebuilt(out[1])["root_leaf"] == 1 and out[2].startswith("ok refit")


# ---- refusals: code, full text, nothing changed --------------------------------------------------------------------------------
def test_refusals_of_every_kind(driver, files):
    cn = files["cornell_counts"]
    packed = files["cornell_packed"]
    n, n_meshes = cn[7], len(packed.meshes)
    cap = rebuilt(driver(files["cornell"], f"lbvh:7:{n}:15")[0])["capacity"]
    assert n - 1 > cap
    kinds = ["refit:{m}:{n}", "lbvh:{m}:{n}:4", "sah:{m}:{n}:0"]
    ops, want = [], []

    def add(op, code, text):
        ops.append(op)
        want.append((code, text))

    for op in kinds:
        for index in (-1, 99, n_meshes):
            add(op.format(m=index, n=n), "HG_E_INVALID", f"hg_refit_mesh: mesh_index {index} out of range ({n_meshes} meshes)")
        add(op.format(m=7, n=n) + ":null", "HG_E_INVALID", "hg_refit_mesh: null triangle array")
        add(op.format(m=7, n=-1), "HG_E_INVALID", "hg_refit_mesh: negative triangle count")
        add(op.format(m=7, n=n - 1), "HG_E_INVALID", f"hg_refit_mesh: mesh 7: {n - 1} triangles, its tree's leaves reach {n}")
        toff = packed.meshes[8].triangleBufferOffset
        add(op.format(m=8, n=cn[8] + 1), "HG_E_INVALID",
            f"hg_refit_mesh: mesh 8: triangles {toff} + {cn[8] + 1} past the scene's {len(packed.triangles)}")
        add(op.format(m=6, n=cn[6] + 1), "HG_E_UNSUPPORTED",
            "hg_refit_mesh: mesh 6 shares triangles with mesh 7, which has another tree")
    for leaf in (16, -1):
        add(f"lbvh:7:{n}:{leaf}", "HG_E_INVALID", f"hg_rebuild_mesh: leaf_size {leaf} outside 0..15")
    add(f"lbvh:7:{n}:1", "HG_E_UNSUPPORTED",
        f"hg_rebuild_mesh: mesh 7: {n - 1} records at leaf size 1, the tree's capacity is {cap}")
    add("lbvh:7:0:4", "HG_E_INVALID", f"hg_refit_mesh: mesh 7: 0 triangles, its tree's leaves reach {n}")
    for cost, shown in (("-1", "-1"), ("nan", "nan"), ("inf", "inf"), ("-0.5", "-0.5")):
        add(f"sah:7:{n}:{cost}", "HG_E_INVALID", f"hg_rebuild_mesh_sah: node_cost {shown} is negative or not finite")
    # precedence: the refit's checks, then the kind's own argument, then the count against the tree
    add(f"lbvh:7:{n - 1}:16", "HG_E_INVALID", f"hg_refit_mesh: mesh 7: {n - 1} triangles, its tree's leaves reach {n}")
    add(f"sah:99:{n}:nan", "HG_E_INVALID", f"hg_refit_mesh: mesh_index 99 out of range ({n_meshes} meshes)")
    out = driver(files["cornell"], *ops)
    assert len(out) == len(ops)
    for op, line, (code, text) in zip(ops, out, want):
        assert line == f"refused {E[code]} {text} same=1", (op, line)
    # without a scene
    out = driver(files["cornell"], "noscene", f"refit:7:{n}", f"lbvh:7:{n}:4", f"sah:7:{n}:2")
    for line in out[1:]:
        refused(line, "HG_E_NOSCENE", "hg_refit_mesh: hg_upload_scene not called")
    # a count above the tree's, where no other tree is in the way: the hazard scene's last triangles
    out = driver(files["leaf17"], "lbvh:4:16:4", "sah:4:16:0", "lbvh:4:17:0", "lbvh:4:17:15")
    refused(out[0], "HG_E_INVALID", "hg_refit_mesh: mesh 4: 16 triangles, its tree's leaves reach 17")
    refused(out[1], "HG_E_INVALID", "hg_refit_mesh: mesh 4: 16 triangles, its tree's leaves reach 17")
    refused(out[2], "HG_E_UNSUPPORTED", "hg_rebuild_mesh: mesh 4: no leaf size up to 15 fits 17 triangles into 0 records")
    refused(out[3], "HG_E_UNSUPPORTED", "hg_rebuild_mesh: mesh 4: 1 records at leaf size 15, the tree's capacity is 0")


def test_the_late_refusal_of_a_rebuild_by_surface_area(driver, files):
    """The records that the collapse leaves are known only after it ran (on the device: the live count): more than the
    slot at the caller's node cost, or at the last rung of the ladder.  Refused with nothing adopted."""
    out = driver(files["hazard"], f"sah:{GRID}:500:0.5", f"refit:{GRID}:500")
    m = re.fullmatch(rf"refused {E['HG_E_UNSUPPORTED']} hg_rebuild_mesh_sah: mesh 3: (\d+) records at node cost 0\.5, the tree's "
                     r"capacity is 143 same=1", out[0])
    assert m and 143 < int(m.group(1)) <= 499, out[0]
    assert out[1] == "ok refit instances=2 extent=500 same=1"
    out = driver(files["leaf17"], "sah:4:17:0")
    m = re.fullmatch(rf"refused {E['HG_E_UNSUPPORTED']} hg_rebuild_mesh_sah: mesh 4: (\d+) records at node cost 256, the last of "
                     r"the ladder; the tree's capacity is 0 same=1", out[0])
    assert m and 1 <= int(m.group(1)) <= 16, out[0]


@pytest.mark.parametrize("what", ["cycle", "range"])
def test_rebuilt_records_that_are_not_a_tree(driver, files, what):
    """adopt() on refs with a cycle, and with a child beyond the scene's records: reported, and nothing but the slot's
    own refs has changed (the harness compares; the entry point then drops the scene)"""
    for name, mesh in (("cornell", 7), ("hazard", GRID), ("hazard", 1)):
        out = driver(files[name], f"{what}:{mesh}", f"refit:{mesh}:1")
        assert out[0] == (f"refused {E['HG_E_INVALID']} hg_rebuild_mesh: mesh {mesh}: the rebuilt records are not a tree; "
                          "upload the scene again same=0"), out[0]
        refused(out[1], "HG_E_NOSCENE", "hg_refit_mesh: hg_upload_scene not called")


def test_asan_mesh_trees_program():
    """host/asan_mesh_trees.cpp under AddressSanitizer + UBSan: the same sequences and refusals on scenes it builds
    itself, and adopt() on adversarial refs (make asan_mesh_trees; a stand-alone program, host code only)."""
    assert "asan_mesh_trees ok" in run_sanitizer_program("asan_mesh_trees")
