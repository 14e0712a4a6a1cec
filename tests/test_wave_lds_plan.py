"""The LDS layout of a wave of the regenerating and streaming kernels (csrc/hg_layout.h hg_wave_lds_plan): where the
wave's copies of the mesh records and of the material table lie, and which of them it has.  A wrong plan either costs
occupancy (more LDS than the budget), only runs slower (a table left in global memory), or lets a table overlap rows a
lane writes, which the rendering tests would see only for the shapes they happen to run.  Here the header is compiled
with g++ (no HIP, no GPU) and swept over 0-80 meshes, 0-255 materials, 1-3 samples per pixel, both kernels' rows at a
shallow and at the deepest LDS stack, each kernel's budget and a budget of 0; the rules are restated below, not the
function's arithmetic."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "halogen-pathtracer_amd" / "csrc"
INCLUDE = ROOT / "include"

# hg_layout.h names float4 and uint2 and leaves them to its includer (as csrc/hg_scene_pack.h does on the host)
DRIVER = r'''
struct alignas(16) float4 { float x, y, z, w; };
struct uint2 { unsigned x, y; };
#include "hg_layout.h"
#include <cstdio>

int main() {
    unsigned long rows, budget;
    while (std::scanf("%lu %lu", &rows, &budget) == 2) {
        for (int nm = 0; nm <= 80; ++nm)
            for (int nt = 0; nt <= 255; ++nt)
                for (unsigned spp = 1; spp <= 3; ++spp) {
                    const HgWaveLdsPlan p = hg_wave_lds_plan(rows, nm, nt, spp, budget);
                    std::printf("%d %d %u %u %u %u %d %d %d\n", nm, nt, spp, p.mesh_word, p.mat_word, p.bytes,
                                int(p.mesh_lds), int(p.mat_lds), int(p.mat_in_sum_rows));
                }
    }
    std::printf("%d %d %u %u\n", HG_WAVE_LDS_BUDGET, HG_REGEN_LDS_BUDGET, HG_ROW_SUM, HG_SUM_ROWS_BYTES);
}
'''

MESH_BYTES, MAT_BYTES, ROW_BYTES = 80, 80, 256
# rows of 64 words (csrc/hg_mega.hip): throughput 0-2, colour 3-5, sample sum 6-8; the streaming kernel's spare row 9
# and leaf-share rows 10-12; then the stack's LDS entries (at most 12 / 16)
STREAM_STATE_ROWS, REGEN_STATE_ROWS, STREAM_LDS_STACK, MEGA_LDS_STACK = 13, 9, 12, 16
SUM_LO, SUM_HI = 6 * ROW_BYTES, 9 * ROW_BYTES


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    d = tmp_path_factory.mktemp("ldsplan")
    (d / "main.cpp").write_text(DRIVER)
    exe = d / "ldsplan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", f"-I{INCLUDE}", "-DHG_MEGA_LDS_STACK=16",
                    str(d / "main.cpp"), "-o", str(exe)], check=True)
    probe = subprocess.run([str(exe)], input="", capture_output=True, text=True, check=True).stdout.split()
    stream_budget, regen_budget, row_sum, sum_bytes = map(int, probe)
    assert (row_sum * ROW_BYTES, row_sum * ROW_BYTES + sum_bytes) == (SUM_LO, SUM_HI)
    shapes = [((STREAM_STATE_ROWS + depth) * ROW_BYTES, b) for depth in (4, STREAM_LDS_STACK) for b in (stream_budget, 0)]
    shapes += [((REGEN_STATE_ROWS + depth) * ROW_BYTES, b) for depth in (4, MEGA_LDS_STACK) for b in (regen_budget, 0)]
    out = subprocess.run([str(exe)], input="".join(f"{r} {b}\n" for r, b in shapes), capture_output=True, text=True,
                         check=True).stdout.splitlines()[:-1]
    per = 81 * 256 * 3
    assert len(out) == per * len(shapes)
    plans = {}
    for k, (rows, budget) in enumerate(shapes):
        for line in out[k * per:(k + 1) * per]:
            nm, nt, spp, mesh_word, mat_word, total, mesh_lds, mat_lds, in_sum = map(int, line.split())
            plans[(rows, budget, nm, nt, spp)] = (mesh_word, mat_word, total, mesh_lds, mat_lds, in_sum)
    return plans, stream_budget, regen_budget


def test_budgets_and_overlaps(sweep):
    """The launch's LDS stays within the budget whenever a table is placed behind the rows (the rows alone may exceed
    the regenerating kernel's budget: then nothing is added); no table overlaps the state rows, the leaf-share words,
    the stack or the other table, except the material table in the sample-sum rows, at 1 sample per pixel only."""
    plans, _, _ = sweep
    in_lds = in_sum_n = behind = 0
    for (rows, budget, nm, nt, spp), (mesh_word, mat_word, total, mesh_lds, mat_lds, in_sum) in plans.items():
        key = (rows, budget, nm, nt, spp)
        assert total >= rows and (total == rows or total <= budget), key
        regions = []
        if mesh_lds:
            assert nm > 0 and mesh_word * 4 == rows, key  # the mesh records keep their place right behind the rows
            regions.append((mesh_word * 4, mesh_word * 4 + nm * MESH_BYTES))
        if mat_lds:
            assert nt > 0 and mat_word * 4 % 16 == 0, key
            lo, hi = mat_word * 4, mat_word * 4 + nt * MAT_BYTES
            if in_sum:
                assert spp == 1 and SUM_LO <= lo and hi <= SUM_HI and SUM_HI <= rows, key
                in_sum_n += 1
            else:
                regions.append((lo, hi))
                behind += 1
            in_lds += 1
        else:
            assert not in_sum, key
        end = rows  # the regions behind the rows: beyond them, disjoint, within the launch's bytes, nothing unused
        for lo, hi in sorted(regions):
            assert lo == end, key
            end = hi
        assert end == total, key
        if budget == 0:
            assert not mesh_lds and not mat_lds and total == rows, key
    assert in_sum_n > 1000 and behind > 1000 and in_lds > in_sum_n


def test_mesh_table_unchanged_and_first(sweep):
    """The mesh records are placed exactly as before the material table existed (behind the rows if that fits the
    budget, whatever the materials), so the material table never displaces them, and a launch whose materials stay in
    global memory or lie in the sample-sum rows asks for the bytes it asked for before."""
    plans, _, _ = sweep
    for (rows, budget, nm, nt, spp), (mesh_word, mat_word, total, mesh_lds, mat_lds, in_sum) in plans.items():
        before = rows + nm * MESH_BYTES if nm > 0 and rows + nm * MESH_BYTES <= budget else 0  # mesh_lds_bytes
        assert mesh_lds == int(before != 0) and mesh_word * 4 == rows, (rows, budget, nm, nt, spp)
        if not mat_lds or in_sum:
            assert total == (before if before else rows), (rows, budget, nm, nt, spp)


def test_material_table_homes(sweep):
    """The preferred home, and no table left in global memory that has a home: at 1 sample a table of at most 768 B
    lies in the sample-sum rows; any other goes behind the mesh records (the rows, if those stay global) exactly when
    the budget allows."""
    plans, _, _ = sweep
    for (rows, budget, nm, nt, spp), (mesh_word, mat_word, total, mesh_lds, mat_lds, in_sum) in plans.items():
        key = (rows, budget, nm, nt, spp)
        if nt == 0 or budget == 0:
            assert not mat_lds, key
            continue
        if spp == 1 and nt * MAT_BYTES <= SUM_HI - SUM_LO:
            assert mat_lds and in_sum and mat_word * 4 == SUM_LO, key
        else:
            end = rows + (nm * MESH_BYTES if mesh_lds else 0)
            assert mat_lds == int(end + nt * MAT_BYTES <= budget) and not in_sum, key


def test_headline_shape(sweep):
    """C3 (7 meshes, 7 materials, at most 9; the streaming kernel at its 12 LDS stack entries, 1 sample): 6,960 B as
    before the material table, both tables in LDS.  7,680 B itself was never run (csrc/hg_tunables.h)."""
    plans, stream_budget, _ = sweep
    rows = (STREAM_STATE_ROWS + STREAM_LDS_STACK) * ROW_BYTES
    for nt in (7, 8, 9):
        mesh_word, mat_word, total, mesh_lds, mat_lds, in_sum = plans[(rows, stream_budget, 7, nt, 1)]
        assert (total, mesh_lds, mat_lds, in_sum) == (6960, 1, 1, 1)
    # one more material, or more samples: behind the mesh records, 7,760 B > the budget, so global memory
    assert plans[(rows, stream_budget, 7, 10, 1)][2:5] == (6960, 1, 0)
    assert plans[(rows, stream_budget, 7, 7, 2)][2:5] == (6960 + 560, 1, 1)
