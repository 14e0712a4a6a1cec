"""The cull table (csrc/hg_cull.h) under AddressSanitizer + UBSan, as a stand-alone program with its own main
(host/asan_cull_table.cpp, make asan_cull_table): hand-made scenes with a leaf root, a singular matrix, 70 meshes, no
cullable mesh and an odd number of entries, their partial re-uploads, and seeded synthetic mesh tables, each table
checked and then walked two entries per fetch, as the kernel walks it, for every launch length.  Host code only."""
from host_programs import run_sanitizer_program


def test_cull_table_under_asan_ubsan():
    out = run_sanitizer_program("asan_cull_table", 200, 5)
    assert "hand-made scenes done" in out and out.rstrip().endswith("cull table ok"), out
    assert "FAILED" not in out and "runtime error" not in out, out
