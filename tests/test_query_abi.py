"""The ray query entry points at the C-ABI boundary (hg_trace_rays, hg_trace_rays_device, hg_camera_rays): declared by
the header, listed by abi.EXPORTS, exported by the library, and hg_ray / hg_ray_hit laid out as the ctypes and numpy
mirrors and the C# structs lay them out.  CPU only."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

from halogen import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "halogen_abi.h"
CS = ROOT / "bindings" / "csharp" / "HalogenNative.cs"
QUERY_EXPORTS = ("hg_trace_rays", "hg_trace_rays_device", "hg_camera_rays")
STRUCTS = {"hg_ray": (abi.HgRay, abi.RAY_DTYPE, 32), "hg_ray_hit": (abi.HgRayHit, abi.RAY_HIT_DTYPE, 48)}
ENUMS = ("HG_HIT_NONE", "HG_HIT_MESH", "HG_HIT_SPHERE", "HG_RAYS_CLOSEST", "HG_RAYS_ANY")


def test_header_declares_and_library_exports_the_queries(built):
    declared = set(re.findall(r"\b(hg_[a-z_]+)\s*\(", HEADER.read_text()))
    for name in QUERY_EXPORTS:
        assert name in declared, name
        assert name in abi.EXPORTS, name
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], check=True, capture_output=True,
                         text=True).stdout
    exported = set(re.findall(r"\bT (hg_[a-z_]+)\b", out))
    assert set(QUERY_EXPORTS) <= exported
    L = abi.lib()
    for name in QUERY_EXPORTS:
        assert getattr(L, name).argtypes is not None, name


def _c_layout(tmp_path):
    """sizeof / offsetof of hg_ray and hg_ray_hit as gcc compiles them from the header (tests/test_abi.py's probe)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "halogen_abi.h"', "int main(void){"]
    for cname, (py, _, _) in STRUCTS.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "hg_query_layout_probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "hg_query_layout_probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {(s, f): int(v) for s, f, v in (ln.split() for ln in out.splitlines())}


def test_ray_records_match_the_header(built, tmp_path):
    res = _c_layout(tmp_path)
    for cname, (py, dt, size) in STRUCTS.items():
        assert res[(cname, "size")] == size == C.sizeof(py) == dt.itemsize, cname
        assert [f for f, _ in py._fields_] == list(dt.names), cname
        for f, _ in py._fields_:
            assert res[(cname, f)] == getattr(py, f).offset == dt.fields[f][1], (cname, f)


def test_enum_values_match_header_and_csharp(built):
    h = dict((k, int(v)) for k, v in re.findall(r"\b(HG_(?:HIT|RAYS)_\w+) = (\d+)", HEADER.read_text()))
    cs = dict((k, int(v)) for k, v in re.findall(r"\b(HG_(?:HIT|RAYS)_\w+) = (\d+)", CS.read_text()))
    assert sorted(h) == sorted(ENUMS)
    assert h == cs
    for k in ENUMS:
        assert getattr(abi, k) == h[k], k
    assert abi.RAY_MODES == {"closest": h["HG_RAYS_CLOSEST"], "any": h["HG_RAYS_ANY"]}


def test_csharp_ray_structs_follow_the_header():
    """Field names in the header's order (`object` is a C# keyword: @object names the same field)."""
    text = CS.read_text()
    for cs_name, (py, _, _) in (("HgRay", STRUCTS["hg_ray"]), ("HgRayHit", STRUCTS["hg_ray_hit"])):
        body = re.search(r"public struct %s\s*\{(.*?)\n    \}" % cs_name, text, re.S).group(1)
        names = [n.strip().lstrip("@") for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 2)[2].split(",")]
        assert names == [f for f, _ in py._fields_], cs_name


def test_numpy_ray_rows_are_the_record(built):
    """An (n, 8) float32 row and a RAY_DTYPE element are the same 32 bytes; a hit is 12 words."""
    r = np.zeros(1, abi.RAY_DTYPE)
    r["origin"], r["t_max"], r["direction"] = (1, 2, 3), np.inf, (0, 0, 1)
    assert r.view(np.float32).tolist() == [1, 2, 3, np.inf, 0, 0, 1, 0]
    assert abi.RAY_HIT_DTYPE.itemsize == 12 * 4
