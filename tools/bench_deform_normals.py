#!/usr/bin/env python3
"""Cost of recomputing the vertex normals on the device when the C3 dragon (871,200 triangles) is posed from its
vertices (HG_DEFORM_NORMALS; the two normal kernels of csrc/hg_deform.hip).  A sibling of tools/bench_deform.py, whose
leg c this repeats.  Not part of bench.py.

  c_given      hg_deform_mesh_device from device positions and given device normals (the path without the flag)
  e_recompute  hg_deform_mesh_device from device positions alone, with the flag
  f_torch      the caller's only other way on the device: torch cross products of the gathered corners, index_add_
               (float atomics), normalise, then c's call with those normals
and the same three with a rebuild with leaves chosen by surface area in place of the refit (`ms_rebuild_sah`).  Also:
the one-time cost of binding the index list with and without the adjacency (built on the host inside the call), the
dragon's valences, whether f's normals have the same bits in two runs of one pose, and how far they are from the
library's.

Every call is synchronous: the host clock around it.  The legs alternate inside each block (a drift lands on all of
them), each leg has a context of its own and sees two poses in turn.  c is given the host twin's normals
(abi.vertex_normals), so c and e must leave the same device scene: asserted.  Median, min and max over the blocks.

  python tools/bench_deform_normals.py --out profiles/deform_normals.json
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch  # before the library's first context (one HIP runtime in the process)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "halogen-pathtracer_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from bench_deform import clock, stats, twist  # noqa: E402
from halogen import abi, scenes  # noqa: E402


def torch_normals(dv, d_idx):
    """Area-weighted vertex normals the way a torch caller would write them: the sum is index_add_'s, in arrival order"""
    a, b, c = dv[d_idx[:, 0]], dv[d_idx[:, 1]], dv[d_idx[:, 2]]
    f = torch.linalg.cross(b - a, c - a)
    s = torch.zeros_like(dv)
    for k in range(3):
        s.index_add_(0, d_idx[:, k], f)
    d = (s * s).sum(dim=1, keepdim=True)
    return torch.where(d > 0, s * torch.rsqrt(d), torch.zeros_like(s)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deform_normals.json"))
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--sah-blocks", type=int, default=5)
    ap.add_argument("--bind-blocks", type=int, default=5)
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_deform_normals: no HIP device (times are measured on the GPU or not at all)")
    sc = scenes.dragon_cornell(args.subdiv)
    di = len(sc.meshes) - 1
    dragon = sc.meshes[di]
    rest_v = dragon.vertices.copy()
    idx = dragon.triangles.copy()
    nv, n_tris = len(rest_v), len(idx)
    packed = sc.pack()
    valence = np.bincount(idx.reshape(-1), minlength=nv)
    d_idx = torch.from_numpy(idx.astype(np.int64)).to("cuda:0")
    poses = []
    for strength in (0.05, 0.1):  # two small poses in turn: every call moves every vertex
        v = twist(rest_v, strength)
        n = abi.vertex_normals(v, idx)
        poses.append({"dv": torch.from_numpy(v).to("cuda:0"), "dn": torch.from_numpy(n).to("cuda:0"), "n": n})

    class Leg:
        def __init__(self, adjacency):
            self.ctx = abi.Context(0)
            self.ctx.set_option(abi.HG_OPT_COUNTERS, 0)
            self.ctx.upload_scene(packed)
            self.ctx.set_mesh_vertices(di, idx, nv, adjacency=adjacency)
            self.turn = 0

        def next(self):
            self.turn ^= 1
            return poses[self.turn]

    legs = {"c_given": Leg(False), "e_recompute": Leg(True), "f_torch": Leg(False)}

    def runs(how):
        kw = {} if how == "refit" else {"how": how}

        def c(leg=legs["c_given"]):
            p = leg.next()
            leg.ctx.deform_mesh(di, p["dv"], p["dn"], **kw)

        def e(leg=legs["e_recompute"]):
            p = leg.next()
            leg.ctx.deform_mesh(di, p["dv"], None, recompute_normals=True, **kw)

        def f(leg=legs["f_torch"]):
            p = leg.next()
            leg.ctx.deform_mesh(di, p["dv"], torch_normals(p["dv"], d_idx), **kw)

        return {"c_given": c, "e_recompute": e, "f_torch": f}

    def measure(fns, blocks):
        for fn in fns.values():
            fn()
            fn()
        out = {k: [] for k in fns}
        for _ in range(blocks):
            for k, fn in fns.items():
                out[k].append(clock(fn))
        return {k: stats(v) for k, v in out.items()}

    def same_scene(what):
        for k in ("tris", "normals"):
            assert np.array_equal(legs["c_given"].ctx.scene_readback(k), legs["e_recompute"].ctx.scene_readback(k)), (what, k)

    result = {"metric": "one pose of the C3 dragon from its positions, normals recomputed (one MI355X)",
              "triangles": n_tris, "vertices": nv,
              "timing": "host clock around synchronous calls, legs alternating inside each block",
              "valence": {"median": float(np.median(valence)), "max": int(valence.max()), "min": int(valence.min())}}
    result["ms_refit"] = measure(runs("refit"), args.blocks)
    for k in ("nodes", "tris", "normals", "meshes"):
        assert np.array_equal(legs["c_given"].ctx.scene_readback(k), legs["e_recompute"].ctx.scene_readback(k)), k
    print({k: round(v["median"], 3) for k, v in result["ms_refit"].items()}, "ms per refit pose", flush=True)
    result["ms_rebuild_sah"] = measure(runs("sah"), args.sah_blocks)
    same_scene("after the rebuilds")
    result["same_device_scene"] = ["c_given", "e_recompute"]
    print({k: round(v["median"], 3) for k, v in result["ms_rebuild_sah"].items()}, "ms per rebuilt pose", flush=True)

    # f's normals: two runs of one pose against each other, and against the library's
    p = poses[0]
    runs_f = [torch_normals(p["dv"], d_idx).cpu().numpy().view(np.uint32) for _ in range(4)]
    differing = [int((r != runs_f[0]).sum()) for r in runs_f[1:]]
    lib_bits = p["n"].view(np.uint32)
    result["f_torch_normals"] = {
        "floats": int(runs_f[0].size),
        "floats_that_differ_between_runs_of_one_pose": differing,
        "bits_differ_between_runs": bool(any(differing)),
        "floats_that_differ_from_the_library": int((runs_f[0] != lib_bits).sum()),
        "max_abs_difference_from_the_library": float(np.abs(runs_f[0].view(np.float32) - p["n"]).max())}
    print(result["f_torch_normals"], flush=True)

    # the one-time cost of a binding, on a context of its own
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_COUNTERS, 0)
        ctx.upload_scene(packed)
        bind = {"plain": lambda: ctx.set_mesh_vertices(di, idx, nv), "adjacency": lambda: ctx.set_mesh_vertices(di, idx, nv, adjacency=True)}
        for fn in bind.values():
            fn()
        out = {k: [] for k in bind}
        for _ in range(args.bind_blocks):
            for k, fn in bind.items():
                out[k].append(clock(fn))
    result["ms_bind"] = {k: stats(v) for k, v in out.items()}
    v = twist(rest_v, 0.07)
    t0 = time.perf_counter()
    abi.vertex_normals(v, idx)
    result["ms_host_twin"] = (time.perf_counter() - t0) * 1e3
    print({k: round(v["median"], 3) for k, v in result["ms_bind"].items()}, "ms per binding", flush=True)
    for leg in legs.values():
        leg.ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
