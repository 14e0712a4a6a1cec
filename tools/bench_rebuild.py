#!/usr/bin/env python3
"""Cost and worth of a device rebuild (hg_rebuild_mesh_device; csrc/hg_lbvh.hip) of the C3 dragon (871,200 triangles),
in one run on one GPU.  Not part of bench.py.

  ms     (a) synchronous calls under the host clock, alternating inside each block (a drift lands on all of them):
         rebuild_device_l4 / _auto   hg_rebuild_mesh_device from a torch tensor on the device, leaf size 4 / 0
         rebuild_host_l4             hg_rebuild_mesh from a host pointer (the 63-MB copy and the order's copy included)
         refit_device                hg_refit_mesh_device, for scale
         build_blas_mt               hg_build_blas_mt (8 threads) on the twisted vertices, alone
         host_build_full_upload      the only way before: hg_build_blas_mt, then a full hg_upload_scene of the scene
                                     with that tree (packing the arrays is not timed)
         lbvh_host_twin              hg_build_blas_lbvh on one host thread, for scale
  trace  (b) Mpaths/s of the C3 frame (32-frame launches, median of 5) after a twist of 0.3, 0.6, 1.2 and 2.4 radians per
         unit height: the refitted rest-pose tree, the LBVH at leaf size 4 (and at the automatic size for the largest
         twist) rebuilt on the device, and BVHGenerator's tree built from the twisted vertices.  No gate.
  --kernels-only  8 device rebuilds and nothing else, for `rocprofv3 --kernel-trace --stats -- python
         tools/bench_rebuild.py --kernels-only`: the per-kernel split (c).

  python tools/bench_rebuild.py --out profiles/rebuild.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch  # before the library's first context (one HIP runtime in the process)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "halogen-pathtracer_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from bench_refit import clock, stats, trace_rate, twist  # noqa: E402
from halogen import abi, render_pass as rp, scene as hs, scenes  # noqa: E402


def on_device(tris):
    return torch.from_numpy(np.frombuffer(bytes(tris), dtype=np.float32).reshape(-1, 18).copy()).to("cuda:0")


def copy_of(tris):
    out = (abi.HalogenTriangle * len(tris))()
    C.memmove(out, tris, C.sizeof(out))
    return out


def with_dragon(sc, di, mesh):
    out = hs.Scene()
    for i, m in enumerate(sc.meshes):
        out.add(mesh if i == di else m)
    for sp in sc.spheres:
        out.add(sp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rebuild.json"))
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--frames", type=int, default=32, help="frames per timed trace block")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_rebuild: no HIP device (times are measured on the GPU or not at all)")
    cfg = scenes.CONFIGS["C3"]
    W, H = cfg.width, cfg.height
    s = rp.clamp_settings(scenes.settings_for(cfg))
    sc = scenes.dragon_cornell(args.subdiv)
    di = len(sc.meshes) - 1
    dragon = sc.meshes[di]
    rest = dragon.vertices.copy()
    indices = scenes.dragon_mesh(args.subdiv)[2]
    params = rp.make_params(s, cfg.camera(), 1, len(sc.spheres), len(sc.meshes), False)
    rest_packed = sc.pack()
    n_tris = dragon.triangle_count
    threads = min(8, len(os.sched_getaffinity(0)))

    def generator_mesh(vertices):  # BVHGenerator's tree from these vertices (hg_build_blas_mt, as RayTracingMesh builds)
        return hs.RayTracingMesh(dragon.name, vertices, dragon.normals, indices, dragon.transform, dragon.material)

    poses = []
    for strength in (0.05, 0.1):  # two small poses in turn: every call moves every triangle
        v = twist(rest, strength)
        dragon.deform(v)
        tris = copy_of(dragon.packed_triangles)
        poses.append({"vertices": v, "tris": tris, "dev": on_device(tris),
                      "packed": with_dragon(sc, di, generator_mesh(v)).pack()})
    result = {"metric": "rebuild of the C3 dragon's BVH (one MI355X)", "triangles": n_tris,
              "timing": "host clock around synchronous calls", "blocks": args.blocks, "host_build_threads": threads}
    mn, mx = (np.ascontiguousarray(a, dtype=np.float32) for a in hs.mesh_bounds_min_max(poses[0]["vertices"]))
    fp = C.POINTER(C.c_float)
    cap = 2 * n_tris + 2
    nodes = (abi.BVHEntry * cap)()
    L = abi.lib()
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_COUNTERS, 0)
        ctx.upload_scene(poses[0]["packed"])
        ctx.resize(W, H)
        if args.kernels_only:
            for k in range(8):
                ctx.rebuild_mesh(di, poses[k & 1]["dev"], 4)
            return
        auto = next(k for k in range(4, 16) if _fits(ctx, di, poses[0]["dev"], k))
        result["auto_leaf_size"] = auto
        turn = [0]

        def pose():
            turn[0] ^= 1
            return poses[turn[0]]

        idx = [indices.copy()]

        def build_mt():
            p = pose()
            n = L.hg_build_blas_mt(p["vertices"].ctypes.data, len(p["vertices"]), idx[0].ctypes.data, n_tris,
                                   mn.ctypes.data_as(fp), mx.ctypes.data_as(fp), 32, C.cast(nodes, C.c_void_p), cap,
                                   threads)
            assert n > 0
            return p

        def full():
            ctx.upload_scene(build_mt()["packed"])

        variants = {"rebuild_device_l4": lambda: ctx.rebuild_mesh(di, pose()["dev"], 4),
                    "rebuild_device_auto": lambda: ctx.rebuild_mesh(di, pose()["dev"], 0),
                    "rebuild_host_l4": lambda: ctx.rebuild_mesh(di, pose()["tris"], 4),
                    "refit_device": lambda: ctx.refit_mesh(di, pose()["dev"]),
                    "build_blas_mt": build_mt,
                    "host_build_full_upload": full,
                    "lbvh_host_twin": lambda: abi.build_blas_lbvh(pose()["tris"], 4)}
        for fn in variants.values():
            fn()
        out = {k: [] for k in variants}
        before = ctx.counters()
        for _ in range(args.blocks):
            for k, fn in variants.items():
                idx[0] = indices.copy()  # (the builder permutes its index list in place; the copy is not timed)
                out[k].append(clock(fn))
        after = ctx.counters()
        full_uploads = (after["scene_uploads"] - after["scene_uploads_partial"]) - \
            (before["scene_uploads"] - before["scene_uploads_partial"])
        assert full_uploads == args.blocks and after["scene_uploads_skipped"] == before["scene_uploads_skipped"], after
        result["ms"] = {k: stats(v) for k, v in out.items()}
        result["host_way_over_device_rebuild"] = result["ms"]["host_build_full_upload"]["median"] / \
            result["ms"]["rebuild_device_l4"]["median"]
        print({k: round(v["median"], 3) for k, v in result["ms"].items()}, "ms", flush=True)

        # (b) the trace rate after a twist
        trace = {}
        for strength in (0.3, 0.6, 1.2, 2.4):
            big = twist(rest, strength)
            row = {}
            ctx.upload_scene(rest_packed)  # a full upload: the rest pose's BVHGenerator tree again
            dragon.deform(big)             # (the Python mesh is refitted only: its order stays the rest pose's)
            ctx.refit_mesh(di, dragon.packed_triangles)
            row["refitted"] = trace_rate(ctx, params, W, H, args.frames, 5)
            ctx.rebuild_mesh(di, on_device(dragon.packed_triangles), 4)
            row["lbvh_l4"] = trace_rate(ctx, params, W, H, args.frames, 5)
            if strength == 1.2 and auto != 4:
                ctx.upload_scene(rest_packed)
                ctx.rebuild_mesh(di, on_device(dragon.packed_triangles), 0)
                row["lbvh_auto"] = trace_rate(ctx, params, W, H, args.frames, 5)
            ctx.upload_scene(with_dragon(sc, di, generator_mesh(big)).pack())
            row["bvhgenerator_rebuilt"] = trace_rate(ctx, params, W, H, args.frames, 5)
            row["lbvh_l4_over_refitted"] = row["lbvh_l4"]["median"] / row["refitted"]["median"]
            row["refitted_over_bvhgenerator"] = row["refitted"]["median"] / row["bvhgenerator_rebuilt"]["median"]
            row["lbvh_l4_over_bvhgenerator"] = row["lbvh_l4"]["median"] / row["bvhgenerator_rebuilt"]["median"]
            trace[f"twist_{strength}"] = row
            print("trace", strength, {k: (round(v["median"], 1) if isinstance(v, dict) else round(v, 3))
                                      for k, v in row.items()}, flush=True)
        result["trace_mpaths_per_s"] = trace
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


def _fits(ctx, di, dev, leaf_size):
    try:
        ctx.rebuild_mesh(di, dev, leaf_size)
        return True
    except abi.HalogenError:
        return False


if __name__ == "__main__":
    main()
