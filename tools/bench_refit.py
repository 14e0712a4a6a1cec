#!/usr/bin/env python3
"""Cost of a device refit (hg_refit_mesh, hg_refit_mesh_device; csrc/hg_refit.hip) of the C3 dragon (871,200
triangles), against the only alternative the library had before: hg_refit_blas on one host thread and a full
hg_upload_scene of the same deformed arrays.  Not part of bench.py.

  refit_host     ms per hg_refit_mesh from a host pointer (the 63-MB copy included)
  refit_device   ms per hg_refit_mesh_device from a torch tensor already on the device
  full_upload    ms per hg_refit_blas (1 thread) + hg_upload_scene of the deformed arrays, in the same run
All three are synchronous: the host clock around the call.  The variants alternate inside each round (a drift lands on
all of them), every call sees another pose (two poses in turn) and every upload here is a full one (after a refit an
unvouched upload always is).  Median, min and max over the blocks; floor_gb_per_s sets the device refit beside the
bytes it cannot avoid (72 B read + 84 B written per triangle, 64 B read + written per record).
  trace          Mpaths/s of the C3 frame on the refitted tree after a large twist, against a tree rebuilt from the
                 twisted vertices: the known price of refitting (the rest pose's split planes), not a gate.
  --kernels-only N device refits and nothing else, for `rocprofv3 --kernel-trace --stats -- python tools/bench_refit.py
                 --kernels-only`: the per-kernel split (hg_refit_repack, hg_refit_level).

  python tools/bench_refit.py --out profiles/refit.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch  # before the library's first context (one HIP runtime in the process)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "halogen-pathtracer_amd"))

from halogen import abi, render_pass as rp, scene as hs, scenes  # noqa: E402


def stats(xs):
    xs = np.asarray(xs, float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "blocks": len(xs)}


def twist(v, strength):
    ang = (v[:, 1] * np.float32(strength)).astype(np.float32)
    out = v.copy()
    out[:, 0] = v[:, 0] * np.cos(ang) - v[:, 2] * np.sin(ang)
    out[:, 2] = v[:, 0] * np.sin(ang) + v[:, 2] * np.cos(ang)
    return out.astype(np.float32)


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def trace_rate(ctx, params, W, H, frames, blocks):
    out = []
    for k in range(blocks + 1):
        ctx.clear_accumulation()
        ctx.set_params(params)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.render(frames, True)
        ctx.synchronize()
        if k:  # the first block warms up
            out.append(W * H * frames / (time.perf_counter() - t0) / 1e6)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refit.json"))
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--frames", type=int, default=32, help="frames per timed trace block")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_refit: no HIP device (times are measured on the GPU or not at all)")
    cfg = scenes.CONFIGS["C3"]
    W, H = cfg.width, cfg.height
    s = rp.clamp_settings(scenes.settings_for(cfg))
    sc = scenes.dragon_cornell(args.subdiv)
    di = len(sc.meshes) - 1
    dragon = sc.meshes[di]
    rest = dragon.vertices.copy()
    params = rp.make_params(s, cfg.camera(), 1, len(sc.spheres), len(sc.meshes), False)
    poses = []
    for strength in (0.05, 0.1):  # two small poses in turn: every call moves every triangle
        dragon.deform(twist(rest, strength))
        tris = (abi.HalogenTriangle * len(dragon.packed_triangles))()
        C.memmove(tris, dragon.packed_triangles, C.sizeof(tris))
        dev = torch.from_numpy(np.frombuffer(bytes(tris), dtype=np.float32).reshape(-1, 18).copy()).to("cuda:0")
        poses.append({"tris": tris, "dev": dev, "packed": sc.pack()})
    n_tris = len(dragon.packed_triangles)
    scratch_bvh = (abi.BVHEntry * len(dragon.bvh))()
    C.memmove(scratch_bvh, dragon.bvh, C.sizeof(scratch_bvh))
    n_records = sum(1 for e in dragon.bvh if e.triangleCount == 0)
    floor_bytes = n_tris * (72 + 36 + 48) + n_records * 128
    result = {"metric": "refit of the C3 dragon (one MI355X)", "triangles": n_tris, "records": n_records,
              "timing": "host clock around synchronous calls", "blocks": args.blocks, "floor_bytes": floor_bytes}
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_COUNTERS, 0)
        ctx.upload_scene(poses[0]["packed"])
        ctx.resize(W, H)
        if args.kernels_only:
            for k in range(8):
                ctx.refit_mesh(di, poses[k & 1]["dev"])
            return
        turn = [0]

        def pose():
            turn[0] ^= 1
            return poses[turn[0]]

        def full():
            p = pose()
            abi.refit_blas(p["tris"], scratch_bvh)  # what keeps the caller's tree current, on one thread
            ctx.upload_scene(p["packed"])

        variants = {"refit_host": lambda: ctx.refit_mesh(di, pose()["tris"]),
                    "refit_device": lambda: ctx.refit_mesh(di, pose()["dev"]),
                    "refit_blas_host_twin": lambda: abi.refit_blas(pose()["tris"], scratch_bvh),
                    "full_upload": full}
        for fn in variants.values():
            fn()
        out = {k: [] for k in variants}
        before = ctx.counters()
        for _ in range(args.blocks):
            for k, fn in variants.items():
                out[k].append(clock(fn))
        after = ctx.counters()
        full_uploads = (after["scene_uploads"] - after["scene_uploads_partial"]) - \
            (before["scene_uploads"] - before["scene_uploads_partial"])
        assert full_uploads == args.blocks and after["scene_uploads_skipped"] == before["scene_uploads_skipped"], after
        result["ms"] = {k: stats(v) for k, v in out.items()}
        for k in ("refit_host", "refit_device"):
            result["ms"][k]["floor_gb_per_s"] = floor_bytes / result["ms"][k]["median"] / 1e6
        result["device_refit_over_full_upload"] = result["ms"]["refit_device"]["median"] / \
            result["ms"]["full_upload"]["median"]
        print({k: round(v["median"], 3) for k, v in result["ms"].items()}, "ms", flush=True)
        # the price of refitting: the C3 frame on the refitted tree after a large twist ...
        big = twist(rest, 1.2)
        dragon.deform(big)
        ctx.refit_mesh(di, dragon.packed_triangles)
        trace = {"refitted": trace_rate(ctx, params, W, H, args.frames, 5)}
    # ... against a tree rebuilt from the twisted vertices
    rebuilt = hs.Scene()
    for m in sc.meshes[:di]:
        rebuilt.add(m)
    rebuilt.add(hs.RayTracingMesh(dragon.name, big, dragon.normals, scenes.dragon_mesh(args.subdiv)[2], dragon.transform,
                                  dragon.material))
    for sp in sc.spheres:
        rebuilt.add(sp)
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_COUNTERS, 0)
        ctx.upload_scene(rebuilt.pack())
        ctx.resize(W, H)
        trace["rebuilt"] = trace_rate(ctx, params, W, H, args.frames, 5)
    trace["refitted_over_rebuilt"] = trace["refitted"]["median"] / trace["rebuilt"]["median"]
    trace["twist_radians_per_unit_height"] = 1.2
    result["trace_mpaths_per_s"] = trace
    print("trace", {k: (round(v["median"], 1) if isinstance(v, dict) else round(v, 3)) for k, v in trace.items()},
          flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
