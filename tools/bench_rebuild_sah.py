#!/usr/bin/env python3
"""Worth and cost of a device rebuild with leaves chosen by surface area (hg_rebuild_mesh_sah_device; csrc/hg_lbvh.hip)
of the C3 dragon (871,200 triangles), in one run on one GPU, by the protocol of tools/bench_rebuild.py (DESIGN.md
section 4.10b).  Not part of bench.py.

  trace  Mpaths/s of the C3 frame (32-frame launches, median [min, max] of 5 blocks after a warm-up block) after a twist
         of 0.3, 0.6, 1.2 and 2.4 radians per unit height:
           refitted              the rest pose's BVHGenerator tree, refitted
           lbvh_l4               the fixed-leaf-size rebuild at leaf size 4 (the baseline, measured here)
           sah_0.5 .. sah_4      the SAH rebuild at node cost 0.5, 1, 2 and 4, each with its record count
           bvhgenerator_rebuilt  BVHGenerator's tree built from the twisted vertices
         The SAH rows need more records than BVHGenerator's tree has (its capacity holds the tree at node cost 4 only),
         so for them the scene is uploaded with the dragon under the L = 1 radix tree of its rest pose, n - 1 records; a
         rebuilt tree takes the first records of that range, as anywhere.
  ms     synchronous calls under the host clock, alternating inside each block: the SAH rebuild at each node cost and the
         fixed-leaf-size rebuild at leaf size 4, from a torch tensor on the device.
  --kernels-only  8 SAH rebuilds at the library's node cost and nothing else, for `rocprofv3 --kernel-trace --stats --
         python tools/bench_rebuild_sah.py --kernels-only`: the per-kernel split.

  python tools/bench_rebuild_sah.py --out profiles/rebuild_sah.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch  # before the library's first context (one HIP runtime in the process)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "halogen-pathtracer_amd"))
sys.path.insert(0, str(ROOT / "tools"))

from bench_rebuild import with_dragon  # noqa: E402
from bench_refit import clock, stats, trace_rate, twist  # noqa: E402
from halogen import abi, render_pass as rp, scene as hs, scenes  # noqa: E402

NODE_COSTS = (0.5, 1.0, 2.0, 4.0)


def rows18(tris):
    return np.frombuffer(bytes(tris), dtype=np.float32).reshape(-1, 18)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rebuild_sah.json"))
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32, help="frames per timed trace block")
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_rebuild_sah: no HIP device (times are measured on the GPU or not at all)")
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
    # the same scene with the dragon under the L = 1 radix tree of its rest pose: room for a tree at any node cost.
    # order1: the position, in the dragon's own (BVHGenerator) triangle order, of the triangle at each position there
    order1, tris1, nodes1 = abi.build_blas_lbvh(dragon.packed_triangles, 1)
    roomy = hs.RayTracingMesh.__new__(hs.RayTracingMesh)
    roomy.__dict__.update(dragon.__dict__)
    roomy.packed_triangles, roomy.bvh = tris1, nodes1
    roomy_packed = with_dragon(sc, di, roomy).pack()
    print(f"{n_tris} triangles; scenes packed", flush=True)

    def moved(strength):
        """The dragon twisted: its triangles in the roomy scene's order on the host (the twin's input, for the record
        count), in BVHGenerator's order on the device (a refit's and the fixed-leaf rebuild's input) and in the roomy
        scene's order on the device (the SAH rebuild's input)"""
        dragon.deform(twist(rest, strength))
        t = rows18(dragon.packed_triangles)
        t1 = np.ascontiguousarray(t[order1])
        return (abi.HalogenTriangle * n_tris).from_buffer_copy(t1.tobytes()), torch.from_numpy(t.copy()).to("cuda:0"), \
            torch.from_numpy(t1).to("cuda:0")

    result = {"metric": "device rebuild of the C3 dragon's BVH with SAH-chosen leaves (one MI355X)", "triangles": n_tris,
              "blocks": args.blocks, "frames_per_block": args.frames}
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_COUNTERS, 0)
        ctx.upload_scene(roomy_packed)
        ctx.resize(W, H)
        if args.kernels_only:
            poses = [moved(k)[2] for k in (0.05, 0.1)]
            for k in range(8):  # (node cost 0: the library's, which fits this capacity at the first rung)
                ctx.rebuild_mesh_sah(di, poses[k & 1], 0.0)
            return

        # ---- the call time, on two small poses in turn (every call moves every triangle)
        poses = [moved(k) for k in (0.05, 0.1)]
        turn = [0]

        def pose(k):
            turn[0] ^= 1
            return poses[turn[0]][k]

        variants = {f"rebuild_sah_device_{c:g}": (lambda c=c: ctx.rebuild_mesh_sah(di, pose(2), c)) for c in NODE_COSTS}
        variants["rebuild_device_l4"] = lambda: ctx.rebuild_mesh(di, pose(2), 4)
        for fn in variants.values():
            fn()
        out = {k: [] for k in variants}
        for _ in range(args.blocks):
            for k, fn in variants.items():
                out[k].append(clock(fn))
        result["ms"] = {k: stats(v) for k, v in out.items()}
        print({k: round(v["median"], 3) for k, v in result["ms"].items()}, "ms", flush=True)

        # ---- the trace rate after a twist
        trace = {}
        for strength in (0.3, 0.6, 1.2, 2.4):
            host, dev, dev1 = moved(strength)
            row = {}
            ctx.upload_scene(rest_packed)  # a full upload: the rest pose's BVHGenerator tree again
            ctx.refit_mesh(di, dev)
            row["refitted"] = trace_rate(ctx, params, W, H, args.frames, args.blocks)
            ctx.rebuild_mesh(di, dev, 4)
            row["lbvh_l4"] = trace_rate(ctx, params, W, H, args.frames, args.blocks)
            for c in NODE_COSTS:
                ctx.upload_scene(roomy_packed)
                ctx.rebuild_mesh_sah(di, dev1, c)
                r = trace_rate(ctx, params, W, H, args.frames, args.blocks)
                r["records"] = (len(abi.build_blas_lbvh_sah(host, c)[2]) - 1) // 2
                r["over_lbvh_l4"] = r["median"] / row["lbvh_l4"]["median"]
                r["over_refitted"] = r["median"] / row["refitted"]["median"]
                row[f"sah_{c:g}"] = r
            gen = hs.RayTracingMesh(dragon.name, twist(rest, strength), dragon.normals, indices, dragon.transform,
                                    dragon.material)
            ctx.upload_scene(with_dragon(sc, di, gen).pack())
            row["bvhgenerator_rebuilt"] = trace_rate(ctx, params, W, H, args.frames, args.blocks)
            row["lbvh_l4_over_refitted"] = row["lbvh_l4"]["median"] / row["refitted"]["median"]
            row["lbvh_l4_records"] = (n_tris + 3) // 4 - 1
            trace[f"twist_{strength}"] = row
            print("trace", strength, {k: (round(v["median"], 1) if isinstance(v, dict) else round(v, 3))
                                      for k, v in row.items()}, flush=True)
            result["trace_mpaths_per_s"] = trace
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result, indent=1) + "\n")  # (kept after every twist)
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
