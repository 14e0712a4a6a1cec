#!/usr/bin/env python3
"""Ray-stream rates of the query kernel (csrc/hg_query.hip) on the C3 dragon scene: the traversal by itself, with no
shading, no sampler and no accumulation, at a ray coherence the caller chooses.  Not part of bench.py.

Three sets of 2^22 rays, on the reference BLAS and on the SAH tree:
  camera   the 1080p camera rays of frame 1 (then of frames 2 and 3, up to 2^22), box opening filling the frame (the C3F
           view), in the render's order: 8x8 pixel tiles, 64 consecutive rays = one tile = one wave, as in the megakernels;
  shuffled the same rays in a seeded random order (incoherent: every lane of a wave in another part of the tree);
  segments unit rays between seeded random point pairs inside the Cornell box, t_max = the pair's distance (occlusion).
Each set is traced closest and any-hit through the device entry point (hg_trace_rays_device: rays and hits stay on the
device, no PCIe transfer in the timed region).  The call is synchronous, so the host clock around it spans the launches
(four of 2^20 rays) and their completion; the same clock around a 64-ray call gives the call's fixed cost.  Per figure:
warm-up calls, then two blocks of `--reps` timed calls, alternating with the other mode's; the faster block's median,
min and max, and both blocks' medians.

Beside each figure stands the megakernel's own ray rate from profiles/r06f_bench.json (Mpaths/s x rays per path of its
framed C3 measurement) for orientation: that kernel also shades, samples and accumulates between its traversals.

  python tools/bench_rays.py --out profiles/query_rays.json
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

from halogen import abi, render_pass as rp, scene as hscene, scenes  # noqa: E402

N_RAYS = 1 << 22


def camera_rays(ctx, params, W, H, n):
    """Camera rays of frames 1, 2, ... in tile-major order (tile row-major, pixel lx + 8 ly inside a tile)."""
    ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8), np.arange(8),
                                 indexing="ij")
    px = np.stack([(tx * 8 + lx).ravel(), (ty * 8 + ly).ravel()], axis=1).astype(np.int32)
    px = px[(px[:, 0] < W) & (px[:, 1] < H)]
    out, frame = [], 1
    while sum(len(r) for r in out) < n:
        out.append(ctx.camera_rays(params, frame, px))
        frame += 1
    rays = np.concatenate(out)[:n]
    return np.ascontiguousarray(rays.view(np.float32).reshape(-1, 8)), frame - 1


def segment_rays(rng, n):
    """Random point pairs inside the Cornell box (5 x 5 x 5 behind the opening at local z 13.5)."""
    lo = np.array(scenes.CORNELL_ROOT) + np.array([-2.5, -2.5, 13.5])
    a = lo + rng.uniform(0.0, 5.0, (n, 3))
    b = lo + rng.uniform(0.0, 5.0, (n, 3))
    d = b - a
    dist = np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:4], rays[:, 4:7] = a, dist, d / dist
    return rays


def timed(ctx, d_rays, mode, warmup, reps):
    for _ in range(warmup):
        hits = ctx.trace_rays(d_rays, mode)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hits = ctx.trace_rays(d_rays, mode)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    n = d_rays.shape[0]
    kind = hits[:, 1].view(torch.int32)
    return {"mrays_per_s": n / np.median(ms) / 1e3, "mrays_per_s_min": n / ms.max() / 1e3,
            "mrays_per_s_max": n / ms.min() / 1e3, "ms_median": float(np.median(ms)), "ms_min": float(ms.min()),
            "ms_max": float(ms.max()), "reps": reps, "hit_frac": float((kind != 0).float().mean().item())}


def primary_ray_work(packed, params, cfg):
    """Tests per camera ray of the view, from the work counters of one frame with maxBounces = 0 (every path is its
    camera ray) on the lockstep kernel, whose traversal the query kernel shares; leaf_lane_util = triangle tests per
    lane slot of the leaf loop's wave-level rounds.  To set beside the megakernel's tests per ray (all bounces)."""
    p = abi.HgParams.from_buffer_copy(params)
    p.maxBounces = 0
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_KERNEL, abi.HG_KERNEL_MEGA)
        ctx.upload_scene(packed)
        ctx.resize(cfg.width, cfg.height)
        ctx.set_params(p)
        ctx.render(1, True)
        c = ctx.counters()
    return {"rays": c["rays"], "tri_tests_per_ray": c["tri_tests"] / c["rays"],
            "aabb_tests_per_ray": c["aabb_tests"] / c["rays"],
            "leaf_lane_util": c["tri_tests"] / (64 * c["tri_rounds"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "query_rays.json"))
    ap.add_argument("--rays", type=int, default=N_RAYS)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trees", default="reference,sah", help="comma-separated: reference, sah")
    ap.add_argument("--sets", default="camera,shuffled,segments", help="comma-separated ray sets")
    ap.add_argument("--modes", default="closest,any", help="comma-separated query modes")
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_rays: no HIP device (rates are measured on the GPU or not at all)")

    ref = json.loads((ROOT / "profiles" / "r06f_bench.json").read_text())
    fr = ref["framed"]
    mega = {"c3f_mrays_per_s": fr["value"] * fr["rays_per_path"], "c3f_mpaths_per_s": fr["value"],
            "c3f_rays_per_path": fr["rays_per_path"], "kernel": fr["roofline"]["kernel"],
            "c3f_tri_tests_per_ray": fr["tri_tests_per_path"] / fr["rays_per_path"],
            "source": "profiles/r06f_bench.json framed (reference BLAS): Mpaths/s x rays per path",
            "sah_c3_mrays_per_s": ref["fast_bvh"]["value"] * ref["fast_bvh"]["counters_per_path"]["rays"],
            "sah_source": "profiles/r06f_bench.json fast_bvh (SAH BLAS, the C3 front view: 54 % primary misses)"}

    cfg = scenes.CONFIGS["C3F"]
    s = rp.clamp_settings(scenes.settings_for(cfg))
    rng = np.random.default_rng(4242)
    perm = rng.permutation(args.rays)
    seg = segment_rays(rng, args.rays)
    result = {"metric": "Mrays/s of hg_trace_rays_device, 2^22-ray sets on the C3 dragon scene (one MI355X)",
              "rays_per_set": args.rays, "launch_rays": 1 << 20, "timing": "host clock around the synchronous call",
              "warmup": args.warmup, "reps": args.reps, "view": cfg.name, "megakernel": mega, "trees": {}}
    modes = args.modes.split(",")
    for builder in args.trees.split(","):
        prev = hscene.set_blas_builder(builder)
        try:
            t0 = time.perf_counter()
            packed = scenes.dragon_cornell(args.subdiv).pack()
            build_s = time.perf_counter() - t0
        finally:
            hscene.set_blas_builder(prev)
        params = rp.make_params(s, cfg.camera(), 1, len(packed.spheres), len(packed.meshes), False)
        tree = {"triangles": len(packed.triangles), "blas_nodes": len(packed.blas), "scene_build_s": build_s, "sets": {}}
        with abi.Context(0) as ctx:
            ctx.upload_scene(packed)
            cam, frames = camera_rays(ctx, params, cfg.width, cfg.height, args.rays)
            tree["camera_frames"] = frames
            tiny = torch.from_numpy(np.ascontiguousarray(cam[:64])).to("cuda:0")
            tree["call_overhead_ms"] = timed(ctx, tiny, "closest", args.warmup, args.reps)["ms_median"]
            for name, rays in (("camera", cam), ("shuffled", cam[perm]), ("segments", seg)):
                if name not in args.sets.split(","):
                    continue
                d_rays = torch.from_numpy(np.ascontiguousarray(rays)).to("cuda:0")
                row = {}
                # alternate the two modes' timed blocks so that a drift of the clock lands on both
                for mode in modes + modes:
                    r = timed(ctx, d_rays, mode, args.warmup, args.reps)
                    row.setdefault(mode, []).append(r)
                out = {}
                for mode, runs in row.items():
                    best = max(runs, key=lambda r: r["mrays_per_s"])
                    out[mode] = dict(best, blocks_mrays_per_s=[r["mrays_per_s"] for r in runs])
                    out[mode]["vs_megakernel_c3f"] = best["mrays_per_s"] / mega["c3f_mrays_per_s"]
                if "any" in out and "closest" in out:
                    out["any_over_closest"] = out["any"]["mrays_per_s"] / out["closest"]["mrays_per_s"]
                tree["sets"][name] = out
                print(f"{builder:9s} {name:8s} " + "  ".join(
                    f"{m} {out[m]['mrays_per_s']:9.1f} Mrays/s [{out[m]['mrays_per_s_min']:.1f}, "
                    f"{out[m]['mrays_per_s_max']:.1f}] hit {out[m]['hit_frac']:.3f}" for m in modes), flush=True)
                del d_rays
        tree["primary_ray_work"] = primary_ray_work(packed, params, cfg)
        result["trees"][builder] = tree
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"out": args.out, "megakernel_c3f_mrays_per_s": mega["c3f_mrays_per_s"]}))


if __name__ == "__main__":
    main()
