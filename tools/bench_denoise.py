#!/usr/bin/env python3
"""Cost of the denoised display (hg_update_guides, hg_readback_begin_denoised; csrc/hg_denoise.hip) at 1080p on the C3
dragon scene, against the plain display of the same library.  Not part of bench.py.

  guides    ms per hg_update_guides (synchronous: the host clock around the call), stable rays.
  display   steady state, no rendering: `begin; end` one behind (depth 2) over an accumulated image, plain and denoised
            with 1..5 iterations, in each display format; ms per display from the host clock around a block of displays
            (the last end waits for the last copy).  Differences of consecutive iteration counts are the cost of the
            added iteration (step 1, 2, 4, 8, 16) and are set beside its byte floor, 48 B per pixel (two 16-B reads, one
            16-B write).  The same for each block shape of the filter's waves (HALOGEN_ATROUS_TILE).
  loop      the per-frame display loop `render(1); begin; end` one behind, render server on and off, plain and denoised
            (the pass's rule: 3 iterations, sigma_color 8 / sqrt(frames)), R11G11B10F, in Mpaths/s.
Every figure: a warm-up block, then `--blocks` timed blocks per variant, the variants alternating inside each round so
that a drift lands on all of them; median, min and max over the blocks.

  python tools/bench_denoise.py --out profiles/denoise.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch  # noqa: F401  before the library's first context (one HIP runtime in the process)

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "halogen-pathtracer_amd"))

from halogen import abi, render_pass as rp, scenes  # noqa: E402

TILES = {"64x1": "0", "16x4": "1", "8x8": "2"}


def stats(xs):
    xs = np.asarray(xs, float)
    return {"median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max()), "blocks": len(xs)}


def rule(frames, iterations=3):
    return rp.DenoiseSettings(iterations=iterations).params(frames)


def display_block(ctx, W, H, fmt, p, n):
    """n displays, one behind; ms per display."""
    ctx.synchronize()
    t0 = time.perf_counter()
    pending = 0
    for _ in range(n):
        ctx.readback_begin(fmt, denoise=p)
        pending += 1
        if pending == 2:
            ctx.readback_end(W, H, copy=False)
            pending -= 1
    while pending:
        ctx.readback_end(W, H, copy=False)
        pending -= 1
    return (time.perf_counter() - t0) * 1e3 / n


def loop_block(ctx, params, W, H, den, n):
    """n frames of render(1); begin; end one behind, from a cleared accumulation; Mpaths/s."""
    ctx.clear_accumulation()
    ctx.set_params(params)
    ctx.synchronize()
    t0 = time.perf_counter()
    pending = 0
    for k in range(n):
        ctx.render(1, True)
        ctx.readback_begin(abi.HG_DISPLAY_R11G11B10F, denoise=rule(k + 1) if den else None)
        pending += 1
        if pending == 2:
            ctx.readback_end(W, H, copy=False)
            pending -= 1
    while pending:
        ctx.readback_end(W, H, copy=False)
        pending -= 1
    return W * H * n / (time.perf_counter() - t0) / 1e6


def rounds(variants, run, blocks):
    """variants: {name: args}; one warm-up pass, then `blocks` rounds over all variants in turn."""
    for a in variants.values():
        run(*a)
    out = {k: [] for k in variants}
    for _ in range(blocks):
        for k, a in variants.items():
            out[k].append(run(*a))
    return {k: stats(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "denoise.json"))
    ap.add_argument("--config", default="C3")
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--displays", type=int, default=40, help="displays per timed block")
    ap.add_argument("--frames", type=int, default=64, help="frames per timed block of the per-frame loop")
    ap.add_argument("--accumulated", type=int, default=4, help="frames in the image the steady-state displays filter")
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_denoise: no HIP device (times are measured on the GPU or not at all)")
    cfg = scenes.CONFIGS[args.config]
    W, H = cfg.width, cfg.height
    s = rp.clamp_settings(scenes.settings_for(cfg))
    packed = (scenes.dragon_cornell(args.subdiv) if cfg.scene == "dragon" else
              {"cornell": scenes.cornell_box, "glass": scenes.nested_glass}[cfg.scene]()).pack()
    cube = scenes.settings_for(cfg).environmentCubemap if s["UseEnvironmentCubemap"] else None
    params = rp.make_params(s, cfg.camera(), 1, len(packed.spheres), len(packed.meshes), cube is not None)
    stable = abi.HgParams.from_buffer_copy(params)
    stable.filterRadius, stable.focalConeAngle = 0.0, 0.0
    floor_bytes = 48 * W * H
    result = {"metric": f"denoised display at {W}x{H} on {cfg.name} (one MI355X)", "width": W, "height": H,
              "timing": "host clock around blocks that end in a wait for the last copy", "blocks": args.blocks,
              "displays_per_block": args.displays, "frames_per_block": args.frames,
              "iteration_byte_floor": floor_bytes}
    with abi.Context(0) as ctx:
        ctx.set_option(abi.HG_OPT_COUNTERS, 0)  # as the passes run it
        ctx.upload_scene(packed)
        if cube is not None:
            ctx.upload_cubemap(cube.face_size, cube.n_mips, cube.texels)
        ctx.resize(W, H)
        ctx.set_params(params)

        def guides():
            t0 = time.perf_counter()
            ctx.update_guides(stable, 1)
            return (time.perf_counter() - t0) * 1e3

        result["update_guides_ms"] = rounds({"stable_rays": ()}, guides, 4 * args.blocks)["stable_rays"]
        g0, _ = ctx.guides()
        result["guide_hit_fraction"] = float(np.isfinite(g0[..., 3]).mean())
        print(f"update_guides {result['update_guides_ms']['median']:.3f} ms, "
              f"{result['guide_hit_fraction']:.3f} of the pixels hit", flush=True)

        ctx.render(args.accumulated, True)
        ctx.synchronize()
        # steady-state displays: formats x (plain, 3, 5 iterations)
        disp = {}
        for fmt_name, fmt in abi.DISPLAY_FORMATS.items():
            variants = {"plain": (ctx, W, H, fmt, None, args.displays)}
            for it in (3, 5):
                variants[f"denoised_{it}"] = (ctx, W, H, fmt, rule(args.accumulated, it), args.displays)
            disp[fmt_name] = rounds(variants, display_block, args.blocks)
            print(fmt_name, {k: round(v["median"], 3) for k, v in disp[fmt_name].items()}, "ms per display", flush=True)
        result["display_ms"] = disp
        # per iteration, per block shape of the filter's waves (RGBA32F)
        per_tile = {}
        for tile, env in TILES.items():
            os.environ["HALOGEN_ATROUS_TILE"] = env
            variants = {"plain": (ctx, W, H, abi.HG_DISPLAY_RGBA32F, None, args.displays)}
            for it in range(1, 6):
                variants[str(it)] = (ctx, W, H, abi.HG_DISPLAY_RGBA32F, rule(args.accumulated, it), args.displays)
            r = rounds(variants, display_block, args.blocks)
            steps = {}
            for it in range(1, 6):
                prev = r["plain"]["median"] if it == 1 else r[str(it - 1)]["median"]
                ms = r[str(it)]["median"] - prev
                steps[f"step_{1 << (it - 1)}"] = {"ms": ms, "floor_gb_per_s": floor_bytes / ms / 1e6 if ms > 0 else None}
            steps["step_1"]["note"] = "includes the untile + demodulation pass in place of nothing"
            per_tile[tile] = {"ms_per_display": r, "added_iteration": steps}
            print(tile, {k: round(v["ms"], 4) for k, v in steps.items()}, "ms per added iteration", flush=True)
        os.environ.pop("HALOGEN_ATROUS_TILE")
        result["iterations_by_wave_block"] = per_tile
        # the per-frame display loop
        loop = {}
        for server in (1, 0):
            ctx.set_option(abi.HG_OPT_SERVER, server)
            r = rounds({"plain": (ctx, params, W, H, False, args.frames),
                        "denoised_3": (ctx, params, W, H, True, args.frames)}, loop_block, args.blocks)
            r["denoised_over_plain"] = r["denoised_3"]["median"] / r["plain"]["median"]
            loop["server_on" if server else "server_off"] = r
            print(f"per-frame loop, server {server}: plain {r['plain']['median']:.1f} Mpaths/s, denoised "
                  f"{r['denoised_3']['median']:.1f} ({r['denoised_over_plain']:.3f})", flush=True)
        result["per_frame_loop_mpaths_per_s"] = loop
        # ... and with the server on, per block shape of the filter's waves
        ctx.set_option(abi.HG_OPT_SERVER, 1)
        by_tile = {}
        for tile, env in TILES.items():
            os.environ["HALOGEN_ATROUS_TILE"] = env
            by_tile[tile] = rounds({"denoised_3": (ctx, params, W, H, True, args.frames)}, loop_block,
                                   args.blocks)["denoised_3"]
        os.environ.pop("HALOGEN_ATROUS_TILE")
        result["per_frame_loop_server_on_by_wave_block"] = by_tile
        print("per-frame loop, server on, denoised:", {k: round(v["median"], 1) for k, v in by_tile.items()},
              "Mpaths/s", flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
