#!/usr/bin/env python3
"""Cost of one pose of the C3 dragon (871,200 triangles) from where a caller holds it, the vertices, by each way to get
it onto the device (hg_deform_mesh_device, hg_skin_mesh_device; csrc/hg_deform.hip).  Not part of bench.py.

  a_host_pack    RayTracingMesh.deform on the host (hg_pack_triangles + hg_refit_blas) + hg_refit_mesh from host memory
                 (72 B a triangle over the bus)
  b_torch_gather a torch gather of device vertices through a device index list into an (n, 18) tensor +
                 hg_refit_mesh_device
  c_deform       hg_deform_mesh_device from the same device vertices (the library's pack kernel and bound index list)
  d_skin         hg_skin_mesh_device from a device bone palette (the skin kernel, then c's path)
and the same four with a rebuild with leaves chosen by surface area in place of the refit (`*_sah`; a and b then also
permute the caller's own index list by the returned order, which c and d leave to the library; a packs on the host and
rebuilds from host memory, without the host twin of the rebuild).

Legs a and b use only entry points the library had before; their code is the same in this build.  Every call is
synchronous: the host clock around it.  The legs alternate inside each block (a drift lands on all of them), each leg has
a context of its own (a rebuild changes the device's triangle order) and sees two poses in turn.  Median, min and max
over the blocks.

  python tools/bench_deform.py --out profiles/deform.json
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

from halogen import abi, scenes  # noqa: E402


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


def palette(n_bones, seed, swing):
    """n_bones rigid bones (12 floats, row-major 3 x 4): small rotations about y and small translations"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_bones, 3, 4), np.float32)
    for k in range(n_bones):
        a = rng.uniform(-swing, swing)
        out[k, :, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        out[k, :, 3] = rng.uniform(-0.02, 0.02, 3)
    return out.reshape(n_bones, 12)


class Leg:
    """One way to pose the dragon, on a context of its own"""

    def __init__(self, packed, di, mesh):
        self.ctx = abi.Context(0)
        self.ctx.set_option(abi.HG_OPT_COUNTERS, 0)
        self.ctx.upload_scene(packed)
        self.di, self.turn = di, 0
        self.idx = mesh.triangles.copy()                              # the caller's own index list, host ...
        self.d_idx = torch.from_numpy(self.idx.astype(np.int64)).to("cuda:0")  # ... and device
        self.n_tris = len(self.idx)

    def next(self, poses):
        self.turn ^= 1
        return poses[self.turn]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deform.json"))
    ap.add_argument("--subdiv", type=int, default=10, help="dragon subdivision (10: the 871,200-triangle C3 dragon)")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--sah-blocks", type=int, default=5)
    ap.add_argument("--bones", type=int, default=64)
    args = ap.parse_args()
    if not abi.gpu_available():
        sys.exit("bench_deform: no HIP device (times are measured on the GPU or not at all)")
    sc = scenes.dragon_cornell(args.subdiv)
    di = len(sc.meshes) - 1
    dragon = sc.meshes[di]
    rest_v, rest_n = dragon.vertices.copy(), dragon.normals.copy()
    nv, n_tris = len(rest_v), dragon.triangle_count
    packed = sc.pack()
    poses = []
    for strength in (0.05, 0.1):  # two small poses in turn: every call moves every vertex
        v = twist(rest_v, strength)
        poses.append({"v": v, "n": rest_n, "dv": torch.from_numpy(v).to("cuda:0"), "dn": torch.from_numpy(rest_n).to("cuda:0")})
    rng = np.random.default_rng(1)
    bone_idx = rng.integers(0, args.bones, (nv, 4)).astype(np.uint16)
    weights = rng.uniform(0, 1, (nv, 4))
    weights = (weights / weights.sum(axis=1, keepdims=True)).astype(np.float32)
    palettes = [torch.from_numpy(palette(args.bones, k, 0.05 * (k + 1))).to("cuda:0") for k in range(2)]
    L = abi.lib()
    host_tris = (abi.HalogenTriangle * n_tris)()

    def make(skin=False):
        leg = Leg(packed, di, dragon)
        if skin is not None:
            leg.ctx.set_mesh_vertices(di, leg.idx, nv)
        if skin:
            leg.ctx.set_mesh_skin(di, rest_v, rest_n, bone_idx, weights, args.bones)
        return leg

    # ---- refit -------------------------------------------------------------------------------------------------------
    legs = {"a_host_pack": make(None), "b_torch_gather": make(None), "c_deform": make(), "d_skin": make(True)}

    def a_refit(leg=legs["a_host_pack"]):
        p = leg.next(poses)
        dragon.deform(p["v"], p["n"])
        leg.ctx.refit_mesh(di, dragon.packed_triangles)

    def b_refit(leg=legs["b_torch_gather"]):
        p = leg.next(poses)
        tris = torch.cat([p["dv"][leg.d_idx].reshape(-1, 9), p["dn"][leg.d_idx].reshape(-1, 9)], dim=1)
        leg.ctx.refit_mesh(di, tris)

    def c_refit(leg=legs["c_deform"]):
        p = leg.next(poses)
        leg.ctx.deform_mesh(di, p["dv"], p["dn"])

    def d_refit(leg=legs["d_skin"]):
        leg.ctx.skin_mesh(di, leg.next(palettes))

    refit = {"a_host_pack": a_refit, "b_torch_gather": b_refit, "c_deform": c_refit, "d_skin": d_refit}
    for fn in refit.values():
        fn()
        fn()
    out = {k: [] for k in refit}
    for _ in range(args.blocks):
        for k, fn in refit.items():
            out[k].append(clock(fn))
    result = {"metric": "one pose of the C3 dragon from its vertices (one MI355X)", "triangles": n_tris, "vertices": nv,
              "bones": args.bones, "timing": "host clock around synchronous calls, legs alternating inside each block",
              "bytes_over_the_bus": {"a_host_pack": n_tris * 72, "b_torch_gather": 0, "c_deform": 0, "d_skin": 0,
                                     "vertices_if_from_the_host": nv * 24},
              "ms_refit": {k: stats(v) for k, v in out.items()}}
    # the three legs that saw the same poses hold the same device scene
    want = {k: legs["a_host_pack"].ctx.scene_readback(k) for k in ("nodes", "tris", "normals", "meshes")}
    for name in ("b_torch_gather", "c_deform"):
        for k, w in want.items():
            assert np.array_equal(legs[name].ctx.scene_readback(k), w), (name, k)
    result["same_device_scene"] = ["a_host_pack", "b_torch_gather", "c_deform"]
    print({k: round(v["median"], 3) for k, v in result["ms_refit"].items()}, "ms per refit pose", flush=True)

    # ---- rebuild with leaves chosen by surface area ---------------------------------------------------------------------
    def a_sah(leg=legs["a_host_pack"]):
        p = leg.next(poses)
        L.hg_pack_triangles(p["v"].ctypes.data, p["n"].ctypes.data, nv, leg.idx.ctypes.data, n_tris,
                            C.cast(host_tris, C.c_void_p))
        order = leg.ctx.rebuild_mesh_sah(di, host_tris, 0.0)
        leg.idx = np.ascontiguousarray(leg.idx[order])

    def b_sah(leg=legs["b_torch_gather"]):
        p = leg.next(poses)
        tris = torch.cat([p["dv"][leg.d_idx].reshape(-1, 9), p["dn"][leg.d_idx].reshape(-1, 9)], dim=1)
        order = leg.ctx.rebuild_mesh_sah(di, tris, 0.0)
        leg.d_idx = leg.d_idx[order.long()]

    def c_sah(leg=legs["c_deform"]):
        p = leg.next(poses)
        leg.ctx.deform_mesh(di, p["dv"], p["dn"], how="sah")

    def d_sah(leg=legs["d_skin"]):
        leg.ctx.skin_mesh(di, leg.next(palettes), how="sah")

    sah = {"a_host_pack": a_sah, "b_torch_gather": b_sah, "c_deform": c_sah, "d_skin": d_sah}
    for fn in sah.values():
        fn()
        fn()
    out = {k: [] for k in sah}
    for _ in range(args.sah_blocks):
        for k, fn in sah.items():
            out[k].append(clock(fn))
    result["ms_rebuild_sah"] = {k: stats(v) for k, v in out.items()}
    want = {k: legs["b_torch_gather"].ctx.scene_readback(k) for k in ("tris", "normals")}
    for k, w in want.items():
        assert np.array_equal(legs["c_deform"].ctx.scene_readback(k), w), k
        assert np.array_equal(legs["a_host_pack"].ctx.scene_readback(k), w), k
    print({k: round(v["median"], 3) for k, v in result["ms_rebuild_sah"].items()}, "ms per rebuilt pose", flush=True)
    for leg in legs.values():
        leg.ctx.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"out": args.out}))


if __name__ == "__main__":
    main()
