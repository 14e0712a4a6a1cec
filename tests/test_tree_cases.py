"""The hand-built scenes of tests/tree_cases.py are what they claim to be, shown on the CPU alone (the oracle and the
scene-pack driver of tests/test_scene_pack.py): the chain is as deep as hg_pack_geometry accepts and most camera rays
climb all of it, every rung of the leaf ladder is seen, the ties are ties, every transformed instance is seen from both
sides.  tests/test_gpu_trees.py then traces them on every kernel.  Also here: hgo_intersect_batch and hgo_camera_rays,
the oracle exports those tests compare the queries with, against the oracle's own debug views and miss counter."""
import ctypes as C

import numpy as np
import pytest

import hg_oracle
import tree_cases as tc
from halogen import abi
from test_refit import driver as refit_driver, write_scene as refit_write_scene  # noqa: F401  (fixtures, both drivers)
from test_scene_pack import driver, parse, write_scene  # noqa: F401

F = np.float32
INF = F(np.inf)


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


@pytest.fixture(scope="module")
def camera(built):
    """Per case: the camera rays of frame 1 and the oracle's hits for them."""
    out = {}
    for name in tc.CASES:
        c = tc.case(name)
        rays = hg_oracle.camera_rays(c.params(1), 1, tc.all_pixels())
        out[name] = dict(rays=rays, hits=hg_oracle.intersect_batch(c.packed, rays))
    return out


# ---- chain62 -----------------------------------------------------------------------------------------------------------
def test_chain62_is_the_deepest_accepted_tree(built, driver):
    c = tc.case("chain62")
    v = parse(driver("pack", write_scene(driver, c.packed)))
    assert v["walk"] == "ok" and v["stack_depth"] == "64" and v["max_depth"] == "62", v
    deeper = tc.chain_case(63)  # one level more is refused
    assert driver("pack", write_scene(driver, deeper.packed)).startswith(f"error {abi.HG_E_UNSUPPORTED} ")
    m = c.packed.meshes
    assert m[1].accelerationBufferOffset == m[2].accelerationBufferOffset == 1
    assert m[1].triangleBufferOffset == m[2].triangleBufferOffset == 2


def test_chain62_refit_plan_is_the_tallest(built, refit_driver):
    """The refit plan (csrc/hg_refit_plan.h, the driver of tests/test_refit.py) has one level per height: 62 here, one
    record each, the same plan for both instances."""
    out = refit_driver("plan", refit_write_scene(refit_driver, tc.case("chain62").packed))
    assert out[-1].startswith("ok "), out
    per_mesh = [dict(kv.split("=") for kv in line.split()[2:]) for line in out[:-1]]
    assert per_mesh[0]["records"] == "0" and per_mesh[1] == per_mesh[2], per_mesh
    n_tris = tc.case("chain62").info["chain_tris"][1]
    assert n_tris == 126 and tc.case("chain62").info["chain_nodes"][1] == 125
    assert (per_mesh[1]["records"], per_mesh[1]["levels"], per_mesh[1]["extent"]) == ("62", "62", str(n_tris)), per_mesh[1]


def test_chain62_camera_rays_climb_the_whole_chain(built):
    """Camera rays only (maxBounces 0), through the stats build.  From the front the oracle's stack reaches 63 entries
    (its convention: the count before a pop) and more than half of the camera rays outgrow the reference's 32; from
    behind the first instance no traversal holds more than 4."""
    c = tc.case("chain62")
    frames = 2
    hg_oracle.stack_stats(reset=True)
    _, cnt = hg_oracle.render(c.packed, c.params(1, MaxBounces=0), frames, True, stats=True)
    over, deepest = hg_oracle.stack_stats(reset=True)
    assert cnt["rays"] == cnt["paths"] == tc.W * tc.H * frames
    print(f"front: deepest {deepest}, {over} of {cnt['rays']} camera rays outgrow 32")
    assert deepest >= 62 and 2 * over >= cnt["rays"], (deepest, over, cnt["rays"])
    _, cnt = hg_oracle.render(c.packed, c.params(1, camera=c.info["behind"], MaxBounces=0), frames, True, stats=True)
    over, deepest = hg_oracle.stack_stats(reset=True)
    print(f"behind: deepest {deepest}, {over} outgrow 32, {cnt['hits']} of {cnt['rays']} hit")
    assert deepest <= 4 and over == 0 and cnt["hits"] > cnt["rays"] // 2, (deepest, over, cnt)


def test_chain62_hits_land_on_many_leaves_of_both_instances(camera):
    h = camera["chain62"]["hits"]
    hit = h["kind"] == abi.HG_HIT_MESH
    assert len(np.unique(h["primitive"][hit & (h["object"] == 1)])) >= 30
    assert (hit & (h["object"] == 2)).sum() >= 50 and (~hit).sum() >= 10
    # the first instance is met from its front, the turned one from behind
    assert np.all(h["orientation"][hit & (h["object"] == 1)] != h["orientation"][hit & (h["object"] == 2)][0])


# ---- leaf_ladder -------------------------------------------------------------------------------------------------------
def test_leaf_ladder_splits_at_the_inline_limit_and_every_leaf_is_seen(camera, driver):
    c = tc.case("leaf_ladder")
    v = parse(driver("pack", write_scene(driver, c.packed)))
    small, large = sum(n <= 15 for n in tc.LADDER), sum(n > 15 for n in tc.LADDER)
    assert (small, large) == (15, 9) and {15, 16, 64, 65} <= set(tc.LADDER)
    assert v["walk"] == "ok" and int(v["inline"]) == small and int(v["table"]) == large, v
    h = camera["leaf_ladder"]["hits"]
    first = np.array(c.info["leaf_first"])
    assert sorted(c.info["leaf_count"]) == tc.LADDER
    leaf = np.searchsorted(first, h["primitive"][h["kind"] == abi.HG_HIT_MESH], side="right") - 1
    seen = np.bincount(leaf, minlength=len(first))
    assert np.all(seen > 0), seen


# ---- ties ----------------------------------------------------------------------------------------------------------------
def candidates(packed):
    """(mesh, triangle index in the scene's array) in the reference's test order when all boxes tie: meshes in buffer
    order, within an entry child A before child B."""
    nodes = tc.bvh_np(packed)
    out = []
    for mi, m in enumerate(packed.meshes):
        todo = [m.accelerationBufferOffset]
        while todo:
            e = nodes[todo.pop()]
            if e["count"]:
                out += [(mi, m.triangleBufferOffset + int(e["indexA"]) + k) for k in range(int(e["count"]))]
            else:
                ia = m.accelerationBufferOffset + int(e["indexA"])
                todo += [ia + 1, ia]
    return np.array(out)


def test_ties_are_ties(camera):
    """With hgo_tri_accept_batch over every (camera ray, mesh, triangle): at least 5 % of the rays have two or more
    accepted triangles at the minimal t; the oracle names the first of them in its test order; no zero-area triangle is
    accepted by any ray, camera or special."""
    c = tc.case("ties")
    packed = c.packed
    eye = np.eye(4, dtype=F).T.reshape(-1)
    for m in packed.meshes:  # identity matrices: the mesh-local ray is the world ray
        assert np.array_equal(np.array(m.worldToLocal.m[:], F).view(np.uint32), eye.view(np.uint32))
    nodes = tc.bvh_np(packed)
    t_root = nodes[3]
    kids = nodes[[3 + t_root["indexA"], 4 + t_root["indexA"]]]
    assert kids["count"].tolist() == [0, 0] and kids[0]["lo"].tobytes() == kids[1]["lo"].tobytes() and \
        kids[0]["hi"].tobytes() == kids[1]["hi"].tobytes()  # identical sibling boxes, inner entries
    cand = candidates(packed)
    assert len(cand) == 3 + 43 + 43
    tris = tc.tris_np(packed)
    fn = hg_oracle.lib().hgo_tri_accept_batch
    fn.restype, fn.argtypes = None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    zero_area = c.info["zero_area"]
    assert len(zero_area) == 3
    specials = tc.special_rays(c, camera["ties"])
    for what, rays in (("camera", camera["ties"]["rays"]), ("special", specials)):
        r8 = np.ascontiguousarray(rays).view(F).reshape(-1, 8)
        n, m = len(r8), len(cand)
        r7 = np.empty((n, m, 7), F)
        r7[:, :, 0:3], r7[:, :, 3:6], r7[:, :, 6] = r8[:, None, 0:3], r8[:, None, 4:7], INF
        t18 = np.ascontiguousarray(np.broadcast_to(tris[cand[:, 1]], (n, m, 18))).reshape(-1, 18)
        out = np.empty((n * m, 5), np.uint32)
        fn(r7.ctypes.data, t18.ctypes.data, out.ctypes.data, n * m)
        out = out.reshape(n, m, 5)
        t = np.where(out[:, :, 0] != 0, out[:, :, 1].view(F), INF)
        assert not np.isfinite(t[:, np.isin(cand[:, 1], zero_area)]).any(), what
        hits = hg_oracle.intersect_batch(packed, rays)
        assert not np.isin(hits["primitive"][hits["kind"] == abi.HG_HIT_MESH], zero_area).any(), what
        if what != "camera":
            continue
        tmin = t.min(axis=1)
        tied = np.isfinite(tmin) & ((t == tmin[:, None]).sum(axis=1) >= 2)
        print(f"ties: {int(tied.sum())} of {n} camera rays have two or more accepted triangles at the minimal t")
        assert tied.sum() >= 0.05 * n
        hit = hits["kind"] == abi.HG_HIT_MESH
        assert np.array_equal(hit, np.isfinite(tmin))
        first = t.argmin(axis=1)  # the first index of the minimum
        assert np.array_equal(hits["t"][hit].view(np.uint32), tmin[hit].view(np.uint32))
        assert np.array_equal(hits["object"][hit], cand[first[hit], 0])
        assert np.array_equal(hits["primitive"][hit], cand[first[hit], 1])
        # the winners include copies in the first mesh, in leaf A and in the later leaves
        t_leaf = np.searchsorted([3, 23, 29, 45], hits["primitive"][hit & (hits["object"] == 1)], side="right")
        assert (hits["object"][hit] == 0).any() and {1, 2, 3} <= set(t_leaf.tolist()), np.bincount(t_leaf)
        assert not (hits["object"][hit] == 2).any()  # the second instance never wins a tie


# ---- transforms ----------------------------------------------------------------------------------------------------------
def test_transforms_every_instance_is_seen_from_both_sides(camera):
    c = tc.case("transforms")
    l2w = [np.array(m.localToWorld.m[:], np.float64).reshape(4, 4).T for m in c.packed.meshes]
    det = [np.linalg.det(m[:3, :3]) for m in l2w]
    assert det[1] < 0 and all(d > 0 for k, d in enumerate(det) if k != 1)
    sv = np.linalg.svd(l2w[2][:3, :3], compute_uv=False)
    assert sv.max() / sv.min() > 0.9e6
    h = camera["transforms"]["hits"]
    hit = h["kind"] == abi.HG_HIT_MESH
    for k, name in enumerate(tc.TRANSFORM_NAMES):
        on = hit & (h["object"] == k)
        sides = set(h["orientation"][on].tolist())
        print(f"{name}: {int(on.sum())} camera rays, orientations {sorted(sides)}")
        assert on.sum() >= 5, name
        if k < 2:
            assert sides == {1.0, -1.0}, name
    assert np.all(h["material"][hit] == h["object"][hit])


# ---- the oracle's query exports against its renders ---------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.CASES)
def test_intersect_batch_names_what_the_debug_views_show(built, name):
    """hgo_camera_rays + hgo_intersect_batch at frame 3 against the oracle's Normal and Albedo views and its primary-miss
    counter (one accumulated frame at FrameCount 3 into a cleared target: c * (1 / 3), AccumulationShader.shader:33)."""
    c = tc.case(name)
    hits = hg_oracle.intersect_batch(c.packed, hg_oracle.camera_rays(c.params(3), 3, tc.all_pixels()))
    hit = hits["kind"] != abi.HG_HIT_NONE
    assert hit.any() and (~hit).any() and np.all(hits["t"][~hit] == INF) and not words(hits)[~hit, 1:].any()
    w = F(1.0) / F(3.0)
    blended = lambda x: F(0.0) * (F(1.0) - w) + x.astype(F) * w
    albedo = np.array([[m.albedo.x, m.albedo.y, m.albedo.z] for m in c.packed.materials], F)
    for mode, want in (("Normal", (hits["normal"] + F(1.0)) / F(2.0)), ("Albedo", albedo[hits["material"]])):
        img, _ = hg_oracle.render(c.packed, c.params(3, DebugMode=mode), 1, True)
        got = img.reshape(-1, 4)[:, :3]
        bad = np.flatnonzero(hit & np.any(got.view(np.uint32) != blended(want).view(np.uint32), axis=1))
        assert bad.size == 0, (name, mode, bad[:8])
    _, cnt = hg_oracle.render(c.packed, c.params(3, MaxBounces=0), 1, True)
    assert cnt["primary_misses"] == int((~hit).sum())


def test_intersect_batch_seeds_the_closest_distance_with_t_max(camera):
    c = tc.case("leaf_ladder")
    rays, hits = camera["leaf_ladder"]["rays"], camera["leaf_ladder"]["hits"]
    hit = hits["kind"] != 0
    for scale, found in ((0.5, False), (2.0, True)):
        cut = rays.copy()
        cut["t_max"] = np.where(hit, hits["t"] * F(scale), F(1.0))
        got = hg_oracle.intersect_batch(c.packed, cut)
        if found:
            assert np.array_equal(words(got), words(hits))
        else:
            assert not got["kind"].any() and np.all(got["t"] == INF) and not words(got)[:, 1:].any()
