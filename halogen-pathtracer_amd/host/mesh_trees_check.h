// mesh_trees_check.h — test support for csrc/hg_mesh_trees.h, shared by tests/test_mesh_trees.py's driver and
// host/asan_mesh_trees.cpp: a scene, its pack and its tree bookkeeping side by side, mesh updates applied to the
// bookkeeping as the device path applies them (hg_refit.hip update_mesh) with the host twins hg_build_blas_lbvh /
// hg_build_blas_lbvh_sah standing in for the device build, and after every adopted rebuild the checks of what the
// bookkeeping then says against the twin's tree.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hg_mesh_trees.h"

struct HgTreesHarness {
    // the caller's arrays, kept current as a caller of the rebuilds keeps them: a rebuilt mesh's triangles are the twin's,
    // its entries the twin's (appended: the count differs from the first tree's), for every instance
    std::vector<HalogenSphere> spheres;
    std::vector<HalogenMeshData> meshes;
    std::vector<PackedHalogenMaterial> materials;
    std::vector<HalogenTriangle> tris;
    std::vector<BVHEntry> blas;
    std::vector<HgDevMesh> dm;  // the device mesh table
    HgMeshTrees trees;
    bool has_scene = false;
    int step = 0;

    HgSceneIn in() const {
        return HgSceneIn{spheres.data(), int32_t(spheres.size()), meshes.data(), int32_t(meshes.size()),
                         materials.data(), int32_t(materials.size()), tris.data(), int32_t(tris.size()),
                         blas.data(), int32_t(blas.size())};
    }

    // A full upload: pack, reset.  "" or the packer's refusal
    std::string upload() {
        HgScenePack p;
        HgPackError err;
        if (hg_pack_spheres_materials(in(), p, err) || hg_pack_geometry(in(), p, err)) return err.text;
        dm = p.dm;
        trees.reset(p.rec, p.leaf, int32_t(tris.size()));
        has_scene = true;
        return "";
    }

    struct Snapshot {
        HgMeshTrees trees;
        std::vector<HgDevMesh> dm;
    };
    Snapshot snapshot() const { return Snapshot{trees, dm}; }
    bool same_as(const Snapshot& s) const {
        return trees == s.trees && dm.size() == s.dm.size() &&
               (dm.empty() || !std::memcmp(dm.data(), s.dm.data(), dm.size() * sizeof(HgDevMesh)));
    }

    static std::string refusal(const HgPackError& err) { return "refused " + std::to_string(err.code) + " " + err.text; }
    static std::string bad(const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
        char msg[256];
        std::snprintf(msg, sizeof msg, fmt, a, b);
        return std::string("bad ") + msg;
    }

    // hg_refit_mesh's checks for n triangles; "ok ..." or "refused <code> <text>"
    std::string refit(int32_t mesh, bool have_tris, int32_t n) {
        const HgRefitPlan* plan = nullptr;
        std::vector<int32_t> instances;
        HgPackError err;
        if (trees.check_refit(has_scene, dm, mesh, have_tris, n, plan, instances, err)) return refusal(err);
        return "ok refit instances=" + std::to_string(instances.size()) + " extent=" + std::to_string(plan->extent);
    }

    // The twin's entries as the compact refs the device writes (include/halogen_abi.h): the inner node with new index j
    // is record rec_min + j, its children are the entries 1 + 2j and 2 + 2j, leaves are inline refs at tri_offset
    static std::vector<uint32_t> compact_refs(const std::vector<BVHEntry>& e, uint32_t rec_min, uint32_t tri_offset) {
        const size_t n_records = (e.size() - 1) / 2;
        std::vector<uint32_t> refs(2 * n_records);
        for (size_t j = 0; j < n_records; ++j)
            for (size_t k = 0; k < 2; ++k) {
                const BVHEntry& c = e[1 + 2 * j + k];
                refs[2 * j + k] = c.triangleCount ? HG_LEAF_BIT | (c.triangleCount << HG_LEAF_CNT_SHIFT) | (tri_offset + c.indexA)
                                                  : rec_min + (c.indexA - 1) / 2;
            }
        return refs;
    }

    // A rebuild of `mesh` from n triangles (the mesh's current ones, sheared so that the order changes): the checks,
    // the twin's tree, adopt, and the checks of the result.  how: HG_DEFORM_REBUILD (leaf_size) or _SAH (node_cost).
    std::string rebuild(int32_t mesh, bool have_tris, int32_t n, int how, int32_t leaf_size, float node_cost) {
        std::vector<int32_t> instances;
        HgMeshTrees::Slot slot;
        uint32_t L = 0, K = 0;
        HgPackError err;
        if (how == HG_DEFORM_REBUILD
                ? trees.check_rebuild(has_scene, dm, mesh, have_tris, n, leaf_size, instances, slot, L, K, err)
                : trees.check_rebuild_sah(has_scene, dm, mesh, have_tris, n, node_cost, instances, slot, err))
            return refusal(err);
        const uint32_t toff = dm[size_t(mesh)].tri_offset;
        std::vector<HalogenTriangle> moved(tris.begin() + toff, tris.begin() + toff + n);
        ++step;
        for (HalogenTriangle& t : moved) {
            t.pointA.x += 0.37f * float(step) * t.pointA.y;
            t.pointB.x += 0.37f * float(step) * t.pointB.y;
            t.pointC.x += 0.37f * float(step) * t.pointC.y;
        }
        std::vector<int32_t> order(size_t(n), 0);
        std::vector<HalogenTriangle> sorted(size_t(n), HalogenTriangle{});
        std::vector<BVHEntry> e(size_t(2 * n), BVHEntry{});
        int64_t count;
        if (how == HG_DEFORM_REBUILD) {
            count = hg_build_blas_lbvh(moved.data(), n, int32_t(L), order.data(), sorted.data(), e.data(), int64_t(e.size()));
        } else {
            float used = node_cost;
            count = hg_build_blas_lbvh_sah(moved.data(), n, node_cost, int64_t(slot.capacity), order.data(), sorted.data(),
                                           e.data(), int64_t(e.size()), &used);
            if (count == HG_E_UNSUPPORTED) {  // the device's late refusal, with the count it would report
                if (node_cost == 0.0f) used = hg_lbvh_sah_rung(HG_LBVH_SAH_RUNGS - 1u);
                count = hg_build_blas_lbvh_sah(moved.data(), n, used, -1, order.data(), sorted.data(), e.data(),
                                               int64_t(e.size()), nullptr);
                if (count < 1) return bad("the twin refused without a limit: %llu", (unsigned long long)(-count));
                if (!HgMeshTrees::check_sah_records(mesh, uint32_t((count - 1) / 2), node_cost, used, slot, err))
                    return bad("the twin refused %llu records, the check accepts them", (unsigned long long)((count - 1) / 2));
                return refusal(err);
            }
        }
        if (count < 1) return bad("the twin failed: %llu", (unsigned long long)(-count));
        e.resize(size_t(count));
        const uint32_t n_records = uint32_t((count - 1) / 2);
        if (how == HG_DEFORM_REBUILD && n_records != K - 1) return bad("K - 1 = %llu, the twin has %llu records", K - 1, n_records);
        const std::vector<uint32_t> refs = compact_refs(e, slot.rec_min, toff);
        HgMeshTrees::Adopted got;
        if (trees.adopt(dm, mesh, instances, slot, refs.data(), n_records, uint32_t(n), got, err)) return refusal(err);
        // the caller's arrays follow
        std::copy(sorted.begin(), sorted.end(), tris.begin() + toff);
        const uint32_t at = uint32_t(blas.size());
        blas.insert(blas.end(), e.begin(), e.end());
        for (int32_t j : instances) meshes[size_t(j)].accelerationBufferOffset = at;
        // ---- what the bookkeeping says now
        const uint32_t root = dm[size_t(mesh)].root_ref;
        for (int32_t j : instances)
            if (dm[size_t(j)].root_ref != root) return bad("instance %llu has another root", (unsigned long long)j);
        if (n_records ? root != slot.rec_min : root != (HG_LEAF_BIT | (uint32_t(n) << HG_LEAF_CNT_SHIFT) | toff))
            return bad("root %llu", root);
        const auto kept = trees.slots.find(toff);
        if (kept == trees.slots.end() || !(kept->second == slot)) return bad("the slot changed");
        const auto planned = trees.plans.find(HgMeshTrees::key(dm[size_t(mesh)]));
        if (planned == trees.plans.end() || &planned->second != got.plan) return bad("the plan is not under the new key");
        const HgRefitPlan& plan = *got.plan;
        if (plan.extent != uint32_t(n)) return bad("extent %llu of %llu triangles", plan.extent, (unsigned long long)n);
        if (plan.records.size() != n_records) return bad("%llu records planned of %llu", plan.records.size(), n_records);
        for (uint32_t r : plan.records)
            if (r < slot.rec_min || r - slot.rec_min >= slot.capacity) return bad("record %llu outside the slot", r);
        // the walk of rec_refs from the new root beside the twin's entries: the same leaves in the same order
        struct Item { uint32_t ref, g; };
        std::vector<Item> stack{{root, 0u}};
        uint32_t next_tri = 0, leaves = 0;
        while (!stack.empty()) {
            const Item it = stack.back();
            stack.pop_back();
            const BVHEntry& t = e[it.g];
            if (t.triangleCount) {
                if (it.ref != (HG_LEAF_BIT | (t.triangleCount << HG_LEAF_CNT_SHIFT) | (toff + t.indexA)))
                    return bad("leaf entry %llu: ref %llu", it.g, it.ref);
                if (t.indexA != next_tri) return bad("leaf entry %llu out of order", it.g);
                next_tri += t.triangleCount;
                ++leaves;
            } else {
                if ((it.ref & HG_LEAF_BIT) || it.ref < slot.rec_min || it.ref - slot.rec_min >= n_records)
                    return bad("inner entry %llu: ref %llu", it.g, it.ref);
                stack.push_back({trees.rec_refs[2 * size_t(it.ref) + 1], t.indexA + 1});
                stack.push_back({trees.rec_refs[2 * size_t(it.ref)], t.indexA});
            }
        }
        if (next_tri != uint32_t(n) || leaves != n_records + 1) return bad("the walk covered %llu triangles in %llu leaves", next_tri, leaves);
        // the stack depth is a full upload's of the scene with the twin's triangles and entries in the mesh's place
        HgScenePack p;
        if (hg_pack_spheres_materials(in(), p, err) || hg_pack_geometry(in(), p, err)) return "bad the twin's scene is rejected: " + err.text;
        if (p.stack_depth != got.stack_depth) return bad("stack depth %llu, a full upload's %llu", got.stack_depth, p.stack_depth);
        char line[160];
        std::snprintf(line, sizeof line, "ok rebuild records=%u leaves=%u rec_min=%u capacity=%u depth=%u root_leaf=%d", n_records,
                      leaves, slot.rec_min, slot.capacity, got.stack_depth, int((root & HG_LEAF_BIT) != 0));
        return line;
    }

    // adopt() on records that are not a tree ("cycle": the first record is its own child; "range": a child beyond the
    // scene's records; or the caller's refs, which may be a tree): the failure is reported and nothing but the slot's
    // part of rec_refs has changed.  As on the device, the scene is gone after a failure.
    std::string adopt_bad(int32_t mesh, const std::string& what, const std::vector<uint32_t>* given = nullptr) {
        std::vector<int32_t> instances;
        HgMeshTrees::Slot slot;
        uint32_t L = 0, K = 0;
        HgPackError err;
        if (mesh < 0 || size_t(mesh) >= dm.size()) return bad("no such mesh");
        const HgRefitPlan* plan = trees.plan_of(dm[size_t(mesh)]);
        if (!plan) return bad("no plan");
        const int32_t n = int32_t(plan->extent);
        if (trees.check_rebuild(has_scene, dm, mesh, true, n, 0, instances, slot, L, K, err)) return refusal(err);
        const uint32_t n_records = given ? uint32_t(given->size() / 2) : std::min(slot.capacity, 2u);
        if (n_records == 0 || n_records > slot.capacity) return bad("no records to corrupt");
        const uint32_t toff = dm[size_t(mesh)].tri_offset;
        std::vector<uint32_t> refs(2 * size_t(n_records), HG_LEAF_BIT | (1u << HG_LEAF_CNT_SHIFT) | toff);
        if (given) refs = *given;
        else refs[0] = what == "cycle" ? slot.rec_min : uint32_t(trees.rec_refs.size() / 2) + 7u;
        Snapshot before = snapshot();
        HgMeshTrees::Adopted got;
        if (trees.adopt(dm, mesh, instances, slot, refs.data(), n_records, uint32_t(n), got, err) == HG_OK)
            return given ? "ok adopted" : bad("records that are not a tree were adopted");
        has_scene = false;
        std::copy(trees.rec_refs.begin() + 2 * size_t(slot.rec_min), trees.rec_refs.begin() + 2 * size_t(slot.rec_min + n_records),
                  before.trees.rec_refs.begin() + 2 * size_t(slot.rec_min));
        if (!same_as(before)) return bad("a failed adopt changed more than the slot's refs");
        return refusal(err);
    }
};
