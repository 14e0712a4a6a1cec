// hg_mesh_trees.h — the host's picture of the device scene's trees, and every decision a mesh update (refit, rebuild,
// deform, skin: hg_refit.hip, hg_lbvh.hip, hg_deform.hip) takes from it before and after its device work.  Plain
// functions of plain arrays and nothing of HIP, in the manner of hg_refit_plan.h and hg_scene_pack.h:
// tests/test_mesh_trees.py and host/asan_mesh_trees.cpp run it with no GPU.  The .hip side keeps the device buffers
// (a tree's plan list among them, under the same key), the launches and fail().
//
// What it holds, from one full upload to the next: the two refs of every node record and the leaf table as the device
// holds them; per tree (root ref << 32 | triangle offset: instances share one) its refit plan, built on first use; per
// rebuilt tree, by its triangle offset (the root ref changes with the tree), the slot of records it had at the upload,
// which is its capacity from then on; the scene's triangle count.  The mesh table (HgDevMesh, hg_layout.h) stays with
// its owner and is handed in.
//
// A refusal is the HG_E_* code plus its text (HgPackError), prefix included: the caller hands both to fail().
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "hg_lbvh.h"
#include "hg_refit_plan.h"
#include "hg_scene_pack.h"

struct HgMeshTrees {
    struct Slot {  // the records [rec_min, rec_min + capacity) a rebuilt tree may use
        uint32_t rec_min = 0, capacity = 0;
        bool operator==(const Slot& o) const { return rec_min == o.rec_min && capacity == o.capacity; }
    };
    std::vector<uint32_t> rec_refs, leaf_table;  // (q0.w, q1.w) per record; (first, count) per leaf-table entry
    std::map<uint64_t, HgRefitPlan> plans;
    std::map<uint32_t, Slot> slots;
    int32_t n_tris = 0;

    static uint64_t key(const HgDevMesh& m) { return (uint64_t(m.root_ref) << 32) | m.tri_offset; }

    void clear() { *this = HgMeshTrees{}; }

    // A full upload laid the records out anew: its records, its leaf table, its triangle count
    void reset(const std::vector<float4>& rec, const std::vector<uint2>& leaf, int32_t scene_tris) {
        clear();
        rec_refs.resize(rec.size() / 2);
        for (size_t r = 0; r < rec.size() / 4; ++r) {
            std::memcpy(&rec_refs[2 * r], &rec[4 * r].w, 4);
            std::memcpy(&rec_refs[2 * r + 1], &rec[4 * r + 1].w, 4);
        }
        leaf_table.resize(leaf.size() * 2);
        if (!leaf.empty()) std::memcpy(leaf_table.data(), leaf.data(), leaf.size() * sizeof(uint2));
        n_tris = scene_tris;
    }

    // The plan of a mesh's tree, built and cached on first use; nullptr: the records are not a tree
    const HgRefitPlan* plan_of(const HgDevMesh& m) {
        auto it = plans.find(key(m));
        if (it == plans.end()) {
            HgRefitPlan plan;
            if (!hg_refit_plan(rec_refs.data(), rec_refs.size() / 2, leaf_table.data(), leaf_table.size() / 2, m.root_ref,
                               m.tri_offset, plan))
                return nullptr;
            it = plans.emplace(key(m), std::move(plan)).first;
        }
        return &it->second;
    }

    // Everything a refit checks before the first device write.  On success: the tree's plan (every other tree's plan is
    // cached too) and the meshes refitted together (the instances of the tree: same root ref, same triangle offset).
    int check_refit(bool has_scene, const std::vector<HgDevMesh>& meshes, int32_t mesh_index, bool have_tris,
                    int32_t tris, const HgRefitPlan*& plan, std::vector<int32_t>& instances, HgPackError& err) {
        const int32_t n_meshes = int32_t(meshes.size());
        if (!has_scene) return hg_pack_fail(err, HG_E_NOSCENE, "hg_refit_mesh: hg_upload_scene not called");
        if (mesh_index < 0 || mesh_index >= n_meshes)
            return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: mesh_index %d out of range (%d meshes)", mesh_index,
                                n_meshes);
        if (!have_tris) return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: null triangle array");
        if (tris < 0) return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: negative triangle count");
        const HgDevMesh& dm = meshes[size_t(mesh_index)];
        if (!(plan = plan_of(dm)))
            return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: mesh %d: the device records are not a tree", mesh_index);
        if (uint32_t(tris) < plan->extent)
            return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: mesh %d: %d triangles, its tree's leaves reach %u",
                                mesh_index, tris, plan->extent);
        if (uint64_t(dm.tri_offset) + uint64_t(tris) > uint64_t(n_tris))
            return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: mesh %d: triangles %u + %d past the scene's %d",
                                mesh_index, dm.tri_offset, tris, n_tris);
        instances.clear();
        const uint64_t lo = dm.tri_offset, hi = lo + uint64_t(tris);
        for (int32_t j = 0; j < n_meshes; ++j) {
            const HgDevMesh& o = meshes[size_t(j)];
            if (key(o) == key(dm)) {
                instances.push_back(j);
                continue;
            }
            // another tree over some of these triangles would go stale
            const HgRefitPlan* other = plan_of(o);  // (std::map: `plan` stays valid)
            if (!other)
                return hg_pack_fail(err, HG_E_INVALID, "hg_refit_mesh: mesh %d: the device records are not a tree", j);
            const uint64_t olo = o.tri_offset, ohi = olo + other->extent;
            if (olo < hi && lo < ohi)
                return hg_pack_fail(err, HG_E_UNSUPPORTED,
                                    "hg_refit_mesh: mesh %d shares triangles with mesh %d, which has another tree",
                                    mesh_index, j);
        }
        return HG_OK;
    }

    // What a rebuild with leaves of a fixed size checks before the first device write: a refit's checks, then its own.
    // On success also the tree's slot, the leaf size L (leaf_size 0: the smallest from 4 that fits) and the K leaves.
    int check_rebuild(bool has_scene, const std::vector<HgDevMesh>& meshes, int32_t mesh_index, bool have_tris,
                      int32_t tris, int32_t leaf_size, std::vector<int32_t>& instances, Slot& slot, uint32_t& L,
                      uint32_t& K, HgPackError& err) {
        const HgRefitPlan* plan = nullptr;
        if (int rc = check_refit(has_scene, meshes, mesh_index, have_tris, tris, plan, instances, err)) return rc;
        if (leaf_size < 0 || leaf_size > int32_t(HG_LBVH_MAX_LEAF))
            return hg_pack_fail(err, HG_E_INVALID, "hg_rebuild_mesh: leaf_size %d outside 0..%u", leaf_size,
                                HG_LBVH_MAX_LEAF);
        if (int rc = check_rebuild_common(meshes[size_t(mesh_index)], mesh_index, tris, *plan, slot, err)) return rc;
        L = leaf_size ? uint32_t(leaf_size) : hg_lbvh_auto_leaf(uint32_t(tris), slot.capacity);
        if (L == 0)
            return hg_pack_fail(err, HG_E_UNSUPPORTED,
                                "hg_rebuild_mesh: mesh %d: no leaf size up to %u fits %d triangles into %u records",
                                mesh_index, HG_LBVH_MAX_LEAF, tris, slot.capacity);
        K = hg_lbvh_leaf_count(uint32_t(tris), L);
        if (K - 1 > slot.capacity)
            return hg_pack_fail(err, HG_E_UNSUPPORTED,
                                "hg_rebuild_mesh: mesh %d: %u records at leaf size %u, the tree's capacity is %u",
                                mesh_index, K - 1, L, slot.capacity);
        return HG_OK;
    }

    // What a rebuild with leaves chosen by surface area checks before the first device launch: a refit's checks, the
    // node cost, what every rebuild checks.  (Whether the live records fit is known only after the collapse on the
    // device: check_sah_records.)
    int check_rebuild_sah(bool has_scene, const std::vector<HgDevMesh>& meshes, int32_t mesh_index, bool have_tris,
                          int32_t tris, float node_cost, std::vector<int32_t>& instances, Slot& slot, HgPackError& err) {
        const HgRefitPlan* plan = nullptr;
        if (int rc = check_refit(has_scene, meshes, mesh_index, have_tris, tris, plan, instances, err)) return rc;
        if (!(node_cost >= 0.0f) || node_cost == hg_u2f(0x7F800000u))
            return hg_pack_fail(err, HG_E_INVALID, "hg_rebuild_mesh_sah: node_cost %g is negative or not finite",
                                double(node_cost));
        return check_rebuild_common(meshes[size_t(mesh_index)], mesh_index, tris, *plan, slot, err);
    }

    // The one late refusal of a rebuild by surface area, still before the first write to the scene: `n_live` records,
    // the device's count at node cost `used` (the caller's, or for node_cost == 0 the last rung of the ladder), against
    // the slot
    static int check_sah_records(int32_t mesh_index, uint32_t n_live, float node_cost, float used, const Slot& slot,
                                 HgPackError& err) {
        if (n_live <= slot.capacity) return HG_OK;
        if (node_cost == 0.0f)
            return hg_pack_fail(err, HG_E_UNSUPPORTED,
                                "hg_rebuild_mesh_sah: mesh %d: %u records at node cost %g, the last of the ladder; the "
                                "tree's capacity is %u", mesh_index, n_live, double(used), slot.capacity);
        return hg_pack_fail(err, HG_E_UNSUPPORTED,
                            "hg_rebuild_mesh_sah: mesh %d: %u records at node cost %g, the tree's capacity is %u",
                            mesh_index, n_live, double(used), slot.capacity);
    }

    struct Adopted {
        uint64_t old_key = 0, new_key = 0;  // of the tree: its device list moves from one to the other
        const HgRefitPlan* plan = nullptr;  // the new tree's
        uint32_t stack_depth = 2;           // the scene's, over all trees: what a full upload with this tree sets
    };

    // A rebuilt tree: the device wrote `n_records` records from slot.rec_min on, whose refs are `refs` (2 per record,
    // compact), over `tris` triangles.  Writes them into rec_refs, plans the tree under its new root (record
    // slot.rec_min, or one inline leaf for no records), moves the tree to its new key, sets the root of every instance
    // and keeps the slot.  HG_E_INVALID: the records are not a tree (cannot happen for sorted keys); then the slot's
    // part of rec_refs holds them and nothing else has changed.  `instances`: check_rebuild*'s, of this state.
    // (More records than the slot holds, or a slot past rec_refs, get the same answer before anything is copied: a
    // guard of the copy for callers other than the device path, whose checks bound n_records and which cannot reach it.)
    int adopt(std::vector<HgDevMesh>& meshes, int32_t mesh_index, const std::vector<int32_t>& instances, const Slot& slot,
              const uint32_t* refs, uint32_t n_records, uint32_t tris, Adopted& out, HgPackError& err) {
        const HgDevMesh first = meshes[size_t(instances[0])];
        if (n_records > slot.capacity || size_t(slot.rec_min) + n_records > rec_refs.size() / 2)
            return hg_pack_fail(err, HG_E_INVALID,
                                "hg_rebuild_mesh: mesh %d: the rebuilt records are not a tree; upload the scene again",
                                mesh_index);
        if (n_records) std::memcpy(&rec_refs[size_t(slot.rec_min) * 2], refs, size_t(n_records) * 2 * sizeof(uint32_t));
        const uint32_t root = n_records ? slot.rec_min : (HG_LEAF_BIT | (tris << HG_LEAF_CNT_SHIFT) | first.tri_offset);
        HgRefitPlan plan;
        if (!hg_refit_plan(rec_refs.data(), rec_refs.size() / 2, leaf_table.data(), leaf_table.size() / 2, root,
                           first.tri_offset, plan))
            return hg_pack_fail(err, HG_E_INVALID,
                                "hg_rebuild_mesh: mesh %d: the rebuilt records are not a tree; upload the scene again",
                                mesh_index);
        slots[first.tri_offset] = slot;
        out.old_key = key(first);
        plans.erase(out.old_key);
        for (int32_t j : instances) meshes[size_t(j)].root_ref = root;
        out.new_key = key(meshes[size_t(instances[0])]);
        out.plan = &(plans[out.new_key] = std::move(plan));
        uint32_t max_depth = 0;
        for (const HgDevMesh& m : meshes)
            if (const HgRefitPlan* p = plan_of(m))
                if (!p->level_off.empty()) max_depth = std::max(max_depth, uint32_t(p->level_off.size() - 1));
        out.stack_depth = hg_stack_depth(max_depth);
        return HG_OK;
    }

    bool operator==(const HgMeshTrees& o) const {
        auto same_plan = [](const HgRefitPlan& a, const HgRefitPlan& b) {
            return a.records == b.records && a.level_off == b.level_off && a.rec_min == b.rec_min &&
                   a.rec_span == b.rec_span && a.extent == b.extent;
        };
        return rec_refs == o.rec_refs && leaf_table == o.leaf_table && slots == o.slots && n_tris == o.n_tris &&
               plans.size() == o.plans.size() &&
               std::equal(plans.begin(), plans.end(), o.plans.begin(), [&](const auto& a, const auto& b) {
                   return a.first == b.first && same_plan(a.second, b.second);
               });
    }

private:
    // What both kinds of rebuild check after a refit's checks and their own argument's: the triangle count, the range
    // of inline leaf refs; and the tree's slot of records
    int check_rebuild_common(const HgDevMesh& dm, int32_t mesh_index, int32_t tris, const HgRefitPlan& plan, Slot& slot,
                             HgPackError& err) const {
        if (uint32_t(tris) != plan.extent || tris == 0)
            return hg_pack_fail(err, HG_E_INVALID, "hg_rebuild_mesh: mesh %d: %d triangles, its tree holds %u", mesh_index,
                                tris, plan.extent);
        if (uint64_t(dm.tri_offset) + uint64_t(tris) > uint64_t(HG_LBVH_MAX_TRIS))
            return hg_pack_fail(err, HG_E_UNSUPPORTED,
                                "hg_rebuild_mesh: mesh %d: triangles %u + %d past 2^27 (inline leaves only)", mesh_index,
                                dm.tri_offset, tris);
        auto it = slots.find(dm.tri_offset);
        if (it != slots.end()) {
            slot = it->second;
        } else {  // not rebuilt since the last full upload: the plan is the uploaded tree's
            slot.rec_min = plan.records.empty() ? 0u : plan.rec_min;
            slot.capacity = plan.records.empty() ? 0u : plan.rec_span;
        }
        return HG_OK;
    }
};
