// pt_host.h — host-side structures shared by the translation units of libptamd.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pt_amd.h"

struct Node8;
struct LeafTri;

// the traversal structure on the device: the 8-wide compressed tree (pt_bvh8.h) and what the kernels need to know about it
struct PtBvh {
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    float pad = 0.f; // padding of every box: 2^-16 of the scene's largest |coordinate| (half of it confines hits: pt_bvh.h hit_in_box)
    const Node8* nodes8 = nullptr;
    const LeafTri* tris8 = nullptr;
    uint32_t num_nodes8 = 0, num_tris8 = 0;
    int levels8 = 0; // levels of the wide tree = upper bound of its traversal stack depth (one pushed group per level)
    float calib_cost = 0.f; // node steps + 0.6 x triangle tests per calibration ray through the chosen tree (0: no calibration ran — small scenes, forced builder)
    int challengers_skipped = 0; // candidate hierarchies that could not be built (out of memory, a failed check): the standing tree stayed uncompared
    int builder = 0; // hierarchy under the wide tree: 0 LBVH (Morton order, Karras 2012), 1 PLOC (Meister & Bittner 2018) — chosen by calibration rays unless PT_BVH_BUILDER=lbvh|ploc
    // refit (pt_update_meshes): k_collapse8 emits the wide tree breadth-first, so the nodes of level d are [level_off[d], level_off[d + 1])
    std::vector<uint32_t> level_off;
    float* d_exact = nullptr;  // exact (unpadded) box of every wide node, float[6] x num_nodes8: allocated by the first refit
    uint32_t* d_refit = nullptr; // [0..5] scene bounds as ordered uints (k_bounds), [6] bounds-check fault bits (PT_BVH_CHECK builds)
};

// d_tri_mesh: mesh (= material record) of every triangle, stored with the leaf triangles (may be null: 0)
hipError_t pt_bvh_build(const float* d_verts, const uint32_t* d_idx, const uint32_t* d_tri_mesh, uint32_t ntri, hipStream_t stream, PtBvh* out);
void pt_bvh_free(PtBvh* b);
// Refit of the wide tree over moved vertices, topology kept (pt_update_meshes).  alloc: the refit's side arrays (may fail: nothing has
// changed then); begin: enqueues the scene bounds; the caller then rewrites the leaf triangles (k_refit_leaves); nodes: one launch
// per level, deepest first; end: waits, takes the new bounds and padding, reports a bounds-check fault (PT_BVH_CHECK builds).
hipError_t pt_bvh_refit_alloc(PtBvh* b);
hipError_t pt_bvh_refit_begin(PtBvh* b, const float* d_verts, const uint32_t* d_idx, uint32_t ntri, hipStream_t stream);
hipError_t pt_bvh_refit_nodes(PtBvh* b, hipStream_t stream);
hipError_t pt_bvh_refit_end(PtBvh* b, hipStream_t stream);
void pt_bvh_warm(hipStream_t stream); // first use in a process: loads the code object of pt_bvh_build.hip (see there)
