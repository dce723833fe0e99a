// pair_tree.hpp -- the host half of a scene upload (scene_upload.cpp is the device half): a desc's
// LinearBVHNode array (BVH.h:63-72) -> child-pair nodes, dTriangle (Triangle.h:11-23, 288 B) -> 48-B
// intersection + 48-B shading records, and the collapse of a pair tree into 4-wide nodes.  No HIP
// runtime call: everything here runs, and is tested (tests/test_pair_tree_host.py), without a device.
#pragma once
#include <string>
#include <vector>

#include "kernels.hpp"
#include "mcpt.h"

namespace mcpt_host {

// The child-pair tree of a desc.  A pair node is 4 float4: per axis (min child 0, min child 1, max
// child 0, max child 1), then (ref 0, ref 1, margin 0, margin 1) -- refs as int bits: >= 0 a pair
// index, the sign bit a leaf (low 24 bits: first record), -1 no child; the margins are the device's
// (launch_cull_margins) and 0 here.
struct PairTree {
    std::vector<float4> pairs;  // the desc's interior nodes in the numbering of `layout` (layout 3: pad
                                // nodes, both refs -1, that nothing references), then the expansion pairs
    int root_ref = 0;           // 0 for a desc without nodes
    int depth = 0;              // the most pair nodes on a root-to-leaf path
    int layout = 0;             // the numbering used: the request, or 0 for an input that is not a tree
    bool contained = true;      // every node box contains its subtree's vertices (what culling needs)
    bool nested = true;         // ... and every child box lies inside its parent's (the occluder cache)
};

// The checks on a desc that need no BVH walk, in the order they fire.  needs_bvh: triangles need nodes
// (a host-BVH upload; a device build ignores the desc's BVH arrays).
bool validate_desc(const mcpt_scene_desc& d, bool needs_bvh, std::string& err);

// validate_desc, the BVH's validation and the tree.  layout_request: -1 by size (2 for trees of at most
// 2 MiB of pair nodes, else 0), or 0-3.  false: err has the first failing check's message.
bool build_pair_tree(const mcpt_scene_desc& d, int layout_request, PairTree& out, std::string& err);

// The records of every triangle in desc order: tri (kTriF4 float4 each) and sh (3 float4 each)
void pack_records(const mcpt_scene_desc& d, std::vector<float4>& tri, std::vector<float4>& sh);

int pairs_to_quads(const std::vector<float4>& pn, int root_ref, std::vector<float4>& qn, int& new_root, int& max_push,
                   std::vector<uint32_t>& src);

}  // namespace mcpt_host
