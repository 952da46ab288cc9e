// bvh_build.hpp — the hierarchies over boxes that flatten.cpp's lowering hands over, written into
// rt_scene.h's node and leaf-slot tables: the SAH build, the list-order chain of the LINEAR and
// MEDIAN modes, the f32 node box, the TLAS-first node order, and the stack a walk needs. Knows
// boxes and tables only: no World, no Hittable and no HIP (tests/bvh_build_main.cpp links it alone).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "rt/rt_scene.h"

namespace rtb {

// One thing to build over, with the f64 box of everything its hit test accepts: a primitive or, in
// a chain, a prebuilt subtree.
struct Item {
    int id;         // the primitive's index; the subtree's root reference
    bool subtree;
    bool costly;    // a Box, a medium or an instance over a BVH: a test that costs more than a node visit
    double lo[3], hi[3];
    double c[3];    // the box's centre
    Item(int id, const double lo[3], const double hi[3], bool costly = false, bool subtree = false);
};

// SAH costs (a primitive test relative to a traversal step) and leaf sizes. Measured on MI355X
// (DESIGN.md §BVH build): c_isect 1.0 / max_leaf 8 keeps the sphere scenes' trees and lets a
// Cornell box's top level (8 wall / box items that every bounce from inside hits anyway)
// collapse: 177 -> 118 ms on C3's geometry. The image does not depend on any of them.
struct SahParams {
    double c_isect = 1.0;   // RT_BUILD_C_ISECT
    int max_leaf = 8;       // RT_BUILD_MAX_LEAF: the largest leaf the cost model may pick
    int force_leaf = 2;     // RT_BUILD_FORCE_LEAF: a set this small is always one leaf
    int root_leaf = 8;      // RT_BUILD_ROOT_LEAF: a whole BVH of at most this many items is one leaf
    // ... unless it holds a costly item (RT_BUILD_SPLIT_BOX_PAIRS = 0: no exception): two Boxes'
    // twelve rect tests in one leaf cost more than a node visit that separates them (C4
    // 1920x1080x100: 108.51 -> 103.52 ms with sets of two split by the SAH,
    // profiles/r04v_ab_c4.log; the random scene's sphere pairs stay leaves, whose split would push
    // its TLAS past the LDS node budget)
    bool split_box_pairs = true;
    // ... and inside an instance's BLAS any set of two (RT_BUILD_SPLIT_BLAS_PAIRS = 0: no): the
    // final scene's 1000-sphere cluster, walked by the lanes that reach it together after the
    // top-level walk (C4 1920x1080x100 with every pair split, the top level's too: 105.84 ->
    // 103.40 ms, profiles/r04w_ab_c4.log; the random scene's top level keeps its pairs, see above)
    bool split_blas_pairs = true;
};
// The parameters for the values of rt_world_set_build_option: a value < 0, or 0 for the sizes and
// the cost, keeps the default; the others are clamped to what a leaf code can hold.
SahParams sah_params(double c_isect, int max_leaf, int force_leaf, int root_leaf, int split_box_pairs,
                     int split_blas_pairs);

// Pads and rounds a box outward to f32 so that neither the f64 slab test nor the conservative f32
// one ever culls a primitive the exact test would hit (the box only gates traversal). pad_abs =
// 2^-18 * M covers the f32 rounding of ray origins with |o| <= 2M and of the slab products
// (DESIGN.md §Traversal precision).
void to_f32_box(const double lo[3], const double hi[3], double pad_abs, float flo[3], float fhi[3]);

// Both builds append to nodes and prim_refs and return the root reference: a node index, or a
// leaf code (the empty one for no items).
// SAH, over primitives only: full sweep over the three axes in centroid order (ties by prim
// index); in_blas: the items are an instance's BLAS (split_blas_pairs). Reorders items.
int build_sah(std::vector<Item>& items, const SahParams& p, double pad_abs, bool in_blas,
              std::vector<rt_bvh_node>& nodes, std::vector<int32_t>& prim_refs);
// LINEAR / MEDIAN: the list in order. Runs of primitives become <=31-prim leaves, a subtree stays
// a child; node k = (segment k, node k+1), both boxes unbounded, so the slab tests return
// t_near = t_min for both and the walk always takes segment k first (list order) with the rest
// of the chain as its one stack entry.
int build_chain(const std::vector<Item>& items, std::vector<rt_bvh_node>& nodes, std::vector<int32_t>& prim_refs);

// Renumbers the nodes: the TLAS's first, in BFS order from root (the kernel copies that prefix
// into LDS), then every other node in the order it has; the instances' BVH roots follow.
struct TlasFirst {
    int n_tlas_nodes, root;
};
TlasFirst renumber_tlas_first(int root, std::vector<rt_bvh_node>& nodes, std::vector<rt_instance>& instances);

// Stack entries a walk from ref needs, the way the kernel's visit uses its stack: it pushes the
// farther child when both are hit, so a node needs 1 + max(n0, n1); with two bit-identical child
// boxes both t_near are equal and child 0 is always taken first, so only it stacks above the
// pushed child 1: max(1 + n0, n1). A leaf needs 0. A node's need depends only on its subtree, so
// walks over one node array share a memo: a subtree walked once costs nothing again (resize as
// nodes are appended; appended nodes must not change afterwards). Iterative, with three colours:
// a cycle in a foreign node graph returns -1 (the memo is then spent) instead of being walked forever.
struct StackMemo {
    std::vector<int> need;
    std::vector<uint8_t> colour;   // 0 new, 1 on the current path, 2 done
    void resize(size_t n_nodes) { need.resize(n_nodes, 0), colour.resize(n_nodes, 0); }
};
int stack_need(const rt_bvh_node* nodes, int ref, StackMemo& memo);

}  // namespace rtb
