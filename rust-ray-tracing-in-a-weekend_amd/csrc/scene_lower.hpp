// scene_lower.hpp — host-only analysis of an rt_scene_soa: validation, and the lowering to
// what the kernels assume (device tables, stack sizes, feature bits). No HIP and no context:
// abi.cpp uploads the result; tests/lower_dump.cpp runs it on a CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "rt/rt_scene.h"

namespace rtl {

struct Lowered {
    std::vector<rt_prim> prims, leaf_prims;   // normalised records; the same in leaf-slot order
    std::vector<rt_bvh_node> nodes;           // device node order and leaf codes
    std::vector<rt_instance> instances;       // pad = the BLAS's base leaf slot
    uint32_t features = 0;                    // rtk::FEAT_* of the scene
    int tlas_depth = 0, blas_depth = 0, n_tlas_nodes = 0, n_blas_bfs = 0;
    int blas_base = 0, stack_entries = 0, stack16_ok = 0;   // SceneDev's fields of these names
    int pre_leaf = 0, pre_root = 0;
    float pre_lo[3] = {}, pre_hi[3] = {};
    int has_lights = 0, has_spheres = 0;
    double pad_extent = 0.0;
    int has_moving = 0;                       // any RT_PRIM_MOVING_SPHERE: its boxes hold for ray times in
    double time_lo = 0.0, time_hi = 0.0;      //   [time_lo, time_hi] only (rt_scene_soa's fields)
};

// Both return RT_OK, or an RT_ERR_* code with its message in err.
int validate(const rt_scene_soa& s, int& tlas_depth, int& blas_depth, int& n_tlas_nodes, std::string& err);
// validates first; hoist: test a huge root-child leaf before the walk (RT_OPT_HOIST)
int lower(const rt_scene_soa& s, bool hoist, Lowered& out, std::string& err);

}  // namespace rtl
