// scene_features.hpp — the scene feature bits and the compiled kernel variants they select.
// No HIP: shared by the kernels (trace_kernel.hpp), the host lowering that derives a scene's
// bits (scene_lower.cpp) and CPU tests.
#pragma once

#include <cstdint>

// The first instance a cast's top-level walk reaches is tested after that walk (trace_world's
// DeferInst), its BLAS walk then starting at stack entry 0; shared with the host, which sizes the
// stack from it (scene_lower.cpp: a scene where no other nested walk can happen needs
// max(TLAS, BLAS) entries instead of their sum)
#ifndef RT_DEFER_INST
#define RT_DEFER_INST 1
#endif

namespace rtk {

// Scene features (which code a kernel variant must contain).
enum : uint32_t {
    FEAT_RECT = 1,      // XY/XZ/YZ rects and boxes
    FEAT_INST = 2,      // Translate / RotateY instances
    FEAT_MEDIUM = 4,    // ConstantMedium
    FEAT_NOISE = 8,     // Perlin noise texture
    FEAT_IMAGE = 16,    // image texture
    FEAT_INST_RECT = 32,    // rects or boxes inside an instance (its child prim or BLAS)
    FEAT_MEDIUM_INST = 64,  // a medium boundary that is not a sphere (box, rect, instance)
    FEAT_INST_MEDIUM = 128, // a medium inside an instance (nested Translate/RotateY over a ConstantMedium)
    FEAT_INST_BLAS = 256,   // an instance over a BVH (a nested walk; instances over one primitive need none)
    FEAT_SHUTTER = 512,     // a MovingSphere whose shutter is not [0, 1] (its centre needs a division)
    FEAT_NEST_MOVING = 1024, // a MovingSphere (nonzero velocity) under an instance or in a medium boundary
    FEAT_IMAGE_UV = 2048,    // an image texture on a rect / box or an instanced primitive (its uv is stored at
                             // the hit; else it is a top-level sphere's, recomputed from the hit normal)
    FEAT_ALL = 4095,
    FEAT_STATIC = 1u << 16,  // kernel-internal (InstC / BoundC): every sphere reached here is static
    FEAT_SET_SPHERES = 0,                                          // compiled variant: spheres + solid/checker
    FEAT_SET_RECTINST = FEAT_RECT | FEAT_INST | FEAT_INST_RECT,    // + rects, boxes, instances of one prim (Cornell)
    FEAT_SET_MEDIA = FEAT_SET_RECTINST | FEAT_MEDIUM | FEAT_MEDIUM_INST,  // + constant media (Cornell smoke)
    // + Perlin and image textures, instances over spheres, media bounded by spheres (final scene)
    FEAT_SET_FINAL = FEAT_RECT | FEAT_INST | FEAT_MEDIUM | FEAT_NOISE | FEAT_IMAGE | FEAT_INST_BLAS
};

// the smallest compiled variant that holds a scene's features
inline uint32_t variant_features(uint32_t scene_features)
{
    if ((scene_features & ~FEAT_SET_SPHERES) == 0) return FEAT_SET_SPHERES;
    if ((scene_features & ~FEAT_SET_RECTINST) == 0) return FEAT_SET_RECTINST;
    if ((scene_features & ~FEAT_SET_MEDIA) == 0) return FEAT_SET_MEDIA;
    if ((scene_features & ~FEAT_SET_FINAL) == 0) return FEAT_SET_FINAL;
    return FEAT_ALL;
}

}  // namespace rtk
