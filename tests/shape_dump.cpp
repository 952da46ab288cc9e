// shape_dump.cpp — the kernel shape a launch resolves to (csrc/launch_shapes.hpp: KernelShape,
// kernel_shape, launch_shape, lds_layout), from the HIP-free headers alone.
//   shape_dump                 every variant feature set x slab32 x lds_stack x f32 x {no TLAS in
//                              LDS, part of it, all of it} x stack16_ok: one JSON line each with the
//                              shape launch_shape resolves, and whether kernel_shape gives the same
//                              shape at the template coordinates it chose ("round_trip")
//   shape_dump V S L F n_lds n_tlas ok n_blas entries n_mat n_tex
//                              that launch's LDS layout over the staged counts: the offsets, the
//                              total and where staged sample starts would begin
// tests/test_launch_shape.py builds it with ASan and UBSan and asserts on the lines.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "launch_shapes.hpp"
#include "scene_features.hpp"

namespace {

void print_shape(const rtk::KernelShape& k)
{
    std::printf("\"features\": %u, \"s32\": %d, \"lds\": %d, \"nall\": %d, \"f32\": %d, \"s16\": %d, \"block_threads\": %d, "
                "\"node_bytes\": %d, \"entry_bytes\": %d, \"stage_shade\": %d, \"stage_blas\": %d, \"min_waves\": %d",
                k.features, k.s32, k.lds, k.nall, k.f32, k.s16, k.block_threads, k.node_bytes, k.entry_bytes, k.stage_shade,
                k.stage_blas, k.min_waves);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 12) {
        int a[11];
        for (int i = 0; i < 11; ++i) a[i] = std::atoi(argv[i + 1]);
        const rtk::KernelShape k = rtk::launch_shape((uint32_t)a[0], a[1] != 0, a[2] != 0, a[3] != 0, a[4], a[5], a[6] != 0);
        const rtk::LdsLayout l = rtk::lds_layout(k, a[4], a[7], a[8], a[9], a[10]);
        std::printf("{");
        print_shape(k);
        std::printf(", \"blas\": %zu, \"stack\": %zu, \"shade\": %zu, \"total\": %zu, \"seeds\": %zu, \"seed_stage_bytes\": %zu}\n",
                    l.blas, l.stack, l.shade, l.total, rtk::lds_seeds_offset(l.total), rtk::seed_stage_bytes_of(k.block_threads));
        return 0;
    }
    if (argc != 1) return 2;
    const uint32_t variants[] = {rtk::FEAT_SET_SPHERES, rtk::FEAT_SET_RECTINST, rtk::FEAT_SET_MEDIA, rtk::FEAT_SET_FINAL,
                                 rtk::FEAT_ALL};
    const int n_tlas = 284;
    for (const uint32_t v : variants)
        for (int bits = 0; bits < 16; ++bits)
            for (const int n_lds : {0, 100, n_tlas}) {
                const bool slab32 = bits & 1, lds = bits & 2, f32 = bits & 4, ok = bits & 8;
                const rtk::KernelShape k = rtk::launch_shape(v, slab32, lds, f32, n_lds, n_tlas, ok);
                std::printf("{\"variant\": %u, \"slab32\": %d, \"lds_stack\": %d, \"prec_f32\": %d, \"n_lds_nodes\": %d, "
                            "\"n_tlas_nodes\": %d, \"stack16_ok\": %d, \"stack16_switch\": %d, \"round_trip\": %d, "
                            "\"block_threads_of\": %d, \"stack16_launch\": %d, ",
                            v, slab32, lds, f32, n_lds, n_tlas, ok, (int)RT_STACK16,
                            k == rtk::kernel_shape(k.features, k.s32, k.lds, k.nall, k.f32) ? 1 : 0,
                            rtk::block_threads_of(v, f32, k.s16), rtk::stack16_launch(slab32, lds, n_lds, n_tlas, ok) ? 1 : 0);
                print_shape(k);
                std::printf("}\n");
            }
    return 0;
}
