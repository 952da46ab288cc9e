// seed_stage_dump.cpp — what rtp::plan (csrc/launch_plan.cpp) decides about the wave-wide sample
// starts (Plan.seed_stage_bytes; csrc/launch_shapes.hpp RT_STAGE_SEEDS) for the cases of a case
// file in tests/golden/launch_plan.json's format: a line of device facts, then one line per case.
// Two optional keys beyond plan_dump's: "stack_entries" replaces the lowered scene's traversal
// stack depth (a deeper scene than any preset), "f32" the precision. Prints one JSON line per case
// with the decision and the facts it follows from. Links the lowering's sources
// (tests/test_lowering.py LOWERING_SOURCES: scene_model.cpp, flatten.cpp, bvh_build.cpp,
// scene_lower.cpp) and launch_plan.cpp and nothing from HIP; tests/test_seed_stage_plan.py builds
// it plain and with ASan and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <string>

#include "rt/rt_abi.h"
#include "launch_plan.hpp"
#include "launch_shapes.hpp"
#include "scene_features.hpp"
#include "scene_lower.hpp"
#include "scene_model.hpp"

namespace {

// the integer after "key": in a flat JSON line (the inputs: everything before "expect"); dflt if absent
long long geti(const std::string& line, const char* key, long long dflt)
{
    const std::string inputs = line.substr(0, line.find("\"expect\""));
    const std::string k = std::string("\"") + key + "\":";
    const size_t at = inputs.find(k);
    if (at == std::string::npos) return dflt;
    return std::strtoll(inputs.c_str() + at + k.size(), nullptr, 10);
}

std::string gets(const std::string& line, const char* key)
{
    const std::string k = std::string("\"") + key + "\": \"";
    const size_t at = line.find(k);
    if (at == std::string::npos) return "";
    return line.substr(at + k.size(), line.find('"', at + k.size()) - at - k.size());
}

const uint8_t* gradient()   // a 4 x 2 RGB image for the image textures (the plan never sees texels)
{
    static uint8_t px[4 * 2 * 3];
    for (int i = 0; i < 4 * 2 * 3; ++i) px[i] = (uint8_t)(i * 10);
    return px;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    if (!std::getline(in, line)) return 2;
    rtp::DeviceFacts dev;
    dev.n_cus = (int)geti(line, "n_cus", dev.n_cus);
    dev.lds_per_cu = (size_t)geti(line, "lds_per_cu", (long long)dev.lds_per_cu);
    dev.lds_per_block = (size_t)geti(line, "lds_per_block", (long long)dev.lds_per_block);

    std::map<int, rtp::SceneFacts> scenes;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const int id = (int)geti(line, "scene", 0);
        if (!scenes.count(id)) {   // rt_ctx_upload_world: flatten (SAH), lower (hoist on)
            rtw::World world{1};
            std::string err;
            rtl::Lowered L;
            if (rtw::build_scene(world, id, gradient(), 4, 2) || rtw::flatten(world, RT_ACCEL_SAH, err) ||
                rtl::lower(world.flat.soa, true, L, err)) {
                std::fprintf(stderr, "seed_stage_dump: scene %d: %s\n", id, err.c_str());
                return 1;
            }
            scenes[id] = rtp::scene_facts(L, world.flat.soa);
        }
        rtp::SceneFacts facts = scenes[id];
        facts.stack_entries = (int)geti(line, "stack_entries", facts.stack_entries);

        rt_render_params p{};
        p.width = (int)geti(line, "width", 64);
        p.height = (int)geti(line, "height", 48);
        p.spp = (int)geti(line, "spp", 16);
        p.spp_chunk = (int)geti(line, "spp_chunk", 0);
        p.row_begin = (int)geti(line, "row_begin", 0);
        p.row_stride = (int)geti(line, "row_stride", 1);
        p.tile_shard = (int)geti(line, "tile_shard", 0);
        if (rtp::bad_geometry(&p)) return 1;
        rtw::Preset pre;
        if (!rtw::scene_preset(id, pre)) return 1;
        rt_camera cam = rtw::camera_new(pre.look_from, pre.look_at, rtw::v3(0.0, 1.0, 0.0), pre.vfov,
                                        (double)p.width / (double)p.height, 0.1, 10.0, 0.0, 1.0);
        if (geti(line, "cam_far", 0)) cam.origin[0] = 1e9, cam.origin[1] = 0.0, cam.origin[2] = 0.0;

        rtp::Options opt;
        opt.slab32 = (int)geti(line, "opt_slab32", 1);
        opt.lds_stack = (int)geti(line, "opt_lds_stack", 1);
        opt.lds_nodes = (int)geti(line, "opt_lds_nodes", 1);
        opt.schedule = (int)geti(line, "sched", RT_SCHED_AUTO);
        opt.precision = (int)geti(line, "prec", RT_PREC_F64);
        opt.ring = (int)geti(line, "ring", 1);
        opt.overlap = (int)geti(line, "overlap", 1);
        opt.block_chunks = (int)geti(line, "block_chunks", 0);
        opt.block_samples = (int)geti(line, "block_samples", 0);
        opt.extra_features = (uint32_t)geti(line, "extra_features", 0);

        rtp::Request rq;
        rq.lay = rtp::layout_of(&p);
        rq.s_begin = 0;
        rq.s_end = p.spp;
        rq.acc_sink = geti(line, "accum", 0) != 0;   // one rt_accum_add of all the samples
        rq.chunk = p.spp_chunk > 0 ? (rq.acc_sink || p.spp_chunk < p.spp ? p.spp_chunk : p.spp) : rtp::auto_chunk(p.spp);
        rq.count_work = geti(line, "count_work", 0) != 0;
        rq.cam_mag = rtp::camera_magnitude(cam);
        if ((long long)rq.lay.rows * rq.lay.w == 0) continue;   // an empty shard launches nothing

        const rtp::Plan pl = rtp::plan(facts, dev, opt, rq, rtp::Retry{(size_t)geti(line, "buf_bytes", 1 << 30), true});
        const bool s16 = pl.variant == rtk::FEAT_SET_SPHERES &&
                         rtk::stack16_launch(pl.slab32 != 0, pl.lds_stack != 0, pl.n_lds_nodes, facts.n_tlas_nodes, facts.stack16_ok != 0);
        std::printf("{\"case\": \"%s\", \"err\": %d, \"seed_stage_bytes\": %zu, \"variant_features\": %u, \"precision\": %d, "
                    "\"schedule\": %d, \"ring\": %d, \"slab32\": %d, \"lds_stack\": %d, \"lds_nodes\": %d, \"n_tlas_nodes\": %d, "
                    "\"stack_entries\": %d, \"stack16_ok\": %d, \"stack16_launch\": %d, \"block_threads\": %d, "
                    "\"switch\": %d, \"slot_bytes\": %zu}\n",
                    gets(line, "case").c_str(), pl.err, pl.seed_stage_bytes, pl.variant, pl.f32 ? RT_PREC_F32 : RT_PREC_F64,
                    pl.schedule, pl.ring ? 1 : 0, pl.slab32, pl.lds_stack, pl.n_lds_nodes, facts.n_tlas_nodes, facts.stack_entries,
                    facts.stack16_ok, s16 ? 1 : 0, rtk::block_threads_of(pl.variant, pl.f32 != 0, s16), (int)RT_STAGE_SEEDS,
                    rtk::kSeedSlotBytes);
    }
    return 0;
}
