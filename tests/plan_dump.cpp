// plan_dump.cpp — what rtp::plan (csrc/launch_plan.cpp) makes of the cases of a case file
// (tests/golden/launch_plan.json: a line of device facts, then one line per case). For every case
// it builds the scene, flattens and lowers it, forms the request as rt_render / rt_accum_add do
// and prints one JSON line per attempt: the case's own bound with the ring allowed ("primary": 1),
// then that bound halved down to 1 MiB, each with the ring allowed and ruled out — the attempts
// run_range's out-of-memory loop can reach. A case may give the camera's shutter ("cam_time0",
// "cam_time1") and the build's time range ("build_time0", "build_time1"); without them both are
// [0, 1]. Links the lowering's sources (tests/test_lowering.py LOWERING_SOURCES: scene_model.cpp,
// flatten.cpp, bvh_build.cpp, scene_lower.cpp) and launch_plan.cpp and nothing from HIP; built with
// ASan and UBSan by tests/test_launch_plan.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <tuple>

#include "rt/rt_abi.h"
#include "launch_plan.hpp"
#include "scene_lower.hpp"
#include "scene_model.hpp"

namespace {

// the integer after "key": in a flat JSON line (the case's inputs: everything before "expect")
long long geti(const std::string& line, const char* key)
{
    const std::string inputs = line.substr(0, line.find("\"expect\""));
    const std::string k = std::string("\"") + key + "\":";
    const size_t at = inputs.find(k);
    if (at == std::string::npos) {
        std::fprintf(stderr, "plan_dump: no key %s in: %s\n", key, line.c_str());
        std::exit(2);
    }
    return std::strtoll(inputs.c_str() + at + k.size(), nullptr, 10);
}

// the number after "key": among the case's inputs, or dflt when the case does not give it
double getd(const std::string& line, const char* key, double dflt)
{
    const std::string inputs = line.substr(0, line.find("\"expect\""));
    const std::string k = std::string("\"") + key + "\":";
    const size_t at = inputs.find(k);
    return at == std::string::npos ? dflt : std::strtod(inputs.c_str() + at + k.size(), nullptr);
}

std::string gets(const std::string& line, const char* key)
{
    const std::string k = std::string("\"") + key + "\": \"";
    const size_t at = line.find(k);
    if (at == std::string::npos) return "";
    return line.substr(at + k.size(), line.find('"', at + k.size()) - at - k.size());
}

// a 4 x 2 RGB image for the image textures (the plan sees table sizes only, never texels)
const uint8_t* gradient()
{
    static uint8_t px[4 * 2 * 3];
    for (int i = 0; i < 4 * 2 * 3; ++i) px[i] = (uint8_t)(i * 10);
    return px;
}

struct Scene {
    rtw::World world{1};
    rtp::SceneFacts facts;
};

void print_plan(const std::string& name, const rtp::Plan& pl, const rtp::SceneFacts& f, const rtp::Retry& retry, int chunk,
                bool primary)
{
    std::printf("{\"case\": \"%s\", \"primary\": %d, \"bound\": %zu, \"ring_allowed\": %d, \"err\": %d, \"err_msg\": \"%s\", ",
                name.c_str(), primary ? 1 : 0, retry.buf_cap, retry.ring_allowed ? 1 : 0, pl.err, pl.err_msg);
    // rt_stats' fields of these names, as abi.cpp's write_stats derives them
    std::printf("\"schedule\": %d, \"n_batches\": %d, \"trace_buf_bytes\": %zu, \"ring_bytes\": %zu, \"overlapped\": %d, "
                "\"lds_nodes\": %d, \"slab32\": %d, \"lds_stack\": %d, \"variant_features\": %u, \"precision\": %d, "
                "\"spp_chunk\": %d, \"n_chunks\": %d, \"n_items\": %llu, \"samples\": %llu, ",
                pl.schedule, pl.n_batches, pl.trace_buf_bytes, pl.ring_bytes, pl.overlap ? 1 : 0, pl.n_lds_nodes, pl.slab32,
                pl.lds_stack, pl.variant, pl.f32 ? RT_PREC_F32 : RT_PREC_F64, chunk, pl.n_chunks,
                (unsigned long long)pl.px * (unsigned long long)pl.n_chunks,
                (unsigned long long)pl.px * (unsigned long long)pl.total);
    // what rt_stats does not show
    std::printf("\"total\": %lld, \"batch\": %lld, \"per_sample\": %d, \"ring\": %d, \"ring_waves\": %d, \"ring_one_bytes\": %zu, "
                "\"half_bytes\": %zu, \"partial_bytes\": %zu, \"block_samples\": %d, \"block_chunks\": %d, "
                "\"n_lds_materials\": %d, \"n_lds_textures\": %d, \"n_lds_blas\": %d, \"open_chunk\": %d, \"own_total\": %d, "
                "\"acc_bytes\": %zu, \"px_bytes\": %zu, \"n_tlas_nodes\": %d, \"n_blas_bfs\": %d}\n",
                pl.total, pl.batch, pl.per_sample ? 1 : 0, pl.ring ? 1 : 0, pl.ring_waves, pl.ring_one_bytes, pl.half_bytes,
                pl.partial_bytes, pl.block_samples, pl.block_chunks, pl.n_lds_materials, pl.n_lds_textures, pl.n_lds_blas,
                pl.open_chunk ? 1 : 0, pl.own_total ? 1 : 0, pl.acc_bytes, pl.px_bytes, f.n_tlas_nodes, f.n_blas_bfs);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    if (!std::getline(in, line)) return 2;
    rtp::DeviceFacts dev;
    dev.n_cus = (int)geti(line, "n_cus");
    dev.lds_per_cu = (size_t)geti(line, "lds_per_cu");
    dev.lds_per_block = (size_t)geti(line, "lds_per_block");

    // a scene per (id, build time range): "build_time0" / "build_time1" (optional) are
    // RT_BUILD_TIME0 / _TIME1, "cam_time0" / "cam_time1" (optional) the camera's shutter
    std::map<std::tuple<int, double, double>, std::unique_ptr<Scene>> scenes;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const int sid = (int)geti(line, "scene");
        const auto id = std::make_tuple(sid, getd(line, "build_time0", 0.0), getd(line, "build_time1", 1.0));
        if (!scenes.count(id)) {   // rt_ctx_upload_world: flatten (SAH), lower (hoist on)
            auto sc = std::make_unique<Scene>();
            std::string err;
            rtl::Lowered L;
            sc->world.build.time0 = std::get<1>(id);
            sc->world.build.time1 = std::get<2>(id);
            if (rtw::build_scene(sc->world, sid, gradient(), 4, 2) || rtw::flatten(sc->world, RT_ACCEL_SAH, err) ||
                rtl::lower(sc->world.flat.soa, true, L, err)) {
                std::fprintf(stderr, "plan_dump: scene %d: %s\n", sid, err.c_str());
                return 1;
            }
            sc->facts = rtp::scene_facts(L, sc->world.flat.soa);
            scenes[id] = std::move(sc);
        }
        const rtp::SceneFacts& facts = scenes[id]->facts;

        rt_render_params p{};
        p.width = (int)geti(line, "width");
        p.height = (int)geti(line, "height");
        p.spp = (int)geti(line, "spp");
        p.spp_chunk = (int)geti(line, "spp_chunk");
        p.row_begin = (int)geti(line, "row_begin");
        p.row_stride = (int)geti(line, "row_stride");
        p.tile_shard = (int)geti(line, "tile_shard");
        if (rtp::bad_geometry(&p)) return 1;
        rtw::Preset pre;
        if (!rtw::scene_preset(sid, pre)) return 1;
        rt_camera cam = rtw::camera_new(pre.look_from, pre.look_at, rtw::v3(0.0, 1.0, 0.0), pre.vfov,
                                        (double)p.width / (double)p.height, 0.1, 10.0, getd(line, "cam_time0", 0.0),
                                        getd(line, "cam_time1", 1.0));   // rt_scene_camera, or the case's shutter
        if (geti(line, "cam_far")) cam.origin[0] = 1e9, cam.origin[1] = 0.0, cam.origin[2] = 0.0;

        rtp::Options opt;
        opt.slab32 = (int)geti(line, "opt_slab32");
        opt.lds_stack = (int)geti(line, "opt_lds_stack");
        opt.lds_nodes = (int)geti(line, "opt_lds_nodes");
        opt.schedule = (int)geti(line, "sched");
        opt.precision = (int)geti(line, "prec");
        opt.ring = (int)geti(line, "ring");
        opt.overlap = (int)geti(line, "overlap");
        opt.block_chunks = (int)geti(line, "block_chunks");
        opt.block_samples = (int)geti(line, "block_samples");
        opt.extra_features = (uint32_t)geti(line, "extra_features");

        const bool accum = geti(line, "accum") != 0;   // one rt_accum_add of all the samples
        rtp::Request rq;
        rq.lay = rtp::layout_of(&p);
        rq.s_begin = 0;
        rq.s_end = p.spp;
        rq.chunk = p.spp_chunk > 0 ? (accum ? p.spp_chunk : std::min(p.spp_chunk, p.spp)) : rtp::auto_chunk(p.spp);
        rq.acc_sink = accum;
        rq.cam_mag = rtp::camera_magnitude(cam);
        rq.cam_time0 = cam.time0;
        rq.cam_time1 = cam.time1;

        const std::string name = gets(line, "case");
        const size_t bound = (size_t)geti(line, "buf_bytes");
        if ((long long)rq.lay.rows * rq.lay.w == 0) {   // run_range's empty range: the all-zero plan
            print_plan(name, rtp::Plan{}, facts, rtp::Retry{bound, true}, rq.chunk, true);
            continue;
        }
        bool primary = true;
        for (size_t b = bound;; b = std::max<size_t>(b / 2, (size_t)1 << 20)) {
            for (const bool ring_allowed : {true, false}) {
                const rtp::Retry retry{b, ring_allowed};
                print_plan(name, rtp::plan(facts, dev, opt, rq, retry), facts, retry, rq.chunk, primary);
                primary = false;
            }
            if (b <= ((size_t)1 << 20)) break;
        }
    }
    return 0;
}
