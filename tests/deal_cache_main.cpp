// deal_cache_main.cpp — drives csrc/deal_cache.cpp (the whole-frame deal order's cache: no HIP, no
// context) from a script, for tests/test_deal_cache.py. One command per line of argv[1], one JSON
// line out per command:
//   render MODE KIND GEN CAM W H   one render: RT_OPT_AUTO_DEAL_ORDER's value; KIND frame | tile_shard |
//                                  row_shard | count | chunks | adaptive; the upload generation; a
//                                  camera id (the camera's origin x); the frame size. A `build`
//                                  decision is finished with the costs of the last `costs` line
//                                  (all 1 without one).
//   costs C0 C1 ...                per-tile costs for the next build
//   order C0 C1 ...                rtd::cost_order of these costs
//   drop                           a new upload / the context's end
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "deal_cache.hpp"

static void print_order(const std::vector<uint32_t>& o)
{
    std::printf("[");
    for (size_t i = 0; i < o.size(); ++i) std::printf("%s%u", i ? "," : "", o[i]);
    std::printf("]");
}

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: deal_cache_main SCRIPT\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    rtd::DealCache cache;
    std::vector<uint64_t> costs;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string cmd;
        if (!(ss >> cmd) || cmd[0] == '#') continue;
        if (cmd == "costs" || cmd == "order") {
            std::vector<uint64_t> v;
            uint64_t x;
            while (ss >> x) v.push_back(x);
            if (cmd == "costs") {
                costs = v;
                std::printf("{\"costs\":%zu}\n", v.size());
            } else {
                std::vector<uint32_t> o(v.size());
                rtd::cost_order(v.data(), (int64_t)v.size(), o.data());
                std::printf("{\"order\":");
                print_order(o);
                std::printf("}\n");
            }
        } else if (cmd == "drop") {
            cache.drop();
            std::printf("{\"state\":%d}\n", (int)cache.state());
        } else if (cmd == "render") {
            int mode = 0, w = 0, h = 0;
            unsigned long long gen = 0;
            double cam_id = 0;
            std::string kind;
            if (!(ss >> mode >> kind >> gen >> cam_id >> w >> h)) {
                std::fprintf(stderr, "bad render line: %s\n", line.c_str());
                return 2;
            }
            rt_render_params p{};
            p.width = w;
            p.height = h;
            p.spp = 4;
            p.row_stride = 1;
            int schedule = RT_SCHED_POOL;
            bool adaptive = false;
            if (kind == "tile_shard") {
                p.tile_shard = 1;
                p.row_stride = 2;
            } else if (kind == "row_shard") {
                p.row_begin = 1;
                p.row_stride = 2;
            } else if (kind == "count") {
                p.count_work = 1;
            } else if (kind == "chunks") {
                schedule = RT_SCHED_CHUNKS;
            } else if (kind == "items") {
                schedule = RT_SCHED_ITEMS;
            } else if (kind == "adaptive") {
                adaptive = true;
                p.tile_shard = 1;
            } else if (kind != "frame") {
                std::fprintf(stderr, "bad kind: %s\n", kind.c_str());
                return 2;
            }
            rt_camera cam{};
            cam.origin[0] = cam_id;
            const int64_t n_tiles = (int64_t)((w + 7) / 8) * ((h + 7) / 8);
            const bool ok = rtd::eligible(p, schedule, adaptive);
            const rtd::Decision d = cache.next(mode, ok, rtd::key_of(gen, cam, p), n_tiles);
            std::printf("{\"eligible\":%d,\"measure\":%d,\"build\":%d,\"ordered\":%d", (int)ok, (int)d.measure, (int)d.build,
                        (int)d.ordered);
            if (d.build) {
                std::vector<uint64_t> c = costs;
                if ((int64_t)c.size() != n_tiles) c.assign((size_t)n_tiles, 1);
                std::printf(",\"built\":");
                print_order(cache.finish_build(c.data()));
            }
            std::printf(",\"state\":%d,\"n_tiles\":%lld,\"order_len\":%zu}\n", (int)cache.state(), (long long)cache.n_tiles(),
                        cache.order().size());
        } else {
            std::fprintf(stderr, "bad command: %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
