// adaptive_schedule_main.cpp — csrc/adaptive_schedule.cpp on a CPU, nothing from HIP: reads one
// command per line of the file given as argv[1] and prints what the module decides, for
// tests/test_adaptive_state_host.py (built there with ASan and UBSan).
//   create W H spp spp_chunk row_begin row_stride row_block tile_shard max_depth min_spp step_spp
//   oneshot W H spp spp_chunk row_begin row_stride row_block tile_shard max_depth out_format min_spp step_spp threshold
//   advance threshold spp_cap max_launches has_map ragged_cap any_zero
//   ragged ragged_cap end chunk
//   next n cap min_r step_r
//   round v chunk
//   restore  hW hH hchunk hmin hstep hhalves hragged  W H chunk min step halves  n_counts counts...
//   group threshold cap min_r step_r use_mask n  (spp err-or-mask) x n
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "adaptive_schedule.hpp"

static void verdict(const char* msg)
{
    if (msg) std::printf("err %s\n", msg);
    else std::printf("ok\n");
}

static double number(std::istringstream& in)
{
    std::string s;
    in >> s;
    if (s == "nan") return std::nan("");
    if (s == "inf") return INFINITY;
    if (s == "-inf") return -INFINITY;
    return std::stod(s);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "create") {
            rt_render_params p{};
            rt_adaptive_params ap{};
            in >> p.width >> p.height >> p.spp >> p.spp_chunk >> p.row_begin >> p.row_stride >> p.row_block >>
                p.tile_shard >> p.max_depth >> ap.min_spp >> ap.step_spp;
            rtas::Schedule s;
            const int auto_chunk = std::min(16, std::max(1, (p.spp + 15) / 16));
            const char* msg = rtas::check_create(&p, &ap, auto_chunk, s);
            if (msg) std::printf("err %s\n", msg);
            else std::printf("ok %d %d %d\n", s.chunk, s.min_r, s.step_r);
        } else if (cmd == "oneshot") {
            rt_render_params p{};
            rt_adaptive_params ap{};
            in >> p.width >> p.height >> p.spp >> p.spp_chunk >> p.row_begin >> p.row_stride >> p.row_block >>
                p.tile_shard >> p.max_depth >> p.out_format >> ap.min_spp >> ap.step_spp;
            ap.threshold = number(in);
            rtas::Schedule s;
            const int auto_chunk = std::min(16, std::max(1, (p.spp + 15) / 16));
            const char* msg = rtas::check_one_shot(&p, &ap, auto_chunk, s);
            if (msg) std::printf("err %s\n", msg);
            else std::printf("ok %d %d %d\n", s.chunk, s.min_r, s.step_r);
        } else if (cmd == "advance") {
            rt_adaptive_advance_params a{};
            int has_map = 0, ragged = 0, any_zero = 0;
            static const double dummy = 0.0;
            a.threshold = number(in);
            in >> a.spp_cap >> a.max_launches >> has_map >> ragged >> any_zero;
            a.tile_error_in = has_map ? &dummy : nullptr;
            verdict(rtas::check_advance(&a, ragged, any_zero != 0));
        } else if (cmd == "ragged") {
            int ragged, end, chunk;
            in >> ragged >> end >> chunk;
            std::printf("%d\n", rtas::ragged_after(ragged, end, chunk));
        } else if (cmd == "next") {
            long long n;
            int cap, min_r, step_r;
            in >> n >> cap >> min_r >> step_r;
            std::printf("%d\n", rtas::next_count(n, cap, min_r, step_r));
        } else if (cmd == "round") {
            int v, chunk;
            in >> v >> chunk;
            std::printf("%d\n", rtas::round_up(v, chunk));
        } else if (cmd == "restore") {
            rt_adaptive_state_header h{};
            rtas::Schedule s;
            int W, H, halves, n;
            in >> h.width >> h.height >> h.spp_chunk >> h.min_spp >> h.step_spp >> h.with_halves >> h.ragged_cap;
            in >> W >> H >> s.chunk >> s.min_r >> s.step_r >> halves >> n;
            std::vector<uint32_t> counts((size_t)n);
            for (auto& c : counts) in >> c;
            verdict(rtas::check_restore(&h, counts.data(), n, W, H, s, halves != 0));
        } else if (cmd == "group") {
            int cap, min_r, step_r, use_mask, n;
            const double thr = number(in);
            in >> cap >> min_r >> step_r >> use_mask >> n;
            std::vector<uint32_t> spp((size_t)n), group((size_t)n);
            std::vector<double> err((size_t)n);
            std::vector<uint8_t> mask((size_t)n);
            for (int i = 0; i < n; ++i) {
                in >> spp[i];
                const double v = number(in);
                err[i] = v;
                mask[i] = v != 0.0;
            }
            const rt_adaptive_group g = rtas::next_group(spp.data(), use_mask ? nullptr : err.data(),
                                                         use_mask ? mask.data() : nullptr, n, thr, cap, min_r, step_r,
                                                         group.data());
            std::printf("%lld %lld %d %d", (long long)g.n_group, (long long)g.n_active, g.n_star, g.n_next);
            for (long long i = 0; i < g.n_group; ++i) std::printf(" %u", group[(size_t)i]);
            std::printf("\n");
        } else if (!cmd.empty()) {
            std::printf("unknown %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
