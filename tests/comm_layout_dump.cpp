// comm_layout_dump.cpp — what csrc/comm_layout.hpp makes of one gathered frame:
//   comm_layout_dump W H world esz [status of rank 0] [status of rank 1] ...
// prints one JSON line: the slab geometry rt_render_gather uses at that frame, world size and
// element size (per rank: its tile count, and where its slab and status trailer lie in rank 0's
// gathered buffer), the element stride handed to the reorder kernel, and the scan of the given
// status words (missing ones are 0). Links launch_plan.cpp (the tile counts) and nothing from
// HIP; built plain and with ASan and UBSan by tests/test_gather_layout.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "comm_layout.hpp"

int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const int width = std::atoi(argv[1]), height = std::atoi(argv[2]), world = std::atoi(argv[3]);
    const size_t esz = (size_t)std::atoi(argv[4]);
    if (width < 1 || height < 1 || world < 1 || (esz != 4 && esz != 8) || argc - 5 > world) return 2;
    std::vector<int32_t> status((size_t)world, 0);
    for (int r = 0; r + 5 < argc; ++r) status[(size_t)r] = (int32_t)std::strtol(argv[r + 5], nullptr, 10);

    const rtc::SlabLayout l0 = rtc::slab_layout(width, height, 0, world, esz);
    std::printf("{\"world\": %d, \"esz\": %zu, \"n_max\": %d, \"slab_elems\": %lld, \"slab_bytes\": %zu, "
                "\"status_off\": %zu, \"stride_elems\": %lld, \"gathered_bytes\": %zu, \"trailer_bytes\": %zu, ",
                l0.world, l0.esz, l0.n_max, l0.slab_elems, l0.slab_bytes, l0.status_off(), l0.stride_elems(),
                l0.gathered_bytes(), rtc::kTrailerBytes);
    std::printf("\"n_mine\": [");
    for (int r = 0; r < world; ++r) {
        const rtc::SlabLayout l = rtc::slab_layout(width, height, r, world, esz);
        // every rank must agree on what it sends and on where rank 0 finds it
        if (l.n_max != l0.n_max || l.slab_bytes != l0.slab_bytes || l.status_at(r) != l0.status_at(r)) return 1;
        std::printf("%s%d", r ? ", " : "", l.n_mine);
    }
    std::printf("], \"status_at\": [");
    for (int r = 0; r < world; ++r) std::printf("%s%zu", r ? ", " : "", l0.status_at(r));
    std::printf("], \"status_of\": [");
    for (int rc = 0; rc >= -8; --rc) std::printf("%s%d", rc ? ", " : "", (int)rtc::status_of(rc));
    const rtc::StatusScan s = rtc::scan_status(status.data(), world);
    std::printf("], \"failed\": %d, \"first\": %d, \"first_rc\": %d}\n", s.failed, s.first, s.first_rc);
    return 0;
}
