// primary_candidates_host.cpp — the host twin of the candidate-table kernel (primary_candidates.hip):
// the same build_pixel over the same tables, pixel by pixel, so the table is checkable on a CPU
// (tests/test_primary_candidates.py through rt_primary_candidates_host, tests/primary_candidates_main.cpp).
#include "primary_candidates.hpp"

namespace rtpc {

TableStats build_host(const rt_bvh_node* nodes, const rt_prim* leaf_prims, int32_t root, const rt_camera& cam, int width,
                      int height, int k_max, Record* out)
{
    TableStats st;
    if (k_max > kSlots) k_max = kSlots;
    for (int y = 0; y < height; ++y) {
        for (int ix = 0; ix < width; ++ix) {
            const Record r = build_pixel(nodes, leaf_prims, root, cone_of(cam, width, height, ix, y), k_max);
            out[(size_t)y * (size_t)width + (size_t)ix] = r;
            st.pixels++;
            if (r.n == kWalk) {
                st.flagged++;
            } else {
                st.candidates += r.n;
                if ((int)r.n > st.max_candidates) st.max_candidates = (int)r.n;
            }
        }
    }
    return st;
}

int64_t sky_tiles_host(const Record* table, int width, int height, uint8_t* flags)
{
    int64_t n = 0;
    const int tx_n = tiles_x_of(width), ty_n = tiles_y_of(height);
    for (int ty = 0; ty < ty_n; ++ty) {
        for (int tx = 0; tx < tx_n; ++tx) {
            const bool sky = tile_all_sky(table, width, height, tx, ty);
            flags[(size_t)ty * (size_t)tx_n + (size_t)tx] = sky ? 1 : 0;
            n += sky;
        }
    }
    return n;
}

}  // namespace rtpc
