// trace_grid.hpp — a launch's pixel grid (between the device layers and the schedules of
// trace_device.hpp): the image row or tile a shard's grid position names, the (tile, chunk) a wave
// of the chunk layout owns (lane_work: trace_chunks and rt_render_features' trace_features), and
// the occupancy a kernel asks of the register allocator.
#pragma once
#include "trace_kernel.hpp"

namespace rtk {

// image row of the shard's local row k: y = row_begin + k*row_stride, or in bands of 2^s rows
// y = (row_begin + (k >> s)*row_stride) << s | (k & (2^s - 1))
__device__ __forceinline__ int image_row(const KParams& P, int k)
{
    const int s = P.row_block_shift;
    return ((P.row_begin + (k >> s) * P.row_stride) << s) + (k & ((1 << s) - 1));
}
// image pixel (X, Y) of the shard's grid pixel (x, k): a row shard's x and image_row(k); a tile
// shard's grid is its tiles side by side (tile m = the frame's tile at position row_begin +
// m*row_stride of the context's tile order, or of raster order)
__device__ __forceinline__ void image_xy(const KParams& P, int x, int k, int& X, int& Y)
{
    if (P.tile_shard) {   // wave-uniform
        unsigned t = (unsigned)P.row_begin + (unsigned)(x >> 3) * (unsigned)P.row_stride;
        if (__builtin_expect(P.tile_order != nullptr, 0)) t = P.tile_order[t];
        // (the division by a runtime value was ~25 VALU instructions in every bounce-loop iteration
        // that starts a sample: 0.7 % of C2's kernel as a world-1 tile shard, profiles/r06d_*)
        const unsigned ty = P.tile_div_magic ? __umulhi(t, P.tile_div_magic) : t / (unsigned)P.img_tiles_x;
        X = (int)(t - ty * (unsigned)P.img_tiles_x) * 8 + (x & 7);
        Y = (int)ty * 8 + k;
    } else {
        X = x;
        Y = image_row(P, k);
    }
}

// lane -> (chunk, pixel): a wave64 owns an 8x8 tile of one chunk
struct LaneWork {
    int x, y, k, chunk, s_begin, s_end;   // x, k: the shard's grid; y: image row
    int ix;                               // image column
    uint32_t pixel;
};
__device__ __forceinline__ bool lane_work(const KParams& P, LaneWork& w)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_tiles = (long long)P.tiles_x * P.tiles_y;
    if (wave >= n_tiles * P.n_chunks) return false;
    w.chunk = (int)(wave / n_tiles);
    const int tile = (int)(wave % n_tiles);
    w.x = (tile % P.tiles_x) * 8 + (lane & 7);
    w.k = (tile / P.tiles_x) * 8 + (lane >> 3);
    if (w.x >= P.width || w.k >= P.n_rows) return false;
    int ix;
    image_xy(P, w.x, w.k, ix, w.y);
    w.pixel = (uint32_t)w.y * (uint32_t)P.img_width + (uint32_t)ix;
    w.ix = ix;
    w.s_begin = P.sample_begin + w.chunk * P.spp_chunk;
    w.s_end = min(P.spp, w.s_begin + P.spp_chunk);
    return true;
}

// minimum waves per SIMD requested from the register allocator (launch_shapes.hpp, RT_MIN_WAVES_*)
template <class C>
constexpr int min_waves() { return C::SHAPE.min_waves; }

}  // namespace rtk
