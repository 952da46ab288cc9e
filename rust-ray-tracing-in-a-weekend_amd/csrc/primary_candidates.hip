// primary_candidates.hip — the primary-candidate table on the device: one thread per image pixel
// walks the TLAS from global memory with the pixel's cone (primary_candidates.hpp, build_pixel: the
// code the host twin runs) and writes the pixel's 16-byte record. Runs once per (scene upload,
// camera, frame size), inside the first render of that key (abi.cpp).
#include "primary_candidates.hpp"
#include "trace_kernel.hpp"

namespace rtk {

__global__ void __launch_bounds__(256) primary_candidates(const rt_bvh_node* __restrict__ nodes,
                                                          const rt_prim* __restrict__ leaf_prims, int32_t root, rt_camera cam,
                                                          int width, int height, int k_max, uint4* __restrict__ table,
                                                          unsigned* __restrict__ flagged)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = (long long)width * height;
    bool walk = false;
    if (i < n) {
        const int y = (int)(i / width), ix = (int)(i - (long long)y * width);
        const rtpc::Record r = rtpc::build_pixel(nodes, leaf_prims, root, rtpc::cone_of(cam, width, height, ix, y), k_max);
        uint4 q;   // record bytes in order: n, slot[0..6]
        q.x = (unsigned)r.n | (unsigned)r.slot[0] << 16;
        q.y = (unsigned)r.slot[1] | (unsigned)r.slot[2] << 16;
        q.z = (unsigned)r.slot[3] | (unsigned)r.slot[4] << 16;
        q.w = (unsigned)r.slot[5] | (unsigned)r.slot[6] << 16;
        table[i] = q;
        walk = r.n == rtpc::kWalk;
    }
    const unsigned long long m = __ballot(walk);   // one add per wave
    if (m != 0 && (threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(flagged, (unsigned)__popcll(m));
}

hipError_t launch_primary_candidates(const SceneDev& S, const rt_camera& cam, int width, int height, int k_max, void* table,
                                     unsigned* flagged, hipStream_t stream)
{
    const long long n = (long long)width * height;
    if (n <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(flagged, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    if (k_max > rtpc::kSlots) k_max = rtpc::kSlots;
    hipLaunchKernelGGL(primary_candidates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, S.nodes, S.leaf_prims,
                       S.tlas_root, cam, width, height, k_max, (uint4*)table, flagged);
    return hipGetLastError();
}

// The table's all-sky tiles (primary_candidates.hpp, tile_all_sky: the host twin's rule): one thread
// per 8x8 raster tile reads its pixels' counts, writes the tile's flag byte and counts the set ones.
__global__ void __launch_bounds__(256) primary_sky_tiles(const rtpc::Record* __restrict__ table, int width, int height,
                                                         uint8_t* __restrict__ flags, unsigned* __restrict__ n_sky)
{
    const int tx_n = rtpc::tiles_x_of(width);
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x, n = (long long)tx_n * rtpc::tiles_y_of(height);
    bool sky = false;
    if (t < n) {
        sky = rtpc::tile_all_sky(table, width, height, (int)(t % tx_n), (int)(t / tx_n));
        flags[t] = sky ? 1 : 0;
    }
    const unsigned long long m = __ballot(sky);   // one add per wave
    if (m != 0 && (threadIdx.x & 63u) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(n_sky, (unsigned)__popcll(m));
}

hipError_t launch_primary_sky_tiles(const void* table, int width, int height, uint8_t* flags, unsigned* n_sky, hipStream_t stream)
{
    const long long n = (long long)rtpc::tiles_x_of(width) * rtpc::tiles_y_of(height);
    if (width <= 0 || height <= 0) return hipSuccess;
    const hipError_t e = hipMemsetAsync(n_sky, 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(primary_sky_tiles, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       (const rtpc::Record*)table, width, height, flags, n_sky);
    return hipGetLastError();
}

}  // namespace rtk
