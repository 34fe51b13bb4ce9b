// pgsd_scan.hpp -- the wave and workgroup scan helpers the units share that scan one value per entry of a list
// (pgsd_neighbour_list.hip: the segment lengths; pgsd_components.hip: the root flags): the inclusive scan and the maximum
// across the 64-lane wavefront and the exclusive scan across a workgroup of SEL_THREADS lanes.  Integer adds only: no order
// matters.  The scan of the workgroup sums themselves is each unit's ONE-workgroup kernel, which calls these in rounds.
// Seen by the HIP compiler alone.
#ifndef PGSD_SCAN_HPP
#define PGSD_SCAN_HPP

#include "pgsd_kernels.hpp"

namespace pgsd_amd
    {
#define NLIST_WAVES (SEL_THREADS / 64)
static_assert(SEL_THREADS == 256, "a workgroup scans four wave sums");

// inclusive scan of one 64-bit value per lane across the 64-lane wavefront
__device__ __forceinline__ uint64_t nlist_wave_scan(uint64_t x)
    {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
        {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, d, 64);
        if (lane >= d)
            x += y;
        }
    return x;
    }

// the largest of one value per lane (every lane ends with the result)
__device__ __forceinline__ uint32_t nlist_wave_max(uint32_t v)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        v = max(v, (uint32_t)__shfl_xor(v, h, 64));
    return v;
    }

// the exclusive scan of one value per lane across the workgroup (wave_sums: NLIST_WAVES words of LDS); *total: the sum
__device__ __forceinline__ uint64_t nlist_block_scan(uint64_t c, uint64_t* wave_sums, uint64_t* total)
    {
    const uint64_t inc = nlist_wave_scan(c);
    if ((threadIdx.x & 63) == 63)
        wave_sums[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint64_t wave_off = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < NLIST_WAVES; w++)
        {
        if (w < (threadIdx.x >> 6))
            wave_off += wave_sums[w];
        sum += wave_sums[w];
        }
    *total = sum;
    return wave_off + inc - c;
    }
    } // namespace pgsd_amd

#endif
