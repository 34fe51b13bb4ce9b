// pgsd_stats.hpp -- device helpers the reductions share (pgsd_stats.hip: chunk statistics and the grouped reductions;
// pgsd_pieces.hpp: the segmented sums of pgsd_cells.hip and pgsd_component_moments.hip): an element of a row in registers
// as a double, and the wave part of the block tree.
// Seen by the HIP compiler alone.
#ifndef PGSD_STATS_HPP
#define PGSD_STATS_HPP

#include "pgsd_kernels.hpp"

namespace pgsd_amd
    {
enum
    {
    STATS_F32 = 0,
    STATS_F64 = 1,
    STATS_I32 = 2,
    STATS_U32 = 3
    };

// word i (a constant once the loops are unrolled) of a row in registers
__device__ __forceinline__ uint32_t stats_word(const RowRegs& r, int i)
    {
    return i < 4 ? r.lo[i] : r.hi[i - 4];
    }

// element c of a row as a double: exact for all four element types
template<int T> __device__ __forceinline__ double stats_elem(const RowRegs& r, int c)
    {
    if constexpr (T == STATS_F64)
        return __longlong_as_double((long long)(((uint64_t)stats_word(r, 2 * c + 1) << 32) | stats_word(r, 2 * c)));
    else if constexpr (T == STATS_F32)
        return (double)__uint_as_float(stats_word(r, c));
    else if constexpr (T == STATS_I32)
        return (double)(int32_t)stats_word(r, c);
    else
        return (double)stats_word(r, c);
    }

// the wave part of the block tree: lane 0 of the wave ends with ((..) + (..)) over the halvings 32, 16, 8, 4, 2, 1
__device__ __forceinline__ double stats_wave_sum(double p)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        p = p + __shfl_down(p, h, 64);
    return p;
    }

// a 64-bit counter across the wave (every lane ends with the result)
__device__ __forceinline__ uint64_t stats_wave_count(uint64_t c)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        c += (uint64_t)__shfl_xor((unsigned long long)c, h, 64);
    return c;
    }
    } // namespace pgsd_amd

#endif
