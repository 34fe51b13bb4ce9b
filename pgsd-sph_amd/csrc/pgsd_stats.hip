// pgsd_stats.hip -- frame statistics on gfx950: per column of a staged per-particle chunk (or of a row list over it) the
// number of NaN and of infinite entries, the minimum and maximum of the entries that are no NaN, and the sum of the
// finite entries in a FIXED order.  pgsd.hoomd.column_stats is the definition and this file equals it exactly, sums
// included, so the pairing of the additions is part of the definition and does not depend on the launch:
//   stats_tile_kernel<G, T, M, NORM2>   one workgroup per tile of SEL_PER_BLOCK entries, the row layout of the selection
//                          kernels: lane t owns entries base + k * SEL_THREADS + t and adds them for k = 0 .. 15 to a
//                          sum that starts at +0.0; the 256 lane sums go through the BLOCK TREE -- inside each of the
//                          four waves p[i] += p[i + h] for h = 32 .. 1 (shuffles), then (w0 + w1) + (w2 + w3) through one
//                          LDS exchange -- and the tile's partial results are written to table[quantity][column][tile]
//                          with plain stores: no atomic, nothing to clear, nothing that depends on the grid
//   stats_final_kernel     ONE workgroup per column: lane t adds the partials of tiles t, t + 256, ... in that order to
//                          +0.0, the same block tree gives the result; minima, maxima and counters likewise (their
//                          order is free)
// An entry that is not finite contributes +0.0, and so does an entry past the end: the identity here, because a sum that
// starts at +0.0 and only ever adds is never -0.0.  Every element is converted to float64 first (exact for float32,
// int32 and uint32); the appended norm2 column of a three-column float chunk is (x*x + y*y) + z*z in float64 without
// contraction.  Shared device helpers and the row layout: pgsd_kernels.hpp; the launchers' host side: pgsd_scratch.hpp.
// The second half of the file holds the grouped reductions: per particle type sums over several staged chunks read row by
// row, in the same tile layout, the same trees and the same scratch.  The conservation sums (moments_tile_kernel;
// pgsd.hoomd.particle_moments is the definition) and the frame displacements (displacement_tile_kernel;
// pgsd.hoomd.particle_displacements) have a tile kernel each and share one table layout, grouped_final_kernel and one
// launcher.
#include "pgsd_stats.hpp" // (stats_elem, stats_wave_sum, stats_wave_count: shared with pgsd_cells.hip)
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
#define STATS_WAVES (SEL_THREADS / 64)

// what a lane, and then a tile, knows about one column
struct StatsAcc
    {
    double sum, mn, mx;
    uint32_t n_nan, n_inf;
    };

// one entry: classified BEFORE anything is added; `ok`: the entry exists
__device__ __forceinline__ void stats_take(StatsAcc& a, double v, bool ok)
    {
    const bool is_nan = !(v == v);
    const bool is_inf = __builtin_fabs(v) == __builtin_huge_val();
    a.n_nan += (ok && is_nan) ? 1u : 0u;
    a.n_inf += (ok && is_inf) ? 1u : 0u;
    a.mn = (ok && v < a.mn) ? v : a.mn; // (a NaN compares false: it takes no part)
    a.mx = (ok && v > a.mx) ? v : a.mx;
    a.sum = a.sum + ((ok && !is_nan && !is_inf) ? v : 0.0);
    }

// the rest of the block tree: the four waves' sums, (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double stats_block_sum(const double* w)
    {
#pragma clang fp contract(off)
    return (w[0] + w[1]) + (w[2] + w[3]);
    }

// a final kernel's walk over one column of the tiles' sums -- lane t adds the partials of tiles t, t + 256, ... in that
// order to +0.0 -- and the wave part of the block tree (lane 0 of each wave ends with its wave's sum)
__device__ __forceinline__ double stats_column_sum(const double* __restrict__ t_sum, uint32_t n_tiles)
    {
#pragma clang fp contract(off)
    double sum = 0.0;
#pragma unroll 8
    for (uint32_t t = threadIdx.x; t < n_tiles; t += SEL_THREADS)
        sum = sum + t_sum[t];
    return stats_wave_sum(sum);
    }

// minimum, maximum and the counters across the wave (every lane ends with the result; the order is free)
__device__ __forceinline__ void stats_wave_rest(StatsAcc& a)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        const double lo = __shfl_xor(a.mn, h, 64), hi = __shfl_xor(a.mx, h, 64);
        a.mn = lo < a.mn ? lo : a.mn;
        a.mx = hi > a.mx ? hi : a.mx;
        a.n_nan += __shfl_xor(a.n_nan, h, 64);
        a.n_inf += __shfl_xor(a.n_inf, h, 64);
        }
    }

// The partial results of every tile: doubles td[(q * C + c) * n_tiles + tile] for q = sum, min, max, and counters
// tu[(q * C + c) * n_tiles + tile] for q = NaN, infinite.
enum
    {
    STATS_Q_SUM = 0,
    STATS_Q_MIN = 1,
    STATS_Q_MAX = 2,
    STATS_Q_NAN = 0,
    STATS_Q_INF = 1
    };

// G = false: entry k is row k (whole rows, neighbouring lanes neighbouring rows: every fetched line is used whole).
// G = true: entry k is row rows[k]; an entry >= N loads nothing, counts nowhere and raises both flag words.
// A lane whose entry lies past the end reads the last one instead (straight-line loads) and takes nothing from it.
template<bool G, int T, int M, bool NORM2>
__global__ __launch_bounds__(SEL_THREADS) void stats_tile_kernel(const StatsArgs s, uint32_t n_tiles, double* td, uint32_t* tu,
                                                                 uint32_t* flag_dev, uint32_t* flag_host)
    {
#pragma clang fp contract(off)
    constexpr int C = M + (NORM2 ? 1 : 0);
    constexpr int RW = (T == STATS_F64 ? 2 : 1) * M;   // 32-bit words of a row
    constexpr int BATCH = RW <= 4 ? 8 : 4;             // rows a lane has in flight
    static_assert(!NORM2 || (M == 3 && (T == STATS_F32 || T == STATS_F64)), "norm2: three float columns");
    __shared__ double wave_d[3][C][STATS_WAVES];
    __shared__ uint32_t wave_u[2][C][STATS_WAVES];
    const uint32_t tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * SEL_PER_BLOCK;
    const uint64_t n = G ? s.n : s.N;
    StatsAcc acc[C];
#pragma unroll
    for (int c = 0; c < C; c++)
        acc[c] = {0.0, __builtin_huge_val(), -__builtin_huge_val(), 0u, 0u};
#pragma unroll
    for (int k0 = 0; k0 < SEL_PER_THREAD; k0 += BATCH)
        {
        RowRegs r[BATCH];
        bool ok[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            {
            const uint64_t k = base + (uint64_t)(k0 + j) * SEL_THREADS + threadIdx.x;
            ok[j] = k < n;
            uint64_t row = min(k, n - 1);
            if constexpr (G)
                {
                row = s.rows[row];
                if (ok[j] && row >= s.N)
                    {
                    __hip_atomic_store(flag_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(flag_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                ok[j] = ok[j] && row < s.N;
                r[j].lo = u32x4 {0u, 0u, 0u, 0u};
                r[j].hi = u32x4 {0u, 0u, 0u, 0u};
                if (ok[j])
                    row_load<RW>((const uint32_t*)s.base + row * RW, r[j]);
                }
            else
                row_load<RW>((const uint32_t*)s.base + row * RW, r[j]);
            }
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            {
            double v[M];
#pragma unroll
            for (int c = 0; c < M; c++)
                {
                v[c] = stats_elem<T>(r[j], c);
                stats_take(acc[c], v[c], ok[j]);
                }
            if constexpr (NORM2)
                stats_take(acc[M], (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], ok[j]);
            }
        }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < C; c++)
        {
        const double sum = stats_wave_sum(acc[c].sum);
        stats_wave_rest(acc[c]);
        if (lane == 0)
            {
            wave_d[STATS_Q_SUM][c][wave] = sum;
            wave_d[STATS_Q_MIN][c][wave] = acc[c].mn;
            wave_d[STATS_Q_MAX][c][wave] = acc[c].mx;
            wave_u[STATS_Q_NAN][c][wave] = acc[c].n_nan;
            wave_u[STATS_Q_INF][c][wave] = acc[c].n_inf;
            }
        }
    __syncthreads();
    if (threadIdx.x < C)
        {
        const uint32_t c = threadIdx.x;
        const double* w = wave_d[STATS_Q_SUM][c];
        td[((size_t)STATS_Q_SUM * C + c) * n_tiles + tile] = stats_block_sum(w);
        w = wave_d[STATS_Q_MIN][c];
        td[((size_t)STATS_Q_MIN * C + c) * n_tiles + tile] = fmin(fmin(w[0], w[1]), fmin(w[2], w[3]));
        w = wave_d[STATS_Q_MAX][c];
        td[((size_t)STATS_Q_MAX * C + c) * n_tiles + tile] = fmax(fmax(w[0], w[1]), fmax(w[2], w[3]));
        const uint32_t* u = wave_u[STATS_Q_NAN][c];
        tu[((size_t)STATS_Q_NAN * C + c) * n_tiles + tile] = u[0] + u[1] + u[2] + u[3];
        u = wave_u[STATS_Q_INF][c];
        tu[((size_t)STATS_Q_INF * C + c) * n_tiles + tile] = u[0] + u[1] + u[2] + u[3];
        }
    }

// The result words: STATS_MAX_COLUMNS x 3 counters (count, NaN, infinite) as uint64, the same number of doubles (min, max,
// sum), and the word that says "an entry was >= N".
enum
    {
    STATS_MAX_COLUMNS = 5,
    STATS_RESULT_WORDS = 6 * STATS_MAX_COLUMNS + 1
    };

// One workgroup PER COLUMN (the grid is the number of columns, which belongs to the call and not to the device: a single
// workgroup walking all columns was measured at 123 us for the 19 532 tiles of 80 M rows and four columns, 12 us for one
// column -- the walk is bound by the latency of its loads, and the columns' walks are independent).  The tiles' partials
// are independent loads (the unrolled trips keep several in flight per lane); the column's sum is added in tile order
// t, t + 256, ... per lane.  The flag word is handed to the host with the results and cleared for the next call, which
// therefore needs no memset.
__global__ __launch_bounds__(SEL_THREADS) void stats_final_kernel(const double* __restrict__ td, const uint32_t* __restrict__ tu,
                                                                  uint32_t n_tiles, uint32_t C, uint64_t n, uint32_t* flag_dev,
                                                                  uint64_t* __restrict__ out)
    {
#pragma clang fp contract(off)
    __shared__ double wave_d[3][STATS_WAVES];
    __shared__ uint64_t wave_u[2][STATS_WAVES];
    const uint32_t c = blockIdx.x;
    const double* t_sum = td + ((size_t)STATS_Q_SUM * C + c) * n_tiles;
    const double* t_min = td + ((size_t)STATS_Q_MIN * C + c) * n_tiles;
    const double* t_max = td + ((size_t)STATS_Q_MAX * C + c) * n_tiles;
    const uint32_t* t_nan = tu + ((size_t)STATS_Q_NAN * C + c) * n_tiles;
    const uint32_t* t_inf = tu + ((size_t)STATS_Q_INF * C + c) * n_tiles;
    double sum = 0.0, mn = __builtin_huge_val(), mx = -__builtin_huge_val();
    uint64_t n_nan = 0, n_inf = 0;
#pragma unroll 8
    for (uint32_t t = threadIdx.x; t < n_tiles; t += SEL_THREADS)
        {
        const double lo = t_min[t], hi = t_max[t];
        sum = sum + t_sum[t];
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
        n_nan += t_nan[t];
        n_inf += t_inf[t];
        }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    sum = stats_wave_sum(sum);
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        const double lo = __shfl_xor(mn, h, 64), hi = __shfl_xor(mx, h, 64);
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
        }
    n_nan = stats_wave_count(n_nan);
    n_inf = stats_wave_count(n_inf);
    if (lane == 0)
        {
        wave_d[STATS_Q_SUM][wave] = sum;
        wave_d[STATS_Q_MIN][wave] = mn;
        wave_d[STATS_Q_MAX][wave] = mx;
        wave_u[STATS_Q_NAN][wave] = n_nan;
        wave_u[STATS_Q_INF][wave] = n_inf;
        }
    __syncthreads();
    if (threadIdx.x == 0)
        {
        double* values = (double*)(out + 3 * STATS_MAX_COLUMNS);
        const uint64_t* u = wave_u[STATS_Q_NAN];
        out[3 * c + 0] = n;
        out[3 * c + 1] = u[0] + u[1] + u[2] + u[3];
        u = wave_u[STATS_Q_INF];
        out[3 * c + 2] = u[0] + u[1] + u[2] + u[3];
        const double* w = wave_d[STATS_Q_MIN];
        values[3 * c + 0] = fmin(fmin(w[0], w[1]), fmin(w[2], w[3]));
        w = wave_d[STATS_Q_MAX];
        values[3 * c + 1] = fmax(fmax(w[0], w[1]), fmax(w[2], w[3]));
        values[3 * c + 2] = stats_block_sum(wave_d[STATS_Q_SUM]);
        if (c == 0)
            {
            out[6 * STATS_MAX_COLUMNS] = *flag_dev;
            *flag_dev = 0u;
            }
        }
    }

// ------------------------------------------------------------------ grouped reductions
// Conservation sums and frame displacements are two PASSES of one shape.  Per entry a pass loads the rows of up to five
// staged chunks and forms Q float64 values without contraction; per type of the launch's group it sums each value over
// the entries of that type where the value is finite, in the order of the statistics above (an entry of another type, a
// value that is not finite and an entry past the end add +0.0), counts the entries of the type, those with a value that
// is not finite, and the entries of no type of the group; the displacements also keep the largest of their last value
// (NaN takes no part) with the smallest entry that attains it.
//   moments_tile_kernel<G, F64, TG>, displacement_tile_kernel<G, F64, TG>
//                          the tile layout of stats_tile_kernel; TG (1, 2, 4) types per launch, all accumulators in
//                          registers.  Adding +0.0 to a sum that started at +0.0 changes no bit, so a wave skips the adds
//                          of a type none of its lanes holds (types lie in long runs in real files).  For the largest
//                          value a lane keeps (mx, k) per type and replaces it on value > mx only, so that -- its entries
//                          ascend -- it keeps the smallest k; across lanes, waves and tiles the rule is "larger mx, then
//                          smaller k", which is associative and commutative: its order is free.  No entry: (-inf,
//                          0xFFFFFFFF).  One table layout for both: partials to td[(q * TG + t) * n_tiles + tile] (the
//                          largest value at q = Q), counters to tu[(c * TG + t) * n_tiles + tile] (c = entries, bad,
//                          largest entry if there is one) and tu[(2 + largest) * TG * n_tiles + tile] (other).
//                          The two bodies stay apart: one inlined body behind two kernels, and even inlined helpers for
//                          the classification and the adds, cost the float64 instances registers with this compiler
//                          (DESIGN.md has the figures).
//   grouped_final_kernel   one workgroup per column of either table: the walk and the tree of stats_final_kernel for a
//                          sum or a counter, the pair rule for a largest value
// The launcher (launch_grouped below) knows a pass by a small description: its args type, Q, whether it keeps a largest
// value, the chunk slot of the typeid, its name, its own refusals and its kernels.
enum
    {
    GROUPED_NO_ENTRY = 0xFFFFFFFFu,
    GROUPED_COUNTERS = 2 * GROUPED_MAX_TYPES + 1 // entries and bad per type, other
    };
// The result words: (Q + largest) x 4 doubles (value q of type t at q * TG + t), the counters, 4 largest entries if
// there are any, the flag word.
constexpr uint32_t grouped_word_counters(uint32_t Q, bool largest)
    {
    return (Q + (largest ? 1 : 0)) * GROUPED_MAX_TYPES;
    }
constexpr uint32_t grouped_word_entries(uint32_t Q, bool largest)
    {
    return grouped_word_counters(Q, largest) + GROUPED_COUNTERS;
    }
constexpr uint32_t grouped_word_flag(uint32_t Q, bool largest)
    {
    return grouped_word_entries(Q, largest) + (largest ? GROUPED_MAX_TYPES : 0);
    }
enum
    {
    MOMENTS_RESULT_WORDS = grouped_word_flag(MOMENTS_QUANTITIES, false) + 1,
    DISPLACEMENT_RESULT_WORDS = grouped_word_flag(DISPLACEMENT_SUMS, true) + 1
    };

// (mx, k) takes (om, ok) where that is the larger value, or the same value at a smaller entry
__device__ __forceinline__ void grouped_pair(double& mx, uint32_t& k, double om, uint32_t ok)
    {
    const bool better = om > mx || (om == mx && ok < k);
    mx = better ? om : mx;
    k = better ? ok : k;
    }

// the pair rule across the wave (every lane ends with the result)
__device__ __forceinline__ void grouped_wave_pair(double& mx, uint32_t& k)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        const double om = __shfl_xor(mx, h, 64);
        const uint32_t ok = __shfl_xor(k, h, 64);
        grouped_pair(mx, k, om, ok);
        }
    }

// ------------------------------------------------------------------ conservation sums
// pgsd.hoomd.particle_moments is the definition.  Per entry nine float64 values -- m; m * v[a]; (0.5 * m) * ((vx*vx +
// vy*vy) + vz*vz); m * e; m * x[a] -- from the rows of typeid, mass, velocity, energy and position; a chunk that is
// stored nowhere is a null pointer (uniform over the launch) and its default row, passed by value.
template<bool G, bool F64, int TG>
__global__ __launch_bounds__(SEL_THREADS) void moments_tile_kernel(const MomentsArgs s, uint32_t n_tiles, double* td,
                                                                   uint32_t* tu, uint32_t* flag_dev, uint32_t* flag_host)
    {
#pragma clang fp contract(off)
    constexpr int T = F64 ? STATS_F64 : STATS_F32;
    constexpr int W1 = F64 ? 2 : 1, W3 = 3 * W1; // 32-bit words of a scalar and of a three-column row
    constexpr int BATCH = F64 ? 2 : 4;           // entries a lane has in flight (up to 17 and 9 words each)
    constexpr int Q = MOMENTS_QUANTITIES, NU = 2 * TG + 1;
    __shared__ double wave_d[Q * TG][STATS_WAVES];
    __shared__ uint32_t wave_u[NU][STATS_WAVES];
    const uint32_t tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * SEL_PER_BLOCK;
    const uint64_t n = G ? s.n : s.N;
    const uint32_t* c_tid = (const uint32_t*)s.chunk[0];
    const uint32_t* c_mass = (const uint32_t*)s.chunk[1];
    const uint32_t* c_vel = (const uint32_t*)s.chunk[2];
    const uint32_t* c_energy = (const uint32_t*)s.chunk[3];
    const uint32_t* c_pos = (const uint32_t*)s.chunk[4];
    double acc[TG][Q];
    uint32_t cnt[TG], bad[TG], other = 0;
    bool seen[TG]; // (wave-uniform) a lane of this wave held an entry of type t: else everything of the type is zero
#pragma unroll
    for (int t = 0; t < TG; t++)
        {
        cnt[t] = bad[t] = 0;
        seen[t] = false;
#pragma unroll
        for (int q = 0; q < Q; q++)
            acc[t][q] = 0.0;
        }
#pragma unroll
    for (int k0 = 0; k0 < SEL_PER_THREAD; k0 += BATCH)
        {
        RowRegs r_tid[BATCH], r_mass[BATCH], r_vel[BATCH], r_energy[BATCH], r_pos[BATCH];
        bool ok[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            {
            const uint64_t k = base + (uint64_t)(k0 + j) * SEL_THREADS + threadIdx.x;
            ok[j] = k < n;
            uint64_t row = min(k, n - 1);
            const u32x4 zero = {0u, 0u, 0u, 0u};
            r_tid[j].lo = r_mass[j].lo = r_vel[j].lo = r_vel[j].hi = r_energy[j].lo = r_pos[j].lo = r_pos[j].hi = zero;
            if constexpr (G)
                {
                row = s.rows[row];
                if (ok[j] && row >= s.N)
                    {
                    __hip_atomic_store(flag_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(flag_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                ok[j] = ok[j] && row < s.N;
                }
            if (!G || ok[j])
                {
                if (c_tid)
                    row_load<1>(c_tid + row, r_tid[j]);
                if (c_mass)
                    row_load<W1>(c_mass + row * W1, r_mass[j]);
                if (c_vel)
                    row_load<W3>(c_vel + row * W3, r_vel[j]);
                if (c_energy)
                    row_load<W1>(c_energy + row * W1, r_energy[j]);
                if (c_pos)
                    row_load<W3>(c_pos + row * W3, r_pos[j]);
                }
            }
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            {
            const double m = c_mass ? stats_elem<T>(r_mass[j], 0) : s.defaults[0];
            const double e = c_energy ? stats_elem<T>(r_energy[j], 0) : s.defaults[4];
            double v[3], x[3], val[Q];
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                v[a] = c_vel ? stats_elem<T>(r_vel[j], a) : s.defaults[1 + a];
                x[a] = c_pos ? stats_elem<T>(r_pos[j], a) : s.defaults[5 + a];
                }
            val[0] = m;
            val[4] = (0.5 * m) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            val[5] = m * e;
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                val[1 + a] = m * v[a];
                val[6 + a] = m * x[a];
                }
            bool fin[Q], all_fin = true;
#pragma unroll
            for (int q = 0; q < Q; q++)
                {
                fin[q] = __builtin_fabs(val[q]) < __builtin_huge_val(); // (false for a NaN as well)
                all_fin = all_fin && fin[q];
                }
            // the entry's place in the group; a negative int32 id, like any id outside the group, belongs to no type
            const uint32_t id = r_tid[j].lo.x;
            const uint32_t ty = c_tid ? id - s.type0 : 0u;
            const bool in = ok[j] && ty < s.n_types && !(c_tid && id < s.type0) && !(s.typeid_signed && (int32_t)id < 0);
            other += (ok[j] && !in) ? 1u : 0u;
#pragma unroll
            for (int t = 0; t < TG; t++)
                {
                const bool mine = in && ty == (uint32_t)t;
                if (__ballot(mine) != 0ull) // (wave-uniform; skipping adds only +0.0 to sums that are never -0.0)
                    {
                    seen[t] = true;
                    cnt[t] += mine ? 1u : 0u;
                    bad[t] += (mine && !all_fin) ? 1u : 0u;
#pragma unroll
                    for (int q = 0; q < Q; q++)
                        acc[t][q] = acc[t][q] + ((mine && fin[q]) ? val[q] : 0.0);
                    }
                }
            }
        }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // (the tree over 64 sums of +0.0 is +0.0: a wave that held no entry of a type writes that without the shuffles)
#pragma unroll
    for (int t = 0; t < TG; t++)
        {
#pragma unroll
        for (int q = 0; q < Q; q++)
            {
            const double sum = seen[t] ? stats_wave_sum(acc[t][q]) : 0.0;
            if (lane == 0)
                wave_d[q * TG + t][wave] = sum;
            }
        if (seen[t])
            {
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1)
                {
                cnt[t] += __shfl_xor(cnt[t], h, 64);
                bad[t] += __shfl_xor(bad[t], h, 64);
                }
            }
        if (lane == 0)
            {
            wave_u[t][wave] = cnt[t];
            wave_u[TG + t][wave] = bad[t];
            }
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        other += __shfl_xor(other, h, 64);
    if (lane == 0)
        wave_u[2 * TG][wave] = other;
    __syncthreads();
    if (threadIdx.x < Q * TG)
        {
        const double* w = wave_d[threadIdx.x];
        td[(size_t)threadIdx.x * n_tiles + tile] = (w[0] + w[1]) + (w[2] + w[3]);
        }
    else if (threadIdx.x >= 64 && threadIdx.x < 64 + NU)
        {
        const uint32_t* u = wave_u[threadIdx.x - 64];
        tu[(size_t)(threadIdx.x - 64) * n_tiles + tile] = u[0] + u[1] + u[2] + u[3];
        }
    }

// what the launcher needs to know of the pass
struct MomentsPass
    {
    using Args = MomentsArgs;
    static constexpr uint32_t Q = MOMENTS_QUANTITIES, TYPEID = 0;
    static constexpr bool LARGEST = false;
    static constexpr const char* what = "conservation sums";
    // the pass's own refusal, or null; whether every chunk it cannot do without has an address
    static const char* refusal(const Args&) { return nullptr; }
    static bool ready(const Args&) { return true; }
    // (without a stored chunk and with a row list N is 2^32: nothing bounds the entries)
    static constexpr uint64_t N_LIMIT = (1ull << 32) + 1;
    template<bool G, bool F64, int TG> static auto kernel() { return moments_tile_kernel<G, F64, TG>; }
    };

// ------------------------------------------------------------------ frame displacements
// pgsd.hoomd.particle_displacements is the definition.  Per entry the rows of position a, image a, position b, image b
// and typeid; u = x + (image . box vectors) per frame in the definition's association (u = x without an image chunk: no
// product is formed), d = u_b - u_a, with the minimum image folded z, y, x into frame b's box, s = (d0*d0 + d1*d1) +
// d2*d2; the values are d[a] and s, and s is the one whose largest is kept.  With `out`, entry k's d goes to
// out[3 k .. 3 k + 2].

// u = x + image . vectors of one frame, in the definition's association
__device__ __forceinline__ void disp_unwrap(double u[3], const RowRegs& image, const double v[6])
    {
#pragma clang fp contract(off)
    const double i0 = stats_elem<STATS_I32>(image, 0), i1 = stats_elem<STATS_I32>(image, 1), i2 = stats_elem<STATS_I32>(image, 2);
    u[0] = u[0] + ((i0 * v[0] + i1 * v[3]) + i2 * v[4]);
    u[1] = u[1] + (i1 * v[1] + i2 * v[5]);
    u[2] = u[2] + i2 * v[2];
    }

// HOOMD's minImage: z (three dimensions only), then y, then x; rint is round-to-nearest-even
__device__ __forceinline__ void disp_fold(double d[3], const double v[6], bool three)
    {
#pragma clang fp contract(off)
    if (three)
        {
        const double n = __builtin_rint(d[2] / v[2]);
        d[2] = d[2] - n * v[2];
        d[1] = d[1] - n * v[5];
        d[0] = d[0] - n * v[4];
        }
    double n = __builtin_rint(d[1] / v[1]);
    d[1] = d[1] - n * v[1];
    d[0] = d[0] - n * v[3];
    n = __builtin_rint(d[0] / v[0]);
    d[0] = d[0] - n * v[0];
    }

template<bool G, bool F64, int TG>
__global__ __launch_bounds__(SEL_THREADS) void displacement_tile_kernel(const DisplacementArgs s, uint32_t n_tiles, double* td,
                                                                        uint32_t* tu, uint32_t* flag_dev, uint32_t* flag_host)
    {
#pragma clang fp contract(off)
    constexpr int T = F64 ? STATS_F64 : STATS_F32;
    constexpr int W3 = F64 ? 6 : 3;    // 32-bit words of a position row
    constexpr int BATCH = F64 ? 2 : 4; // entries a lane has in flight (up to 19 and 13 words each)
    constexpr int Q = DISPLACEMENT_SUMS, NU = 3 * TG + 1;
    __shared__ double wave_d[(Q + 1) * TG][STATS_WAVES];
    __shared__ uint32_t wave_u[NU][STATS_WAVES];
    const uint32_t tile = blockIdx.x;
    const uint64_t base = (uint64_t)tile * SEL_PER_BLOCK;
    const uint64_t n = G ? s.n : s.N;
    const uint32_t* c_pa = (const uint32_t*)s.chunk[0];
    const uint32_t* c_ia = (const uint32_t*)s.chunk[1];
    const uint32_t* c_pb = (const uint32_t*)s.chunk[2];
    const uint32_t* c_ib = (const uint32_t*)s.chunk[3];
    const uint32_t* c_tid = (const uint32_t*)s.chunk[4];
    double acc[TG][Q], mx[TG];
    uint32_t cnt[TG], bad[TG], at[TG], other = 0;
    bool seen[TG]; // (wave-uniform) a lane of this wave held an entry of type t: else everything of the type is nothing
#pragma unroll
    for (int t = 0; t < TG; t++)
        {
        cnt[t] = bad[t] = 0;
        seen[t] = false;
        mx[t] = -__builtin_huge_val();
        at[t] = GROUPED_NO_ENTRY;
#pragma unroll
        for (int q = 0; q < Q; q++)
            acc[t][q] = 0.0;
        }
#pragma unroll
    for (int k0 = 0; k0 < SEL_PER_THREAD; k0 += BATCH)
        {
        RowRegs r_pa[BATCH], r_ia[BATCH], r_pb[BATCH], r_ib[BATCH], r_tid[BATCH];
        bool ok[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            {
            const uint64_t k = base + (uint64_t)(k0 + j) * SEL_THREADS + threadIdx.x;
            ok[j] = k < n;
            uint64_t row = min(k, n - 1);
            const u32x4 zero = {0u, 0u, 0u, 0u};
            r_pa[j].lo = r_pa[j].hi = r_pb[j].lo = r_pb[j].hi = r_ia[j].lo = r_ib[j].lo = r_tid[j].lo = zero;
            if constexpr (G)
                {
                row = s.rows[row];
                if (ok[j] && row >= s.N)
                    {
                    __hip_atomic_store(flag_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(flag_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                ok[j] = ok[j] && row < s.N;
                }
            if (!G || ok[j])
                {
                row_load<W3>(c_pa + row * W3, r_pa[j]);
                row_load<W3>(c_pb + row * W3, r_pb[j]);
                if (c_ia)
                    row_load<3>(c_ia + row * 3, r_ia[j]);
                if (c_ib)
                    row_load<3>(c_ib + row * 3, r_ib[j]);
                if (c_tid)
                    row_load<1>(c_tid + row, r_tid[j]);
                }
            }
#pragma unroll
        for (int j = 0; j < BATCH; j++)
            {
            const uint64_t k = base + (uint64_t)(k0 + j) * SEL_THREADS + threadIdx.x;
            double ua[3], d[3], val[Q];
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                ua[a] = stats_elem<T>(r_pa[j], a);
                d[a] = stats_elem<T>(r_pb[j], a);
                }
            if (c_ia)
                disp_unwrap(ua, r_ia[j], s.va);
            if (c_ib)
                disp_unwrap(d, r_ib[j], s.vb);
#pragma unroll
            for (int a = 0; a < 3; a++)
                d[a] = d[a] - ua[a];
            if (s.minimum_image)
                disp_fold(d, s.vb, s.dimensions == 3);
            const double sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            if (s.out && ok[j])
                {
                double* o = s.out + 3 * k;
                o[0] = d[0];
                o[1] = d[1];
                o[2] = d[2];
                }
            val[0] = d[0];
            val[1] = d[1];
            val[2] = d[2];
            val[3] = sq;
            bool fin[Q], all_fin = true;
#pragma unroll
            for (int q = 0; q < Q; q++)
                {
                fin[q] = __builtin_fabs(val[q]) < __builtin_huge_val(); // (false for a NaN as well)
                all_fin = all_fin && fin[q];
                }
            // the entry's place in the group; a negative int32 id, like any id outside the group, belongs to no type
            const uint32_t id = r_tid[j].lo.x;
            const uint32_t ty = c_tid ? id - s.type0 : 0u;
            const bool in = ok[j] && ty < s.n_types && !(c_tid && id < s.type0) && !(s.typeid_signed && (int32_t)id < 0);
            other += (ok[j] && !in) ? 1u : 0u;
#pragma unroll
            for (int t = 0; t < TG; t++)
                {
                const bool mine = in && ty == (uint32_t)t;
                if (__ballot(mine) != 0ull) // (wave-uniform; skipping adds only +0.0 to sums that are never -0.0)
                    {
                    seen[t] = true;
                    cnt[t] += mine ? 1u : 0u;
                    bad[t] += (mine && !all_fin) ? 1u : 0u;
#pragma unroll
                    for (int q = 0; q < Q; q++)
                        acc[t][q] = acc[t][q] + ((mine && fin[q]) ? val[q] : 0.0);
                    const bool larger = mine && sq > mx[t]; // (a NaN compares false; the lane's entries ascend)
                    mx[t] = larger ? sq : mx[t];
                    at[t] = larger ? (uint32_t)k : at[t];
                    }
                }
            }
        }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < TG; t++)
        {
#pragma unroll
        for (int q = 0; q < Q; q++)
            {
            const double sum = seen[t] ? stats_wave_sum(acc[t][q]) : 0.0;
            if (lane == 0)
                wave_d[q * TG + t][wave] = sum;
            }
        if (seen[t])
            {
            grouped_wave_pair(mx[t], at[t]);
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1)
                {
                cnt[t] += __shfl_xor(cnt[t], h, 64);
                bad[t] += __shfl_xor(bad[t], h, 64);
                }
            }
        if (lane == 0)
            {
            wave_d[Q * TG + t][wave] = mx[t];
            wave_u[t][wave] = cnt[t];
            wave_u[TG + t][wave] = bad[t];
            wave_u[2 * TG + t][wave] = at[t];
            }
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        other += __shfl_xor(other, h, 64);
    if (lane == 0)
        wave_u[3 * TG][wave] = other;
    __syncthreads();
    if (threadIdx.x < Q * TG)
        {
        const double* w = wave_d[threadIdx.x];
        td[(size_t)threadIdx.x * n_tiles + tile] = (w[0] + w[1]) + (w[2] + w[3]);
        }
    else if (threadIdx.x >= 64 && threadIdx.x < 64 + TG)
        {
        const uint32_t t = threadIdx.x - 64;
        const double* w = wave_d[Q * TG + t];
        const uint32_t* u = wave_u[2 * TG + t];
        double m = w[0];
        uint32_t k = u[0];
#pragma unroll
        for (int i = 1; i < STATS_WAVES; i++)
            grouped_pair(m, k, w[i], u[i]);
        td[(size_t)(Q * TG + t) * n_tiles + tile] = m;
        tu[(size_t)(2 * TG + t) * n_tiles + tile] = k;
        }
    else if (threadIdx.x >= 128 && threadIdx.x < 128 + 2 * TG + 1)
        {
        const uint32_t c = threadIdx.x - 128 < 2 * TG ? threadIdx.x - 128 : 3 * TG; // entries and bad per type, then other
        const uint32_t* u = wave_u[c];
        tu[(size_t)c * n_tiles + tile] = u[0] + u[1] + u[2] + u[3];
        }
    }

struct DisplacementPass
    {
    using Args = DisplacementArgs;
    static constexpr uint32_t Q = DISPLACEMENT_SUMS, TYPEID = 4;
    static constexpr bool LARGEST = true;
    static constexpr const char* what = "frame displacements";
    static const char* refusal(const Args& d)
        {
        if (d.minimum_image && (d.chunk[1] || d.chunk[3]))
            return "the minimum image is taken without image chunks";
        if (d.dimensions != 2 && d.dimensions != 3)
            return "dimensions is 2 or 3";
        return nullptr;
        }
    static bool ready(const Args& d) { return d.chunk[0] && d.chunk[2]; }
    static constexpr uint64_t N_LIMIT = 1ull << 32;
    template<bool G, bool F64, int TG> static auto kernel() { return displacement_tile_kernel<G, F64, TG>; }
    };

// One workgroup per column: the first Q * TG columns are the sums (stats_final_kernel's walk t, t + 256, ... per lane,
// then the block tree), the next TG -- with `largest` -- the largest values with their entries (the pair rule; the order
// is free), the last 2 * TG + 1 the counters that are summed (entries and bad per type, other).  out: see
// grouped_word_*; the flag word is handed over and cleared as there.
__global__ __launch_bounds__(SEL_THREADS) void grouped_final_kernel(const double* __restrict__ td, const uint32_t* __restrict__ tu,
                                                                    uint32_t n_tiles, uint32_t Q, uint32_t TG, uint32_t largest,
                                                                    uint32_t* flag_dev, uint64_t* __restrict__ out)
    {
#pragma clang fp contract(off)
    __shared__ double wave_d[STATS_WAVES];
    __shared__ uint64_t wave_u[STATS_WAVES];
    const uint32_t b = blockIdx.x;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n_sums = Q * TG, n_d = n_sums + largest * TG;
    double* values = (double*)out;
    if (b < n_sums)
        {
        const double sum = stats_column_sum(td + (size_t)b * n_tiles, n_tiles);
        if (lane == 0)
            wave_d[wave] = sum;
        __syncthreads();
        if (threadIdx.x == 0)
            values[b] = stats_block_sum(wave_d);
        }
    else if (b < n_d)
        {
        const double* t_max = td + (size_t)b * n_tiles;
        const uint32_t* t_at = tu + (size_t)(2 * TG + (b - n_sums)) * n_tiles;
        double mx = -__builtin_huge_val();
        uint32_t at = GROUPED_NO_ENTRY;
#pragma unroll 8
        for (uint32_t t = threadIdx.x; t < n_tiles; t += SEL_THREADS)
            grouped_pair(mx, at, t_max[t], t_at[t]);
        grouped_wave_pair(mx, at);
        if (lane == 0)
            {
            wave_d[wave] = mx;
            wave_u[wave] = at;
            }
        __syncthreads();
        if (threadIdx.x == 0)
            {
            for (int i = 1; i < STATS_WAVES; i++)
                grouped_pair(mx, at, wave_d[i], (uint32_t)wave_u[i]);
            values[b] = mx;
            out[grouped_word_entries(Q, largest) + (b - n_sums)] = at;
            }
        }
    else
        {
        const uint32_t j = b - n_d; // entries and bad per type, then other
        const uint32_t* t_cnt = tu + (size_t)(j < 2 * TG ? j : (2 + largest) * TG) * n_tiles;
        uint64_t count = 0;
#pragma unroll 8
        for (uint32_t t = threadIdx.x; t < n_tiles; t += SEL_THREADS)
            count += t_cnt[t];
        count = stats_wave_count(count);
        if (lane == 0)
            wave_u[wave] = count;
        __syncthreads();
        if (threadIdx.x == 0)
            out[grouped_word_counters(Q, largest) + j] = wave_u[0] + wave_u[1] + wave_u[2] + wave_u[3];
        }
    if (b == 0 && threadIdx.x == 0)
        {
        out[grouped_word_flag(Q, largest)] = *flag_dev;
        *flag_dev = 0u;
        }
    }

// ------------------------------------------------------------------ host side
namespace
    {
// Grow-only, per device (g_stats_lock held): the result words, the device flag word and the table of the tiles'
// partials in one allocation; the pinned twin of the result words; the pinned, device-mapped flag word.
// the head of the allocation: the result words of any of the reductions (chunk statistics, conservation sums, frame
// displacements, whose 34 words fit as it is), then the flag word
constexpr size_t STATS_HEAD_WORDS = (STATS_RESULT_WORDS > MOMENTS_RESULT_WORDS ? STATS_RESULT_WORDS : MOMENTS_RESULT_WORDS);
static_assert(DISPLACEMENT_RESULT_WORDS <= STATS_HEAD_WORDS, "the displacements' result words fit the head as it is");
constexpr size_t STATS_HEAD_BYTES = (STATS_HEAD_WORDS + 1) * sizeof(uint64_t);
// (growth policy, head and bytes per tile: restated by tests/test_gpu_scratch_reuse.py)
Scratch g_stats_scratch("chunk statistics", 1.25, 1u << 16, STATS_HEAD_WORDS * sizeof(uint64_t), sizeof(uint64_t));
std::mutex g_stats_lock;

// The launch scope of either reduction and the parts of its scratch space: head (result words, flag word), then the
// tiles' doubles (td_bytes of them), then their counters (tu_bytes).  A fresh allocation's head is cleared -- the flag
// word starts clear; from then on the final kernel clears it behind every call -- and the pinned flag word is lowered.
struct StatsLaunch
    {
    LaunchScope scope;
    uint64_t *result = nullptr, *host = nullptr;
    uint32_t *flag_dev = nullptr, *flag_host = nullptr, *flag_host_dev = nullptr, *tu = nullptr;
    double* td = nullptr;
    StatsLaunch(size_t td_bytes, size_t tu_bytes, hipStream_t stream, std::string* err)
        : scope(g_stats_lock, g_stats_scratch, STATS_HEAD_BYTES + td_bytes + tu_bytes, stream, err, STATS_HEAD_BYTES)
        {
        if (scope.rc() != PGSD_SUCCESS)
            return;
        const Scratch::Block& mem = scope.mem();
        result = (uint64_t*)mem.dev;
        flag_dev = (uint32_t*)(mem.dev + STATS_HEAD_WORDS * sizeof(uint64_t));
        td = (double*)(mem.dev + STATS_HEAD_BYTES);
        tu = (uint32_t*)(mem.dev + STATS_HEAD_BYTES + td_bytes);
        host = (uint64_t*)mem.host;
        flag_host = (uint32_t*)mem.mapped;
        flag_host_dev = (uint32_t*)mem.mapped_dev;
        __atomic_store_n(flag_host, 0u, __ATOMIC_RELEASE);
        }
    // the result words to the pinned twin, the stream's verdict; true where an entry was outside (either flag word)
    int finish(const char* what, size_t result_words, size_t flag_word, bool* outside)
        {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(host, result, result_words * sizeof(uint64_t), hipMemcpyDeviceToHost, scope.stream());
        const int rc = scope.finish(what, e);
        *outside = rc == PGSD_SUCCESS && (__atomic_load_n(flag_host, __ATOMIC_ACQUIRE) != 0 || host[flag_word] != 0);
        return rc;
        }
    };

template<bool G, int T, int M, bool NORM2>
void stats_tile_launch(const StatsArgs& s, uint32_t n_tiles, double* td, uint32_t* tu, uint32_t* flag_dev, uint32_t* flag_host,
                       hipStream_t stream)
    {
    hipLaunchKernelGGL((stats_tile_kernel<G, T, M, NORM2>), dim3(n_tiles), dim3(SEL_THREADS), 0, stream, s, n_tiles, td, tu,
                       flag_dev, flag_host);
    }

template<bool G, int T>
void stats_tile_dispatch(const StatsArgs& s, uint32_t n_tiles, double* td, uint32_t* tu, uint32_t* flag_dev,
                         uint32_t* flag_host, hipStream_t stream)
    {
    switch (s.M)
        {
        case 1: return stats_tile_launch<G, T, 1, false>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        case 2: return stats_tile_launch<G, T, 2, false>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        case 3:
            if constexpr (T == STATS_F32 || T == STATS_F64)
                if (s.norm2)
                    return stats_tile_launch<G, T, 3, true>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
            return stats_tile_launch<G, T, 3, false>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        default: return stats_tile_launch<G, T, 4, false>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        }
    }

template<bool G>
void stats_tile_by_type(const StatsArgs& s, uint32_t n_tiles, double* td, uint32_t* tu, uint32_t* flag_dev,
                        uint32_t* flag_host, hipStream_t stream)
    {
    switch (s.type)
        {
        case PGSD_TYPE_FLOAT: return stats_tile_dispatch<G, STATS_F32>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        case PGSD_TYPE_DOUBLE: return stats_tile_dispatch<G, STATS_F64>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        case PGSD_TYPE_INT32: return stats_tile_dispatch<G, STATS_I32>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        default: return stats_tile_dispatch<G, STATS_U32>(s, n_tiles, td, tu, flag_dev, flag_host, stream);
        }
    }
    } // namespace

int launch_chunk_stats(const StatsArgs& s, uint64_t* out_counts, double* out_values, hipStream_t stream, std::string* err)
    {
    std::string why;
    if (!out_counts || !out_values || !chunk_stats_supported(s.type, s.M, s.norm2, &why))
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, "chunk statistics: " + why);
    const uint32_t C = s.M + (s.norm2 ? 1u : 0u);
    const uint64_t n = s.rows ? s.n : s.N;
    if (n >= (1ull << 32) || s.N >= (1ull << 32))
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, "chunk statistics: 2^32 rows or entries and more are not indexed");
    if (n == 0)
        {
        chunk_stats_of_nothing(C, out_counts, out_values);
        return PGSD_SUCCESS;
        }
    if (s.N == 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT,
                           "chunk statistics: an entry of the row list lies outside the chunk (nothing was computed)");
    if (!s.base)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t n_tiles = (uint32_t)((n + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK);
    const size_t td_bytes = (size_t)3 * C * n_tiles * sizeof(double), tu_bytes = (size_t)2 * C * n_tiles * sizeof(uint32_t);
    StatsLaunch sc(td_bytes, tu_bytes, stream, err);
    if (sc.scope.rc() != PGSD_SUCCESS)
        return sc.scope.rc();
    if (s.rows)
        stats_tile_by_type<true>(s, n_tiles, sc.td, sc.tu, sc.flag_dev, sc.flag_host_dev, stream);
    else
        stats_tile_by_type<false>(s, n_tiles, sc.td, sc.tu, sc.flag_dev, sc.flag_host_dev, stream);
    hipLaunchKernelGGL(stats_final_kernel, dim3(C), dim3(SEL_THREADS), 0, stream, sc.td, sc.tu, n_tiles, C, n, sc.flag_dev,
                       sc.result);
    bool outside = false;
    const int rc = sc.finish("chunk statistics", STATS_RESULT_WORDS, 6 * STATS_MAX_COLUMNS, &outside);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (outside)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT,
                           "chunk statistics: an entry of the row list lies outside the chunk (nothing was computed)");
    const double* values = (const double*)(sc.host + 3 * STATS_MAX_COLUMNS);
    std::copy(sc.host, sc.host + 3 * C, out_counts);
    std::copy(values, values + 3 * C, out_values);
    return PGSD_SUCCESS;
    }

namespace
    {
template<class Pass, bool G, bool F64>
void grouped_tile_by_group(const typename Pass::Args& a, uint32_t TG, uint32_t n_tiles, const StatsLaunch& sc, hipStream_t stream)
    {
    const auto launch = [&](auto kernel)
    {
        hipLaunchKernelGGL(kernel, dim3(n_tiles), dim3(SEL_THREADS), 0, stream, a, n_tiles, sc.td, sc.tu, sc.flag_dev,
                           sc.flag_host_dev);
    };
    switch (TG)
        {
        case 1: return launch(Pass::template kernel<G, F64, 1>());
        case 2: return launch(Pass::template kernel<G, F64, 2>());
        default: return launch(Pass::template kernel<G, F64, 4>());
        }
    }

// Either grouped reduction: out_counts n_types x (entries, bad[, largest entry or UINT64_MAX]), then the entries of no
// type of the group; out_values n_types x (Q sums[, the largest value]).
template<class Pass>
int launch_grouped(const typename Pass::Args& a, uint64_t* out_counts, double* out_values, hipStream_t stream, std::string* err)
    {
    constexpr uint32_t Q = Pass::Q, L = Pass::LARGEST ? 1 : 0;
    const auto fail = [err](const char* why)
    { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(Pass::what) + ": " + why); };
    static const char* outside_msg = "an entry of the row list lies outside the chunks (nothing was computed)";
    if (!out_counts || !out_values || a.n_types < 1 || a.n_types > GROUPED_MAX_TYPES || (!a.chunk[Pass::TYPEID] && a.n_types != 1))
        return fail("1 to 4 types, one without a typeid chunk");
    if (const char* why = Pass::refusal(a))
        return fail(why);
    const uint64_t n = a.rows ? a.n : a.N;
    if (n >= (1ull << 32) || a.N >= Pass::N_LIMIT)
        return fail("2^32 rows or entries and more are not indexed");
    if (n == 0)
        {
        grouped_of_nothing(Q, Pass::LARGEST, a.n_types, out_counts, out_values);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return fail(outside_msg);
    if (!Pass::ready(a))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t TG = a.n_types == 3 ? 4u : a.n_types; // the kernels' group sizes: 1, 2, 4
    const uint32_t n_d = (Q + L) * TG, n_u = (2 + L) * TG + 1;
    const uint32_t n_tiles = (uint32_t)((n + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK);
    const size_t td_bytes = (size_t)n_d * n_tiles * sizeof(double), tu_bytes = (size_t)n_u * n_tiles * sizeof(uint32_t);
    StatsLaunch sc(td_bytes, tu_bytes, stream, err);
    if (sc.scope.rc() != PGSD_SUCCESS)
        return sc.scope.rc();
    if (a.rows)
        a.f64 ? grouped_tile_by_group<Pass, true, true>(a, TG, n_tiles, sc, stream)
              : grouped_tile_by_group<Pass, true, false>(a, TG, n_tiles, sc, stream);
    else
        a.f64 ? grouped_tile_by_group<Pass, false, true>(a, TG, n_tiles, sc, stream)
              : grouped_tile_by_group<Pass, false, false>(a, TG, n_tiles, sc, stream);
    // one workgroup per sum and per largest value, and per counter that is summed (entries, bad, other)
    hipLaunchKernelGGL(grouped_final_kernel, dim3(n_d + 2 * TG + 1), dim3(SEL_THREADS), 0, stream, sc.td, sc.tu, n_tiles, Q, TG,
                       L, sc.flag_dev, sc.result);
    bool outside = false;
    const int rc = sc.finish(Pass::what, grouped_word_flag(Q, Pass::LARGEST) + 1, grouped_word_flag(Q, Pass::LARGEST), &outside);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (outside)
        return fail(outside_msg);
    const double* values = (const double*)sc.host;
    const uint64_t* counters = sc.host + grouped_word_counters(Q, Pass::LARGEST);
    const uint64_t* entries = sc.host + grouped_word_entries(Q, Pass::LARGEST);
    for (uint32_t t = 0; t < a.n_types; t++)
        {
        out_counts[(2 + L) * t + 0] = counters[t];
        out_counts[(2 + L) * t + 1] = counters[TG + t];
        if (Pass::LARGEST)
            out_counts[(2 + L) * t + 2] = entries[t] == GROUPED_NO_ENTRY ? UINT64_MAX : entries[t];
        for (uint32_t q = 0; q < Q + L; q++)
            out_values[(Q + L) * t + q] = values[q * TG + t];
        }
    out_counts[(2 + L) * a.n_types] = counters[2 * TG];
    return PGSD_SUCCESS;
    }
    } // namespace

int launch_frame_moments(const MomentsArgs& m, uint64_t* out_counts, double* out_sums, hipStream_t stream, std::string* err)
    {
    return launch_grouped<MomentsPass>(m, out_counts, out_sums, stream, err);
    }

int launch_frame_displacements(const DisplacementArgs& d, uint64_t* out_counts, double* out_values, hipStream_t stream,
                               std::string* err)
    {
    return launch_grouped<DisplacementPass>(d, out_counts, out_values, stream, err);
    }
    } // namespace pgsd_amd
