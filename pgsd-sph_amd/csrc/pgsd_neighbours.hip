// pgsd_neighbours.hip -- the neighbour census on gfx950: per entry of a row list in cell order (pgsd_order_rows_by_cell_device
// leaves such a list and its cell ids) the entries of the periodically adjacent cells that lie strictly inside a range r,
// the nearest of them, and over the list the count histogram, the closest pair and a pair histogram over given edges.
// pgsd.hoomd.particle_neighbours is the definition and this file equals it exactly: every result is an integer count or a
// minimum with a tie rule, so none depends on the order in which candidates are visited; the arithmetic of one pair
// (pgsd.hoomd.pair_distance2: the difference, HOOMD's single-shift minimum image z, y, x as compares and selects, then
// (dx*dx + dy*dy) + dz*dz) is float64 without contraction and without a division.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          CSR offsets; every kernel here reads the device flag first and does nothing where it is set,
//                          and clamps what it takes from the offsets to n
//   neighbours_compact_kernel   lane per entry: xs[k] = position[rows[k]] in the chunk's own element type, so that the
//                          pair loop reads runs instead of gathering: ids are x-fastest, hence the x cells of one (y, z)
//                          row of the grid are ONE run of xs wherever x does not wrap, two where it does
//   neighbours_pair_kernel<F64, HIST>   lane per entry i: the candidates by traverse_candidates (pgsd_traverse.hpp), in
//                          the order the SPH kernel sums define -- the census needs no order and takes theirs: the
//                          deduplicated offsets, the x-runs, the fold, d2 and the strict compare are written there,
//                          once for the three pair units.  The functor skips j == i by list position; the lane keeps
//                          its count and the smallest (d2, position) pair.  HIST: the edge table and the pair histogram
//                          live in LDS; the bin is the one numpy.searchsorted(edges2, d2, 'right') - 1 names, found by
//                          bisection of the table.  The summary is made here as well: the count histogram, the ordered
//                          pairs and the pair histogram go through LDS counters and 64-bit integer atomics (the integer
//                          scheme of pgsd_census.hip); count_min, count_max and the closest pair leave as one partial
//                          per workgroup
//   neighbours_final_kernel   one workgroup: the partials in a fixed strided scan, then the head words of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp; the launcher's host side: pgsd_scratch.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define NBR_WAVES (SEL_THREADS / 64)
// one workgroup's share of the minima: the closest pair among its entries (d2, then the smaller position i; j is i's
// nearest) and the count range over its entries that have a cell (cmin > cmax: it has none)
struct NeighboursPartial
    {
    double d2;
    uint32_t i, j, cmin, cmax;
    };

// is (d2, i) before (e2, k) in the order of the closest pair and of a lane's nearest: the smaller d2, then the smaller position
__device__ __forceinline__ bool nbr_before(double d2, uint32_t i, double e2, uint32_t k)
    {
    return d2 < e2 || (d2 == e2 && i < k);
    }

__device__ __forceinline__ void nbr_merge(NeighboursPartial& p, double d2, uint32_t i, uint32_t j, uint32_t cmin, uint32_t cmax)
    {
    if (nbr_before(d2, i, p.d2, p.i))
        {
        p.d2 = d2;
        p.i = i;
        p.j = j;
        }
    p.cmin = min(p.cmin, cmin);
    p.cmax = max(p.cmax, cmax);
    }

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void neighbours_compact_kernel(const NeighboursArgs a, const uint32_t* flag_dev,
                                                                         void* __restrict__ xs)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= a.n || *flag_dev != 0)
        return;
    const uint64_t row = a.rows[k];
    if (row >= a.N) // (the check kernel has refused such a list: nothing is loaded for it)
        return;
    compact_position<F64>(a.pos, row, xs, k);
    }

// words: the summary in device memory -- the head (word 2, the ordered pairs, is added to here), the count histogram and
// the pair histogram, zeroed by the launcher
template<bool F64, bool HIST>
__global__ __launch_bounds__(SEL_THREADS) void neighbours_pair_kernel(const NeighboursArgs a, const uint32_t* __restrict__ offs,
                                                                      const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                      const double* __restrict__ edges2,
                                                                      uint32_t* __restrict__ out_count,
                                                                      double* __restrict__ out_nearest2,
                                                                      uint32_t* __restrict__ out_nearest,
                                                                      unsigned long long* __restrict__ words,
                                                                      NeighboursPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_count[NEIGHBOURS_COUNT_BINS];
    __shared__ unsigned long long s_pairs;
    __shared__ double s_edges[HIST ? NEIGHBOURS_MAX_BINS + 1 : 1];
    __shared__ unsigned long long s_hist[HIST ? NEIGHBOURS_MAX_BINS : 1];
    __shared__ NeighboursPartial s_part[NBR_WAVES];
    if (*flag_dev != 0)
        return;
    const uint32_t bins = HIST ? min(a.bins, (uint32_t)NEIGHBOURS_MAX_BINS) : 0u;
    for (uint32_t t = threadIdx.x; t < NEIGHBOURS_COUNT_BINS; t += SEL_THREADS)
        s_count[t] = 0;
    if (threadIdx.x == 0)
        s_pairs = 0;
    if constexpr (HIST)
        {
        for (uint32_t t = threadIdx.x; t < bins; t += SEL_THREADS)
            s_hist[t] = 0;
        for (uint32_t t = threadIdx.x; t <= bins; t += SEL_THREADS)
            s_edges[t] = edges2[t];
        }
    __syncthreads();
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    uint32_t count = 0, best = NEIGHBOURS_NONE;
    double best2 = __builtin_huge_val();
    if (has)
        traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                            [&](uint32_t j, double, double, double, double d2)
                            {
                                // (the self pair as a flag, not as an early return: with the return the call
                                // measured 34.2 ms where this form, like the unit's former own loop, takes 33.9 --
                                // DESIGN.md §8, "One traversal")
                                const bool other = j != k;
                                count += other ? 1u : 0u;
                                if (other && nbr_before(d2, j, best2, best))
                                    {
                                    best2 = d2;
                                    best = j;
                                    }
                                if constexpr (HIST)
                                    {
                                    // the largest b with edges[b] <= d2: searchsorted(edges2, d2, 'right') - 1; a pair
                                    // outside [edges[0], edges[bins]) is in no bin
                                    if (other && bins > 0 && s_edges[0] <= d2 && d2 < s_edges[bins])
                                        {
                                        uint32_t b = 0, e = bins;
                                        while (e - b > 1)
                                            {
                                            const uint32_t mid = (b + e) >> 1;
                                            if (s_edges[mid] <= d2)
                                                b = mid;
                                            else
                                                e = mid;
                                            }
                                        atomicAdd(&s_hist[b], 1ull);
                                        }
                                    }
                            });
    if (live)
        {
        if (out_count)
            out_count[k] = count;
        if (out_nearest2)
            out_nearest2[k] = best2;
        if (out_nearest)
            out_nearest[k] = best;
        }
    if (has)
        atomicAdd(&s_count[min(count, (uint32_t)NEIGHBOURS_COUNT_BINS - 1u)], 1u);
    // the wave's share: the pairs, the count range and the closest pair, every lane ending with the result
    const uint64_t wave_pairs = stats_wave_count((uint64_t)count);
    NeighboursPartial p = {best2, best == NEIGHBOURS_NONE ? NEIGHBOURS_NONE : k, best, has ? count : NEIGHBOURS_NONE,
                           has ? count : 0u};
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        const double o2 = __shfl_xor(p.d2, h, 64);
        const uint32_t oi = __shfl_xor(p.i, h, 64), oj = __shfl_xor(p.j, h, 64);
        const uint32_t omin = __shfl_xor(p.cmin, h, 64), omax = __shfl_xor(p.cmax, h, 64);
        nbr_merge(p, o2, oi, oj, omin, omax);
        }
    if ((threadIdx.x & 63) == 0)
        {
        s_part[threadIdx.x >> 6] = p;
        if (wave_pairs)
            atomicAdd(&s_pairs, (unsigned long long)wave_pairs);
        }
    __syncthreads();
    if (threadIdx.x == 0)
        {
        NeighboursPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < NBR_WAVES; w++)
            nbr_merge(q, s_part[w].d2, s_part[w].i, s_part[w].j, s_part[w].cmin, s_part[w].cmax);
        part[blockIdx.x] = q;
        if (s_pairs)
            atomicAdd(&words[2], s_pairs);
        }
    for (uint32_t t = threadIdx.x; t < NEIGHBOURS_COUNT_BINS; t += SEL_THREADS)
        {
        const uint32_t v = s_count[t];
        if (v)
            atomicAdd(&words[NEIGHBOURS_HEAD_WORDS + t], (unsigned long long)v);
        }
    if constexpr (HIST)
        {
        for (uint32_t t = threadIdx.x; t < bins; t += SEL_THREADS)
            {
            const unsigned long long v = s_hist[t];
            if (v)
                atomicAdd(&words[NEIGHBOURS_HEAD_WORDS + NEIGHBOURS_COUNT_BINS + t], v);
            }
        }
    }

// One workgroup.  closest2: the word behind the summary's last.
__global__ __launch_bounds__(SEL_THREADS) void neighbours_final_kernel(const NeighboursArgs a, const uint32_t* __restrict__ offs,
                                                                       const uint32_t* flag_dev,
                                                                       const NeighboursPartial* __restrict__ part,
                                                                       uint32_t n_parts, unsigned long long* __restrict__ words,
                                                                       double* __restrict__ closest2)
    {
    __shared__ NeighboursPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    NeighboursPartial p = {__builtin_huge_val(), NEIGHBOURS_NONE, NEIGHBOURS_NONE, NEIGHBOURS_NONE, 0u};
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        {
        const NeighboursPartial q = part[t];
        nbr_merge(p, q.d2, q.i, q.j, q.cmin, q.cmax);
        }
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        nbr_merge(p, s_part[t].d2, s_part[t].i, s_part[t].j, s_part[t].cmin, s_part[t].cmax);
    const uint64_t n = a.n;
    const uint64_t somewhere = min((uint64_t)offs[a.n_cells], n);
    const bool any = p.i != NEIGHBOURS_NONE && p.i < n && p.j < n;
    words[0] = n;
    words[1] = n - somewhere;
    words[3] = p.cmin <= p.cmax ? p.cmin : 0u;
    words[4] = p.cmax;
    words[5] = any ? p.i : NEIGHBOURS_NONE;
    words[6] = any ? a.rows[p.i] : NEIGHBOURS_NONE;
    words[7] = any ? a.rows[p.j] : NEIGHBOURS_NONE;
    *closest2 = any ? p.d2 : __builtin_huge_val();
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), the partials (one per workgroup), the edge
// table and the summary with the closest distance behind it; the pinned flag word is the host's view of a refused list,
// the pinned host block the landing place of the summary.
constexpr size_t NBR_SUMMARY_BYTES = ((size_t)NEIGHBOURS_HEAD_WORDS + NEIGHBOURS_COUNT_BINS + NEIGHBOURS_MAX_BINS + 1) * sizeof(uint64_t);
Scratch g_neighbours_scratch("neighbour census", 1.25, 1u << 16, NBR_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_neighbours_lock;

const char* neighbours_refused = "a cell id descends or lies outside [0, n_cells], or an entry of the row list lies outside "
                                 "the position chunk (nothing was computed)";
    } // namespace

void warm_neighbours_kernels()
    {
    warm_kernel((const void*)neighbours_pair_kernel<false, false>);
    }

int launch_neighbours(const NeighboursArgs& a, const double* edges2, uint32_t* out_count, double* out_nearest2,
                      uint32_t* out_nearest, uint64_t* out_summary, double* out_closest2, hipStream_t stream, std::string* err)
    {
    static const char* what = "neighbour census";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_summary || !out_closest2)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.bins > NEIGHBOURS_MAX_BINS)
        return fail("the pair histogram holds at most 1024 bins");
    if (a.bins > 0 && !edges2)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint64_t n = a.n;
    const uint32_t bins = a.bins;
    const size_t summary_words = (size_t)NEIGHBOURS_HEAD_WORDS + NEIGHBOURS_COUNT_BINS + bins;
    if (n == 0)
        {
        neighbours_of_nothing(bins, out_summary, out_closest2);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return fail(neighbours_refused);
    if (!a.rows || !a.cell || !a.pos)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t n_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    const size_t xs_bytes = round16((size_t)n * 3 * (a.f64 ? sizeof(double) : sizeof(float)));
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(NeighboursPartial));
    const size_t edges_bytes = round16(((size_t)bins + 1) * sizeof(double));
    const size_t words_bytes = (summary_words + 1) * sizeof(uint64_t);
    LaunchScope scope(g_neighbours_lock, g_neighbours_scratch, 16 + offs_bytes + xs_bytes + part_bytes + edges_bytes + words_bytes,
                      stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    NeighboursPartial* part = (NeighboursPartial*)(dev + 16 + offs_bytes + xs_bytes);
    double* edges_dev = (double*)((char*)part + part_bytes);
    unsigned long long* words = (unsigned long long*)((char*)edges_dev + edges_bytes);
    double* closest2 = (double*)(words + summary_words);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    hipError_t e = hipSuccess;
    if (bins)
        e = hipMemcpyAsync(edges_dev, edges2, ((size_t)bins + 1) * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess)
        e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs, words,
                            words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(neighbours_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs);
            if (bins)
                hipLaunchKernelGGL((neighbours_pair_kernel<true, true>), per_entry, block, 0, stream, a, offs, flag_dev, xs,
                                   edges_dev, out_count, out_nearest2, out_nearest, words, part);
            else
                hipLaunchKernelGGL((neighbours_pair_kernel<true, false>), per_entry, block, 0, stream, a, offs, flag_dev, xs,
                                   edges_dev, out_count, out_nearest2, out_nearest, words, part);
            }
        else
            {
            hipLaunchKernelGGL(neighbours_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs);
            if (bins)
                hipLaunchKernelGGL((neighbours_pair_kernel<false, true>), per_entry, block, 0, stream, a, offs, flag_dev, xs,
                                   edges_dev, out_count, out_nearest2, out_nearest, words, part);
            else
                hipLaunchKernelGGL((neighbours_pair_kernel<false, false>), per_entry, block, 0, stream, a, offs, flag_dev, xs,
                                   edges_dev, out_count, out_nearest2, out_nearest, words, part);
            }
        hipLaunchKernelGGL(neighbours_final_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, part, n_blocks, words,
                           closest2);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, words, words_bytes, hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return fail(neighbours_refused);
    const uint64_t* landed = (const uint64_t*)scope.mem().host;
    std::copy(landed, landed + summary_words, out_summary);
    memcpy(out_closest2, landed + summary_words, sizeof(double));
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
