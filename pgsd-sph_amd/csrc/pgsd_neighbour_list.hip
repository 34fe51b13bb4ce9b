// pgsd_neighbour_list.hip -- neighbour lists on gfx950: the neighbours the census (pgsd_neighbours.hip) counts, handed over
// as a CSR pair list of a row list in cell order.  pgsd.hoomd.neighbour_list is the definition and this file equals it
// exactly: the segment of entry i holds the list positions j != i (j > i for the half list) of the entries inside the
// range, in the order the SPH kernel sums define, and -- where asked -- pgsd.hoomd.pair_distance2 of each pair bit for bit.
// The output size is not known before a kernel has run, so the list is made in two calls, count -> scan -> fill:
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          cells' CSR offsets; every kernel here reads the device flag first and does nothing where it is set
//   nlist_compact_kernel   lane per entry: xs[k] = position[rows[k]] in the chunk's own element type (compact_position)
//   nlist_count_kernel<F64>   lane per entry i over traverse_candidates (pgsd_traverse.hpp: the cell walk, the x-runs, the
//                          fold, d2 and the strict compare are written there, once for the four pair units): the functor
//                          counts j != i, or j > i, as a flag.  It leaves the entry's count, the workgroup's sum as a
//                          64-bit word (256 counts below 2^32 each do not fit 32 bits) and the workgroup's largest count
//   nlist_scan_kernel      ONE workgroup in a launch of its own, the shape pgsd_select.hip measured as the faster one on
//                          this part (the note above select_scan_kernel: no ticket counter, no look-back, no spin across
//                          workgroups): the exclusive scan of the workgroup sums in rounds of 256 with a 64-bit carry, the
//                          largest count, the four summary words
//   nlist_offsets_kernel   lane per entry: the workgroup's base plus the exclusive scan of its own 256 counts;
//                          offsets[n] by the lane that owns the last entry.  Integer adds only: no order matters
//   nlist_fill_kernel<F64, D2>   the count kernel's traversal once more; the functor stores j (and d2: the D2 instances,
//                          so that the plain list pays nothing for it) at a running index inside the lane's segment.
//                          Two clamps: a segment is stored into only where it ascends and ends inside the capacity, and
//                          never beyond its own end.  An entry that finds another number of neighbours than its segment
//                          holds, a segment that descends or leaves the capacity raise the mismatch word
// No float atomic anywhere, no private (scratch) memory in any instance, plain vector stores only.  The lane-per-entry
// fill writes strided segments: DESIGN.md §8, "Neighbour lists", has its measured cost.  Shared device helpers:
// pgsd_stats.hpp, pgsd_kernels.hpp; the launchers' host side: pgsd_scratch.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scan.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
// (the wave and workgroup scan helpers -- nlist_wave_scan, nlist_wave_max, nlist_block_scan -- are pgsd_scan.hpp's, shared
// with pgsd_components.hip)
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void nlist_compact_kernel(const NeighbourListArgs a, const uint32_t* flag_dev,
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

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void nlist_count_kernel(const NeighbourListArgs a, const uint32_t* __restrict__ offs,
                                                                  const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                  uint32_t* __restrict__ counts,
                                                                  unsigned long long* __restrict__ block_sums,
                                                                  uint32_t* __restrict__ block_longest)
    {
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ unsigned long long s_sum[NLIST_WAVES];
    __shared__ uint32_t s_max[NLIST_WAVES];
    if (*flag_dev != 0)
        return;
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    const bool half = a.half != 0;
    uint32_t count = 0;
    if (has)
        traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                            [&](uint32_t j, double, double, double, double)
                            {
                                // (a flag, not an early return: neighbours_pair_kernel has the measured reason)
                                const bool keep = half ? j > k : j != k;
                                count += keep ? 1u : 0u;
                            });
    if (live)
        counts[k] = count;
    const uint64_t wave_sum = stats_wave_count((uint64_t)count);
    const uint32_t wave_max = nlist_wave_max(count);
    if ((threadIdx.x & 63) == 0)
        {
        s_sum[threadIdx.x >> 6] = wave_sum;
        s_max[threadIdx.x >> 6] = wave_max;
        }
    __syncthreads();
    if (threadIdx.x == 0)
        {
        block_sums[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        block_longest[blockIdx.x] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
        }
    }

// One workgroup.  words: n, the entries nowhere, the pairs, the longest segment.
__global__ __launch_bounds__(SEL_THREADS) void nlist_scan_kernel(const NeighbourListArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev,
                                                                 const unsigned long long* __restrict__ block_sums,
                                                                 const uint32_t* __restrict__ block_longest, uint32_t n_blocks,
                                                                 unsigned long long* __restrict__ block_base,
                                                                 unsigned long long* __restrict__ words)
    {
    __shared__ uint64_t wave_sums[NLIST_WAVES];
    __shared__ uint32_t s_max[NLIST_WAVES];
    if (*flag_dev != 0)
        return;
    uint64_t carry = 0; // (every lane keeps the same carry: the round's total comes back from the scan)
    uint32_t longest = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SEL_THREADS)
        {
        const uint32_t i = b0 + threadIdx.x;
        const uint64_t c = i < n_blocks ? block_sums[i] : 0;
        longest = max(longest, i < n_blocks ? block_longest[i] : 0u);
        uint64_t total;
        const uint64_t before = nlist_block_scan(c, wave_sums, &total);
        if (i < n_blocks)
            block_base[i] = carry + before;
        carry += total;
        __syncthreads(); // (wave_sums is written again in the next round)
        }
    longest = nlist_wave_max(longest);
    if ((threadIdx.x & 63) == 0)
        s_max[threadIdx.x >> 6] = longest;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    const uint64_t n = a.n;
    words[0] = n;
    words[1] = n - min((uint64_t)offs[a.n_cells], n);
    words[2] = carry;
    words[3] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    }

__global__ __launch_bounds__(SEL_THREADS) void nlist_offsets_kernel(uint64_t n, const uint32_t* flag_dev,
                                                                    const uint32_t* __restrict__ counts,
                                                                    const unsigned long long* __restrict__ block_base,
                                                                    unsigned long long* __restrict__ out_offsets)
    {
    __shared__ uint64_t wave_sums[NLIST_WAVES];
    if (*flag_dev != 0)
        return;
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool live = k < n;
    const uint64_t c = live ? counts[k] : 0;
    uint64_t total;
    const uint64_t at = block_base[blockIdx.x] + nlist_block_scan(c, wave_sums, &total);
    if (live)
        out_offsets[k] = at;
    if (k + 1 == n)
        out_offsets[n] = at + c;
    }

// mismatch: one device word, zeroed by the launcher
template<bool F64, bool D2>
__global__ __launch_bounds__(SEL_THREADS) void nlist_fill_kernel(const NeighbourListArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                 const unsigned long long* __restrict__ offsets,
                                                                 uint64_t capacity, uint32_t* __restrict__ out_neighbours,
                                                                 double* __restrict__ out_distance2, uint32_t* mismatch)
    {
    typedef typename std::conditional<F64, double, float>::type elem_t;
    if (*flag_dev != 0)
        return;
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k64 >= n)
        return;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const int32_t c = a.cell[k];
    const bool has = c >= 0 && (uint32_t)c < a.n_cells;
    const bool half = a.half != 0;
    const uint64_t begin = offsets[k64], end = offsets[k64 + 1];
    // the first clamp: a segment is stored into only where it ascends, ends inside the capacity and -- the first one --
    // begins the list; the second: `stop`, its own end (begin itself where the segment is unsound: nothing is stored)
    const bool sound = begin <= end && end <= capacity && (k != 0 || begin == 0);
    const uint64_t stop = sound ? end : begin;
    uint64_t at = begin;
    if (has)
        traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                            [&](uint32_t j, double, double, double, double d2)
                            {
                                const bool keep = half ? j > k : j != k;
                                if (keep && at < stop)
                                    {
                                    out_neighbours[at] = j;
                                    if constexpr (D2)
                                        out_distance2[at] = d2;
                                    }
                                at += keep ? 1u : 0u;
                            });
    if (!sound || at != end)
        __hip_atomic_store(mismatch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the cells'
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), the counts (n words), the workgroup sums, bases
// and largest counts (one each per workgroup) and the summary words -- for the fill the mismatch word in their place;
// the pinned flag word is the host's view of a refused list, the pinned host block the landing place of the summary (of
// the mismatch word and offsets[n]).
Scratch g_nlist_scratch("neighbour list", 1.25, 1u << 16, NLIST_SUMMARY_WORDS * sizeof(uint64_t), sizeof(uint64_t));
std::mutex g_nlist_lock;

const char* nlist_refused = "a cell id descends or lies outside [0, n_cells], or an entry of the row list lies outside "
                            "the position chunk (nothing was computed)";

// what both launchers refuse before they reserve anything; n > 0
int nlist_refuse(const NeighbourListArgs& a, const char* what, std::string* err)
    {
    const int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.N == 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + nlist_refused);
    if (!a.rows || !a.cell || !a.pos)
        return PGSD_ERROR_INVALID_ARGUMENT;
    return PGSD_SUCCESS;
    }
    } // namespace

void warm_neighbour_list_kernels()
    {
    warm_kernel((const void*)nlist_scan_kernel);
    }

int launch_neighbour_offsets(const NeighbourListArgs& a, uint64_t* out_offsets, uint64_t* out_summary, hipStream_t stream,
                             std::string* err)
    {
    static const char* what = "neighbour list";
    if (!out_offsets || !out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint64_t n = a.n;
    if (n == 0)
        {
        // no entry: offsets[0] = 0 is one memset on the stream, no kernel
        drop_stale_error();
        hipError_t e = hipMemsetAsync(out_offsets, 0, sizeof(uint64_t), stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(stream);
        const int rc = hip_check(e, what, err);
        if (rc == PGSD_SUCCESS)
            std::fill(out_summary, out_summary + NLIST_SUMMARY_WORDS, (uint64_t)0);
        return rc;
        }
    int rc = nlist_refuse(a, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    const uint32_t n_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    const size_t xs_bytes = round16((size_t)n * 3 * (a.f64 ? sizeof(double) : sizeof(float)));
    const size_t counts_bytes = round16((size_t)n * sizeof(uint32_t));
    const size_t sums_bytes = round16((size_t)n_blocks * sizeof(uint64_t));
    const size_t longest_bytes = round16((size_t)n_blocks * sizeof(uint32_t));
    const size_t words_bytes = NLIST_SUMMARY_WORDS * sizeof(uint64_t);
    LaunchScope scope(g_nlist_lock, g_nlist_scratch,
                      16 + offs_bytes + xs_bytes + counts_bytes + 2 * sums_bytes + longest_bytes + words_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    uint32_t* counts = (uint32_t*)((char*)xs + xs_bytes);
    unsigned long long* block_sums = (unsigned long long*)((char*)counts + counts_bytes);
    unsigned long long* block_base = (unsigned long long*)((char*)block_sums + sums_bytes);
    uint32_t* block_longest = (uint32_t*)((char*)block_base + sums_bytes);
    unsigned long long* words = (unsigned long long*)((char*)block_longest + longest_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   words, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(nlist_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs);
            hipLaunchKernelGGL(nlist_count_kernel<true>, per_entry, block, 0, stream, a, offs, flag_dev, xs, counts, block_sums,
                               block_longest);
            }
        else
            {
            hipLaunchKernelGGL(nlist_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs);
            hipLaunchKernelGGL(nlist_count_kernel<false>, per_entry, block, 0, stream, a, offs, flag_dev, xs, counts, block_sums,
                               block_longest);
            }
        hipLaunchKernelGGL(nlist_scan_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, block_sums, block_longest, n_blocks,
                           block_base, words);
        hipLaunchKernelGGL(nlist_offsets_kernel, per_entry, block, 0, stream, n, flag_dev, counts, block_base,
                           (unsigned long long*)out_offsets);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, words, words_bytes, hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + nlist_refused);
    const uint64_t* landed = (const uint64_t*)scope.mem().host;
    std::copy(landed, landed + NLIST_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }

int launch_neighbour_list(const NeighbourListArgs& a, const uint64_t* offsets, uint64_t capacity, uint32_t* out_neighbours,
                          double* out_distance2, hipStream_t stream, std::string* err)
    {
    static const char* what = "neighbour list";
    const auto fail = [err](const std::string& why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    const uint64_t n = a.n;
    if (n == 0)
        return PGSD_SUCCESS;
    if (!offsets || (capacity > 0 && !out_neighbours))
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = nlist_refuse(a, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    const uint32_t n_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    const size_t xs_bytes = round16((size_t)n * 3 * (a.f64 ? sizeof(double) : sizeof(float)));
    const size_t words_bytes = sizeof(uint64_t);
    LaunchScope scope(g_nlist_lock, g_nlist_scratch, 16 + offs_bytes + xs_bytes + words_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    uint32_t* mismatch = (uint32_t*)((char*)xs + xs_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    uint64_t* landed = (uint64_t*)scope.mem().host; // the mismatch word, then offsets[n]
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    const unsigned long long* segs = (const unsigned long long*)offsets;
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   mismatch, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(nlist_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs);
            if (out_distance2)
                hipLaunchKernelGGL((nlist_fill_kernel<true, true>), per_entry, block, 0, stream, a, offs, flag_dev, xs, segs,
                                   capacity, out_neighbours, out_distance2, mismatch);
            else
                hipLaunchKernelGGL((nlist_fill_kernel<true, false>), per_entry, block, 0, stream, a, offs, flag_dev, xs, segs,
                                   capacity, out_neighbours, out_distance2, mismatch);
            }
        else
            {
            hipLaunchKernelGGL(nlist_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs);
            if (out_distance2)
                hipLaunchKernelGGL((nlist_fill_kernel<false, true>), per_entry, block, 0, stream, a, offs, flag_dev, xs, segs,
                                   capacity, out_neighbours, out_distance2, mismatch);
            else
                hipLaunchKernelGGL((nlist_fill_kernel<false, false>), per_entry, block, 0, stream, a, offs, flag_dev, xs, segs,
                                   capacity, out_neighbours, out_distance2, mismatch);
            }
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(&landed[0], mismatch, sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&landed[1], offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return fail(nlist_refused);
    const uint64_t held = landed[1];
    if (held > capacity)
        return fail("the capacity of " + std::to_string(capacity) + " entries is too small for the " + std::to_string(held)
                    + " pairs the offsets hold (the outputs are unspecified inside the capacity and untouched outside it)");
    if (landed[0] != 0)
        return fail("the offsets do not belong to this list: an entry finds another number of neighbours than its segment "
                    "holds, or they descend (offsets[n] is " + std::to_string(held) + ", the capacity "
                    + std::to_string(capacity) + " entries; the outputs are unspecified inside the capacity and untouched "
                    "outside it)");
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
