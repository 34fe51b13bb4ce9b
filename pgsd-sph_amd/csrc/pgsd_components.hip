// pgsd_components.hip -- fragments on gfx950: the connected components of a row list in cell order within a linking length,
// the friends-of-friends grouping of a frame.  pgsd.hoomd.neighbour_components is the definition and this file equals it
// exactly: the edges are the pairs of the half neighbour list (pgsd_neighbour_list.hip: i -- j, i < j by list position,
// iff i -> j lies strictly inside the range), label[k] is the smallest list position of k's component, component[k] the
// dense id in ascending order of that smallest member, sizes[c] the entries of component c.  Nothing here is a float, so
// nothing depends on an order of evaluation.  The parent array of the union-find is out_label itself:
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          cells' CSR offsets; every kernel here reads the device flag first and does nothing where it is set
//   comp_open_kernel<F64>  lane per entry: xs[k] = position[rows[k]] (compact_position), parent[k] = k, size_at[k] = 0
//   comp_link_kernel<F64>  lane per entry k over traverse_candidates (pgsd_traverse.hpp: the cell walk, the fold, d2 and the
//                          strict compare are written there, once): every candidate j > k is united with k in a lock-free
//                          union-find in the manner of ECL-CC (Jaiganesh and Burtscher, HPDC 2018).  The two progress
//                          arguments stand above comp_find and comp_unite
//   comp_flatten_kernel    a launch of its own, so that it is ordered behind every hook: label[k] = the root of k, which is
//                          the smallest member (a hook puts the larger root under the smaller); size_at[root] grows by
//                          integer atomicAdds, one per distinct root of a wave (integer adds commute)
//   comp_roots_kernel      lane per entry: the root flag label[k] == k, the workgroup's number of roots; per wave one
//                          integer atomicAdd of its singletons and one 64-bit atomicMax of (size << 32) | ~label, whose
//                          maximum is the largest component and among equal sizes the smallest label
//   comp_scan_kernel       ONE workgroup in a launch of its own (nlist_scan_kernel's shape: no ticket counter, no look-back,
//                          no spin across workgroups): the exclusive scan of the workgroups' root counts in rounds of 256,
//                          the six summary words
//   comp_number_kernel     lane per entry: a root's dense id is its workgroup's base plus the exclusive scan of the flags;
//                          sizes[id] = size_at[root], then size_at[root] = id (only the root's own lane touches that word)
//   comp_component_kernel  lane per entry: component[k] = size_at[label[k]], the id its root left there
// No float anywhere in the result, no float atomic, no private (scratch) memory in any instance, no spin on another
// workgroup's progress: a lane that fails a compare-exchange makes progress on its own, so the grid needs no co-residency.
// The scan helpers are pgsd_scan.hpp's; shared device helpers: pgsd_stats.hpp, pgsd_kernels.hpp; the launcher's host side:
// pgsd_scratch.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scan.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
// the device words behind the scratch parts: the six of the summary, the largest-component key, the give-up word
#define COMP_WORDS 8
#define COMP_KEY 6
#define COMP_GAVE_UP 7

// Every access to the parent array while hooks may be in flight is one of these: relaxed, agent scope, vector memory.
__device__ __forceinline__ uint32_t comp_load(const uint32_t* parent, uint32_t x)
    {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

__device__ __forceinline__ void comp_store(uint32_t* parent, uint32_t x, uint32_t v)
    {
    __hip_atomic_store(parent + x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

// The root of x's tree, with path halving.  THE INVARIANT parent[y] <= y holds for every y at every moment: the open
// kernel stores y, a hook stores a smaller root into a root, and the halving store below puts g = parent[p] <= p < x into
// parent[x].  PROGRESS: the loop goes from x to p = parent[x] only where p < x, so the index strictly decreases and the
// loop ends after at most x steps whatever other lanes do.  The halving store only ever targets an entry that was seen
// with a smaller parent -- never a root, and an entry that is no root never becomes one again --, so it cannot undo a
// hook; what it stores is an ancestor of x, and ancestors stay ancestors, so the trees' membership is untouched.
__device__ __forceinline__ uint32_t comp_find(uint32_t* parent, uint32_t x)
    {
    uint32_t p = comp_load(parent, x);
    while (p < x)
        {
        const uint32_t g = comp_load(parent, p);
        if (g < p)
            comp_store(parent, x, g);
        x = p;
        p = g;
        }
    return x;
    }

// Unite the trees of *mine (an ancestor of the lane's own entry, or the entry) and j: find both roots; where they differ,
// hook the larger root under the smaller with a compare-exchange that expects the root to be its own parent still.
// PROGRESS: only a hook changes a root, and the halving store never targets one, so the compare-exchange fails only
// because another lane's hook of that same root succeeded in between.  A root is hooked once in the whole launch (it is
// no root afterwards), the next attempt finds other roots, so every failure of this lane stands for another successful
// hook, and there are at most n - 1 of those: no more than n attempts are ever needed.  The loop still carries that hard
// cap; false: it was reached (the launcher refuses the result).  On success *mine is the root both now hang under.
__device__ __forceinline__ bool comp_unite(uint32_t* parent, uint32_t* mine, uint32_t j, uint64_t n)
    {
    uint32_t a = *mine, b = j;
    for (uint64_t attempt = 0; attempt <= n; attempt++)
        {
        a = comp_find(parent, a);
        b = comp_find(parent, b);
        if (a == b)
            {
            *mine = a;
            return true;
            }
        const uint32_t hi = max(a, b), lo = min(a, b);
        uint32_t expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            {
            *mine = lo;
            return true;
            }
        }
    return false;
    }

// the largest of one 64-bit value per lane (every lane ends with the result)
__device__ __forceinline__ uint64_t comp_wave_max(uint64_t v)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        v = max(v, (uint64_t)__shfl_xor((unsigned long long)v, h, 64));
    return v;
    }

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void comp_open_kernel(const NeighboursArgs a, const uint32_t* flag_dev,
                                                                void* __restrict__ xs, uint32_t* __restrict__ parent,
                                                                uint32_t* __restrict__ size_at)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= a.n || *flag_dev != 0)
        return;
    parent[k] = (uint32_t)k; // (n < 2^32)
    size_at[k] = 0;
    const uint64_t row = a.rows[k];
    if (row >= a.N) // (the check kernel has refused such a list: nothing is loaded for it)
        return;
    compact_position<F64>(a.pos, row, xs, k);
    }

// words[COMP_GAVE_UP]: raised by a lane whose hook reached its cap
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void comp_link_kernel(const NeighboursArgs a, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                uint32_t* parent, unsigned long long* words)
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
    if (c < 0 || (uint32_t)c >= a.n_cells) // an entry without a cell has no edge: a component of its own
        return;
    uint32_t mine = k; // the last root this lane saw above k: an ancestor of k from then on
    bool done = true;
    traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                        [&](uint32_t j, double, double, double, double)
                        {
                            // the half list's filter: the edge i -- j belongs to the smaller list position
                            if (j > k)
                                done = comp_unite(parent, &mine, j, n) && done;
                        });
    if (!done)
        __hip_atomic_store(&words[COMP_GAVE_UP], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }

// label[k] = the root of k.  Other lanes of this launch store roots into the same array while this one walks it: what
// they store is an ancestor of the entry they store it into, so the walk -- whose index strictly decreases -- ends at the
// same root; the accesses stay relaxed atomics so that none is kept in a register.
__global__ __launch_bounds__(SEL_THREADS) void comp_flatten_kernel(uint64_t n, const uint32_t* flag_dev, uint32_t* label,
                                                                   uint32_t* __restrict__ size_at)
    {
    if (*flag_dev != 0)
        return;
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool live = k < n;
    uint32_t x = live ? (uint32_t)k : 0u;
    if (live)
        {
        uint32_t p = comp_load(label, x);
        while (p < x)
            {
            x = p;
            p = comp_load(label, x);
            }
        comp_store(label, (uint32_t)k, x);
        }
    // One add per distinct root of the wave instead of one per lane: neighbours in cell order mostly share their root, and
    // a piece that holds most of the list would otherwise send every lane's add to one word.  Each round retires at least
    // its leader, so the loop ends after at most 64 rounds; it waits for nobody outside the wave.
    const int lane = threadIdx.x & 63;
    bool pending = live;
    for (int round = 0; round < 64; round++)
        {
        const unsigned long long waiting = __ballot(pending);
        if (!waiting)
            break;
        const int leader = __ffsll(waiting) - 1;
        const uint32_t root = (uint32_t)__shfl((int)x, leader, 64);
        const bool mine = pending && x == root;
        const unsigned long long same = __ballot(mine);
        if (lane == leader)
            atomicAdd(&size_at[root], (uint32_t)__popcll(same));
        pending = pending && !mine;
        }
    }

__global__ __launch_bounds__(SEL_THREADS) void comp_roots_kernel(uint64_t n, const uint32_t* flag_dev,
                                                                 const uint32_t* __restrict__ label,
                                                                 const uint32_t* __restrict__ size_at,
                                                                 unsigned long long* __restrict__ block_sums,
                                                                 unsigned long long* words)
    {
    __shared__ unsigned long long s_sum[NLIST_WAVES];
    if (*flag_dev != 0)
        return;
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool root = k < n && label[k] == (uint32_t)k;
    const uint32_t size = root ? size_at[k] : 0u;
    const uint64_t roots = stats_wave_count(root ? 1u : 0u);
    const uint64_t singles = stats_wave_count(root && size == 1u ? 1u : 0u);
    const uint64_t key = comp_wave_max(root ? ((uint64_t)size << 32) | (uint64_t)(~(uint32_t)k) : 0ull);
    if ((threadIdx.x & 63) == 0)
        {
        s_sum[threadIdx.x >> 6] = roots;
        if (singles)
            atomicAdd(&words[3], (unsigned long long)singles);
        if (key)
            atomicMax(&words[COMP_KEY], (unsigned long long)key);
        }
    __syncthreads();
    if (threadIdx.x == 0)
        block_sums[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    }

// One workgroup.  words: n, the entries nowhere, the components, the singletons (counted by comp_roots_kernel), the
// largest size and its label (from the key).
__global__ __launch_bounds__(SEL_THREADS) void comp_scan_kernel(uint64_t n, uint32_t n_cells, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev,
                                                                const unsigned long long* __restrict__ block_sums,
                                                                uint32_t n_blocks, unsigned long long* __restrict__ block_base,
                                                                unsigned long long* words)
    {
    __shared__ uint64_t wave_sums[NLIST_WAVES];
    if (*flag_dev != 0)
        return;
    uint64_t carry = 0; // (every lane keeps the same carry: the round's total comes back from the scan)
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SEL_THREADS)
        {
        const uint32_t i = b0 + threadIdx.x;
        const uint64_t c = i < n_blocks ? block_sums[i] : 0;
        uint64_t total;
        const uint64_t before = nlist_block_scan(c, wave_sums, &total);
        if (i < n_blocks)
            block_base[i] = carry + before;
        carry += total;
        __syncthreads(); // (wave_sums is written again in the next round)
        }
    if (threadIdx.x != 0)
        return;
    const uint64_t key = words[COMP_KEY];
    words[0] = n;
    words[1] = n - min((uint64_t)offs[n_cells], n);
    words[2] = carry;
    words[4] = key >> 32;
    words[5] = (uint64_t)(~(uint32_t)key);
    }

// out_sizes: null, or n words of which the first `components` are written
__global__ __launch_bounds__(SEL_THREADS) void comp_number_kernel(uint64_t n, const uint32_t* flag_dev,
                                                                  const uint32_t* __restrict__ label,
                                                                  const unsigned long long* __restrict__ block_base,
                                                                  uint32_t* __restrict__ size_at, uint32_t* __restrict__ out_sizes)
    {
    __shared__ uint64_t wave_sums[NLIST_WAVES];
    if (*flag_dev != 0)
        return;
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool root = k < n && label[k] == (uint32_t)k;
    uint64_t total;
    const uint64_t id = block_base[blockIdx.x] + nlist_block_scan(root ? 1u : 0u, wave_sums, &total);
    if (!root || id >= n) // (there are no more roots than entries: the clamp never bites on a sound scan)
        return;
    if (out_sizes)
        out_sizes[id] = size_at[k];
    size_at[k] = (uint32_t)id;
    }

__global__ __launch_bounds__(SEL_THREADS) void comp_component_kernel(uint64_t n, const uint32_t* flag_dev,
                                                                     const uint32_t* __restrict__ label,
                                                                     const uint32_t* __restrict__ id_at,
                                                                     uint32_t* __restrict__ out_component)
    {
    if (*flag_dev != 0)
        return;
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t root = label[k];
    if (root < n) // (label[k] <= k: the clamp never bites)
        out_component[k] = id_at[root];
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the cells'
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), size_at (n words: the sizes at the roots, then
// the dense ids), the workgroups' root counts and bases (one 64-bit word each per workgroup) and the eight device words;
// the pinned flag word is the host's view of a refused list, the pinned host block the landing place of the words.
Scratch g_comp_scratch("components", 1.25, 1u << 16, COMP_WORDS * sizeof(uint64_t), sizeof(uint64_t));
std::mutex g_comp_lock;

const char* comp_refused = "a cell id descends or lies outside [0, n_cells], or an entry of the row list lies outside "
                           "the position chunk (nothing was computed)";
    } // namespace

void warm_components_kernels()
    {
    warm_kernel((const void*)comp_scan_kernel);
    }

int launch_components(const NeighboursArgs& a, uint32_t* out_label, uint32_t* out_component, uint32_t* out_sizes,
                      uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "components";
    static_assert(COMPONENTS_SUMMARY_WORDS <= COMP_KEY, "the summary words come first");
    if (!out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint64_t n = a.n;
    if (n == 0)
        {
        std::fill(out_summary, out_summary + COMPONENTS_SUMMARY_WORDS, (uint64_t)0);
        return PGSD_SUCCESS;
        }
    if (!out_label)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.N == 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + comp_refused);
    if (!a.rows || !a.cell || !a.pos)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t n_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    const size_t xs_bytes = round16((size_t)n * 3 * (a.f64 ? sizeof(double) : sizeof(float)));
    const size_t size_bytes = round16((size_t)n * sizeof(uint32_t));
    const size_t sums_bytes = round16((size_t)n_blocks * sizeof(uint64_t));
    const size_t words_bytes = COMP_WORDS * sizeof(uint64_t);
    LaunchScope scope(g_comp_lock, g_comp_scratch, 16 + offs_bytes + xs_bytes + size_bytes + 2 * sums_bytes + words_bytes, stream,
                      err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    uint32_t* size_at = (uint32_t*)((char*)xs + xs_bytes);
    unsigned long long* block_sums = (unsigned long long*)((char*)size_at + size_bytes);
    unsigned long long* block_base = (unsigned long long*)((char*)block_sums + sums_bytes);
    unsigned long long* words = (unsigned long long*)((char*)block_base + sums_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   words, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(comp_open_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs, out_label, size_at);
            hipLaunchKernelGGL(comp_link_kernel<true>, per_entry, block, 0, stream, a, offs, flag_dev, xs, out_label, words);
            }
        else
            {
            hipLaunchKernelGGL(comp_open_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs, out_label, size_at);
            hipLaunchKernelGGL(comp_link_kernel<false>, per_entry, block, 0, stream, a, offs, flag_dev, xs, out_label, words);
            }
        hipLaunchKernelGGL(comp_flatten_kernel, per_entry, block, 0, stream, n, flag_dev, out_label, size_at);
        hipLaunchKernelGGL(comp_roots_kernel, per_entry, block, 0, stream, n, flag_dev, out_label, size_at, block_sums, words);
        hipLaunchKernelGGL(comp_scan_kernel, dim3(1), block, 0, stream, n, a.n_cells, offs, flag_dev, block_sums, n_blocks,
                           block_base, words);
        if (out_component || out_sizes)
            hipLaunchKernelGGL(comp_number_kernel, per_entry, block, 0, stream, n, flag_dev, out_label, block_base, size_at,
                               out_sizes);
        if (out_component)
            hipLaunchKernelGGL(comp_component_kernel, per_entry, block, 0, stream, n, flag_dev, out_label, size_at, out_component);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, words, words_bytes, hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + comp_refused);
    const uint64_t* landed = (const uint64_t*)scope.mem().host;
    if (landed[COMP_GAVE_UP] != 0)
        return launch_fail(err, PGSD_ERROR_DEVICE, std::string(what) + ": the pass gave up: internal error (a hook reached the "
                                                   "cap of its retries; the outputs are unspecified)");
    std::copy(landed, landed + COMPONENTS_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
