// pgsd_component_moments.hip -- component fields on gfx950: mass, momentum, kinetic and internal energy, first moment,
// origin and extent per connected component of a row list (pgsd_components_device leaves the labels and the dense ids).
// pgsd.hoomd.component_moments is the definition and this file equals it exactly, sums included.  A frame can have as many
// components as entries, so the segment key is the dense id, the entries are SORTED by it (the cell order's stable radix
// sort, through enqueue_sort_pairs) and every result stays in the caller's device arrays.  The sum of a component is the
// cell fields' (pgsd_cells.hip) over the component's entries in list order: pieces of 1024 entries counted from the
// component's first entry, 64 lanes striding by 64, the wave tree, the piece sums added to +0.0 in ascending order, a
// value that is not finite counting as +0.0.  The position enters as the single-shift minimum-image displacement from the
// component's ROOT -- its smallest member, the first entry of its sorted segment -- to the entry; the root's own
// displacement is +0.0 by definition.
//   cmom_key_kernel      lane per entry: label[k] > k, a label that is no root, an id >= components or other than its
//                        root's, a row >= N raise both flag words (the cell fields' protocol); key = the id, value = k
//   (sort)               the pairs by key, stably: order_passes(components - 1) passes
//   cmom_offsets_kernel  lane per c in [0, components]: the lower bound of c in the sorted keys
//   cmom_verify_kernel   what only the sorted list shows: every component has an entry, every entry's label is its
//                        segment's first entry, and the first entries ascend with the id -- the ids are the dense ascending
//                        numbering of the labels
//   cmom_piece_kernel    one WAVE per slab of 1024 sorted entries: the cell fields' walk, pgsd_pieces.hpp's
//                        pieces_walk_slab, with this unit's policy; the root's position is wave-uniform per piece; the
//                        extent goes through a wave min / max with strict comparisons from +0.0, so neither bound is
//                        ever -0.0
//   cmom_long_kernel     lane per slab and word: the piece sums of a component of more than 1024 entries added to +0.0 in
//                        ascending order, its counters added, its extents merged
//   cmom_flags_kernel    lane per component: wide, and the wave's share of the summary through integer atomics (counts
//                        added, the largest mass and span as order-preserving integer keys)
//   cmom_pick_kernel     lane per component: the smallest id that attains each largest key
// Every kernel behind the first reads the device flag first and does nothing where it is set; whatever is derived from
// offsets, labels, ids or sorted values is clamped to n or components before it indexes anything.  No atomic on a float,
// no result depends on the launch grid, no spin, no contraction wherever a value is formed or added.
#include "pgsd_pieces.hpp"
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
#define CMOM_WAVES (SEL_THREADS / 64)
enum
    {
    CMOM_Q = MOMENTS_QUANTITIES,
    CMOM_SLOT_WORDS = CMOM_Q + 1 + CMOM_EXTENT, // nine sums, the bad entries (a 64-bit counter), lo[3], hi[3]
    CMOM_NO_PIECE = PIECES_NONE,
    CMOM_WORK_BYTES = 48 // bad entries, wide components, the largest mass key, the largest span key (64 bits each); two ids
    };

__device__ __forceinline__ void cmom_raise(uint32_t* flag_dev, uint32_t* flag_host)
    {
    __hip_atomic_store(flag_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(flag_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }

__global__ __launch_bounds__(SEL_THREADS) void cmom_key_kernel(const ComponentMomentsArgs s, uint32_t* keys, uint32_t* vals,
                                                               uint32_t* flag_dev, uint32_t* flag_host)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= s.n)
        return;
    const uint32_t l = s.label[k], c = s.component[k];
    bool bad = l > k || c >= s.components || s.rows[k] >= s.N;
    if (!bad) // (l <= k < n)
        bad = s.label[l] != l || s.component[l] != c;
    if (bad)
        cmom_raise(flag_dev, flag_host);
    keys[k] = min(c, s.components - 1u);
    vals[k] = (uint32_t)k;
    }

__global__ __launch_bounds__(SEL_THREADS) void cmom_offsets_kernel(const uint32_t* keys, uint64_t n, uint32_t components,
                                                                   const uint32_t* flag_dev, uint32_t* offs)
    {
    const uint64_t c = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (c > components || *flag_dev != 0)
        return;
    uint64_t lo = 0, hi = n; // the first sorted position whose id is not below c
    while (lo < hi)
        {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)keys[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
        }
    offs[c] = (uint32_t)lo;
    }

__global__ __launch_bounds__(SEL_THREADS) void cmom_verify_kernel(const uint32_t* label, const uint32_t* keys, const uint32_t* vals,
                                                                  const uint32_t* offs, uint64_t n, uint32_t components,
                                                                  uint32_t* flag_dev, uint32_t* flag_host)
    {
    const uint64_t p = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (p >= n + components || *flag_dev != 0)
        return;
    bool bad;
    if (p < n)
        {
        // the entry's label is the first entry of its segment
        const uint64_t k = min((uint64_t)vals[p], n - 1);
        const uint32_t c = min(keys[p], components - 1u);
        const uint64_t o = min((uint64_t)offs[c], n - 1);
        bad = label[k] != vals[o];
        }
    else
        {
        // the segment is not empty, and its first entry lies below the next segment's
        const uint32_t c = (uint32_t)(p - n);
        const uint64_t lo = min((uint64_t)offs[c], n), hi = min((uint64_t)offs[c + 1], n);
        bad = hi <= lo;
        if (!bad && c + 1u < components)
            bad = vals[lo] >= vals[min(hi, n - 1)];
        }
    if (bad)
        cmom_raise(flag_dev, flag_host);
    }

// one element of a staged float chunk as a double (a wave-uniform address: the root's position)
template<bool F64> __device__ __forceinline__ double cmom_scalar(const void* base, uint64_t at)
    {
    if constexpr (F64)
        return ((const double*)base)[at];
    else
        return (double)((const float*)base)[at];
    }

// the smaller / the larger of two bounds by a strict comparison (neither is a NaN, neither is -0.0)
__device__ __forceinline__ double cmom_lower(double a, double b)
    {
    return b < a ? b : a;
    }
__device__ __forceinline__ double cmom_upper(double a, double b)
    {
    return b > a ? b : a;
    }
__device__ __forceinline__ double cmom_wave_lower(double p)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        p = cmom_lower(p, __shfl_xor(p, h, 64));
    return p;
    }
__device__ __forceinline__ double cmom_wave_upper(double p)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        p = cmom_upper(p, __shfl_xor(p, h, 64));
    return p;
    }

// The walk over a slab's piece starts, the steps of a piece, the nine values and the two-slot partials table are
// pgsd_pieces.hpp's, shared with the cell fields.  What is the component fields' own: the segment id is the sorted key,
// an entry is reached through the sorted values and the list, the position is replaced by the displacement from the
// piece's root (three wave-uniform loads per piece), and a piece carries its extent beside its sums.
template<bool F64> struct ComponentPieces
    {
    static constexpr int BATCH = 2; // steps a lane has in flight
    const ComponentMomentsArgs& s;
    const uint32_t* __restrict__ keys;
    const uint32_t* __restrict__ vals;
    double* __restrict__ out_sums;
    double* __restrict__ out_extent;
    double* __restrict__ out_origin;
    uint32_t* __restrict__ out_flags;
    double* __restrict__ part;
    uint32_t segments;
    // of the piece that is open
    uint32_t root;
    double x0[3], lo[3], hi[3];
    bool is_root[BATCH];

    __device__ __forceinline__ uint32_t id(uint64_t p) const
        {
        return keys[p];
        }
    __device__ __forceinline__ bool summed(uint32_t id) const
        {
        return id < segments;
        }
    // the root: the first entry of the sorted segment (the sort is stable: the component's smallest member)
    __device__ __forceinline__ void open(uint32_t c, uint64_t c_lo)
        {
        const uint64_t n = s.n;
        root = min((uint32_t)__builtin_amdgcn_readfirstlane(vals[min(c_lo, n - 1)]), (uint32_t)(n - 1));
        const uint64_t root_row = s.rows[root];
#pragma unroll
        for (int a = 0; a < 3; a++)
            x0[a] = lo[a] = hi[a] = 0.0;
        if (s.chunk[4] && root_row < s.N) // (the check kernel has refused a list with such a row)
            {
#pragma unroll
            for (int a = 0; a < 3; a++)
                x0[a] = cmom_scalar<F64>(s.chunk[4], root_row * 3 + a);
            }
        }
    __device__ __forceinline__ uint64_t row(uint64_t p, bool ok, int i)
        {
        const uint32_t k = ok ? min(vals[p], (uint32_t)(s.n - 1)) : 0u;
        is_root[i] = k == root;
        return ok ? s.rows[k] : 0;
        }
    // root -> entry under the single-shift minimum image (pgsd.hoomd.pair_displacement): z, then y, then x; the root's own
    // displacement is +0.0 by definition; the extent takes what is finite by strict comparisons
    __device__ __forceinline__ void place(double* x, bool ok, int i)
        {
#pragma clang fp contract(off)
        const double Lx = s.vectors[0], Ly = s.vectors[1], Lz = s.vectors[2];
        const double xyLy = s.vectors[3], xzLz = s.vectors[4], yzLz = s.vectors[5];
        const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5; // (exact halves)
        double dx = x[0] - x0[0], dy = x[1] - x0[1], dz = 0.0;
        if (s.dimensions != 2)
            {
            dz = x[2] - x0[2];
            const bool up = dz >= hz, down = dz < -hz;
            dx = up ? dx - xzLz : (down ? dx + xzLz : dx);
            dy = up ? dy - yzLz : (down ? dy + yzLz : dy);
            dz = up ? dz - Lz : (down ? dz + Lz : dz);
            }
            {
            const bool up = dy >= hy, down = dy < -hy;
            dx = up ? dx - xyLy : (down ? dx + xyLy : dx);
            dy = up ? dy - Ly : (down ? dy + Ly : dy);
            }
            {
            const bool up = dx >= hx, down = dx < -hx;
            dx = up ? dx - Lx : (down ? dx + Lx : dx);
            }
        x[0] = is_root[i] ? 0.0 : dx;
        x[1] = is_root[i] ? 0.0 : dy;
        x[2] = is_root[i] ? 0.0 : dz;
#pragma unroll
        for (int a = 0; a < 3; a++)
            {
            const bool fin = __builtin_fabs(x[a]) < __builtin_huge_val(); // (false for a NaN as well)
            if (ok && fin)
                {
                lo[a] = cmom_lower(lo[a], x[a]);
                hi[a] = cmom_upper(hi[a], x[a]);
                }
            }
        }
    __device__ __forceinline__ void close(uint32_t c, uint32_t w, bool is_long, bool is_first, const double* sum, uint64_t n_bad,
                                          uint32_t lane)
        {
        constexpr int Q = CMOM_Q;
#pragma unroll
        for (int a = 0; a < 3; a++)
            {
            lo[a] = cmom_wave_lower(lo[a]);
            hi[a] = cmom_wave_upper(hi[a]);
            }
        if (lane != 0)
            return;
        if (is_long)
            {
            double* out = part + ((size_t)2 * w + (is_first ? 1 : 0)) * CMOM_SLOT_WORDS;
#pragma unroll
            for (int q = 0; q < Q; q++)
                out[q] = sum[q];
            ((uint64_t*)out)[Q] = n_bad;
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                out[Q + 1 + a] = lo[a];
                out[Q + 4 + a] = hi[a];
                }
            }
        else
            {
#pragma unroll
            for (int q = 0; q < Q; q++)
                out_sums[(size_t)c * Q + q] = sum[q];
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                out_extent[(size_t)c * CMOM_EXTENT + a] = lo[a];
                out_extent[(size_t)c * CMOM_EXTENT + 3 + a] = hi[a];
                }
            out_flags[(size_t)2 * c] = (uint32_t)n_bad;
            }
        if (is_first)
            {
#pragma unroll
            for (int a = 0; a < 3; a++)
                out_origin[(size_t)c * 3 + a] = x0[a];
            }
        }
    };

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void cmom_piece_kernel(const ComponentMomentsArgs s, const uint32_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ vals, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, double* __restrict__ out_sums,
                                                                 double* __restrict__ out_extent, double* __restrict__ out_origin,
                                                                 uint32_t* __restrict__ out_flags, double* __restrict__ part,
                                                                 uint32_t* __restrict__ first, uint32_t n_slabs)
    {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * CMOM_WAVES + (threadIdx.x >> 6));
    if (w >= n_slabs || *flag_dev != 0)
        return;
    ComponentPieces<F64> P = {s, keys, vals, out_sums, out_extent, out_origin, out_flags, part, s.components};
    pieces_walk_slab<F64>(s, P, offs, w, lane, first);
    }

__global__ __launch_bounds__(SEL_THREADS) void cmom_long_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const double* __restrict__ part,
                                                                const uint32_t* __restrict__ first, uint64_t n, uint32_t components,
                                                                uint32_t n_slabs, double* __restrict__ out_sums,
                                                                double* __restrict__ out_extent, uint32_t* __restrict__ out_flags)
    {
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t w = (uint32_t)(i / CMOM_SLOT_WORDS), q = (uint32_t)(i % CMOM_SLOT_WORDS);
    if (i / CMOM_SLOT_WORDS >= n_slabs || *flag_dev != 0)
        return;
    const uint32_t at = first[w];
    if (at == CMOM_NO_PIECE || at >= n)
        return;
    const uint32_t c = min(keys[at], components - 1u);
    const uint64_t c_lo = min((uint64_t)offs[c], n), c_hi = min((uint64_t)offs[c + 1], n);
    double sum = 0.0; // a sum, or a bound of the extent (which starts at +0.0 too)
    uint64_t count = 0;
    pieces_long_slots<CMOM_SLOT_WORDS>(part, w, c_lo, c_hi, n_slabs, [&](const double* slot)
                                       {
                                       if (q < CMOM_Q)
                                           sum = sum + slot[q];
                                       else if (q == CMOM_Q)
                                           count += ((const uint64_t*)slot)[CMOM_Q];
                                       else if (q < CMOM_Q + 4)
                                           sum = cmom_lower(sum, slot[q]);
                                       else
                                           sum = cmom_upper(sum, slot[q]);
                                       });
    if (q < CMOM_Q)
        out_sums[(size_t)c * CMOM_Q + q] = sum;
    else if (q == CMOM_Q)
        out_flags[(size_t)2 * c] = (uint32_t)count;
    else
        out_extent[(size_t)c * CMOM_EXTENT + (q - CMOM_Q - 1)] = sum;
    }

// an integer that orders like the double; a NaN (a sum whose pieces overflowed both ways) orders like -inf, and every
// key is above 0, the word's initial value
__device__ __forceinline__ unsigned long long cmom_order_key(double x)
    {
    if (x != x)
        x = -__builtin_huge_val();
    if (x == 0.0)
        x = 0.0; // (-0.0 and +0.0 are one value)
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
    }

__device__ __forceinline__ unsigned long long cmom_wave_max(unsigned long long v)
    {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        const unsigned long long o = __shfl_xor(v, h, 64);
        v = o > v ? o : v;
        }
    return v;
    }

// the largest extent over the axes of one component
__device__ __forceinline__ double cmom_span(const double* __restrict__ out_extent, uint32_t c)
    {
#pragma clang fp contract(off)
    double span = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        span = cmom_upper(span, out_extent[(size_t)c * CMOM_EXTENT + 3 + a] - out_extent[(size_t)c * CMOM_EXTENT + a]);
    return span;
    }

// work: 64-bit words bad, wide, mass key, span key; then the 32-bit ids heaviest, widest
__global__ __launch_bounds__(SEL_THREADS) void cmom_flags_kernel(const ComponentMomentsArgs s, const uint32_t* flag_dev,
                                                                 const double* __restrict__ out_sums,
                                                                 const double* __restrict__ out_extent,
                                                                 uint32_t* __restrict__ out_flags, unsigned long long* work)
    {
#pragma clang fp contract(off)
    if (*flag_dev != 0)
        return;
    const uint64_t i = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const bool active = i < s.components;
    const uint32_t c = active ? (uint32_t)i : 0u;
    uint32_t wide = 0;
    const uint32_t dims = s.dimensions == 2 ? 2u : 3u;
#pragma unroll
    for (int a = 0; a < 3; a++)
        {
        const double span = out_extent[(size_t)c * CMOM_EXTENT + 3 + a] - out_extent[(size_t)c * CMOM_EXTENT + a];
        if ((uint32_t)a < dims && span >= s.vectors[a] * 0.5)
            wide = 1;
        }
    if (active)
        out_flags[(size_t)2 * c + 1] = wide;
    const uint64_t n_bad = stats_wave_count(active ? out_flags[(size_t)2 * c] : 0u);
    const uint64_t n_wide = stats_wave_count(active ? wide : 0u);
    const unsigned long long k_mass = cmom_wave_max(active ? cmom_order_key(out_sums[(size_t)c * CMOM_Q]) : 0ull);
    const unsigned long long k_span = cmom_wave_max(active ? cmom_order_key(cmom_span(out_extent, c)) : 0ull);
    if ((threadIdx.x & 63) == 0)
        {
        if (n_bad)
            atomicAdd(&work[0], (unsigned long long)n_bad);
        if (n_wide)
            atomicAdd(&work[1], (unsigned long long)n_wide);
        // (a word only grows: a key that is not above what the word holds already cannot change it, and most are not)
        if (k_mass > __hip_atomic_load(&work[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&work[2], k_mass);
        if (k_span > __hip_atomic_load(&work[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(&work[3], k_span);
        }
    }

__global__ __launch_bounds__(SEL_THREADS) void cmom_pick_kernel(uint32_t components, const uint32_t* flag_dev,
                                                                const double* __restrict__ out_sums,
                                                                const double* __restrict__ out_extent, unsigned long long* work)
    {
    if (*flag_dev != 0)
        return;
    const uint64_t i = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (i >= components)
        return;
    const uint32_t c = (uint32_t)i;
    uint32_t* ids = (uint32_t*)(work + 4);
    if (cmom_order_key(out_sums[(size_t)c * CMOM_Q]) == work[2])
        atomicMin(&ids[0], c);
    if (cmom_order_key(cmom_span(out_extent, c)) == work[3])
        atomicMin(&ids[1], c);
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// summary's work words (48), two key and two value buffers of n words, the sort's digit table and totals, the offsets
// (components + 1 words), the slabs' first long pieces (one word each) and the partials (two slots of sixteen words per
// slab); the pinned flag word is the host's view of a refused list.
Scratch g_cmom_scratch("component fields", 1.25, 1u << 16, 0, sizeof(uint64_t));
std::mutex g_cmom_lock;
const char* const cmom_refused = "label and component are not a components result of this list (a label above its entry or "
                                 "that is no root, an id that is not the dense ascending number of its label or lies outside "
                                 "[0, components)), or an entry of the row list lies outside the chunks (nothing was computed)";
    } // namespace

void warm_component_moments_kernels()
    {
    warm_kernel((const void*)cmom_offsets_kernel);
    }

int launch_component_moments(const ComponentMomentsArgs& a, double* out_sums, double* out_extent, double* out_origin,
                             uint32_t* out_flags, uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "component fields";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_sums || !out_extent || !out_origin || !out_flags || !out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint64_t n = a.n;
    const uint32_t components = a.components;
    if (n == 0 || n >= (1ull << 32))
        return fail("a list holds 1 to 2^32 - 1 entries");
    if (a.N >= (1ull << 32) + 1)
        return fail("2^32 rows or entries and more are not indexed");
    if (components < 1 || components > n)
        return fail("a list of n entries has 1 to n components");
    if (a.N == 0)
        return fail(cmom_refused);
    if (!a.rows || !a.label || !a.component || !(a.present & (1u << 4)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    for (int i = 1; i < GROUPED_CHUNKS; i++)
        if ((a.present & (1u << i)) && !a.chunk[i])
            return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t n_slabs = (uint32_t)((n + CELLS_PIECE - 1) / CELLS_PIECE);
    const size_t list_bytes = round16((size_t)n * sizeof(uint32_t));
    const size_t table_bytes = round16(sort_pairs_table_words(n) * sizeof(uint32_t)), totals_bytes = 256 * sizeof(uint32_t);
    const size_t offs_bytes = round16(((size_t)components + 1) * sizeof(uint32_t)), first_bytes = round16((size_t)n_slabs * sizeof(uint32_t));
    const size_t part_bytes = (size_t)n_slabs * 2 * CMOM_SLOT_WORDS * sizeof(double);
    const size_t head = 16 + CMOM_WORK_BYTES;
    LaunchScope scope(g_cmom_lock, g_cmom_scratch,
                      head + 4 * list_bytes + table_bytes + totals_bytes + offs_bytes + first_bytes + part_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    unsigned long long* work = (unsigned long long*)(dev + 16);
    char* at = dev + head;
    uint32_t* keys[2] = {(uint32_t*)at, (uint32_t*)(at + list_bytes)};
    uint32_t* vals[2] = {(uint32_t*)(at + 2 * list_bytes), (uint32_t*)(at + 3 * list_bytes)};
    at += 4 * list_bytes;
    uint32_t* table = (uint32_t*)at;
    uint32_t* totals = (uint32_t*)(at + table_bytes);
    at += table_bytes + totals_bytes;
    uint32_t* offs = (uint32_t*)at;
    uint32_t* first = (uint32_t*)(at + offs_bytes);
    double* part = (double*)(at + offs_bytes + first_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    uint32_t* host_flag_dev = (uint32_t*)scope.mem().mapped_dev;
    const dim3 block(SEL_THREADS);
    const auto blocks_for = [](uint64_t lanes) { return dim3((unsigned)((lanes + SEL_THREADS - 1) / SEL_THREADS)); };
    __atomic_store_n(host_flag, 0u, __ATOMIC_RELEASE);
    // the flag and the counters at zero, the two ids at "none"
    hipError_t e = hipMemsetAsync(dev, 0, 16 + 32, stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(dev + 16 + 32, 0xFF, 16, stream);
    if (e == hipSuccess)
        {
        hipLaunchKernelGGL(cmom_key_kernel, blocks_for(n), block, 0, stream, a, keys[0], vals[0], flag_dev, host_flag_dev);
        const unsigned r = enqueue_sort_pairs(keys, vals, table, totals, n, (uint64_t)components - 1, stream);
        hipLaunchKernelGGL(cmom_offsets_kernel, blocks_for((uint64_t)components + 1), block, 0, stream, keys[r], n, components,
                           flag_dev, offs);
        hipLaunchKernelGGL(cmom_verify_kernel, blocks_for(n + components), block, 0, stream, a.label, keys[r], vals[r], offs, n,
                           components, flag_dev, host_flag_dev);
        const dim3 per_slab((n_slabs + CMOM_WAVES - 1) / CMOM_WAVES);
        if (a.f64)
            hipLaunchKernelGGL(cmom_piece_kernel<true>, per_slab, block, 0, stream, a, keys[r], vals[r], offs, flag_dev, out_sums,
                               out_extent, out_origin, out_flags, part, first, n_slabs);
        else
            hipLaunchKernelGGL(cmom_piece_kernel<false>, per_slab, block, 0, stream, a, keys[r], vals[r], offs, flag_dev, out_sums,
                               out_extent, out_origin, out_flags, part, first, n_slabs);
        hipLaunchKernelGGL(cmom_long_kernel, blocks_for((uint64_t)n_slabs * CMOM_SLOT_WORDS), block, 0, stream, keys[r], offs,
                           flag_dev, part, first, n, components, n_slabs, out_sums, out_extent, out_flags);
        hipLaunchKernelGGL(cmom_flags_kernel, blocks_for(components), block, 0, stream, a, flag_dev, out_sums, out_extent, out_flags,
                           work);
        hipLaunchKernelGGL(cmom_pick_kernel, blocks_for(components), block, 0, stream, components, flag_dev, out_sums, out_extent,
                           work);
        e = hipGetLastError();
        }
    uint64_t h_work[CMOM_WORK_BYTES / sizeof(uint64_t)] = {};
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_work, work, CMOM_WORK_BYTES, hipMemcpyDeviceToHost, stream);
    int rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return fail(cmom_refused);
    const uint32_t* ids = (const uint32_t*)(h_work + 4);
    out_summary[0] = n;
    out_summary[1] = components;
    out_summary[2] = h_work[0];
    out_summary[3] = h_work[1];
    out_summary[4] = ids[0];
    out_summary[5] = ids[1];
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
