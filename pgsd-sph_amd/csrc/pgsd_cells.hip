// pgsd_cells.hip -- cell fields on gfx950: mass, momentum, kinetic and internal energy and first moment per grid cell of
// a row list in cell order (pgsd_order_rows_by_cell_device leaves such a list and its cell ids).  pgsd.hoomd.cell_moments
// is the definition and this file equals it exactly, sums included.  A grid has up to 2^20 cells, so the sum is
// SEGMENTED and its order is the cell's own -- it depends on the cell's entries alone, not on where the cell lies in the
// list, on the grid of the launch or on the device:
//   a cell's entries, in list order, are cut into PIECES of 1024 counted from the cell's first entry; in a piece lane l of
//   64 adds entries l, l + 64, ... to +0.0 (an entry past the end and a value that is not finite add +0.0); the 64 lane
//   sums go through the wave tree of the statistics (p[i] += p[i + h], h = 32 .. 1); the piece sums are added to +0.0 in
//   ascending order.
//   cells_check_kernel     lane per entry: a row >= N, an id outside [0, n_cells] or below its predecessor raises both
//                          flag words (order_key_kernel's protocol); every later kernel reads the device flag first and
//                          does nothing where it is set, and clamps what it derives from the offsets to n
//   cells_offsets_kernel   lane per c in [0, n_cells + 1]: offs[c] = the lower bound of c in cell[0 .. n), by binary
//                          search; one writer per word, plain stores, nothing to clear
//   cells_piece_kernel     one WAVE per slab of 1024 consecutive sorted entries, four per workgroup; the wave owns the
//                          pieces that START in its slab (k is a start iff cell[k] < n_cells and (k - offs[cell[k]]) %
//                          1024 == 0), found by ballot and handled in ascending order; per piece ceil(len / 64)
//                          wave-uniform steps of gathered loads, nine trees and one counter.  A wave touches at most 2047
//                          entries whatever the grid.  The piece of a cell of at most 1024 entries is the cell: lane 0
//                          stores it into the result table.  A longer cell's pieces go to a partials table of TWO slots
//                          per slab (the argument is at the kernel)
//   cells_long_kernel      lane per slab and value: where the slab holds the first piece of a long cell the lane adds
//                          that cell's piece sums to +0.0 in ascending order and stores the result
// No global atomic on a float, no contraction wherever a value is formed or added.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp; the order of the sum, shared with the component fields: pgsd_pieces.hpp; the launchers' host side:
// pgsd_scratch.hpp.
#include "pgsd_pieces.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
#define CELLS_WAVES (SEL_THREADS / 64)
enum
    {
    CELLS_Q = MOMENTS_QUANTITIES,
    CELLS_SLOT_WORDS = CELLS_Q + 1, // nine sums and the bad entries (a 64-bit counter) of a piece
    CELLS_NO_PIECE = PIECES_NONE
    };

__device__ __forceinline__ void cells_raise(uint32_t* flag_dev, uint32_t* flag_host)
    {
    __hip_atomic_store(flag_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(flag_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }

// rows: null for the offsets call, which has no rows to check
__global__ __launch_bounds__(SEL_THREADS) void cells_check_kernel(const uint32_t* rows, const int32_t* cell, uint64_t n,
                                                                  uint64_t N, uint32_t n_cells, uint32_t* flag_dev,
                                                                  uint32_t* flag_host)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= n)
        return;
    const int32_t c = cell[k];
    bool bad = c < 0 || (uint32_t)c > n_cells || (k > 0 && c < cell[k - 1]);
    if (rows)
        bad = bad || rows[k] >= N;
    if (bad)
        cells_raise(flag_dev, flag_host);
    }

__global__ __launch_bounds__(SEL_THREADS) void cells_offsets_kernel(const int32_t* cell, uint64_t n, uint32_t n_cells,
                                                                    const uint32_t* flag_dev, uint32_t* offs)
    {
    const uint32_t c = blockIdx.x * SEL_THREADS + threadIdx.x;
    if (c > n_cells + 1u || *flag_dev != 0)
        return;
    uint64_t lo = 0, hi = n; // the first position whose id is not below c
    while (lo < hi)
        {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)cell[mid] < (int64_t)c)
            lo = mid + 1;
        else
            hi = mid;
        }
    offs[c] = (uint32_t)lo;
    }

// The walk over a slab's piece starts, the steps of a piece, the nine values and the two-slot partials table (with the
// argument why two slots suffice) are pgsd_pieces.hpp's, shared with the component fields.  What is the cell fields' own:
// the segment id is the cell id, the row is the list's, the position is summed as it is, and a piece lands in the result
// table or in its slot of the partials.
struct CellsPieces
    {
    static constexpr int BATCH_F32 = 4, BATCH_F64 = 2; // steps a lane has in flight (up to 16 and 8 words each)
    const int32_t* cell;
    const uint32_t* rows;
    double* __restrict__ table;
    uint64_t* __restrict__ table_bad;
    double* __restrict__ part;
    uint32_t segments;
    __device__ __forceinline__ uint32_t id(uint64_t p) const
        {
        return (uint32_t)cell[p];
        }
    __device__ __forceinline__ bool summed(uint32_t id) const
        {
        return (int32_t)id >= 0 && id < segments;
        }
    __device__ __forceinline__ void open(uint32_t, uint64_t) const {}
    __device__ __forceinline__ uint64_t row(uint64_t p, bool ok, int) const
        {
        return ok ? rows[p] : 0;
        }
    __device__ __forceinline__ void place(double*, bool, int) const {}
    __device__ __forceinline__ void close(uint32_t c, uint32_t w, bool is_long, bool is_first, const double* sum, uint64_t n_bad,
                                          uint32_t lane) const
        {
        if (lane == 0)
            {
            double* out = is_long ? part + ((size_t)2 * w + (is_first ? 1 : 0)) * CELLS_SLOT_WORDS : table + (size_t)c * CELLS_Q;
#pragma unroll
            for (int q = 0; q < CELLS_Q; q++)
                out[q] = sum[q];
            if (is_long)
                ((uint64_t*)out)[CELLS_Q] = n_bad;
            else
                table_bad[c] = n_bad;
            }
        }
    };
template<bool F64> struct CellsPiecesOf : CellsPieces
    {
    static constexpr int BATCH = F64 ? CellsPieces::BATCH_F64 : CellsPieces::BATCH_F32;
    };

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void cells_piece_kernel(const CellMomentsArgs s, const uint32_t* __restrict__ offs,
                                                                  const uint32_t* flag_dev, double* __restrict__ table,
                                                                  uint64_t* __restrict__ table_bad, double* __restrict__ part,
                                                                  uint32_t* __restrict__ first, uint32_t n_slabs)
    {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * CELLS_WAVES + (threadIdx.x >> 6));
    if (w >= n_slabs || *flag_dev != 0)
        return;
    CellsPiecesOf<F64> P;
    P.cell = s.cell;
    P.rows = s.rows;
    P.table = table;
    P.table_bad = table_bad;
    P.part = part;
    P.segments = s.n_cells;
    pieces_walk_slab<F64>(s, P, offs, w, lane, first);
    }

__global__ __launch_bounds__(SEL_THREADS) void cells_long_kernel(const int32_t* __restrict__ cell, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const double* __restrict__ part,
                                                                 const uint32_t* __restrict__ first, uint64_t n,
                                                                 uint32_t n_cells, uint32_t n_slabs, double* __restrict__ table,
                                                                 uint64_t* __restrict__ table_bad)
    {
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t w = (uint32_t)(i / CELLS_SLOT_WORDS), q = (uint32_t)(i % CELLS_SLOT_WORDS);
    if (w >= n_slabs || *flag_dev != 0)
        return;
    const uint32_t at = first[w];
    if (at == CELLS_NO_PIECE || at >= n)
        return;
    const uint32_t c = min((uint32_t)cell[at], n_cells - 1u);
    const uint64_t c_lo = min((uint64_t)offs[c], n), c_hi = min((uint64_t)offs[c + 1], n);
    double sum = 0.0;
    uint64_t count = 0;
    pieces_long_slots<CELLS_SLOT_WORDS>(part, w, c_lo, c_hi, n_slabs, [&](const double* slot)
                                        {
                                        if (q < CELLS_Q)
                                            sum = sum + slot[q];
                                        else
                                            count += ((const uint64_t*)slot)[CELLS_Q];
                                        });
    if (q < CELLS_Q)
        table[(size_t)c * CELLS_Q + q] = sum;
    else
        table_bad[c] = count;
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the slabs' first long pieces (one word each), the result table (n_cells x 9 doubles and
// n_cells counters) and the partials (two slots of ten words per slab); the pinned flag word is the host's view of a
// refused list.
Scratch g_cells_scratch("cell fields", 1.25, 1u << 16, 0, sizeof(uint64_t));
std::mutex g_cells_lock;

int cells_arguments(uint64_t n, uint32_t n_cells, std::string* err, const char* what)
    {
    if (n >= (1ull << 32))
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": a list holds fewer than 2^32 entries");
    if (n_cells < 1 || n_cells > CELLS_MAX_CELLS)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": a grid holds 1 to 2^20 cells");
    return PGSD_SUCCESS;
    }
    } // namespace

void warm_cells_kernels()
    {
    warm_kernel((const void*)cells_offsets_kernel);
    }

int launch_cell_offsets(const int32_t* cell, uint64_t n, uint32_t n_cells, uint32_t* out_offsets, hipStream_t stream,
                        std::string* err)
    {
    static const char* what = "cell offsets";
    int rc = cells_arguments(n, n_cells, err, what);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (!out_offsets || (n > 0 && !cell))
        return PGSD_ERROR_INVALID_ARGUMENT;
    LaunchScope scope(g_cells_lock, g_cells_scratch, 16, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    uint32_t* flag_dev = (uint32_t*)scope.mem().dev;
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    __atomic_store_n(host_flag, 0u, __ATOMIC_RELEASE);
    const dim3 block(SEL_THREADS);
    hipError_t e;
    if (n == 0)
        e = hipMemsetAsync(out_offsets, 0, ((size_t)n_cells + 2) * sizeof(uint32_t), stream);
    else
        {
        e = hipMemsetAsync(flag_dev, 0, sizeof(uint32_t), stream);
        if (e == hipSuccess)
            {
            hipLaunchKernelGGL(cells_check_kernel, dim3((unsigned)((n + SEL_THREADS - 1) / SEL_THREADS)), block, 0, stream,
                               (const uint32_t*)nullptr, cell, n, (uint64_t)0, n_cells, flag_dev,
                               (uint32_t*)scope.mem().mapped_dev);
            hipLaunchKernelGGL(cells_offsets_kernel, dim3((n_cells + 2 + SEL_THREADS - 1) / SEL_THREADS), block, 0, stream, cell,
                               n, n_cells, flag_dev, out_offsets);
            e = hipGetLastError();
            }
        }
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT,
                           std::string(what) + ": a cell id descends or lies outside [0, n_cells] (nothing was written)");
    return PGSD_SUCCESS;
    }

int launch_cell_moments(const CellMomentsArgs& a, uint64_t* out_counts, double* out_sums, hipStream_t stream, std::string* err)
    {
    static const char* what = "cell fields";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_counts || !out_sums)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_arguments(a.n, a.n_cells, err, what);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.N >= (1ull << 32) + 1)
        return fail("2^32 rows or entries and more are not indexed");
    const uint64_t n = a.n;
    const uint32_t n_cells = a.n_cells;
    if (n == 0)
        {
        std::fill(out_counts, out_counts + 2 * (size_t)n_cells + 1, (uint64_t)0);
        std::fill(out_sums, out_sums + (size_t)CELLS_Q * n_cells, 0.0);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return fail(cells_refused);
    if (!a.rows || !a.cell)
        return PGSD_ERROR_INVALID_ARGUMENT;
    for (int i = 1; i < GROUPED_CHUNKS; i++)
        if ((a.present & (1u << i)) && !a.chunk[i])
            return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t n_slabs = (uint32_t)((n + CELLS_PIECE - 1) / CELLS_PIECE);
    const size_t offs_bytes = round16(((size_t)n_cells + 2) * sizeof(uint32_t)), first_bytes = round16((size_t)n_slabs * sizeof(uint32_t));
    const size_t table_bytes = (size_t)n_cells * CELLS_Q * sizeof(double), bad_bytes = (size_t)n_cells * sizeof(uint64_t);
    const size_t part_bytes = (size_t)n_slabs * 2 * CELLS_SLOT_WORDS * sizeof(double);
    LaunchScope scope(g_cells_lock, g_cells_scratch, 16 + offs_bytes + first_bytes + table_bytes + bad_bytes + part_bytes, stream,
                      err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    uint32_t* first = (uint32_t*)(dev + 16 + offs_bytes);
    double* table = (double*)(dev + 16 + offs_bytes + first_bytes);
    uint64_t* table_bad = (uint64_t*)((char*)table + table_bytes);
    double* part = (double*)((char*)table_bad + bad_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS);
    // (the table is zeroed for the empty cells: +0.0 and no bad entry)
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   table, table_bytes + bad_bytes, stream);
    if (e == hipSuccess)
        {
        const dim3 per_slab((n_slabs + CELLS_WAVES - 1) / CELLS_WAVES);
        if (a.f64)
            hipLaunchKernelGGL(cells_piece_kernel<true>, per_slab, block, 0, stream, a, offs, flag_dev, table, table_bad, part,
                               first, n_slabs);
        else
            hipLaunchKernelGGL(cells_piece_kernel<false>, per_slab, block, 0, stream, a, offs, flag_dev, table, table_bad, part,
                               first, n_slabs);
        const uint64_t long_lanes = (uint64_t)n_slabs * CELLS_SLOT_WORDS;
        hipLaunchKernelGGL(cells_long_kernel, dim3((unsigned)((long_lanes + SEL_THREADS - 1) / SEL_THREADS)), block, 0, stream,
                           a.cell, offs, flag_dev, part, first, n, n_cells, n_slabs, table, table_bad);
        e = hipGetLastError();
        }
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return fail(cells_refused);
    // success: the result table straight into the caller's sums, the offsets and counters through host copies
    std::vector<uint32_t> h_offs((size_t)n_cells + 2);
    std::vector<uint64_t> h_bad(n_cells);
    e = hipMemcpyAsync(out_sums, table, table_bytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_offs.data(), offs, h_offs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h_bad.data(), table_bad, bad_bytes, hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    for (uint32_t c = 0; c < n_cells; c++)
        {
        out_counts[2 * (size_t)c + 0] = h_offs[c + 1] - h_offs[c];
        out_counts[2 * (size_t)c + 1] = h_bad[c];
        }
    out_counts[2 * (size_t)n_cells] = h_offs[n_cells + 1] - h_offs[n_cells];
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
