// pgsd_order.hip -- cell order on gfx950: sort a row list by grid cell.
//   order_key_kernel       a key per list entry: the cell of the entry's row, plus a segment offset for the ghost run
//   radix_*_kernel         a stable least-significant-digit radix sort of (key, entry number) pairs, 8 bits per pass:
//                          histogram, scan, scatter
//   order_apply_kernel     the permutation applied to the caller's lists
// Shared device helpers: pgsd_select.hpp (the fraction, the wave scan), pgsd_kernels.hpp; the launcher's host side:
// pgsd_scratch.hpp.
#include "pgsd_select.hpp"
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
// ------------------------------------------------------------------ cell order (sort a row list by grid cell)
// pgsd.hoomd.cell_ids and cell_order are the definitions.  A key per list entry -- the cell of the entry's row in a
// uniform cx x cy x cz grid over the wrapped fractions the selections compare, plus a segment offset for the ghost run --,
// a stable least-significant-digit radix sort of (key, entry number) pairs at 8 bits per pass, and a pass that applies
// the permutation to the caller's lists.
//
// Key: lane per entry k.  i_a = min(int(f_a * c_a), c_a - 1) in float64 without contraction, the NaN test BEFORE the
// conversion; id = i_x + cx * (i_y + cy * i_z), or n_cells for a row with a NaN fraction ("nowhere", which sorts last);
// key = id + (k >= n_owned ? n_cells + 1 : 0): the ghost run's keys lie above every owned key, so ONE sort keeps the two
// runs apart.  The kernel also copies rows[k] into the scratch space (the apply pass writes the caller's list in place)
// and raises both flag words -- one in device memory for the apply pass, one pinned for the host -- at an entry >= N,
// whose position is not read.
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void order_key_kernel(const OrderArgs o, const uint32_t* rows, uint32_t* keys,
                                                                uint32_t* vals, uint32_t* rows_copy, uint32_t* flag_dev,
                                                                uint32_t* flag_host)
    {
#pragma clang fp contract(off)
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= o.n)
        return;
    const uint64_t i = rows[k];
    uint32_t id = o.n_cells;
    if (i < o.d.N)
        {
        double x, y, z;
        if constexpr (F64)
            {
            const double* q = (const double*)o.d.pos + i * 3;
            x = q[0];
            y = q[1];
            z = q[2];
            }
        else
            {
            const float* q = (const float*)o.d.pos + i * 3;
            x = (double)q[0];
            y = (double)q[1];
            z = (double)q[2];
            }
        double s[3];
        domain_skew(o.d, x, y, z, s);
        uint32_t cell = 0, stride = 1;
        bool somewhere = true;
#pragma unroll
        for (int a = 0; a < 3; a++)
            {
            if (a == 2 && o.d.dims == 2)
                break;
            const double f = domain_wrap(s[a]);
            uint32_t at = 0;
            if (f == f)
                at = min((uint32_t)(f * (double)o.cells[a]), o.cells[a] - 1u);
            else
                somewhere = false;
            cell += at * stride;
            stride *= o.cells[a];
            }
        if (somewhere)
            id = cell;
        }
    else
        {
        __hip_atomic_store(flag_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(flag_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    keys[k] = id + (k >= o.n_owned ? o.n_cells + 1u : 0u);
    vals[k] = (uint32_t)k;
    rows_copy[k] = (uint32_t)i;
    }

// One pass of the sort orders the pairs by the 8 bits of the key at `shift`, keeping the order of equal digits.  A
// workgroup owns a tile of 4096 consecutive pairs and each of its four waves a contiguous quarter of it: wave w takes
// pairs w * 1024 + step * 64 + lane in 16 steps, so (tile, wave, step, lane) is ascending list order.
//   histogram   the tile's count of every digit, in LDS, written digit-major into table[digit * n_tiles + tile]: plain
//               stores of a number that does not depend on the order of the LDS adds
//   scan        one workgroup per digit turns its row of the table into exclusive prefixes over the tiles (in place) and
//               leaves the digit's total in totals[digit]
//   scatter     every workgroup scans the 256 totals itself (256 lanes, one value each), so pair p of digit d goes to
//               totals-before(d) + table[d][tile] + (d's count in the tile's earlier waves) + (in this wave's earlier
//               steps) + (among this step's lower lanes).  The last term is a match mask -- one ballot per digit bit --
//               and a popcount; the two before it are per-wave digit counters in LDS that the first lane of every match
//               group advances.
// Nothing crosses workgroups inside a kernel: three launches per pass and no fence.  (One workgroup scanning the whole
// table as select_scan_kernel scans block counts would walk 256 x n_tiles counts 256 at a time, a barrier-separated
// dependent step each: 2442 tiles at 10 M pairs make 2442 such steps per pass against 10 here.)
#define SORT_DIGIT_BITS 8
#define SORT_RADIX (1 << SORT_DIGIT_BITS)
#define SORT_STEPS 16
#define SORT_WAVES (SEL_THREADS / 64)
#define SORT_WAVE_RUN (64 * SORT_STEPS)
#define SORT_TILE (SORT_WAVES * SORT_WAVE_RUN)
static_assert(SORT_RADIX == SEL_THREADS, "one lane per digit in the scan of the totals");

__global__ __launch_bounds__(SEL_THREADS) void radix_hist_kernel(const uint32_t* keys, uint64_t n, uint32_t shift,
                                                                 uint32_t n_tiles, uint32_t* table)
    {
    __shared__ uint32_t hist[SORT_RADIX];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE;
#pragma unroll
    for (int s = 0; s < SORT_TILE / SEL_THREADS; s++)
        {
        const uint64_t i = base + (uint64_t)s * SEL_THREADS + threadIdx.x;
        if (i < n)
            atomicAdd(&hist[(keys[i] >> shift) & (SORT_RADIX - 1u)], 1u);
        }
    __syncthreads();
    table[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = hist[threadIdx.x];
    }

// exclusive scan of one value per lane across the workgroup (wave scans joined through `wave_sums`); *total: the sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t c, uint32_t* wave_sums, uint32_t* total)
    {
    const uint32_t inc = wave_inclusive_scan(c);
    if ((threadIdx.x & 63) == 63)
        wave_sums[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t wave_off = 0, all = 0;
    for (uint32_t w = 0; w < SORT_WAVES; w++)
        {
        if (w < (threadIdx.x >> 6))
            wave_off += wave_sums[w];
        all += wave_sums[w];
        }
    __syncthreads(); // wave_sums may be written again
    *total = all;
    return wave_off + inc - c;
    }

__global__ __launch_bounds__(SEL_THREADS) void radix_scan_kernel(uint32_t* table, uint32_t n_tiles, uint32_t* totals)
    {
    __shared__ uint32_t wave_sums[SORT_WAVES];
    uint32_t* row = table + (uint64_t)blockIdx.x * n_tiles;
    uint32_t carry = 0; // the same in every lane
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += SEL_THREADS)
        {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t c = t < n_tiles ? row[t] : 0;
        uint32_t sum;
        const uint32_t before = block_exclusive_scan(c, wave_sums, &sum);
        if (t < n_tiles)
            row[t] = carry + before;
        carry += sum;
        }
    if (threadIdx.x == 0)
        totals[blockIdx.x] = carry;
    }

__global__ __launch_bounds__(SEL_THREADS) void radix_scatter_kernel(const uint32_t* keys_in, const uint32_t* vals_in, uint64_t n,
                                                                    uint32_t shift, uint32_t n_tiles, const uint32_t* table,
                                                                    const uint32_t* totals, uint32_t* keys_out,
                                                                    uint32_t* vals_out)
    {
    __shared__ uint32_t off[SORT_WAVES][SORT_RADIX]; // per wave: digit counts, then where the wave's next pair of a digit goes
    __shared__ uint32_t wave_sums[SORT_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t base = (uint64_t)blockIdx.x * SORT_TILE + (uint64_t)wave * SORT_WAVE_RUN + lane;
#pragma unroll
    for (uint32_t w = 0; w < SORT_WAVES; w++)
        off[w][threadIdx.x] = 0;
    uint32_t key[SORT_STEPS], val[SORT_STEPS];
#pragma unroll
    for (int s = 0; s < SORT_STEPS; s++)
        {
        const uint64_t i = base + (uint64_t)s * 64;
        key[s] = val[s] = 0;
        if (i < n)
            {
            key[s] = keys_in[i];
            val[s] = vals_in[i];
            }
        }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SORT_STEPS; s++)
        if (base + (uint64_t)s * 64 < n)
            atomicAdd(&off[wave][(key[s] >> shift) & (SORT_RADIX - 1u)], 1u);
    __syncthreads();
    // lane d of the workgroup: digit d's first place in the output, this tile's share of it, wave by wave
    uint32_t sum;
    uint32_t at = block_exclusive_scan(totals[threadIdx.x], wave_sums, &sum) + table[(uint64_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < SORT_WAVES; w++)
        {
        const uint32_t c = off[w][threadIdx.x];
        off[w][threadIdx.x] = at;
        at += c;
        }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SORT_STEPS; s++)
        {
        const bool valid = base + (uint64_t)s * 64 < n;
        const uint32_t d = (key[s] >> shift) & (SORT_RADIX - 1u);
        uint64_t same = __ballot(valid); // the lanes of this step that hold digit d
#pragma unroll
        for (int b = 0; b < SORT_DIGIT_BITS; b++)
            {
            const bool bit = (d >> b) & 1u;
            const uint64_t set = __ballot(bit);
            same &= bit ? set : ~set;
            }
        const uint32_t rank = (uint32_t)__popcll(same & below);
        // every lane of the group reads the counter, then its first lane advances it: one wave's LDS operations complete
        // in program order, and the wave barriers keep the compiler from moving them across each other
        const uint32_t first = off[wave][d];
        __builtin_amdgcn_wave_barrier();
        if (valid && rank == 0)
            off[wave][d] = first + (uint32_t)__popcll(same);
        __builtin_amdgcn_wave_barrier();
        const uint64_t to = (uint64_t)first + rank;
        if (valid && to < n)
            {
            keys_out[to] = key[s];
            vals_out[to] = val[s];
            }
        }
    }

// rows[k] = rows_copy[perm[k]], cell[k] = key - the segment's offset, the ghosts' shifts permuted like their rows (a ghost
// pair stays in the ghost segment: perm[k] >= n_owned where k >= n_owned).  Writes the caller's memory, and nothing if the
// key pass raised the flag.
__global__ __launch_bounds__(SEL_THREADS) void order_apply_kernel(const uint32_t* keys, const uint32_t* perm,
                                                                  const uint32_t* rows_copy, const int32_t* shift_copy,
                                                                  uint64_t n, uint64_t n_owned, uint32_t n_cells,
                                                                  const uint32_t* flag_dev, uint32_t* rows, int32_t* shift,
                                                                  int32_t* cell)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= n || *flag_dev != 0)
        return;
    const uint64_t p = perm[k];
    if (p >= n)
        return;
    rows[k] = rows_copy[p];
    if (cell)
        cell[k] = (int32_t)(keys[k] - (k >= n_owned ? n_cells + 1u : 0u));
    if (shift && k >= n_owned && p >= n_owned)
        {
#pragma unroll
        for (int a = 0; a < 3; a++)
            shift[(k - n_owned) * 3 + a] = shift_copy[(p - n_owned) * 3 + a];
        }
    }

// Cell order.  The scratch space (grow-only, per device, g_select_lock held) holds, in 32-bit words: two key and two
// value buffers of n (the passes ping-pong between them), the copy of the row list (n) and of the ghosts' shifts
// (3 x ghosts), the digit table (256 x tiles), the digit totals (256) and the device flag word; the pinned flag word is
// the host's view of "an entry was >= N".  (Growth policy and word count: restated by tests/test_gpu_scratch_reuse.py.)
static Scratch g_order_scratch("cell order", 1.25, (1u << 14) * sizeof(uint32_t), 0, sizeof(uint64_t));

void warm_order_kernels()
    {
    warm_kernel((const void*)radix_scan_kernel);
    }

// the number of 8-bit passes that cover every key of a call: the bits of the largest one
static unsigned order_passes(uint64_t max_key)
    {
    unsigned bits = 1;
    while (bits < 32 && (max_key >> bits) != 0)
        bits++;
    return (bits + SORT_DIGIT_BITS - 1) / SORT_DIGIT_BITS;
    }

// The sort alone, for a unit whose keys are not grid cells (pgsd_component_moments.hip): the passes of order_passes(max_key)
// over the caller's (key, value) pairs, enqueued on `stream` with no synchronisation.  keys[0] / vals[0] hold the n pairs,
// keys[1] / vals[1] are their ping-pong twins, table takes sort_pairs_table_words(n) words and totals 256; the result lies
// in keys[r] / vals[r] for the returned r.  A key above max_key is sorted by its low digits only; no store lands at an
// index >= n whatever the keys hold.
size_t sort_pairs_table_words(uint64_t n)
    {
    return (size_t)SORT_RADIX * (size_t)((n + SORT_TILE - 1) / SORT_TILE);
    }

unsigned enqueue_sort_pairs(uint32_t* const keys[2], uint32_t* const vals[2], uint32_t* table, uint32_t* totals, uint64_t n,
                            uint64_t max_key, hipStream_t stream)
    {
    const uint64_t n_tiles = (n + SORT_TILE - 1) / SORT_TILE;
    const dim3 block(SEL_THREADS), per_tile((unsigned)n_tiles);
    const unsigned passes = order_passes(max_key);
    unsigned cur = 0;
    for (unsigned p = 0; p < passes; p++, cur ^= 1u)
        {
        const uint32_t at = p * SORT_DIGIT_BITS;
        hipLaunchKernelGGL(radix_hist_kernel, per_tile, block, 0, stream, keys[cur], n, at, (uint32_t)n_tiles, table);
        hipLaunchKernelGGL(radix_scan_kernel, dim3(SORT_RADIX), block, 0, stream, table, (uint32_t)n_tiles, totals);
        hipLaunchKernelGGL(radix_scatter_kernel, per_tile, block, 0, stream, keys[cur], vals[cur], n, at, (uint32_t)n_tiles,
                           table, totals, keys[cur ^ 1u], vals[cur ^ 1u]);
        }
    return cur;
    }

int launch_order_rows(const OrderArgs& o, uint32_t* rows, int32_t* shift, int32_t* out_cell, hipStream_t stream,
                      std::string* err)
    {
    const uint64_t n = o.n;
    if (n == 0)
        return PGSD_SUCCESS;
    uint64_t n_cells = 1;
    for (int a = 0; a < 3; a++)
        {
        if (o.cells[a] < 1 || o.cells[a] > ORDER_MAX_AXIS_CELLS)
            return PGSD_ERROR_INVALID_ARGUMENT;
        n_cells *= o.cells[a];
        }
    if (n >= (1ull << 32) || o.n_owned > n || n_cells != o.n_cells || !o.d.pos || !rows || o.d.N >= (1ull << 32)
        || (o.d.dims == 2 && o.cells[2] != 1))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint64_t n_ghost = n - o.n_owned;
    const uint64_t n_tiles = (n + SORT_TILE - 1) / SORT_TILE;
    const auto round4 = [](uint64_t words) { return (words + 3) & ~3ull; }; // 16-byte aligned parts
    const uint64_t part = round4(n), shift_words = shift ? round4(3 * n_ghost) : 0, table_words = round4(SORT_RADIX * n_tiles);
    const size_t words = (size_t)(5 * part + shift_words + table_words + SORT_RADIX + 4);
    LaunchScope scope(g_select_lock, g_order_scratch, words * sizeof(uint32_t), stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    uint32_t* dev = (uint32_t*)scope.mem().dev;
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    uint32_t* keys[2] = {dev, dev + part};
    uint32_t* vals[2] = {dev + 2 * part, dev + 3 * part};
    uint32_t* rows_copy = dev + 4 * part;
    int32_t* shift_copy = (int32_t*)(dev + 5 * part);
    uint32_t* table = dev + 5 * part + shift_words;
    uint32_t* totals = table + table_words;
    uint32_t* flag_dev = totals + SORT_RADIX;
    __atomic_store_n(host_flag, 0u, __ATOMIC_RELEASE);
    const dim3 block(SEL_THREADS), per_entry((unsigned)((n + SEL_THREADS - 1) / SEL_THREADS)), per_tile((unsigned)n_tiles);
    hipError_t e = hipMemsetAsync(flag_dev, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess && shift && n_ghost > 0)
        e = hipMemcpyAsync(shift_copy, shift, 3 * n_ghost * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess)
        {
        PGSD_LAUNCH_BY_F64(o.d.f64, order_key_kernel, per_entry, stream, o, rows, keys[0], vals[0], rows_copy, flag_dev,
                           (uint32_t*)scope.mem().mapped_dev);
        const unsigned passes = order_passes(n_ghost > 0 ? 2 * n_cells + 1 : n_cells);
        unsigned cur = 0;
        for (unsigned p = 0; p < passes; p++, cur ^= 1u)
            {
            const uint32_t at = p * SORT_DIGIT_BITS;
            hipLaunchKernelGGL(radix_hist_kernel, per_tile, block, 0, stream, keys[cur], n, at, (uint32_t)n_tiles, table);
            hipLaunchKernelGGL(radix_scan_kernel, dim3(SORT_RADIX), block, 0, stream, table, (uint32_t)n_tiles, totals);
            hipLaunchKernelGGL(radix_scatter_kernel, per_tile, block, 0, stream, keys[cur], vals[cur], n, at,
                               (uint32_t)n_tiles, table, totals, keys[cur ^ 1u], vals[cur ^ 1u]);
            }
        hipLaunchKernelGGL(order_apply_kernel, per_entry, block, 0, stream, keys[cur], vals[cur], rows_copy, shift_copy, n,
                           o.n_owned, o.n_cells, flag_dev, rows, n_ghost > 0 ? shift : nullptr, out_cell);
        e = hipGetLastError();
        }
    const int rc = scope.finish("cell order", e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT,
                           "cell order: an entry of the row list lies outside the position chunk (nothing was reordered)");
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
