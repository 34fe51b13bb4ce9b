// pgsd_select.hip -- stream compaction on gfx950: everything that ends in the one-block scan and lives in the compaction
// scratch.
//   select_*_kernel        stream compaction for filtered snapshots: wave ballot / popcount scans give each workgroup's
//                          count, a one-block scan turns counts into offsets (= per-chunk row and byte counts) and
//                          hands the total to the host, a scatter pass writes the index list (pgsd_select_rows)
//   domain_* / halo_* / where_*_kernel   the same compaction with the predicate evaluated in both passes instead of a
//                          flag array: the rows inside a spatial domain, a domain plus its ghost layer, the rows of a
//                          particle group (type set, value ranges)
//   plan_*_kernel          the row plan of sparse indexed reads: touched blocks marked, scanned into slots, rows remapped
// Shared device helpers: pgsd_select.hpp (which also maps the sibling units), pgsd_kernels.hpp; the launchers' host
// side: pgsd_scratch.hpp.
#include "pgsd_select.hpp"
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
// ------------------------------------------------------------------ select (compaction)
// (SEL_THREADS, SEL_PER_THREAD, SEL_PER_BLOCK: pgsd_kernels.hpp -- pgsd_stats.hip shares the row layout)
// number of non-zero flag bytes among the 16 this lane owns
__device__ __forceinline__ uint32_t sel_load16(const uint8_t* flags, uint64_t base, uint64_t N, uint32_t* mask)
    {
    uint32_t m = 0;
    if (base + SEL_PER_THREAD <= N && ((uintptr_t)(flags + base) & 15) == 0)
        {
        u32x4 v = *(const u32x4*)(flags + base);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++)
            m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) != 0 ? 1u : 0u) << k;
        }
    else
        {
        for (int k = 0; k < 16; k++)
            if (base + k < N && flags[base + k] != 0)
                m |= 1u << k;
        }
    *mask = m;
    return (uint32_t)__popc(m);
    }

// exclusive scan of the block counts by ONE workgroup; also writes the total -- to device memory and straight into the
// caller's pinned word (a system-scope store: no copy command behind the kernels)
__device__ __forceinline__ void select_scan_block(const uint32_t* block_counts, uint32_t n_blocks, uint64_t* block_offsets,
                                                  uint64_t* out_count, uint64_t* out_count_host, uint32_t* wave_sums,
                                                  uint64_t* carry)
    {
    if (threadIdx.x == 0)
        *carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SEL_THREADS)
        {
        uint32_t i = b0 + threadIdx.x;
        uint32_t c = i < n_blocks ? block_counts[i] : 0;
        uint32_t inc = wave_inclusive_scan(c);
        if ((threadIdx.x & 63) == 63)
            wave_sums[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t wave_off = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++)
            wave_off += wave_sums[w];
        if (i < n_blocks)
            block_offsets[i] = *carry + wave_off + inc - c;
        __syncthreads();
        if (threadIdx.x == SEL_THREADS - 1)
            *carry += (uint64_t)wave_off + inc;
        __syncthreads();
        }
    if (threadIdx.x == 0)
        {
        *out_count = *carry;
        __hip_atomic_store(out_count_host, *carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }

__global__ __launch_bounds__(SEL_THREADS) void select_count_kernel(const uint8_t* flags, uint64_t N, uint32_t* block_counts)
    {
    __shared__ uint32_t wave_sums[SEL_THREADS / 64];
    uint64_t base = ((uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x) * SEL_PER_THREAD;
    uint32_t mask;
    uint32_t c = base < N ? sel_load16(flags, base, N, &mask) : 0;
    uint32_t inc = wave_inclusive_scan(c);
    if ((threadIdx.x & 63) == 63)
        wave_sums[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
    }

// (A launch of its own: letting the LAST counting workgroup scan -- a ticket counter, release / acquire at device scope
// in every workgroup -- was measured at 87-95 us per call against 37-44: on a part whose eight L2s are not coherent
// with each other such fences write back and invalidate whole caches; profiles/r05_select_bench.jsonl.)
__global__ __launch_bounds__(SEL_THREADS) void select_scan_kernel(const uint32_t* block_counts, uint32_t n_blocks,
                                                                  uint64_t* block_offsets, uint64_t* out_count,
                                                                  uint64_t* out_count_host)
    {
    __shared__ uint32_t wave_sums[SEL_THREADS / 64];
    __shared__ uint64_t carry;
    select_scan_block(block_counts, n_blocks, block_offsets, out_count, out_count_host, wave_sums, &carry);
    }

__global__ __launch_bounds__(SEL_THREADS) void select_scatter_kernel(const uint8_t* flags, uint64_t N,
                                                                     const uint64_t* block_offsets,
                                                                     uint32_t* out_index)
    {
    // The kept rows of this block are compacted in LDS first (each lane drops its <= 16 indices at
    // its block-local rank), then the block writes them out as one dense, coalesced run: lane i
    // stores element i of the run instead of 16 scattered stores per lane.
    __shared__ uint32_t wave_sums[SEL_THREADS / 64];
    __shared__ uint32_t local[SEL_PER_BLOCK];
    uint64_t base = ((uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x) * SEL_PER_THREAD;
    uint32_t mask = 0;
    uint32_t c = base < N ? sel_load16(flags, base, N, &mask) : 0;
    uint32_t inc = wave_inclusive_scan(c);
    if ((threadIdx.x & 63) == 63)
        wave_sums[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint32_t wave_off = 0, total = 0;
    for (uint32_t w = 0; w < SEL_THREADS / 64; w++)
        {
        if (w < (threadIdx.x >> 6))
            wave_off += wave_sums[w];
        total += wave_sums[w];
        }
    uint32_t pos = wave_off + inc - c;
    while (mask)
        {
        int k = __ffs((int)mask) - 1;
        mask &= mask - 1;
        local[pos++] = (uint32_t)(base + (uint64_t)k);
        }
    __syncthreads();
    uint32_t* out = out_index + block_offsets[blockIdx.x];
    // 16-byte stores where the run's start allows, 4-byte stores for the ragged ends
    const uint32_t lead = (uint32_t)((4u - (((uintptr_t)out >> 2) & 3u)) & 3u);
    const uint32_t head = lead < total ? lead : total;
    if (threadIdx.x < head)
        out[threadIdx.x] = local[threadIdx.x];
    const uint32_t nvec = (total - head) >> 2;
    for (uint32_t v = threadIdx.x; v < nvec; v += SEL_THREADS)
        {
        const uint32_t e = head + 4 * v;
        u32x4 q = {local[e], local[e + 1], local[e + 2], local[e + 3]};
        *(u32x4*)(out + e) = q;
        }
    for (uint32_t e = head + 4 * nvec + threadIdx.x; e < total; e += SEL_THREADS)
        out[e] = local[e];
    }

// ------------------------------------------------------------------ domain selection (restart of a domain-decomposed run)
// The rows of a staged position chunk whose fractional coordinates lie in [lo, hi) per axis: HOOMD's
// BoxDim::makeFraction in float64, in the operation order of pgsd.hoomd.domain_rows (the numpy model, which is the
// definition), no contraction into FMAs -- a particle on a split plane must land in the same cell as the model says.
// Lane t of a workgroup owns rows base + k * SEL_THREADS + t, k < SEL_PER_THREAD (consecutive lanes, consecutive rows:
// coalesced 12-byte loads); bit k of its mask is row k's verdict.  Count pass, the one-block scan of pgsd_select_rows,
// scatter pass; the scatter orders a workgroup's rows by (k, wave, lane) through wave ballots, i.e. ascending.
// (the fraction itself -- domain_skew(), domain_wrap(), domain_inside() -- and domain_load_rows(): pgsd_select.hpp)
template<bool F64> __device__ __forceinline__ uint32_t domain_mask(const DomainArgs& d, uint64_t base)
    {
    double p[SEL_PER_THREAD][3];
    domain_load_rows<F64>(d.pos, d.N, base, p);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        {
        const uint64_t i = base + (uint64_t)k * SEL_THREADS + threadIdx.x;
        if (i < d.N && domain_inside(d, p[k][0], p[k][1], p[k][2]))
            m |= 1u << k;
        }
    return m;
    }

// the count pass of a predicate selection: the workgroup's number of kept rows (the bits of every lane's mask)
__device__ __forceinline__ void mask_count_block(uint32_t m, uint32_t* block_counts)
    {
    __shared__ uint32_t wave_sums[SEL_THREADS / 64];
    const uint32_t c = (uint32_t)__popc(m);
    const uint32_t inc = wave_inclusive_scan(c);
    if ((threadIdx.x & 63) == 63)
        wave_sums[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = wave_sums[0] + wave_sums[1] + wave_sums[2] + wave_sums[3];
    }

// the scatter pass: bit k of lane t's mask is row base + k * SEL_THREADS + t; the kept rows are ordered by (k, wave,
// lane) -- ascending -- in LDS and leave as one dense run at the workgroup's offset
__device__ __forceinline__ void mask_scatter_block(uint32_t m, uint64_t base, const uint64_t* block_offsets, uint32_t* out_index)
    {
    constexpr uint32_t W = SEL_THREADS / 64;
    __shared__ uint32_t cnt[SEL_PER_THREAD][W]; // kept rows per (k, wave), then their exclusive prefix in (k, wave) order
    __shared__ uint32_t total;
    __shared__ uint32_t local[SEL_PER_BLOCK];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        {
        const uint64_t b = __ballot((m >> k) & 1u);
        if (lane == 0)
            cnt[k][wave] = (uint32_t)__popcll(b);
        }
    __syncthreads();
    if (threadIdx.x == 0)
        {
        uint32_t acc = 0;
        for (int k = 0; k < SEL_PER_THREAD; k++)
            for (uint32_t w = 0; w < W; w++)
                {
                const uint32_t c = cnt[k][w];
                cnt[k][w] = acc;
                acc += c;
                }
        total = acc;
        }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        {
        const uint64_t b = __ballot((m >> k) & 1u);
        if ((m >> k) & 1u)
            local[cnt[k][wave] + (uint32_t)__popcll(b & below)] = (uint32_t)(base + (uint64_t)k * SEL_THREADS + threadIdx.x);
        }
    __syncthreads();
    const uint32_t n = total;
    uint32_t* out = out_index + block_offsets[blockIdx.x];
    // 16-byte stores where the run's start allows, 4-byte stores for the ragged ends
    const uint32_t lead = (uint32_t)((4u - (((uintptr_t)out >> 2) & 3u)) & 3u);
    const uint32_t head = lead < n ? lead : n;
    if (threadIdx.x < head)
        out[threadIdx.x] = local[threadIdx.x];
    const uint32_t nvec = (n - head) >> 2;
    for (uint32_t v = threadIdx.x; v < nvec; v += SEL_THREADS)
        {
        const uint32_t e = head + 4 * v;
        u32x4 q = {local[e], local[e + 1], local[e + 2], local[e + 3]};
        *(u32x4*)(out + e) = q;
        }
    for (uint32_t e = head + 4 * nvec + threadIdx.x; e < n; e += SEL_THREADS)
        out[e] = local[e];
    }

template<bool F64> __global__ __launch_bounds__(SEL_THREADS) void domain_count_kernel(const DomainArgs d, uint32_t* block_counts)
    {
    mask_count_block(domain_mask<F64>(d, (uint64_t)blockIdx.x * SEL_PER_BLOCK), block_counts);
    }

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void domain_scatter_kernel(const DomainArgs d, const uint64_t* block_offsets,
                                                                     uint32_t* out_index)
    {
    const uint64_t base = (uint64_t)blockIdx.x * SEL_PER_BLOCK;
    mask_scatter_block(domain_mask<F64>(d, base), base, block_offsets, out_index);
    }

// ------------------------------------------------------------------ ghost layer (a cell plus the halo its neighbours reach)
// pgsd.hoomd.halo_rows is the definition.  A row is OWNED when domain_inside() holds; it is a GHOST when on every
// axis its wrapped fraction is inside or in one of the axis' four bands and on at least one it is in a band.  The bands'
// bounds arrive computed (HaloArgs: pgsd.hoomd.halo_bands, host float64): the kernel only compares, in the model's
// fixed order -- inside, below, below wrapped, above, above wrapped --, so the result equals the model, planes included.
// An undivided axis has no bands and counts as inside.  Return value: HALO_OWNED, or HALO_GHOST | code << 2 with two
// bits per axis (0: no shift, 1: -1, 2: +1 box vectors), or 0.
enum
    {
    HALO_OWNED = 1,
    HALO_GHOST = 2
    };

__device__ __forceinline__ uint32_t halo_class(const HaloArgs& h, double x, double y, double z)
    {
#pragma clang fp contract(off)
    double s[3];
    domain_skew(h.d, x, y, z, s);
    bool owned = true, reached = true, in_band = false;
    uint32_t code = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
        {
        if (a == 2 && h.d.dims == 2)
            break;
        const double f = domain_wrap(s[a]);
        const bool in = h.d.lo[a] <= f && f < h.d.hi[a];
        owned = owned && in;
        if (!h.divided[a] || in)
            continue;
        const double* b = h.band[a];
        uint32_t shift = 0;
        bool hit = true;
        if (b[0] <= f && f < b[1])
            shift = 0;
        else if (b[2] <= f && f < b[3])
            shift = 1;
        else if (b[4] <= f && f < b[5])
            shift = 0;
        else if (b[6] <= f && f < b[7])
            shift = 2;
        else
            hit = false;
        reached = reached && hit;
        in_band = in_band || hit;
        code |= shift << (2 * a);
        }
    if (owned)
        return HALO_OWNED;
    return reached && in_band ? HALO_GHOST | (code << 2) : 0u;
    }

// both verdicts of this lane's SEL_PER_THREAD rows from one pass over their positions: bit k of *owned / *ghost
template<bool F64> __device__ __forceinline__ void halo_masks(const HaloArgs& h, uint64_t base, uint32_t* owned, uint32_t* ghost)
    {
    double p[SEL_PER_THREAD][3];
    domain_load_rows<F64>(h.d.pos, h.d.N, base, p);
    uint32_t mo = 0, mg = 0;
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        {
        const uint64_t i = base + (uint64_t)k * SEL_THREADS + threadIdx.x;
        const uint32_t c = i < h.d.N ? halo_class(h, p[k][0], p[k][1], p[k][2]) : 0u;
        mo |= (c & 1u) << k;
        mg |= ((c >> 1) & 1u) << k;
        }
    *owned = mo;
    *ghost = mg;
    }

// (mask_count_block and mask_scatter_block keep their LDS arrays per function, not per call: a barrier between the two
// uses lets every lane finish reading the first use's before the second overwrites them)
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void halo_count_kernel(const HaloArgs h, uint32_t* owned_counts, uint32_t* ghost_counts)
    {
    uint32_t mo, mg;
    halo_masks<F64>(h, (uint64_t)blockIdx.x * SEL_PER_BLOCK, &mo, &mg);
    mask_count_block(mo, owned_counts);
    __syncthreads();
    mask_count_block(mg, ghost_counts);
    }

// owned rows at out_rows[0, n_owned), ghost rows behind them, each ascending; *n_owned is the count word the scan of the
// owned block counts left in device memory
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void halo_scatter_kernel(const HaloArgs h, const uint64_t* owned_offsets,
                                                                   const uint64_t* ghost_offsets, const uint64_t* n_owned,
                                                                   uint32_t* out_rows)
    {
    const uint64_t base = (uint64_t)blockIdx.x * SEL_PER_BLOCK;
    uint32_t mo, mg;
    halo_masks<F64>(h, base, &mo, &mg);
    mask_scatter_block(mo, base, owned_offsets, out_rows);
    __syncthreads();
    mask_scatter_block(mg, base, ghost_offsets, out_rows + *n_owned);
    }

// one lane per ghost row: its position again, its class again, the three shifts (the ghosts are few beside N: no payload
// travels through the LDS compaction)
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void halo_shift_kernel(const HaloArgs h, const uint32_t* ghost_rows, uint64_t n_ghost,
                                                                 int32_t* out_shift)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= n_ghost)
        return;
    const uint64_t i = ghost_rows[k];
    uint32_t code = 0;
    if (i < h.d.N)
        {
        double x, y, z;
        if constexpr (F64)
            {
            const double* q = (const double*)h.d.pos + i * 3;
            x = q[0];
            y = q[1];
            z = q[2];
            }
        else
            {
            const float* q = (const float*)h.d.pos + i * 3;
            x = (double)q[0];
            y = (double)q[1];
            z = (double)q[2];
            }
        code = halo_class(h, x, y, z) >> 2;
        }
#pragma unroll
    for (int a = 0; a < 3; a++)
        {
        const uint32_t c = (code >> (2 * a)) & 3u;
        out_shift[k * 3 + a] = c == 1u ? -1 : c == 2u ? 1 : 0;
        }
    }

// ------------------------------------------------------------------ group selection (read a particle group)
// The rows that satisfy every term of a predicate over up to four staged per-particle chunks and -- optionally -- lie
// in a domain: pgsd.hoomd.where_rows is the definition (WhereArgs, pgsd_internal.hpp, restates it).  Same structure as
// the domain selection: lane t owns rows base + k * SEL_THREADS + t, both passes evaluate the predicate (no flag
// array), count -> one-block scan -> scatter.  A term reads the 4 (8: float64) bytes of its column at a stride of the
// chunk's row: neighbouring lanes read neighbouring rows, so every fetched line is used by the wave that fetched it,
// whole for M = 1 and one column in M of it otherwise (HBM traffic is the whole chunk either way).  Element type and
// kind are the same for every lane: plain branches, which a wave takes as one.
// (a lane whose row lies past the end reads row N - 1 instead -- straight-line loads, no branch per row; where_mask has
// cleared its bit already)
__device__ __forceinline__ uint32_t where_term_mask(const WhereTerm& t, uint64_t N, uint64_t base)
    {
    uint32_t m = 0;
    if (t.type == PGSD_TYPE_DOUBLE)
        {
        double v[SEL_PER_THREAD];
#pragma unroll
        for (int k = 0; k < SEL_PER_THREAD; k++)
            {
            const uint64_t i = min(base + (uint64_t)k * SEL_THREADS + threadIdx.x, N - 1);
            v[k] = __builtin_nontemporal_load((const double*)t.base + (i * t.M + t.column));
            }
#pragma unroll
        for (int k = 0; k < SEL_PER_THREAD; k++)
            m |= (v[k] == v[k] && !(v[k] < t.lo) && !(v[k] >= t.hi) ? 1u : 0u) << k;
        }
    else
        {
        uint32_t x[SEL_PER_THREAD];
#pragma unroll
        for (int k = 0; k < SEL_PER_THREAD; k++)
            {
            const uint64_t i = min(base + (uint64_t)k * SEL_THREADS + threadIdx.x, N - 1);
            x[k] = __builtin_nontemporal_load((const uint32_t*)t.base + (i * t.M + t.column));
            }
        if (t.kind == WHERE_SET)
            {
#pragma unroll
            for (int k = 0; k < SEL_PER_THREAD; k++)
                m |= (x[k] < 64u ? (uint32_t)((t.set >> x[k]) & 1ull) : 0u) << k;
            }
        else
            {
#pragma unroll
            for (int k = 0; k < SEL_PER_THREAD; k++)
                {
                const double v = t.type == PGSD_TYPE_FLOAT   ? (double)__uint_as_float(x[k])
                                 : t.type == PGSD_TYPE_INT32 ? (double)(int32_t)x[k]
                                                             : (double)x[k];
                m |= (v == v && !(v < t.lo) && !(v >= t.hi) ? 1u : 0u) << k;
                }
            }
        }
    return m;
    }

// bit k: row base + k * SEL_THREADS + threadIdx.x exists and passes (rows past N pass no term; a selection of the
// domain alone gets them refused by domain_mask)
__device__ __forceinline__ uint32_t where_mask(const WhereArgs& w, uint64_t base)
    {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        m |= (base + (uint64_t)k * SEL_THREADS + threadIdx.x < w.N ? 1u : 0u) << k;
    // (a loop, not four copies: all terms' loads hoisted to the top cost 247 registers against 120-odd, half the waves)
#pragma nounroll
    for (uint32_t j = 0; j < w.n_terms; j++)
        m &= where_term_mask(w.t[j], w.N, base);
    if (w.has_domain)
        m &= w.d.f64 ? domain_mask<true>(w.d, base) : domain_mask<false>(w.d, base);
    return m;
    }

__global__ __launch_bounds__(SEL_THREADS) void where_count_kernel(const WhereArgs w, uint32_t* block_counts)
    {
    mask_count_block(where_mask(w, (uint64_t)blockIdx.x * SEL_PER_BLOCK), block_counts);
    }

__global__ __launch_bounds__(SEL_THREADS) void where_scatter_kernel(const WhereArgs w, const uint64_t* block_offsets,
                                                                    uint32_t* out_index)
    {
    const uint64_t base = (uint64_t)blockIdx.x * SEL_PER_BLOCK;
    mask_scatter_block(where_mask(w, base), base, block_offsets, out_index);
    }

// ------------------------------------------------------------------ row plan (sparse indexed reads)
// The chunk's N rows are cut into blocks of R rows.  mark: lane per entry, touched[rows[k] / R] = 1 (a plain vector
// store: lanes racing on one word all store the same value); scan: the one-block scan above over the ceil(N / R) flags
// gives block b's slot in the compact staging and T, the number of touched blocks; remap: rows2[k] = slot * R + rows[k] % R.
// An entry >= N marks nothing and becomes 0xFFFFFFFF, which the gather's bounds check refuses.  Grid-stride, 4 bytes per
// entry in and out: nothing to tune here next to the file reads the plan saves.
__global__ __launch_bounds__(SEL_THREADS) void plan_mark_kernel(const uint32_t* rows, uint64_t n, uint64_t N, uint32_t R,
                                                                uint32_t* touched)
    {
    for (uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * SEL_THREADS)
        {
        const uint32_t r = rows[k];
        if (r < N)
            touched[r / R] = 1u;
        }
    }

__global__ __launch_bounds__(SEL_THREADS) void plan_remap_kernel(const uint32_t* rows, uint64_t n, uint64_t N, uint32_t R,
                                                                 const uint64_t* slot, uint32_t* rows2)
    {
    for (uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * SEL_THREADS)
        {
        const uint32_t r = rows[k];
        uint32_t v = 0xFFFFFFFFu;
        if (r < N)
            {
            const uint32_t b = r / R;
            v = (uint32_t)slot[b] * R + (r - b * R);
            }
        rows2[k] = v;
        }
    }

    } // namespace pgsd_amd

using namespace pgsd_amd;

namespace
    {
// The scratch space of a compaction over nb blocks: the count (u64), the block counts (u32) rounded to 8 bytes, the block
// offsets (u64).  Sets lie one behind the other (the halo selection compacts two lists).
struct CompactionSet
    {
    uint64_t* count;
    uint32_t* block_counts;
    uint64_t* block_offsets;
    static size_t counts_bytes(uint64_t nb) // the u32 block counts, rounded to 8 bytes
        {
        return (size_t)((nb * 4 + 7) & ~7ull);
        }
    static size_t bytes(uint64_t nb)
        {
        return 8 + counts_bytes(nb) + (size_t)nb * 8;
        }
    CompactionSet(char* base, uint64_t nb, unsigned set = 0)
        {
        char* at = base + set * bytes(nb);
        count = (uint64_t*)at;
        block_counts = (uint32_t*)(at + 8);
        block_offsets = (uint64_t*)(at + 8 + counts_bytes(nb));
        }
    };

// per device (g_select_lock held): the sets of the largest call so far, and the two pinned words the scans leave their
// counts in (the halo selection's second scan writes into the second).  (The factor and the floor here, in pgsd_census.hip,
// pgsd_order.hip and pgsd_stats.hip, and the layouts beside them are restated by tests/test_gpu_scratch_reuse.py, which
// sizes its calls to cross each family's first capacity: change them together.)
Scratch g_select_scratch("pgsd_select_rows", 2.0, 1u << 16, 0, 2 * sizeof(uint64_t));

uint64_t blocks_of(uint64_t N, uint64_t per_block = SEL_PER_BLOCK)
    {
    return (N + per_block - 1) / per_block;
    }

// the one-block scan of a set's block counts; the total goes to set.count and to the pinned word behind `host_word_dev`
void enqueue_scan(const CompactionSet& set, uint64_t nb, void* host_word_dev, hipStream_t stream)
    {
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, stream, set.block_counts, (uint32_t)nb,
                       set.block_offsets, set.count, (uint64_t*)host_word_dev);
    }

// word i of the scratch's pinned block, after LaunchScope::finish
uint64_t host_count(const Scratch::Block& mem, int i = 0)
    {
    return __atomic_load_n((const uint64_t*)mem.mapped + i, __ATOMIC_ACQUIRE);
    }
    } // namespace

namespace pgsd_amd
    {
void warm_compaction_kernels()
    {
    warm_kernel((const void*)select_scan_kernel);
    }

// count -> scan -> scatter of a predicate selection over N rows (0 < N < 2^32) on `stream`; `launch(count pass?,
// blocks, block counts, block offsets)` enqueues the predicate's own kernel for either pass
template<class Launch>
static int select_by_predicate(uint64_t N, const char* what, uint64_t* out_count, hipStream_t stream, std::string* err,
                               Launch launch)
    {
    const uint64_t nb = blocks_of(N);
    LaunchScope scope(g_select_lock, g_select_scratch, CompactionSet::bytes(nb), stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    const CompactionSet set(scope.mem().dev, nb);
    launch(true, dim3((unsigned)nb), set.block_counts, set.block_offsets);
    enqueue_scan(set, nb, scope.mem().mapped_dev, stream);
    launch(false, dim3((unsigned)nb), set.block_counts, set.block_offsets);
    const int rc = scope.finish(what);
    if (rc == PGSD_SUCCESS)
        *out_count = host_count(scope.mem());
    return rc;
    }

int launch_select_domain(const DomainArgs& d, uint32_t* out_rows, uint64_t* out_count, hipStream_t stream, std::string* err)
    {
    *out_count = 0;
    if (d.N == 0)
        return PGSD_SUCCESS;
    if (d.N >= (1ull << 32) || !d.pos || !out_rows)
        return PGSD_ERROR_INVALID_ARGUMENT;
    return select_by_predicate(d.N, "domain selection", out_count, stream, err,
                               [&](bool count, dim3 grid, uint32_t* block_counts, uint64_t* block_offsets)
                               {
                                   if (count)
                                       PGSD_LAUNCH_BY_F64(d.f64, domain_count_kernel, grid, stream, d, block_counts);
                                   else
                                       PGSD_LAUNCH_BY_F64(d.f64, domain_scatter_kernel, grid, stream, d, block_offsets, out_rows);
                               });
    }

int launch_select_where(const WhereArgs& w, uint32_t* out_rows, uint64_t* out_count, hipStream_t stream, std::string* err)
    {
    *out_count = 0;
    if (w.N == 0)
        return PGSD_SUCCESS;
    if (w.N >= (1ull << 32) || w.n_terms > WHERE_MAX_TERMS || (w.n_terms == 0 && !w.has_domain) || !out_rows
        || (w.has_domain && (!w.d.pos || w.d.N != w.N)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    for (uint32_t j = 0; j < w.n_terms; j++)
        {
        const WhereTerm& t = w.t[j];
        const bool integer = t.type == PGSD_TYPE_UINT32 || t.type == PGSD_TYPE_INT32;
        if (!t.base || t.column >= t.M || !(integer || t.type == PGSD_TYPE_FLOAT || t.type == PGSD_TYPE_DOUBLE)
            || (t.kind != WHERE_RANGE && !(t.kind == WHERE_SET && integer)))
            return PGSD_ERROR_INVALID_ARGUMENT;
        }
    return select_by_predicate(w.N, "group selection", out_count, stream, err,
                               [&](bool count, dim3 grid, uint32_t* block_counts, uint64_t* block_offsets)
                               {
                                   if (count)
                                       hipLaunchKernelGGL(where_count_kernel, grid, dim3(SEL_THREADS), 0, stream, w,
                                                          block_counts);
                                   else
                                       hipLaunchKernelGGL(where_scatter_kernel, grid, dim3(SEL_THREADS), 0, stream, w,
                                                          block_offsets, out_rows);
                               });
    }

// Ghost layer: one count pass leaves two block-count arrays, the one-block scan runs once per array, one scatter pass
// writes the owned rows and -- behind them, at the owned count the first scan left in device memory -- the ghost rows;
// with the counts on the host, one lane per ghost row works out its shifts.
int launch_select_halo(const HaloArgs& h, uint32_t* out_rows, int32_t* out_shift, uint64_t out_counts[2], hipStream_t stream,
                       std::string* err)
    {
    out_counts[0] = out_counts[1] = 0;
    const uint64_t N = h.d.N;
    if (N == 0)
        return PGSD_SUCCESS;
    if (N >= (1ull << 32) || !h.d.pos || !out_rows || !out_shift)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint64_t nb = blocks_of(N);
    LaunchScope scope(g_select_lock, g_select_scratch, 2 * CompactionSet::bytes(nb), stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    const Scratch::Block& mem = scope.mem();
    const CompactionSet owned(mem.dev, nb, 0), ghost(mem.dev, nb, 1);
    const dim3 grid((unsigned)nb);
    PGSD_LAUNCH_BY_F64(h.d.f64, halo_count_kernel, grid, stream, h, owned.block_counts, ghost.block_counts);
    enqueue_scan(owned, nb, (uint64_t*)mem.mapped_dev, stream);
    enqueue_scan(ghost, nb, (uint64_t*)mem.mapped_dev + 1, stream);
    PGSD_LAUNCH_BY_F64(h.d.f64, halo_scatter_kernel, grid, stream, h, owned.block_offsets, ghost.block_offsets, owned.count,
                       out_rows);
    int rc = scope.finish("halo selection");
    if (rc != PGSD_SUCCESS)
        return rc;
    // (a row has one verdict: n_owned + n_ghost <= N, the room of out_rows)
    const uint64_t n_owned = host_count(mem, 0), n_ghost = host_count(mem, 1);
    if (n_ghost > 0)
        {
        const dim3 sgrid((unsigned)((n_ghost + SEL_THREADS - 1) / SEL_THREADS));
        PGSD_LAUNCH_BY_F64(h.d.f64, halo_shift_kernel, sgrid, stream, h, out_rows + n_owned, n_ghost, out_shift);
        rc = scope.finish("halo selection");
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    out_counts[0] = n_owned;
    out_counts[1] = n_ghost;
    return PGSD_SUCCESS;
    }

int launch_row_plan(RowPlan& p, hipStream_t stream, std::string* err)
    {
    if (p.R == 0)
        p.R = tuning().plan_block_rows;
    p.blocks.clear();
    p.run_first.clear();
    p.run_blocks.clear();
    p.staged_rows = 0;
    // (rows2 = slot * R + rest stays below T * R <= N + R, which must stay clear of the 0xFFFFFFFF of a refused entry)
    if (p.N + p.R >= (1ull << 32) || (p.n > 0 && (!p.rows || !p.rows2)))
        return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT,
                           "row plan: no row list, or the chunk's rows do not fit 32-bit indices");
    if (p.n == 0 || p.N == 0)
        {
        // nothing can be touched; every entry (all of them >= N) is refused
        if (p.n > 0 && hipMemsetAsync(p.rows2, 0xFF, p.n * 4, stream) != hipSuccess)
            return PGSD_ERROR_DEVICE;
        return p.n > 0 && hipStreamSynchronize(stream) != hipSuccess ? PGSD_ERROR_DEVICE : PGSD_SUCCESS;
        }
    const uint64_t nb = blocks_of(p.N, p.R);
    LaunchScope scope(g_select_lock, g_select_scratch, CompactionSet::bytes(nb), stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    // the set's block counts are the touched flags, its block offsets the slots
    const CompactionSet set(scope.mem().dev, nb);
    uint32_t* touched = set.block_counts;
    const dim3 grid((unsigned)std::min<uint64_t>((p.n + SEL_THREADS - 1) / SEL_THREADS, (uint64_t)num_cus() * 8)), block(SEL_THREADS);
    std::vector<uint32_t> flags(nb);
    hipError_t e = hipMemsetAsync(touched, 0, nb * 4, stream);
    if (e == hipSuccess)
        {
        hipLaunchKernelGGL(plan_mark_kernel, grid, block, 0, stream, p.rows, p.n, p.N, p.R, touched);
        enqueue_scan(set, nb, scope.mem().mapped_dev, stream);
        hipLaunchKernelGGL(plan_remap_kernel, grid, block, 0, stream, p.rows, p.n, p.N, p.R, set.block_offsets, p.rows2);
        e = hipGetLastError();
        }
    // the touched flags go back to the host (4 bytes per block: 78 KB at 80 M rows and R = 4096)
    if (e == hipSuccess)
        e = hipMemcpyAsync(flags.data(), touched, nb * 4, hipMemcpyDeviceToHost, stream);
    const int rc = scope.finish("row plan", e);
    if (rc != PGSD_SUCCESS)
        return rc;
    const uint64_t T = host_count(scope.mem());
    p.blocks.reserve(T);
    for (uint64_t b = 0; b < nb; b++)
        {
        if (!flags[b])
            continue;
        if (!p.blocks.empty() && p.blocks.back() + 1 == b)
            p.run_blocks.back()++;
        else
            {
            p.run_first.push_back((uint32_t)b);
            p.run_blocks.push_back(1);
            }
        p.blocks.push_back((uint32_t)b);
        }
    if (p.blocks.size() != T)
        return launch_fail(err, PGSD_ERROR_DEVICE, "row plan: the scan's count and the touched flags disagree");
    // a short last block has the highest slot: it shortens the staging and leaves no hole in it
    p.staged_rows = T * p.R;
    if (T > 0 && p.blocks.back() == nb - 1)
        p.staged_rows -= nb * p.R - p.N;
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd

extern "C" int pgsd_select_rows(const uint8_t* flags, uint64_t N, uint32_t* out_index, uint64_t* out_count_host, void* stream_)
    try
    {
    if (!out_count_host || (N > 0 && (!flags || !out_index)) || N >= (1ull << 32))
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (!pgsd_device_available())
        {
        set_last_error("pgsd_select_rows: no HIP device visible (the HIP path has no CPU fallback)");
        return PGSD_ERROR_NO_DEVICE;
        }
    if (N == 0)
        {
        *out_count_host = 0;
        return PGSD_SUCCESS;
        }
    // the scratch space lives on the GPU the FLAGS live on (a process with several GPUs need not have made it current)
    int device = -1;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, flags) == hipSuccess && attr.type == hipMemoryTypeDevice)
        device = attr.device;
    else
        (void)hipGetLastError();
    hipStream_t stream = (hipStream_t)stream_;
    const uint64_t nb = blocks_of(N);
    std::string msg;
    LaunchScope scope(g_select_lock, g_select_scratch, CompactionSet::bytes(nb), stream, &msg, 0, device);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc(); // (the scratch space has set the last error itself)
    const CompactionSet set(scope.mem().dev, nb);
    const dim3 grid((unsigned)nb), block(SEL_THREADS);
    hipLaunchKernelGGL(select_count_kernel, grid, block, 0, stream, flags, N, set.block_counts);
    enqueue_scan(set, nb, scope.mem().mapped_dev, stream);
    hipLaunchKernelGGL(select_scatter_kernel, grid, block, 0, stream, flags, N, set.block_offsets, out_index);
    int rc = hip_check(hipGetLastError(), "select kernel launch failed", &msg);
    if (rc == PGSD_SUCCESS)
        rc = scope.finish("pgsd_select_rows", hipSuccess);
    if (rc != PGSD_SUCCESS)
        {
        set_last_error(msg);
        return rc;
        }
    *out_count_host = host_count(scope.mem());
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }
