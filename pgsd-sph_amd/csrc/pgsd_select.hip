// pgsd_select.hip -- the smaller gfx950 kernels around the pack path:
//   compare_bytes_kernel   packed chunk == reference rows?  (the GPU-side elision test of pgsd.hoomd: numpy's equality,
//                          repeating references; reads only, 0.82-0.86 of the HBM peak)
//   select_*_kernel        stream compaction for filtered snapshots: wave ballot / popcount scans give each workgroup's
//                          count, a one-block scan turns counts into offsets (= per-chunk row and byte counts) and
//                          hands the total to the host, a scatter pass writes the index list (pgsd_select_rows)
//   domain_* / where_*_kernel   the same compaction with the predicate evaluated in both passes instead of a flag array:
//                          the rows inside a spatial domain, the rows of a particle group (type set, value ranges)
//   axis_hist_kernel / cell_count_kernel   the domain census: the same fractions binned per axis / counted per cell of a
//                          rectilinear grid, in LDS counters flushed with integer atomics
//   pgsd_device_alloc / _free / _copy   device memory owned by the library (pgsd.fl.DeviceBuffer)
// Shared device helpers: pgsd_kernels.hpp.
#include "pgsd_kernels.hpp"

namespace pgsd_amd
    {
// ------------------------------------------------------------------ packed chunk == reference rows ?
// pgsd.hoomd elides a per-particle array that equals frame 0's, or the schema's default where frame 0 has no such chunk
// (hoomd.py:654-694: numpy.array_equal / a broadcast comparison).  For arrays that live in HBM the test runs here: the
// chunk is packed as usual, then its packed bytes are compared with the reference rows (also in device memory) -- 16
// bytes per lane and load, four loads of each side in flight, grid-stride.  Bandwidth-bound when the arrays are equal
// (2 x chunk bytes read -- 1 x against a short REPEATING reference, which stays in the L2 --, nothing written).
// Equality is numpy's: integer chunks by their bytes, float chunks by VALUE -- a NaN differs from everything, itself
// included, +0.0 equals -0.0 -- decided on the bit patterns (no floating-point instruction, so no denormal mode can
// come into it).  Arrays that differ differ early, so a PROBE launch -- four workgroups per job over its first 64
// KiB -- runs first: the full launch's workgroups of a job the probe marked leave at once (had they all found the
// difference themselves, thousands of waves would each have sent their mark across PCIe: 237 us for two moving arrays
// of 10 M rows against 129 us for six equal ones).  A difference further in is still found by the full launch; the
// first workgroup to see it marks the job and the others stop at their next stride.  The flag words are never
// cleared: a launch marks with its own generation number.
// The common case is "equal": the test is shaped for it.  Per 16-byte vector: OR of the XORs (any bit differs?) and, for
// float chunks, the largest |x| bit pattern of the CHUNK's words shifted left by one (sign out): above 0xff000000 it
// is a NaN, which equals nothing -- itself included.  Only when bits differ does the slow look decide whether it is
// a +0.0 / -0.0 pair (equal by value) -- a path an equal array never takes and a different one leaves the kernel on.
template <int MODE> __device__ __forceinline__ uint32_t cmp_differ16(const u32x4 x, const u32x4 y)
    {
    const uint32_t differ = (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    if (MODE == CMP_BYTES)
        return differ;
    if (MODE == CMP_F32)
        {
        const uint32_t m = max(max(x.x << 1, x.y << 1), max(x.z << 1, x.w << 1));
        uint32_t bad = m > 0xff000000u ? 1u : 0u; // a NaN among the chunk's four floats
        if (differ != 0)
            {
            const uint32_t a[4] = {x.x, x.y, x.z, x.w}, b[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int k = 0; k < 4; k++) // bits differ: equal all the same when both are zeros of either sign
                bad |= ((a[k] ^ b[k]) != 0 && ((a[k] | b[k]) << 1) != 0) ? 1u : 0u;
            }
        return bad;
        }
    // CMP_F64: two doubles per vector, little endian (low word first).  (hi << 1) | (lo != 0) > 0xffe00000: a NaN
    const uint32_t t0 = (x.y << 1) | (x.x != 0 ? 1u : 0u), t1 = (x.w << 1) | (x.z != 0 ? 1u : 0u);
    uint32_t bad = max(t0, t1) > 0xffe00000u ? 1u : 0u;
    if (differ != 0)
        {
        const uint32_t al[2] = {x.x, x.z}, ah[2] = {x.y, x.w}, bl[2] = {y.x, y.z}, bh[2] = {y.y, y.w};
#pragma unroll
        for (int k = 0; k < 2; k++)
            bad |= (((al[k] ^ bl[k]) | (ah[k] ^ bh[k])) != 0 && (((ah[k] | bh[k]) << 1) | al[k] | bl[k]) != 0) ? 1u : 0u;
        }
    return bad;
    }

// one element of `es` bytes (1: a byte of an integer chunk) at byte offset `at`, assembled from bytes: the slow road of
// unaligned pointers and of the last bytes
__device__ __forceinline__ bool cmp_differ_element(const char* pa, const char* pb, uint64_t at, uint64_t at_b, uint32_t es,
                                                   uint32_t mode)
    {
    uint64_t a = 0, b = 0;
    for (uint32_t k = 0; k < es; k++)
        {
        a |= (uint64_t)(uint8_t)pa[at + k] << (8 * k);
        b |= (uint64_t)(uint8_t)pb[at_b + k] << (8 * k);
        }
    if (mode == CMP_F32)
        return ((a ^ b) != 0 && ((a | b) & 0x7fffffffull) != 0) || (a & 0x7fffffffull) > 0x7f800000ull;
    if (mode == CMP_F64)
        return ((a ^ b) != 0 && ((a | b) & 0x7fffffffffffffffull) != 0) || (a & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
    return a != b;
    }

template <int MODE, bool PERIODIC>
__device__ __forceinline__ bool cmp_vector_loop(const u32x4* a, const u32x4* b, uint64_t n16, uint64_t period16, const uint32_t* df,
                                                uint32_t gen)
    {
    const uint64_t per_block = 256 * 4;
    for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < n16; base += (uint64_t)gridDim.x * per_block)
        {
        if (__hip_atomic_load(df, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen)
            return false; // somebody else has the answer
        // a repeating reference: ONE modulo per lane and stride, the three further vectors by a conditional step back
        // (period16 >= 256 is checked by the host)
        uint64_t bi = PERIODIC ? (base + threadIdx.x) % period16 : 0;
        u32x4 x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
            {
            const uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
            x[k] = (u32x4)(0u);
            y[k] = (u32x4)(0u);
            if (i < n16)
                {
                x[k] = __builtin_nontemporal_load(a + i);
                y[k] = PERIODIC ? b[bi] : __builtin_nontemporal_load(b + i);
                }
            if (PERIODIC)
                {
                bi += 256;
                if (bi >= period16)
                    bi -= period16;
                }
            }
        uint32_t acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            acc |= cmp_differ16<MODE>(x[k], y[k]);
        if (acc != 0)
            return true;
        }
    return false;
    }

__global__ __launch_bounds__(256) void compare_bytes_kernel(const CompareArgs args)
    {
    CompareJob jb = args.j[blockIdx.y];
    uint32_t* df = args.dflags + blockIdx.y;
    if (args.limit != 0 && jb.bytes > args.limit)
        jb.bytes = args.limit;
    if (__hip_atomic_load(df, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == args.gen)
        return; // marked by the probe (or by a quicker workgroup)
    bool diff = false;
    const char* pa = (const char*)jb.a;
    const char* pb = (const char*)jb.b;
    uint64_t done = 0; // bytes covered by the vector loop
    if ((((uintptr_t)pa | (uintptr_t)pb) & 15) == 0)
        {
        const u32x4* a = (const u32x4*)pa;
        const u32x4* b = (const u32x4*)pb;
        const uint64_t n16 = jb.bytes >> 4;
        const uint64_t p16 = jb.period >> 4;
        done = n16 << 4;
        if (jb.period == 0)
            diff = jb.mode == CMP_F32   ? cmp_vector_loop<CMP_F32, false>(a, b, n16, 0, df, args.gen)
                   : jb.mode == CMP_F64 ? cmp_vector_loop<CMP_F64, false>(a, b, n16, 0, df, args.gen)
                                        : cmp_vector_loop<CMP_BYTES, false>(a, b, n16, 0, df, args.gen);
        else
            diff = jb.mode == CMP_F32   ? cmp_vector_loop<CMP_F32, true>(a, b, n16, p16, df, args.gen)
                   : jb.mode == CMP_F64 ? cmp_vector_loop<CMP_F64, true>(a, b, n16, p16, df, args.gen)
                                        : cmp_vector_loop<CMP_BYTES, true>(a, b, n16, p16, df, args.gen);
        }
    // what the vector loop left: the last bytes, or everything when a side is not 16-byte aligned -- element by element
    const uint32_t es = jb.mode == CMP_F32 ? 4u : jb.mode == CMP_F64 ? 8u : 1u;
    for (uint64_t i = done + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * es; i + es <= jb.bytes && !diff;
         i += (uint64_t)gridDim.x * 256 * es)
        diff = cmp_differ_element(pa, pb, i, jb.period ? i % jb.period : i, es, jb.mode);
    const uint64_t who = __ballot(diff);
    if (who != 0 && (uint32_t)(__ffsll((unsigned long long)who) - 1) == (threadIdx.x & 63u))
        {
        __hip_atomic_store(df, args.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(args.hflags + blockIdx.y, args.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }

void warm_select_kernels()
    {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)compare_bytes_kernel);
    (void)hipGetLastError();
    }

int launch_compare(uint32_t n_jobs, const CompareJob* jobs, uint32_t gen, uint32_t* dflags, uint32_t* hflags,
                   hipStream_t stream, std::string* err)
    {
    if (n_jobs == 0)
        return PGSD_SUCCESS;
    if (n_jobs > CMP_MAX_JOBS || !jobs || !dflags || !hflags)
        return PGSD_ERROR_INVALID_ARGUMENT;
    CompareArgs args;
    memset(&args, 0, sizeof(args));
    args.dflags = dflags;
    args.hflags = hflags;
    args.gen = gen;
    args.n_jobs = n_jobs;
    uint64_t most = 0;
    for (uint32_t i = 0; i < n_jobs; i++)
        {
        args.j[i] = jobs[i];
        most = std::max<uint64_t>(most, jobs[i].bytes);
        }
    // one workgroup per 16 KiB of the longest job, at most eight per CU of the part (2048): grid-stride beyond
    uint64_t blocks = (most + 16383) / 16384;
    blocks = std::min<uint64_t>(std::max<uint64_t>(blocks, 1), 2048);
    // whatever an earlier call of this thread left in the runtime's last-error slot (a failed hipMalloc, the caller's own
    // calls) is not this launch's: the slot is read again right behind the launches
    (void)hipGetLastError();
    if (most > 65536)
        {
        args.limit = 65536;
        hipLaunchKernelGGL(compare_bytes_kernel, dim3(4, n_jobs), dim3(256), 0, stream, args); // 16 KiB per workgroup
        args.limit = 0;
        }
    hipLaunchKernelGGL(compare_bytes_kernel, dim3((unsigned)blocks, n_jobs), dim3(256), 0, stream, args);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        {
        if (err)
            *err = std::string("compare kernel launch failed: ") + hipGetErrorString(e);
        return PGSD_ERROR_DEVICE;
        }
    return PGSD_SUCCESS;
    }

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

// inclusive scan of one value per lane across the 64-lane wavefront
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x)
    {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
        {
        uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d)
            x += y;
        }
    return x;
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
// (the two halves of the fraction, shared with the ghost layer's halo_class() below)
__device__ __forceinline__ void domain_skew(const DomainArgs& d, double x, double y, double z, double s[3])
    {
#pragma clang fp contract(off)
    s[0] = ((x + d.L[0] / 2.0) - ((d.xz - d.yz * d.xy) * z + d.xy * y)) / d.L[0];
    s[1] = ((y + d.L[1] / 2.0) - d.yz * z) / d.L[1];
    s[2] = (z + d.L[2] / 2.0) / d.L[2];
    }

__device__ __forceinline__ double domain_wrap(double s)
    {
#pragma clang fp contract(off)
    double f = s - floor(s);
    if (f >= 1.0)
        f = 0.0;
    return f;
    }

__device__ __forceinline__ bool domain_inside(const DomainArgs& d, double x, double y, double z)
    {
#pragma clang fp contract(off)
    double s[3];
    domain_skew(d, x, y, z, s);
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++)
        {
        if (a == 2 && d.dims == 2)
            break;
        const double f = domain_wrap(s[a]);
        in = in && d.lo[a] <= f && f < d.hi[a];
        }
    return in;
    }

// the SEL_PER_THREAD rows of this lane as doubles (zeros past the end): rows base + k * SEL_THREADS + threadIdx.x
template<bool F64>
__device__ __forceinline__ void domain_load_rows(const void* pos, uint64_t N, uint64_t base, double p[SEL_PER_THREAD][3])
    {
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        {
        const uint64_t i = base + (uint64_t)k * SEL_THREADS + threadIdx.x;
        p[k][0] = p[k][1] = p[k][2] = 0.0;
        if (i < N)
            {
            if constexpr (F64)
                {
                const double* q = (const double*)pos + i * 3;
                p[k][0] = __builtin_nontemporal_load(q);
                p[k][1] = __builtin_nontemporal_load(q + 1);
                p[k][2] = __builtin_nontemporal_load(q + 2);
                }
            else
                {
                const u32x3 v = __builtin_nontemporal_load((const u32x3_a4*)((const uint32_t*)pos + i * 3));
                p[k][0] = (double)__uint_as_float(v.x);
                p[k][1] = (double)__uint_as_float(v.y);
                p[k][2] = (double)__uint_as_float(v.z);
                }
            }
        }
    }

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

// ------------------------------------------------------------------ domain census (which decomposition to ask for)
// pgsd.hoomd.axis_histograms and domain_counts are the definitions.  The fraction is the selections' own -- domain_skew()
// and domain_wrap() over domain_load_rows()' rows --, binned instead of compared with one cell: a histogram of `bins`
// bins per axis (a power of two: f * bins is exact and below bins, every edge k / bins an exact double), or the rows of
// every cell of a rectilinear grid (a row's cell on an axis: the number of interior bounds b with b <= f, the model's
// comparison).  A NaN fraction (NaN or infinite coordinates) is tested for BEFORE the conversion to an integer and
// counted in no bin / in `nowhere`.  A workgroup keeps its counters in LDS, strides over 4096-row tiles (the grid is
// capped by the launcher), and adds its non-zero counters to the global ones at the end: integer adds commute, so the
// result does not depend on the order.
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void axis_hist_kernel(const DomainArgs d, uint32_t bins, uint64_t n_tiles,
                                                                uint32_t* hist)
    {
#pragma clang fp contract(off)
    __shared__ uint32_t lds[3 * CENSUS_MAX_BINS];
    const uint32_t n_counters = 3 * bins;
    for (uint32_t i = threadIdx.x; i < n_counters; i += SEL_THREADS)
        lds[i] = 0;
    __syncthreads();
    const double scale = (double)bins;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        {
        const uint64_t base = tile * SEL_PER_BLOCK;
        double p[SEL_PER_THREAD][3];
        domain_load_rows<F64>(d.pos, d.N, base, p);
#pragma unroll
        for (int k = 0; k < SEL_PER_THREAD; k++)
            {
            const uint64_t i = base + (uint64_t)k * SEL_THREADS + threadIdx.x;
            if (i >= d.N)
                continue;
            double s[3];
            domain_skew(d, p[k][0], p[k][1], p[k][2], s);
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                if (a == 2 && d.dims == 2)
                    break;
                const double f = domain_wrap(s[a]);
                if (f == f)
                    atomicAdd(&lds[a * bins + (uint32_t)(f * scale)], 1u);
                }
            }
        }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_counters; i += SEL_THREADS)
        {
        const uint32_t c = lds[i];
        if (c)
            atomicAdd(&hist[i], c);
        }
    }

// counts: n[0] * n[1] * n[2] cell counters, then the `nowhere` counter
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void cell_count_kernel(const CellArgs c, uint64_t n_tiles, uint32_t* counts)
    {
    __shared__ double bound[3][CENSUS_MAX_AXIS_CELLS - 1];
    __shared__ uint32_t lds[CENSUS_MAX_CELLS + 1];
    const uint32_t n_cells = c.n[0] * c.n[1] * c.n[2];
    for (uint32_t i = threadIdx.x; i <= n_cells; i += SEL_THREADS)
        lds[i] = 0;
    for (uint32_t i = threadIdx.x; i < 3 * (CENSUS_MAX_AXIS_CELLS - 1); i += SEL_THREADS)
        {
        const uint32_t a = i / (CENSUS_MAX_AXIS_CELLS - 1), j = i % (CENSUS_MAX_AXIS_CELLS - 1);
        if (j + 1 < c.n[a])
            bound[a][j] = c.bounds[a][j];
        }
    __syncthreads();
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)
        {
        const uint64_t base = tile * SEL_PER_BLOCK;
        double p[SEL_PER_THREAD][3];
        domain_load_rows<F64>(c.d.pos, c.d.N, base, p);
#pragma unroll
        for (int k = 0; k < SEL_PER_THREAD; k++)
            {
            const uint64_t i = base + (uint64_t)k * SEL_THREADS + threadIdx.x;
            if (i >= c.d.N)
                continue;
            double s[3];
            domain_skew(c.d, p[k][0], p[k][1], p[k][2], s);
            uint32_t cell = 0, stride = 1;
            bool somewhere = true;
#pragma unroll
            for (int a = 0; a < 3; a++)
                {
                if (a == 2 && c.d.dims == 2)
                    break;
                const double f = domain_wrap(s[a]);
                somewhere = somewhere && f == f;
                // the number of bounds <= f: the upper bound of f in the ascending list (none for a NaN)
                uint32_t at = 0, len = c.n[a] - 1;
                while (len > 0)
                    {
                    const uint32_t half = len >> 1;
                    if (bound[a][at + half] <= f)
                        {
                        at += half + 1;
                        len -= half + 1;
                        }
                    else
                        len = half;
                    }
                cell += at * stride;
                stride *= c.n[a];
                }
            atomicAdd(&lds[somewhere ? cell : n_cells], 1u);
            }
        }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= n_cells; i += SEL_THREADS)
        {
        const uint32_t v = lds[i];
        if (v)
            atomicAdd(&counts[i], v);
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
    } // namespace pgsd_amd

using namespace pgsd_amd;

namespace
    {
struct SelectScratch
    {
    void* dev = nullptr;
    size_t cap = 0;
    uint64_t* host_count = nullptr;     // pinned, device-mapped: the scan writes the count into it (two words: the halo
                                        // selection's second scan writes into the second)
    uint64_t* host_count_dev = nullptr; // ... through this alias
    };
std::mutex g_select_lock;
std::map<int, SelectScratch> g_select_scratch;

// the scratch space of a compaction of N rows on `device` (current; g_select_lock held): the count (u64), the block counts
// (u32) rounded to 8 bytes, the block offsets (u64) -- `sets` such triples, one behind the other (the halo selection
// compacts two lists) --; and the pinned words the scans leave their counts in
size_t select_set_bytes(uint64_t nb)
    {
    return 8 + (size_t)(((nb * 4 + 7) & ~7ull) + nb * 8);
    }

int select_scratch(int device, uint64_t N, SelectScratch** out, uint64_t per_block = SEL_PER_BLOCK, unsigned sets = 1)
    {
    SelectScratch& sc = g_select_scratch[device];
    const uint64_t nb = (N + per_block - 1) / per_block;
    const size_t need = sets * select_set_bytes(nb);
    if (need > sc.cap)
        {
        if (sc.dev)
            (void)hipFree(sc.dev);
        sc.dev = nullptr;
        sc.cap = 0;
        const size_t cap = std::max<size_t>(need * 2, 1u << 16);
        if (hipMalloc(&sc.dev, cap) != hipSuccess)
            {
            sc.dev = nullptr;
            set_last_error("pgsd_select_rows: cannot allocate the scratch space");
            return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
            }
        sc.cap = cap;
        }
    if (!sc.host_count)
        {
        void* alias = nullptr;
        if (hipHostMalloc((void**)&sc.host_count, 2 * sizeof(uint64_t), hipHostMallocMapped) != hipSuccess
            || hipHostGetDevicePointer(&alias, sc.host_count, 0) != hipSuccess)
            {
            if (sc.host_count)
                (void)hipHostFree(sc.host_count);
            sc.host_count = nullptr;
            set_last_error("pgsd_select_rows: cannot allocate pinned memory");
            return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
            }
        sc.host_count_dev = (uint64_t*)alias;
        }
    *out = &sc;
    return PGSD_SUCCESS;
    }

// SelectScratch's small sibling for the census: the global counters (3 x CENSUS_MAX_BINS words, which also hold
// CENSUS_MAX_CELLS + 1), their pinned landing place on the host, and the grid cap (g_select_lock held)
struct CensusScratch
    {
    uint32_t* dev = nullptr;
    uint32_t* host = nullptr;
    unsigned max_blocks = 0; // 2 x compute units
    };
std::map<int, CensusScratch> g_census_scratch;
constexpr size_t CENSUS_WORDS = 3 * CENSUS_MAX_BINS;
static_assert(CENSUS_MAX_CELLS + 1 <= CENSUS_WORDS, "the cell counters share the histogram's room");

int census_scratch(int device, CensusScratch** out)
    {
    CensusScratch& sc = g_census_scratch[device];
    if (!sc.dev && hipMalloc((void**)&sc.dev, CENSUS_WORDS * sizeof(uint32_t)) != hipSuccess)
        {
        sc.dev = nullptr;
        set_last_error("domain census: cannot allocate the counters");
        return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
        }
    if (!sc.host && hipHostMalloc((void**)&sc.host, CENSUS_WORDS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
        {
        sc.host = nullptr;
        set_last_error("domain census: cannot allocate pinned memory");
        return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
        }
    if (!sc.max_blocks)
        {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1)
            cus = 256;
        sc.max_blocks = 2u * (unsigned)cus;
        }
    *out = &sc;
    return PGSD_SUCCESS;
    }
    } // namespace

namespace pgsd_amd
    {
// count -> scan -> scatter of a predicate selection over N rows (0 < N < 2^32) on `stream`; `launch(count pass?,
// blocks, block counts, block offsets)` enqueues the predicate's own kernel for either pass
template<class Launch>
static int select_by_predicate(uint64_t N, const char* what, uint64_t* out_count, hipStream_t stream, std::string* err,
                               Launch launch)
    {
    std::lock_guard<std::mutex> guard(g_select_lock);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    SelectScratch* sc = nullptr;
    int rc = select_scratch(device, N, &sc);
    if (rc != PGSD_SUCCESS)
        {
        if (err)
            *err = last_error();
        return rc;
        }
    (void)hipGetLastError(); // (see pgsd_select_rows)
    const uint64_t n_blocks = (N + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK;
    uint32_t* block_counts = (uint32_t*)((char*)sc->dev + 8);
    uint64_t* block_offsets = (uint64_t*)((char*)sc->dev + 8 + ((n_blocks * 4 + 7) & ~7ull));
    launch(true, (unsigned)n_blocks, block_counts, block_offsets);
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, stream, block_counts, (uint32_t)n_blocks,
                       block_offsets, (uint64_t*)sc->dev, sc->host_count_dev);
    launch(false, (unsigned)n_blocks, block_counts, block_offsets);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream); // the kernels are through: the count is in the pinned word
    if (e != hipSuccess)
        {
        if (err)
            *err = std::string(what) + ": " + hipGetErrorString(e);
        return PGSD_ERROR_DEVICE;
        }
    *out_count = __atomic_load_n(sc->host_count, __ATOMIC_ACQUIRE);
    return PGSD_SUCCESS;
    }

int launch_select_domain(const DomainArgs& d, uint32_t* out_rows, uint64_t* out_count, hipStream_t stream, std::string* err)
    {
    *out_count = 0;
    if (d.N == 0)
        return PGSD_SUCCESS;
    if (d.N >= (1ull << 32) || !d.pos || !out_rows)
        return PGSD_ERROR_INVALID_ARGUMENT;
    return select_by_predicate(d.N, "domain selection", out_count, stream, err,
                               [&](bool count, unsigned n_blocks, uint32_t* block_counts, uint64_t* block_offsets)
                               {
                                   if (count && d.f64)
                                       hipLaunchKernelGGL(domain_count_kernel<true>, dim3(n_blocks), dim3(SEL_THREADS), 0,
                                                          stream, d, block_counts);
                                   else if (count)
                                       hipLaunchKernelGGL(domain_count_kernel<false>, dim3(n_blocks), dim3(SEL_THREADS), 0,
                                                          stream, d, block_counts);
                                   else if (d.f64)
                                       hipLaunchKernelGGL(domain_scatter_kernel<true>, dim3(n_blocks), dim3(SEL_THREADS), 0,
                                                          stream, d, block_offsets, out_rows);
                                   else
                                       hipLaunchKernelGGL(domain_scatter_kernel<false>, dim3(n_blocks), dim3(SEL_THREADS), 0,
                                                          stream, d, block_offsets, out_rows);
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
                               [&](bool count, unsigned n_blocks, uint32_t* block_counts, uint64_t* block_offsets)
                               {
                                   if (count)
                                       hipLaunchKernelGGL(where_count_kernel, dim3(n_blocks), dim3(SEL_THREADS), 0, stream,
                                                          w, block_counts);
                                   else
                                       hipLaunchKernelGGL(where_scatter_kernel, dim3(n_blocks), dim3(SEL_THREADS), 0, stream,
                                                          w, block_offsets, out_rows);
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
    std::lock_guard<std::mutex> guard(g_select_lock);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    SelectScratch* sc = nullptr;
    int rc = select_scratch(device, N, &sc, SEL_PER_BLOCK, 2);
    if (rc != PGSD_SUCCESS)
        {
        if (err)
            *err = last_error();
        return rc;
        }
    (void)hipGetLastError(); // (see pgsd_select_rows)
    const uint64_t nb = (N + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK;
    uint64_t* count[2];
    uint32_t* block_counts[2];
    uint64_t* block_offsets[2];
    for (int j = 0; j < 2; j++)
        {
        char* set = (char*)sc->dev + j * select_set_bytes(nb);
        count[j] = (uint64_t*)set;
        block_counts[j] = (uint32_t*)(set + 8);
        block_offsets[j] = (uint64_t*)(set + 8 + ((nb * 4 + 7) & ~7ull));
        }
    const dim3 grid((unsigned)nb), block(SEL_THREADS);
    if (h.d.f64)
        hipLaunchKernelGGL(halo_count_kernel<true>, grid, block, 0, stream, h, block_counts[0], block_counts[1]);
    else
        hipLaunchKernelGGL(halo_count_kernel<false>, grid, block, 0, stream, h, block_counts[0], block_counts[1]);
    for (int j = 0; j < 2; j++)
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), block, 0, stream, block_counts[j], (uint32_t)nb, block_offsets[j],
                           count[j], sc->host_count_dev + j);
    if (h.d.f64)
        hipLaunchKernelGGL(halo_scatter_kernel<true>, grid, block, 0, stream, h, block_offsets[0], block_offsets[1], count[0],
                           out_rows);
    else
        hipLaunchKernelGGL(halo_scatter_kernel<false>, grid, block, 0, stream, h, block_offsets[0], block_offsets[1], count[0],
                           out_rows);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream); // the kernels are through: the counts are in the pinned words
    uint64_t n_owned = 0, n_ghost = 0;
    if (e == hipSuccess)
        {
        // (a row has one verdict: n_owned + n_ghost <= N, the room of out_rows)
        n_owned = __atomic_load_n(sc->host_count, __ATOMIC_ACQUIRE);
        n_ghost = __atomic_load_n(sc->host_count + 1, __ATOMIC_ACQUIRE);
        }
    if (e == hipSuccess && n_ghost > 0)
        {
        const dim3 sgrid((unsigned)((n_ghost + SEL_THREADS - 1) / SEL_THREADS));
        if (h.d.f64)
            hipLaunchKernelGGL(halo_shift_kernel<true>, sgrid, block, 0, stream, h, out_rows + n_owned, n_ghost, out_shift);
        else
            hipLaunchKernelGGL(halo_shift_kernel<false>, sgrid, block, 0, stream, h, out_rows + n_owned, n_ghost, out_shift);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipStreamSynchronize(stream);
        }
    if (e != hipSuccess)
        {
        if (err)
            *err = std::string("halo selection: ") + hipGetErrorString(e);
        return PGSD_ERROR_DEVICE;
        }
    out_counts[0] = n_owned;
    out_counts[1] = n_ghost;
    return PGSD_SUCCESS;
    }

// One census pass over N rows (0 < N < 2^32) on `stream`: `words` global counters zeroed, `launch(blocks, tiles,
// counters)` enqueues the kernel over min(tiles, 2 x compute units) workgroups, the counters land in pinned memory and
// -- after the one stream wait -- in out[0 .. words) as 64-bit counts.
template<class Launch>
static int census_pass(uint64_t N, size_t words, const char* what, uint64_t* out, hipStream_t stream, std::string* err,
                       Launch launch)
    {
    std::lock_guard<std::mutex> guard(g_select_lock);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    CensusScratch* sc = nullptr;
    int rc = census_scratch(device, &sc);
    if (rc != PGSD_SUCCESS)
        {
        if (err)
            *err = last_error();
        return rc;
        }
    (void)hipGetLastError(); // (see pgsd_select_rows)
    const uint64_t n_tiles = (N + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK;
    const unsigned n_blocks = (unsigned)std::min<uint64_t>(n_tiles, sc->max_blocks);
    hipError_t e = hipMemsetAsync(sc->dev, 0, words * sizeof(uint32_t), stream);
    if (e == hipSuccess)
        {
        launch(n_blocks, n_tiles, sc->dev);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(sc->host, sc->dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (e != hipSuccess)
        {
        if (err)
            *err = std::string(what) + ": " + hipGetErrorString(e);
        return PGSD_ERROR_DEVICE;
        }
    for (size_t i = 0; i < words; i++)
        out[i] = sc->host[i];
    return PGSD_SUCCESS;
    }

int launch_axis_histograms(const DomainArgs& d, uint32_t bins, uint64_t* out_hist, hipStream_t stream, std::string* err)
    {
    if (bins < 2 || bins > CENSUS_MAX_BINS || (bins & (bins - 1)) != 0 || !out_hist)
        return PGSD_ERROR_INVALID_ARGUMENT;
    std::fill(out_hist, out_hist + 3 * (size_t)bins, 0ull);
    if (d.N == 0)
        return PGSD_SUCCESS;
    if (d.N >= (1ull << 32) || !d.pos)
        return PGSD_ERROR_INVALID_ARGUMENT;
    return census_pass(d.N, 3 * (size_t)bins, "axis histograms", out_hist, stream, err,
                       [&](unsigned n_blocks, uint64_t n_tiles, uint32_t* hist)
                       {
                           if (d.f64)
                               hipLaunchKernelGGL(axis_hist_kernel<true>, dim3(n_blocks), dim3(SEL_THREADS), 0, stream, d,
                                                  bins, n_tiles, hist);
                           else
                               hipLaunchKernelGGL(axis_hist_kernel<false>, dim3(n_blocks), dim3(SEL_THREADS), 0, stream, d,
                                                  bins, n_tiles, hist);
                       });
    }

int launch_cell_counts(const CellArgs& c, uint64_t* out_counts, uint64_t* out_nowhere, hipStream_t stream, std::string* err)
    {
    uint64_t n_cells = 1;
    for (int a = 0; a < 3; a++)
        {
        if (c.n[a] < 1 || c.n[a] > CENSUS_MAX_AXIS_CELLS)
            return PGSD_ERROR_INVALID_ARGUMENT;
        n_cells *= c.n[a];
        }
    if (n_cells > CENSUS_MAX_CELLS || !out_counts || !out_nowhere)
        return PGSD_ERROR_INVALID_ARGUMENT;
    std::fill(out_counts, out_counts + n_cells, 0ull);
    *out_nowhere = 0;
    if (c.d.N == 0)
        return PGSD_SUCCESS;
    if (c.d.N >= (1ull << 32) || !c.d.pos)
        return PGSD_ERROR_INVALID_ARGUMENT;
    std::vector<uint64_t> all(n_cells + 1);
    int rc = census_pass(c.d.N, n_cells + 1, "cell counts", all.data(), stream, err,
                         [&](unsigned n_blocks, uint64_t n_tiles, uint32_t* counts)
                         {
                             if (c.d.f64)
                                 hipLaunchKernelGGL(cell_count_kernel<true>, dim3(n_blocks), dim3(SEL_THREADS), 0, stream, c,
                                                    n_tiles, counts);
                             else
                                 hipLaunchKernelGGL(cell_count_kernel<false>, dim3(n_blocks), dim3(SEL_THREADS), 0, stream, c,
                                                    n_tiles, counts);
                         });
    if (rc != PGSD_SUCCESS)
        return rc;
    std::copy(all.begin(), all.begin() + n_cells, out_counts);
    *out_nowhere = all[n_cells];
    return PGSD_SUCCESS;
    }

// Cell order.  The scratch space (grow-only, per device, g_select_lock held) holds, in 32-bit words: two key and two
// value buffers of n (the passes ping-pong between them), the copy of the row list (n) and of the ghosts' shifts
// (3 x ghosts), the digit table (256 x tiles), the digit totals (256) and the device flag word; the pinned flag word is
// the host's view of "an entry was >= N".
struct OrderScratch
    {
    uint32_t* dev = nullptr;
    size_t cap_words = 0;
    uint32_t* host_flag = nullptr;     // pinned, device-mapped
    uint32_t* host_flag_dev = nullptr; // ... through this alias
    };
static std::map<int, OrderScratch> g_order_scratch;

static int order_scratch(int device, size_t words, OrderScratch** out)
    {
    OrderScratch& sc = g_order_scratch[device];
    if (words > sc.cap_words)
        {
        if (sc.dev)
            (void)hipFree(sc.dev);
        sc.dev = nullptr;
        sc.cap_words = 0;
        const size_t cap = std::max<size_t>(words + words / 4, 1u << 14);
        if (hipMalloc((void**)&sc.dev, cap * sizeof(uint32_t)) != hipSuccess)
            {
            sc.dev = nullptr;
            (void)hipGetLastError();
            set_last_error("cell order: cannot allocate the scratch space");
            return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
            }
        sc.cap_words = cap;
        }
    if (!sc.host_flag)
        {
        void* alias = nullptr;
        if (hipHostMalloc((void**)&sc.host_flag, sizeof(uint64_t), hipHostMallocMapped) != hipSuccess
            || hipHostGetDevicePointer(&alias, sc.host_flag, 0) != hipSuccess)
            {
            if (sc.host_flag)
                (void)hipHostFree(sc.host_flag);
            sc.host_flag = nullptr;
            set_last_error("cell order: cannot allocate pinned memory");
            return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
            }
        sc.host_flag_dev = (uint32_t*)alias;
        }
    *out = &sc;
    return PGSD_SUCCESS;
    }

// the number of 8-bit passes that cover every key of a call: the bits of the largest one
static unsigned order_passes(uint64_t max_key)
    {
    unsigned bits = 1;
    while (bits < 32 && (max_key >> bits) != 0)
        bits++;
    return (bits + SORT_DIGIT_BITS - 1) / SORT_DIGIT_BITS;
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
    std::lock_guard<std::mutex> guard(g_select_lock);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    const uint64_t n_ghost = n - o.n_owned;
    const uint64_t n_tiles = (n + SORT_TILE - 1) / SORT_TILE;
    const auto round4 = [](uint64_t words) { return (words + 3) & ~3ull; }; // 16-byte aligned parts
    const uint64_t part = round4(n), shift_words = shift ? round4(3 * n_ghost) : 0, table_words = round4(SORT_RADIX * n_tiles);
    OrderScratch* sc = nullptr;
    int rc = order_scratch(device, (size_t)(5 * part + shift_words + table_words + SORT_RADIX + 4), &sc);
    if (rc != PGSD_SUCCESS)
        {
        if (err)
            *err = last_error();
        return rc;
        }
    (void)hipGetLastError(); // (see pgsd_select_rows)
    uint32_t* keys[2] = {sc->dev, sc->dev + part};
    uint32_t* vals[2] = {sc->dev + 2 * part, sc->dev + 3 * part};
    uint32_t* rows_copy = sc->dev + 4 * part;
    int32_t* shift_copy = (int32_t*)(sc->dev + 5 * part);
    uint32_t* table = sc->dev + 5 * part + shift_words;
    uint32_t* totals = table + table_words;
    uint32_t* flag_dev = totals + SORT_RADIX;
    __atomic_store_n(sc->host_flag, 0u, __ATOMIC_RELEASE);
    const dim3 block(SEL_THREADS), per_entry((unsigned)((n + SEL_THREADS - 1) / SEL_THREADS)), per_tile((unsigned)n_tiles);
    hipError_t e = hipMemsetAsync(flag_dev, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess && shift && n_ghost > 0)
        e = hipMemcpyAsync(shift_copy, shift, 3 * n_ghost * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess)
        {
        if (o.d.f64)
            hipLaunchKernelGGL(order_key_kernel<true>, per_entry, block, 0, stream, o, rows, keys[0], vals[0], rows_copy,
                               flag_dev, sc->host_flag_dev);
        else
            hipLaunchKernelGGL(order_key_kernel<false>, per_entry, block, 0, stream, o, rows, keys[0], vals[0], rows_copy,
                               flag_dev, sc->host_flag_dev);
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
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (e != hipSuccess)
        {
        if (err)
            *err = std::string("cell order: ") + hipGetErrorString(e);
        return PGSD_ERROR_DEVICE;
        }
    if (__atomic_load_n(sc->host_flag, __ATOMIC_ACQUIRE) != 0)
        {
        if (err)
            *err = "cell order: an entry of the row list lies outside the position chunk (nothing was reordered)";
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
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
        {
        if (err)
            *err = "row plan: no row list, or the chunk's rows do not fit 32-bit indices";
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    if (p.n == 0 || p.N == 0)
        {
        // nothing can be touched; every entry (all of them >= N) is refused
        if (p.n > 0 && hipMemsetAsync(p.rows2, 0xFF, p.n * 4, stream) != hipSuccess)
            return PGSD_ERROR_DEVICE;
        return p.n > 0 && hipStreamSynchronize(stream) != hipSuccess ? PGSD_ERROR_DEVICE : PGSD_SUCCESS;
        }
    std::lock_guard<std::mutex> guard(g_select_lock);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    SelectScratch* sc = nullptr;
    int rc = select_scratch(device, p.N, &sc, p.R);
    if (rc != PGSD_SUCCESS)
        {
        if (err)
            *err = last_error();
        return rc;
        }
    (void)hipGetLastError(); // (see pgsd_select_rows)
    const uint64_t nb = (p.N + p.R - 1) / p.R;
    uint32_t* touched = (uint32_t*)((char*)sc->dev + 8);
    uint64_t* slot = (uint64_t*)((char*)sc->dev + 8 + ((nb * 4 + 7) & ~7ull));
    const unsigned grid = (unsigned)std::min<uint64_t>((p.n + SEL_THREADS - 1) / SEL_THREADS, (uint64_t)num_cus() * 8);
    std::vector<uint32_t> flags(nb);
    hipError_t e = hipMemsetAsync(touched, 0, nb * 4, stream);
    if (e == hipSuccess)
        {
        hipLaunchKernelGGL(plan_mark_kernel, dim3(grid), dim3(SEL_THREADS), 0, stream, p.rows, p.n, p.N, p.R, touched);
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, stream, touched, (uint32_t)nb, slot,
                           (uint64_t*)sc->dev, sc->host_count_dev);
        hipLaunchKernelGGL(plan_remap_kernel, dim3(grid), dim3(SEL_THREADS), 0, stream, p.rows, p.n, p.N, p.R, slot, p.rows2);
        e = hipGetLastError();
        }
    // the touched flags go back to the host (4 bytes per block: 78 KB at 80 M rows and R = 4096)
    if (e == hipSuccess)
        e = hipMemcpyAsync(flags.data(), touched, nb * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (e != hipSuccess)
        {
        if (err)
            *err = std::string("row plan: ") + hipGetErrorString(e);
        return PGSD_ERROR_DEVICE;
        }
    const uint64_t T = __atomic_load_n(sc->host_count, __ATOMIC_ACQUIRE);
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
        {
        if (err)
            *err = "row plan: the scan's count and the touched flags disagree";
        return PGSD_ERROR_DEVICE;
        }
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
    std::lock_guard<std::mutex> guard(g_select_lock);
    // the scratch space lives on the GPU the FLAGS live on (a process with several GPUs need not have made it current)
    int current = 0, device = 0;
    if (hipGetDevice(&current) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    device = current;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, flags) == hipSuccess && attr.type == hipMemoryTypeDevice)
        device = attr.device;
    else
        (void)hipGetLastError();
    struct DeviceScope // restore the caller's current device on every way out
        {
        int back;
        bool on;
        ~DeviceScope()
            {
            if (on)
                (void)hipSetDevice(back);
            }
        } scope {current, device != current};
    if (scope.on && hipSetDevice(device) != hipSuccess)
        return PGSD_ERROR_DEVICE;
    SelectScratch* scp = nullptr;
    int rc = select_scratch(device, N, &scp);
    if (rc != PGSD_SUCCESS)
        return rc;
    SelectScratch& sc = *scp;
    // whatever an earlier call of this thread left in the runtime's last-error slot (a failed hipMalloc, the caller's own
    // calls) is not this launch's: the slot is read again right behind the launches
    (void)hipGetLastError();
    uint64_t* out_count = (uint64_t*)sc.dev;
    void* workspace = (char*)sc.dev + 8;
    hipStream_t stream = (hipStream_t)stream_;
    uint64_t n_blocks = (N + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK;
        {
        uint32_t* block_counts = (uint32_t*)workspace;
        uint64_t* block_offsets = (uint64_t*)((char*)workspace + ((n_blocks * 4 + 7) & ~7ull));
        hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, stream, flags, N,
                           block_counts);
        hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, stream, block_counts,
                           (uint32_t)n_blocks, block_offsets, out_count, sc.host_count_dev);
        hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)n_blocks), dim3(SEL_THREADS), 0, stream, flags,
                           N, block_offsets, out_index);
        }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        {
        set_last_error(std::string("select kernel launch failed: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    e = hipStreamSynchronize(stream); // the kernels are through: the count is in the pinned word
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_select_rows: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    *out_count_host = __atomic_load_n(sc.host_count, __ATOMIC_ACQUIRE);
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" void* pgsd_device_alloc(int device, size_t bytes, const void* pattern, size_t pattern_bytes)
    try
    {
    if (!pgsd_device_available())
        {
        set_last_error("pgsd_device_alloc: no HIP device visible (the HIP path has no CPU fallback)");
        return nullptr;
        }
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (device >= 0 && device != prev && hipSetDevice(device) != hipSuccess)
        {
        set_last_error("pgsd_device_alloc: no device " + std::to_string(device));
        return nullptr;
        }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (e == hipSuccess && pattern && pattern_bytes > 0 && bytes > 0)
        {
        // the pattern repeated over a host image of at most 1 MiB (a multiple of the pattern), copied piecewise
        const size_t reps = std::max<size_t>(1, std::min<size_t>((1u << 20) / pattern_bytes, (bytes + pattern_bytes - 1) / pattern_bytes));
        std::vector<char> img(reps * pattern_bytes);
        for (size_t r = 0; r < reps; r++)
            memcpy(img.data() + r * pattern_bytes, pattern, pattern_bytes);
        for (size_t at = 0; at < bytes && e == hipSuccess; at += img.size())
            e = hipMemcpy((char*)p + at, img.data(), std::min(img.size(), bytes - at), hipMemcpyHostToDevice);
        }
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_device_alloc: ") + hipGetErrorString(e));
        if (p)
            (void)hipFree(p);
        p = nullptr;
        }
    if (device >= 0 && prev >= 0 && device != prev)
        (void)hipSetDevice(prev);
    return p;
    }
catch (...)
    {
        pgsd_amd::abi_guard();
        return nullptr;
    }

extern "C" int pgsd_device_free(int device, void* ptr)
    try
    {
    if (!ptr)
        return PGSD_SUCCESS;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (device >= 0 && device != prev)
        (void)hipSetDevice(device);
    const hipError_t e = hipFree(ptr);
    if (device >= 0 && prev >= 0 && device != prev)
        (void)hipSetDevice(prev);
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_device_free: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_device_copy(int device, void* dst, const void* src, size_t bytes)
    try
    {
    if (bytes == 0)
        return PGSD_SUCCESS;
    if (!dst || !src)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (device >= 0 && device != prev)
        (void)hipSetDevice(device);
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDefault); // either side may be host memory
    if (device >= 0 && prev >= 0 && device != prev)
        (void)hipSetDevice(prev);
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_device_copy: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }
