// pgsd_sph_samples.hip -- the SPH samples on gfx950: the SPH interpolant of a row list in cell order at points of the
// caller's choosing -- per point p the entries j of the periodically adjacent cells of the point's cell that lie strictly
// inside the kernel support 2h of it, the density sigma * sum_j m_j W_pj, the Shepard sum sigma * sum_j V_j W_pj and per
// value column c sigma * sum_j V_j W_pj f_j[c] (normalised: sum_j V_j W_pj f_j[c] / sum_j V_j W_pj) -- and over the points
// how many are nowhere, outside the box, empty or not finite, the largest count with its point and the ranges of the two
// sums.  The first pass here whose centre is no entry of the list.
// pgsd.hoomd.sph_samples is the definition and this file equals it exactly, the floats bit for bit: the grid, the
// support, the list and the ORDER of the candidates are the SPH kernel sums' (pgsd_sph.hip, pgsd_traverse.hpp) around the
// point's cell, which is the cell order's key (pgsd_order.hip: domain_skew, domain_wrap, the NaN test before the integer
// conversion); d2, rr = sqrt(d2), q = rr * inv_h and w = sph_weight(q) are the sums'; then a_m += m_j * w, vw = V_j * w,
// a_v += vw, a_f[c] += vw * f_j[c] with the stored V_k = m_k / rho_k -- float64 without contraction.  r2, inv_h and sigma
// come from the host; after the last candidate density = sigma * a_m, shepard = sigma * a_v, values[c] = sigma * a_f[c] or
// a_f[c] / a_v.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          CSR offsets; every kernel here reads the device flag first and does nothing where it is set
//   samp_compact_kernel<F64>   lane per entry: xs[k] = position[rows[k]] in the chunk's own element type, m[k], V[k] = m /
//                          rho and the value table n x CP as float64 (exact conversions; the default of a chunk stored
//                          nowhere broadcast; the columns behind C are +0.0)
//   samp_point_kernel<F64, KERNEL, CP>   lane per point: its cell and whether it lies outside the box from the same
//                          fraction s, the count and the 2 + CP accumulators in registers (CP is a template parameter: an
//                          accumulator array indexed at run time would be private memory), the candidates by
//                          traverse_candidates_around (pgsd_traverse.hpp) in the defined order.  The four counters go
//                          through LDS and 64-bit integer atomics, one per counter and workgroup; the ranges and the
//                          largest count leave as one partial per workgroup
//   samp_final_kernel      one workgroup: the partials in a fixed strided scan, then the words of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp, pgsd_select.hpp, pgsd_traverse.hpp; the launcher's host side: pgsd_scratch.hpp and pgsd_cells.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_select.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define SAMP_WAVES (SEL_THREADS / 64)
// one workgroup's share of what is no counter: the smallest and largest shepard (0) and density (1) over its points that
// have a cell (+inf / -inf: it has none, or NaNs only) and the largest count with its point (SPH_NONE: it has none)
struct SampPartial
    {
    double lo[2], hi[2];
    uint32_t count, at;
    };

__device__ __forceinline__ void samp_merge(SampPartial& p, const SampPartial& o)
    {
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        p.lo[s] = o.lo[s] < p.lo[s] ? o.lo[s] : p.lo[s];
        p.hi[s] = o.hi[s] > p.hi[s] ? o.hi[s] : p.hi[s];
        }
    // the larger count, then the smaller point; an empty slot never replaces anything
    if (o.at != SPH_NONE && (p.at == SPH_NONE || o.count > p.count || (o.count == p.count && o.at < p.at)))
        {
        p.count = o.count;
        p.at = o.at;
        }
    }

__device__ __forceinline__ SampPartial samp_nothing()
    {
    SampPartial p;
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        p.lo[s] = __builtin_huge_val();
        p.hi[s] = -__builtin_huge_val();
        }
    p.count = 0;
    p.at = SPH_NONE;
    return p;
    }

// vals: n x CP, row k the C value columns of entry k in the order of the slots, then +0.0
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void samp_compact_kernel(const SphSamplesArgs a, const uint32_t* flag_dev,
                                                                   void* __restrict__ xs, double* __restrict__ ms,
                                                                   double* __restrict__ vs, double* __restrict__ vals,
                                                                   uint32_t CP)
    {
#pragma clang fp contract(off)
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= a.n || *flag_dev != 0)
        return;
    const uint64_t row = a.rows[k];
    if (row >= a.N) // (the check kernel has refused such a list: nothing is loaded for it)
        return;
    compact_position<F64>(a.pos, row, xs, k);
    const double m = a.mass ? column_value(a.mass, a.mass_f64, row) : a.mass_default;
    const double rho = a.density ? column_value(a.density, a.density_f64, row) : a.density_default;
    ms[k] = m;
    vs[k] = m / rho;
    double* out = vals + (size_t)k * CP;
    uint32_t col = 0;
#pragma unroll
    for (int s = 0; s < SPHS_MAX_VALUES; s++)
        {
        const uint32_t width = a.value_columns[s];
        const void* base = a.value[s];
        const uint32_t f64 = a.value_f64[s];
        const double fill = a.value_default[s];
        for (uint32_t c = 0; c < width && col < CP; c++, col++)
            out[col] = base ? column_value(base, f64, row * width + c) : fill;
        }
    for (; col < CP; col++)
        out[col] = 0.0;
    }

// words: the summary in device memory, zeroed by the launcher (words 1 .. 4 -- nowhere, outside, empty, not_finite -- are
// added to here)
template<bool F64, int KERNEL, int CP>
__global__ __launch_bounds__(SEL_THREADS) void samp_point_kernel(const SphSamplesArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                 const double* __restrict__ ms, const double* __restrict__ vs,
                                                                 const double* __restrict__ vals, uint32_t* __restrict__ out_count,
                                                                 double* __restrict__ out_density, double* __restrict__ out_shepard,
                                                                 double* __restrict__ out_values,
                                                                 unsigned long long* __restrict__ words,
                                                                 SampPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_counts[4]; // nowhere, outside, empty, not_finite
    __shared__ SampPartial s_part[SAMP_WAVES];
    if (*flag_dev != 0)
        return;
    if (threadIdx.x < 4)
        s_counts[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t p64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t p = (uint32_t)p64; // (K < 2^32)
    const bool live = p64 < a.K;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    uint32_t cell = 0;
    bool somewhere = live, outside = false;
    if (live)
        {
        x0 = a.points[(size_t)p * 3 + 0];
        x1 = a.points[(size_t)p * 3 + 1];
        x2 = a.points[(size_t)p * 3 + 2];
        // the key kernel's cell (pgsd_order.hip); outside: the same fraction before its wrap
        double s[3];
        domain_skew(a.d, x0, x1, x2, s);
        uint32_t stride = 1;
#pragma unroll
        for (int ax = 0; ax < 3; ax++)
            {
            if (ax == 2 && a.d.dims == 2)
                break;
            const double f = domain_wrap(s[ax]);
            uint32_t at = 0;
            if (f == f)
                at = min((uint32_t)(f * (double)a.cells[ax]), a.cells[ax] - 1u);
            else
                somewhere = false;
            outside = outside || s[ax] < 0.0 || s[ax] >= 1.0;
            cell += at * stride;
            stride *= a.cells[ax];
            }
        }
    const bool has = live && somewhere;
    constexpr int W = CP > 0 ? CP : 1;
    double a_m = 0.0, a_v = 0.0;
    double a_f[W];
#pragma unroll
    for (int c = 0; c < W; c++)
        a_f[c] = 0.0;
    uint32_t count = 0;
    if (has)
        {
        const double inv_h = a.inv_h;
        traverse_candidates_around((const elem_t*)xs, offs, a.n, x0, x1, x2, cell, traverse_grid(a),
                                   [&](uint32_t j, double, double, double, double d2)
                                   {
#pragma clang fp contract(off)
                                       const double rr = __builtin_sqrt(d2);
                                       const double q = rr * inv_h;
                                       const double w = sph_weight<KERNEL>(q);
                                       count = count + 1u;
                                       a_m = a_m + ms[j] * w;
                                       const double vw = vs[j] * w;
                                       a_v = a_v + vw;
                                       if constexpr (CP > 0)
                                           {
                                           const double* __restrict__ f = vals + (size_t)j * CP;
#pragma unroll
                                           for (int c = 0; c < CP; c++)
                                               a_f[c] = a_f[c] + vw * f[c];
                                           }
                                   });
        }
    // (a point without a cell: every value is +0.0, whatever `normalise` says)
    const double density = has ? a.sigma * a_m : 0.0, shepard = has ? a.sigma * a_v : 0.0;
    const uint32_t C = a.C;
    bool finite = __builtin_fabs(density) < __builtin_huge_val() && __builtin_fabs(shepard) < __builtin_huge_val();
    if constexpr (CP > 0)
        {
#pragma unroll
        for (int c = 0; c < CP; c++)
            {
            const double v = has ? (a.normalise ? a_f[c] / a_v : a.sigma * a_f[c]) : 0.0;
            if ((uint32_t)c < C)
                {
                finite = finite && __builtin_fabs(v) < __builtin_huge_val();
                if (live && out_values)
                    out_values[(size_t)p * C + c] = v;
                }
            }
        }
    if (live)
        {
        if (out_count)
            out_count[p] = count;
        if (out_density)
            out_density[p] = density;
        if (out_shepard)
            out_shepard[p] = shepard;
        if (!somewhere)
            atomicAdd(&s_counts[0], 1u);
        }
    SampPartial part_p = samp_nothing();
    if (has)
        {
        if (outside)
            atomicAdd(&s_counts[1], 1u);
        if (count == 0)
            atomicAdd(&s_counts[2], 1u);
        if (!finite)
            atomicAdd(&s_counts[3], 1u);
        // (a NaN passes no compare: it replaces neither bound)
        part_p.lo[0] = shepard < part_p.lo[0] ? shepard : part_p.lo[0];
        part_p.hi[0] = shepard > part_p.hi[0] ? shepard : part_p.hi[0];
        part_p.lo[1] = density < part_p.lo[1] ? density : part_p.lo[1];
        part_p.hi[1] = density > part_p.hi[1] ? density : part_p.hi[1];
        part_p.count = count;
        part_p.at = p;
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        SampPartial o;
#pragma unroll
        for (int s = 0; s < 2; s++)
            {
            o.lo[s] = __shfl_xor(part_p.lo[s], h, 64);
            o.hi[s] = __shfl_xor(part_p.hi[s], h, 64);
            }
        o.count = __shfl_xor(part_p.count, h, 64);
        o.at = __shfl_xor(part_p.at, h, 64);
        samp_merge(part_p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = part_p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SampPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < SAMP_WAVES; w++)
            samp_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        }
    if (threadIdx.x < 4 && s_counts[threadIdx.x])
        atomicAdd(&words[1 + threadIdx.x], (unsigned long long)s_counts[threadIdx.x]);
    }

// One workgroup.  The words: K, nowhere, outside, empty, not_finite (added by the point kernel), the largest count and its
// point, then as bit patterns the minimum and maximum of shepard and of density.
__global__ __launch_bounds__(SEL_THREADS) void samp_final_kernel(const SphSamplesArgs a, const uint32_t* flag_dev,
                                                                 const SampPartial* __restrict__ part, uint32_t n_parts,
                                                                 unsigned long long* __restrict__ words)
    {
    __shared__ SampPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SampPartial p = samp_nothing();
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        samp_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        samp_merge(p, s_part[t]);
    const bool any = p.at != SPH_NONE && p.at < a.K;
    words[0] = a.K;
    words[5] = any ? p.count : 0u;
    words[6] = any ? p.at : SPH_NONE;
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        words[7 + 2 * s] = (unsigned long long)__double_as_longlong(p.lo[s]);
        words[8 + 2 * s] = (unsigned long long)__double_as_longlong(p.hi[s]);
        }
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), masses and volumes (n doubles each), the value
// table (n x CP doubles), the partials (one per workgroup of points) and the summary; the pinned flag word is the host's
// view of a refused list, the pinned host block the landing place of the summary.
constexpr size_t SAMP_SUMMARY_BYTES = (size_t)SPHS_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_samp_scratch("SPH samples", 1.25, 1u << 16, SAMP_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_samp_lock;

struct SampBuffers
    {
    const uint32_t* offs;
    const uint32_t* flag_dev;
    const void* xs;
    const double *ms, *vs, *vals;
    uint32_t* out_count;
    double *out_density, *out_shepard, *out_values;
    unsigned long long* words;
    SampPartial* part;
    };

// the instantiated width that holds C columns
uint32_t samp_padded(uint32_t C)
    {
    return C == 0 ? 0u : (C == 1 ? 1u : (C <= 4 ? 4u : 8u));
    }

template<bool F64, int KERNEL, int CP>
void samp_launch_one(dim3 grid, dim3 block, hipStream_t stream, const SphSamplesArgs& a, const SampBuffers& b)
    {
    hipLaunchKernelGGL((samp_point_kernel<F64, KERNEL, CP>), grid, block, 0, stream, a, b.offs, b.flag_dev, b.xs, b.ms, b.vs, b.vals,
                       b.out_count, b.out_density, b.out_shepard, b.out_values, b.words, b.part);
    }

template<bool F64, int KERNEL>
void samp_launch_point(uint32_t CP, dim3 grid, dim3 block, hipStream_t stream, const SphSamplesArgs& a, const SampBuffers& b)
    {
    switch (CP)
        {
        case 0: samp_launch_one<F64, KERNEL, 0>(grid, block, stream, a, b); break;
        case 1: samp_launch_one<F64, KERNEL, 1>(grid, block, stream, a, b); break;
        case 4: samp_launch_one<F64, KERNEL, 4>(grid, block, stream, a, b); break;
        default: samp_launch_one<F64, KERNEL, 8>(grid, block, stream, a, b); break;
        }
    }
    } // namespace

void warm_sph_samples_kernels()
    {
    warm_kernel((const void*)samp_point_kernel<false, SPH_WENDLAND_C2, 4>);
    }

int launch_sph_samples(const SphSamplesArgs& a, uint32_t* out_count, double* out_density, double* out_shepard,
                       double* out_values, uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "SPH samples";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.kernel != SPH_WENDLAND_C2 && a.kernel != SPH_CUBIC_SPLINE)
        return fail("the kernel is 0 (Wendland C2) or 1 (cubic spline)");
    if (a.K >= (1ull << 32))
        return fail("a call takes fewer than 2^32 points");
    uint32_t C = 0;
    for (int s = 0; s < SPHS_MAX_VALUES; s++)
        {
        if (a.value_columns[s] > SPHS_MAX_WIDTH)
            return fail("a value chunk has 1 to 4 columns");
        C += a.value_columns[s];
        }
    if (C > SPHS_MAX_COLUMNS || C != a.C)
        return fail("the value chunks have at most 8 columns together");
    const uint64_t n = a.n, K = a.K;
    if (K == 0)
        {
        sph_samples_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    if (n > 0 && a.N == 0)
        return fail(cells_refused);
    if (!a.points || (n > 0 && (!a.rows || !a.cell || !a.pos)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t CP = samp_padded(C);
    const uint32_t n_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const uint32_t p_blocks = (uint32_t)((K + SEL_THREADS - 1) / SEL_THREADS);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    const size_t xs_bytes = round16((size_t)n * 3 * (a.f64 ? sizeof(double) : sizeof(float)));
    const size_t col_bytes = round16((size_t)n * sizeof(double));
    const size_t vals_bytes = round16((size_t)n * CP * sizeof(double));
    const size_t part_bytes = round16((size_t)p_blocks * sizeof(SampPartial));
    const size_t words_bytes = SAMP_SUMMARY_BYTES;
    LaunchScope scope(g_samp_lock, g_samp_scratch, 16 + offs_bytes + xs_bytes + 2 * col_bytes + vals_bytes + part_bytes + words_bytes,
                      stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    double* ms = (double*)((char*)xs + xs_bytes);
    double* vs = (double*)((char*)ms + col_bytes);
    double* vals = (double*)((char*)vs + col_bytes);
    SampPartial* part = (SampPartial*)((char*)vals + vals_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks), per_point(p_blocks);
    const SampBuffers b = {offs, flag_dev, xs, ms, vs, vals, out_count, out_density, out_shepard, out_values, words, part};
    hipError_t e;
    if (n > 0)
        e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs, words,
                            words_bytes, stream);
    else
        {
        // a list of no entry: nothing to check, every offset is 0 and every point that has a cell is empty
        __atomic_store_n(host_flag, 0u, __ATOMIC_RELEASE);
        e = hipMemsetAsync(flag_dev, 0, 16 + offs_bytes, stream);
        if (e == hipSuccess)
            e = hipMemsetAsync(words, 0, words_bytes, stream);
        }
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            if (n > 0)
                hipLaunchKernelGGL(samp_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs, ms, vs, vals, CP);
            if (a.kernel == SPH_WENDLAND_C2)
                samp_launch_point<true, SPH_WENDLAND_C2>(CP, per_point, block, stream, a, b);
            else
                samp_launch_point<true, SPH_CUBIC_SPLINE>(CP, per_point, block, stream, a, b);
            }
        else
            {
            if (n > 0)
                hipLaunchKernelGGL(samp_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs, ms, vs, vals, CP);
            if (a.kernel == SPH_WENDLAND_C2)
                samp_launch_point<false, SPH_WENDLAND_C2>(CP, per_point, block, stream, a, b);
            else
                samp_launch_point<false, SPH_CUBIC_SPLINE>(CP, per_point, block, stream, a, b);
            }
        hipLaunchKernelGGL(samp_final_kernel, dim3(1), block, 0, stream, a, flag_dev, part, p_blocks, words);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, words, words_bytes, hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return fail(cells_refused);
    const uint64_t* landed = (const uint64_t*)scope.mem().host;
    std::copy(landed, landed + SPHS_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
