// pgsd_sph_adaptive.hip -- the SPH kernel sums with a per-particle smoothing length on gfx950: per entry i of a row list
// in cell order the candidates inside its own support (count), the three weighted pair sums of pgsd_sph.hip with the
// entry's own h_i (gather: the support 2 h_i) or the pair's mean (mean: the support h_i + h_j) and, in gather mode, the
// grad-h factor omega_i = 1 - a_o / (D a_m); over the list their ranges, the range of the count, the pairs, the entries
// whose h is not valid and the deviation from the stored density.  pgsd.hoomd.sph_adaptive_sums is the definition and this
// file equals it exactly, the floats bit for bit.  The grid is made for the declared bound 2 h_max, so THE ORDER of the
// candidates is pgsd_sph.hip's for the range 2 h_max; one pair is float64 without contraction.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp)
//   spha_compact_kernel<F64>   lane per entry: xs[k], ms[k], vs[k] as sph_compact_kernel and hs[k], the float64 h.  A
//                          valid h above the declared h_max raises both flag words (value 2): the call is refused.  An
//                          entry whose h is not valid gets a NaN position in xs: d2 < r2 is false for it as a candidate
//                          and as a centre, so the pair loop needs neither a load nor a branch for it
//   spha_pair_kernel<F64, KERNEL, MODE>   lane per entry i: x_i, h_i and the accumulators in registers, the candidates by
//                          traverse_candidates (pgsd_traverse.hpp).  gather: the lane's own r2_i is the traversal's r2, the
//                          body is the uniform pass's plus F and one accumulator.  mean: the traversal filters with
//                          (2 h_max)^2, the functor loads hs[j] and applies d2 < s*s.  The volume sum is a run-time `if` on
//                          a uniform value (eight instances, not sixteen).  Counters and pairs go through LDS counters and
//                          one 64-bit integer atomic per workgroup, the rest leaves as one partial per workgroup
//   spha_final_kernel      one workgroup: the partials in a fixed strided scan, then the words of the summary
//   spha_range_kernel, spha_range_final_kernel   (n, bad, h_min, h_max) of the staged slength chunk over a row list: a
//                          grid-stride reduction with one partial per workgroup, then one workgroup; it runs before any
//                          cell order exists, because the grid depends on its result
// No float atomic anywhere, no private (scratch) memory in any instance.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define SPHA_WAVES (SEL_THREADS / 64)
#define SPHA_RANGE_BLOCKS 1024u
// one workgroup's share of what is no count: per value (slength, number, density, shepard, omega) the smallest and the
// largest over its live entries (+inf / -inf: none, or NaNs only), the deviation of the largest magnitude with its list
// position, and the smallest count with its position and the largest count (SPH_NONE: it has no live entry)
struct SphaPartial
    {
    double lo[5], hi[5];
    double dev;
    uint32_t at, cmin, cmax, cmin_at;
    };

struct SphaRange
    {
    double lo, hi;
    unsigned long long bad;
    };

__device__ __forceinline__ bool spha_valid(double h)
    {
    return h > 0.0 && h < __builtin_huge_val();
    }

// does the deviation (d, i) replace (e, k): the larger magnitude, then the smaller position; an empty slot never does
__device__ __forceinline__ bool spha_dev_before(double d, uint32_t i, double e, uint32_t k)
    {
    if (i == SPH_NONE)
        return false;
    if (k == SPH_NONE)
        return true;
    const double ad = __builtin_fabs(d), ae = __builtin_fabs(e);
    return ad > ae || (ad == ae && i < k);
    }

__device__ __forceinline__ void spha_merge(SphaPartial& p, const SphaPartial& o)
    {
#pragma unroll
    for (int s = 0; s < 5; s++)
        {
        p.lo[s] = o.lo[s] < p.lo[s] ? o.lo[s] : p.lo[s];
        p.hi[s] = o.hi[s] > p.hi[s] ? o.hi[s] : p.hi[s];
        }
    if (spha_dev_before(o.dev, o.at, p.dev, p.at))
        {
        p.dev = o.dev;
        p.at = o.at;
        }
    // the smaller count, then the smaller position
    if (o.cmin_at != SPH_NONE && (p.cmin_at == SPH_NONE || o.cmin < p.cmin || (o.cmin == p.cmin && o.cmin_at < p.cmin_at)))
        {
        p.cmin = o.cmin;
        p.cmin_at = o.cmin_at;
        }
    p.cmax = o.cmax > p.cmax ? o.cmax : p.cmax;
    }

__device__ __forceinline__ SphaPartial spha_nothing()
    {
    SphaPartial p;
#pragma unroll
    for (int s = 0; s < 5; s++)
        {
        p.lo[s] = __builtin_huge_val();
        p.hi[s] = -__builtin_huge_val();
        }
    p.dev = 0.0;
    p.at = SPH_NONE;
    p.cmin = 0;
    p.cmax = 0;
    p.cmin_at = SPH_NONE;
    return p;
    }

// pgsd.hoomd.sph_sigma of one valid h, in that function's association
template<int KERNEL> __device__ __forceinline__ double spha_sigma(double h, bool three)
    {
#pragma clang fp contract(off)
    const double pi = 3.141592653589793;
    if (three)
        return KERNEL == SPH_WENDLAND_C2 ? 21.0 / (16.0 * pi * (h * h * h)) : 1.0 / (pi * (h * h * h));
    return KERNEL == SPH_WENDLAND_C2 ? 7.0 / (4.0 * pi * (h * h)) : 10.0 / (7.0 * pi * (h * h));
    }

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void spha_compact_kernel(const SphAdaptiveArgs a, uint32_t* flag_dev,
                                                                   uint32_t* flag_host, void* __restrict__ xs,
                                                                   double* __restrict__ ms, double* __restrict__ vs,
                                                                   double* __restrict__ hs)
    {
    typedef typename std::conditional<F64, double, float>::type elem_t;
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (*flag_dev != 0 || k >= a.n)
        return;
    const uint64_t row = a.rows[k];
    if (row >= a.N) // (the check kernel has refused such a list: nothing is loaded for it)
        return;
    const double h = a.slength ? column_value(a.slength, a.slength_f64, row) : a.h_default;
    const bool valid = spha_valid(h);
    if (valid && h > a.h_max)
        {
        // a listed smoothing length above the declared bound: the grid was not made for it
        *flag_dev = 2u;
        *flag_host = 2u;
        return;
        }
    hs[k] = h;
    if (valid)
        compact_position<F64>(a.pos, row, xs, k);
    else
        {
        elem_t* o = (elem_t*)xs + k * 3;
        o[0] = o[1] = o[2] = (elem_t)__builtin_nan("");
        }
    const double m = a.mass ? column_value(a.mass, a.mass_f64, row) : a.mass_default;
    ms[k] = m;
    if (a.volume)
        vs[k] = m / (a.density ? column_value(a.density, a.density_f64, row) : a.density_default);
    }

// words: the summary in device memory, zeroed by the launcher (words 2, 3, 4 and 21 -- bad_h, not_finite, surface and
// pairs -- are added to here)
template<bool F64, int KERNEL, int MODE>
__global__ __launch_bounds__(SEL_THREADS) void spha_pair_kernel(const SphAdaptiveArgs a, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                const double* __restrict__ ms, const double* __restrict__ vs,
                                                                const double* __restrict__ hs, uint32_t* __restrict__ out_count,
                                                                double* __restrict__ out_number, double* __restrict__ out_density,
                                                                double* __restrict__ out_shepard, double* __restrict__ out_omega,
                                                                unsigned long long* __restrict__ words,
                                                                SphaPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_bad, s_not_finite, s_surface;
    __shared__ unsigned long long s_pairs;
    __shared__ SphaPartial s_part[SPHA_WAVES];
    if (*flag_dev != 0)
        return;
    if (threadIdx.x == 0)
        {
        s_bad = 0;
        s_not_finite = 0;
        s_surface = 0;
        s_pairs = 0;
        }
    __syncthreads();
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    const double h_i = has ? hs[k] : 0.0;
    const bool ok = has && spha_valid(h_i);
    const bool vol = a.volume != 0; // (uniform: a scalar branch)
    const bool three = a.dims != 2;
    const double D = three ? 3.0 : 2.0;
    double a_n = 0.0, a_m = 0.0, a_v = 0.0, a_o = 0.0;
    uint32_t count = 0;
    if (ok)
        {
        TraverseGrid g = traverse_grid(a);
        if constexpr (MODE == SPHA_GATHER)
            {
            const double s_i = 2.0 * h_i;
            const double inv_i = 1.0 / h_i;
            g.r2 = s_i * s_i; // (h_i <= h_max: inside what the grid was made for)
            traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, g,
                                [&](uint32_t j, double, double, double, double d2)
                                {
#pragma clang fp contract(off)
                                    const double rr = __builtin_sqrt(d2);
                                    const double q = rr * inv_i;
                                    const double w = sph_weight<KERNEL>(q);
                                    const double F = sphg_factor<KERNEL>(q);
                                    const double mj = ms[j];
                                    a_n = a_n + w;
                                    a_m = a_m + mj * w;
                                    if (vol)
                                        a_v = a_v + vs[j] * w;
                                    a_o = a_o + mj * (D * w + (q * q) * F);
                                    count++;
                                });
            }
        else
            {
            traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, g,
                                [&](uint32_t j, double, double, double, double d2)
                                {
#pragma clang fp contract(off)
                                    const double s = h_i + hs[j];
                                    if (d2 < s * s)
                                        {
                                        const double hij = 0.5 * s;
                                        const double ih = 1.0 / hij;
                                        const double q = __builtin_sqrt(d2) * ih;
                                        const double w = sph_weight<KERNEL>(q);
                                        const double p = three ? (ih * ih) * ih : ih * ih;
                                        const double wp = w * p;
                                        const double mj = ms[j];
                                        a_n = a_n + wp;
                                        a_m = a_m + mj * wp;
                                        if (vol)
                                            a_v = a_v + vs[j] * wp;
                                        count++;
                                        }
                                });
            }
        }
    // (an entry without a cell or with an h that is not valid: every value is +0.0, written, not computed)
    double number = 0.0, density = 0.0, shepard = 0.0, omega = 0.0;
    if (ok)
        {
        const double scale = MODE == SPHA_GATHER ? spha_sigma<KERNEL>(h_i, three) : a.sigma;
        number = scale * a_n;
        density = scale * a_m;
        shepard = scale * a_v;
        if constexpr (MODE == SPHA_GATHER)
            omega = 1.0 - a_o / (D * a_m);
        }
    if (live)
        {
        if (out_count)
            out_count[k] = count;
        if (out_number)
            out_number[k] = number;
        if (out_density)
            out_density[k] = density;
        if (vol && out_shepard)
            out_shepard[k] = shepard;
        if (MODE == SPHA_GATHER && out_omega)
            out_omega[k] = omega;
        }
    SphaPartial p = spha_nothing();
    if (has && !ok)
        atomicAdd(&s_bad, 1u);
    if (ok)
        {
        // (a NaN passes no compare: it replaces neither bound)
        p.lo[0] = h_i;
        p.hi[0] = h_i;
        p.lo[1] = number < p.lo[1] ? number : p.lo[1];
        p.hi[1] = number > p.hi[1] ? number : p.hi[1];
        p.lo[2] = density < p.lo[2] ? density : p.lo[2];
        p.hi[2] = density > p.hi[2] ? density : p.hi[2];
        if constexpr (MODE == SPHA_GATHER)
            {
            p.lo[4] = omega < p.lo[4] ? omega : p.lo[4];
            p.hi[4] = omega > p.hi[4] ? omega : p.hi[4];
            }
        p.cmin = p.cmax = count;
        p.cmin_at = k;
        if (count)
            atomicAdd(&s_pairs, (unsigned long long)count);
        if (!(__builtin_fabs(density) < __builtin_huge_val()))
            atomicAdd(&s_not_finite, 1u);
        if (vol)
            {
            p.lo[3] = shepard < p.lo[3] ? shepard : p.lo[3];
            p.hi[3] = shepard > p.hi[3] ? shepard : p.hi[3];
            if (a.surface && shepard < a.surface_below)
                atomicAdd(&s_surface, 1u);
            const uint64_t row = a.rows[k];
            const double rho = a.density ? column_value(a.density, a.density_f64, row < a.N ? row : 0) : a.density_default;
            const double dev = density - rho;
            if (dev == dev)
                {
                p.dev = dev;
                p.at = k;
                }
            }
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        SphaPartial o;
#pragma unroll
        for (int s = 0; s < 5; s++)
            {
            o.lo[s] = __shfl_xor(p.lo[s], h, 64);
            o.hi[s] = __shfl_xor(p.hi[s], h, 64);
            }
        o.dev = __shfl_xor(p.dev, h, 64);
        o.at = __shfl_xor(p.at, h, 64);
        o.cmin = __shfl_xor(p.cmin, h, 64);
        o.cmax = __shfl_xor(p.cmax, h, 64);
        o.cmin_at = __shfl_xor(p.cmin_at, h, 64);
        spha_merge(p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SphaPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < SPHA_WAVES; w++)
            spha_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        if (s_bad)
            atomicAdd(&words[2], (unsigned long long)s_bad);
        if (s_not_finite)
            atomicAdd(&words[3], (unsigned long long)s_not_finite);
        if (s_surface)
            atomicAdd(&words[4], (unsigned long long)s_surface);
        if (s_pairs)
            atomicAdd(&words[21], s_pairs);
        }
    }

// One workgroup.  The words: SPHA_SUMMARY_WORDS of pgsd_internal.hpp.
__global__ __launch_bounds__(SEL_THREADS) void spha_final_kernel(const SphAdaptiveArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const SphaPartial* __restrict__ part,
                                                                 uint32_t n_parts, unsigned long long* __restrict__ words)
    {
    __shared__ SphaPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SphaPartial p = spha_nothing();
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        spha_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        spha_merge(p, s_part[t]);
    const uint64_t n = a.n;
    const uint64_t somewhere = min((uint64_t)offs[a.n_cells], n);
    const bool any = p.at != SPH_NONE && p.at < n;
    const bool some = p.cmin_at != SPH_NONE && p.cmin_at < n;
    words[0] = n;
    words[1] = n - somewhere;
    words[5] = any ? p.at : SPH_NONE;
    words[6] = any ? a.rows[p.at] : SPH_NONE;
    words[7] = some ? p.cmin : 0;
    words[8] = some ? p.cmax : 0;
    words[9] = some ? p.cmin_at : SPH_NONE;
#pragma unroll
    for (int s = 0; s < 5; s++)
        {
        words[10 + 2 * s] = (unsigned long long)__double_as_longlong(p.lo[s]);
        words[11 + 2 * s] = (unsigned long long)__double_as_longlong(p.hi[s]);
        }
    words[20] = (unsigned long long)__double_as_longlong(any ? p.dev : 0.0);
    }

__device__ __forceinline__ void spha_range_merge(SphaRange& p, const SphaRange& o)
    {
    p.lo = o.lo < p.lo ? o.lo : p.lo;
    p.hi = o.hi > p.hi ? o.hi : p.hi;
    p.bad += o.bad;
    }

// grid-stride over the list (rows: null: every row of the chunk, n == N); one partial per workgroup.  An entry >= N
// raises both flag words.
__global__ __launch_bounds__(SEL_THREADS) void spha_range_kernel(const void* __restrict__ slength, uint32_t f64,
                                                                 const uint32_t* __restrict__ rows, uint64_t n, uint64_t N,
                                                                 uint32_t* flag_dev, uint32_t* flag_host,
                                                                 SphaRange* __restrict__ part)
    {
    __shared__ SphaRange s_part[SPHA_WAVES];
    if (*flag_dev != 0)
        return;
    SphaRange p = {__builtin_huge_val(), -__builtin_huge_val(), 0ull};
    for (uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * SEL_THREADS)
        {
        const uint64_t row = rows ? rows[k] : k;
        if (row >= N)
            {
            *flag_dev = 1u;
            *flag_host = 1u;
            continue;
            }
        const double h = column_value(slength, f64, row);
        if (spha_valid(h))
            {
            p.lo = h < p.lo ? h : p.lo;
            p.hi = h > p.hi ? h : p.hi;
            }
        else
            p.bad++;
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        SphaRange o;
        o.lo = __shfl_xor(p.lo, h, 64);
        o.hi = __shfl_xor(p.hi, h, 64);
        o.bad = __shfl_xor(p.bad, h, 64);
        spha_range_merge(p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SphaRange q = s_part[0];
#pragma unroll
        for (int w = 1; w < SPHA_WAVES; w++)
            spha_range_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        }
    }

// one workgroup: the partials in a fixed strided scan; words: n, bad, h_min, h_max (bit patterns)
__global__ __launch_bounds__(SEL_THREADS) void spha_range_final_kernel(const uint32_t* flag_dev, const SphaRange* __restrict__ part,
                                                                       uint32_t n_parts, uint64_t n,
                                                                       unsigned long long* __restrict__ words)
    {
    __shared__ SphaRange s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SphaRange p = {__builtin_huge_val(), -__builtin_huge_val(), 0ull};
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        spha_range_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        spha_range_merge(p, s_part[t]);
    words[0] = n;
    words[1] = p.bad;
    words[2] = (unsigned long long)__double_as_longlong(p.lo);
    words[3] = (unsigned long long)__double_as_longlong(p.hi);
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The unit's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the offsets
// (n_cells + 2 words), the compacted positions (n x 3 elements), masses, volumes and smoothing lengths (n doubles each),
// the partials (one per workgroup) and the summary; the range call takes the flag word, its partials and four words.  The
// pinned flag word is the host's view of a refused list, the pinned host block the landing place of the summary.
constexpr size_t SPHA_SUMMARY_BYTES = (size_t)SPHA_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_spha_scratch("adaptive SPH sums", 1.25, 1u << 16, SPHA_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_spha_lock;

template<bool F64, int KERNEL>
void spha_launch_pair(uint32_t mode, dim3 grid, dim3 block, hipStream_t stream, const SphAdaptiveArgs& a, const uint32_t* offs,
                      const uint32_t* flag_dev, const void* xs, const double* ms, const double* vs, const double* hs,
                      uint32_t* out_count, double* out_number, double* out_density, double* out_shepard, double* out_omega,
                      unsigned long long* words, SphaPartial* part)
    {
    if (mode == SPHA_GATHER)
        hipLaunchKernelGGL((spha_pair_kernel<F64, KERNEL, SPHA_GATHER>), grid, block, 0, stream, a, offs, flag_dev, xs, ms, vs, hs,
                           out_count, out_number, out_density, out_shepard, out_omega, words, part);
    else
        hipLaunchKernelGGL((spha_pair_kernel<F64, KERNEL, SPHA_MEAN>), grid, block, 0, stream, a, offs, flag_dev, xs, ms, vs, hs,
                           out_count, out_number, out_density, out_shepard, out_omega, words, part);
    }
    } // namespace

void warm_sph_adaptive_kernels()
    {
    warm_kernel((const void*)spha_pair_kernel<false, SPH_WENDLAND_C2, SPHA_GATHER>);
    }

int launch_sph_smoothing_range(const void* slength, uint32_t f64, const uint32_t* rows, uint64_t n, uint64_t N,
                               uint64_t* out_words, hipStream_t stream, std::string* err)
    {
    static const char* what = "smoothing range";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_words || !slength)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (n >= (1ull << 32))
        return fail("a list holds fewer than 2^32 entries");
    if (N >= (1ull << 32))
        return fail("chunks of 2^32 rows or more have no 32-bit row list");
    if (n == 0)
        {
        sph_range_of_nothing(out_words);
        return PGSD_SUCCESS;
        }
    const uint32_t n_blocks = (uint32_t)std::min<uint64_t>((n + SEL_THREADS - 1) / SEL_THREADS, SPHA_RANGE_BLOCKS);
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(SphaRange));
    const size_t words_bytes = 4 * sizeof(uint64_t);
    LaunchScope scope(g_spha_lock, g_spha_scratch, 16 + part_bytes + words_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    SphaRange* part = (SphaRange*)(dev + 16);
    unsigned long long* words = (unsigned long long*)(dev + 16 + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    __atomic_store_n(host_flag, 0u, __ATOMIC_RELEASE);
    hipError_t e = hipMemsetAsync(flag_dev, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess)
        {
        const dim3 block(SEL_THREADS);
        hipLaunchKernelGGL(spha_range_kernel, dim3(n_blocks), block, 0, stream, slength, f64, rows, n, N, flag_dev,
                           (uint32_t*)scope.mem().mapped_dev, part);
        hipLaunchKernelGGL(spha_range_final_kernel, dim3(1), block, 0, stream, flag_dev, part, n_blocks, n, words);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, words, words_bytes, hipMemcpyDeviceToHost, stream);
    const int rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (__atomic_load_n(host_flag, __ATOMIC_ACQUIRE) != 0)
        return fail("an entry of the row list lies outside the chunk (nothing was computed)");
    const uint64_t* landed = (const uint64_t*)scope.mem().host;
    std::copy(landed, landed + 4, out_words);
    return PGSD_SUCCESS;
    }

int launch_sph_adaptive_sums(const SphAdaptiveArgs& a, uint32_t* out_count, double* out_number, double* out_density,
                             double* out_shepard, double* out_omega, uint64_t* out_summary, hipStream_t stream,
                             std::string* err)
    {
    static const char* what = "adaptive SPH sums";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.kernel != SPH_WENDLAND_C2 && a.kernel != SPH_CUBIC_SPLINE)
        return fail("the kernel is 0 (Wendland C2) or 1 (cubic spline)");
    if (a.mode != SPHA_GATHER && a.mode != SPHA_MEAN)
        return fail("the mode is 0 (gather) or 1 (mean)");
    if (!(a.h_max > 0.0 && a.h_max < HUGE_VAL))
        return fail("h_max must be finite and positive");
    const uint64_t n = a.n;
    if (n == 0)
        {
        sph_adaptive_sums_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return fail(cells_refused);
    if (!a.rows || !a.cell || !a.pos)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t n_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    const size_t xs_bytes = round16((size_t)n * 3 * (a.f64 ? sizeof(double) : sizeof(float)));
    const size_t col_bytes = round16((size_t)n * sizeof(double));
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(SphaPartial));
    const size_t words_bytes = SPHA_SUMMARY_BYTES;
    LaunchScope scope(g_spha_lock, g_spha_scratch, 16 + offs_bytes + xs_bytes + 3 * col_bytes + part_bytes + words_bytes, stream,
                      err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    double* ms = (double*)((char*)xs + xs_bytes);
    double* vs = (double*)((char*)ms + col_bytes);
    double* hs = (double*)((char*)vs + col_bytes);
    SphaPartial* part = (SphaPartial*)((char*)hs + col_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    uint32_t* host_flag_dev = (uint32_t*)scope.mem().mapped_dev;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, host_flag_dev, offs, words, words_bytes,
                                   stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(spha_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, host_flag_dev, xs, ms, vs, hs);
            if (a.kernel == SPH_WENDLAND_C2)
                spha_launch_pair<true, SPH_WENDLAND_C2>(a.mode, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, hs, out_count,
                                                        out_number, out_density, out_shepard, out_omega, words, part);
            else
                spha_launch_pair<true, SPH_CUBIC_SPLINE>(a.mode, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, hs,
                                                         out_count, out_number, out_density, out_shepard, out_omega, words, part);
            }
        else
            {
            hipLaunchKernelGGL(spha_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, host_flag_dev, xs, ms, vs, hs);
            if (a.kernel == SPH_WENDLAND_C2)
                spha_launch_pair<false, SPH_WENDLAND_C2>(a.mode, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, hs,
                                                         out_count, out_number, out_density, out_shepard, out_omega, words, part);
            else
                spha_launch_pair<false, SPH_CUBIC_SPLINE>(a.mode, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, hs,
                                                          out_count, out_number, out_density, out_shepard, out_omega, words, part);
            }
        hipLaunchKernelGGL(spha_final_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, part, n_blocks, words);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, words, words_bytes, hipMemcpyDeviceToHost, stream);
    rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    const uint32_t flag = __atomic_load_n(host_flag, __ATOMIC_ACQUIRE);
    if (flag == 2u)
        return fail("a listed smoothing length exceeds h_max (nothing was computed)");
    if (flag != 0)
        return fail(cells_refused);
    const uint64_t* landed = (const uint64_t*)scope.mem().host;
    std::copy(landed, landed + SPHA_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
