// pgsd_sph.hip -- the SPH kernel sums on gfx950: per entry i of a row list in cell order the three weighted pair sums
// sigma * sum_j W_ij, sigma * sum_j m_j W_ij and sigma * sum_j (m_j / rho_j) W_ij over the entries j of the periodically
// adjacent cells that lie strictly inside the kernel support 2h (i itself among them), and over the list their ranges,
// the largest deviation of the summation density from the stored one and the entries below a Shepard threshold.
// pgsd.hoomd.sph_kernel_sums is the definition and this file equals it exactly, the floats bit for bit: a float sum
// depends on its order, so the ORDER of the candidates is part of the definition -- oz over the offsets of the z axis
// ({0} at one cell, {0, +1} at two, {-1, 0, +1} otherwise), inside it oy, inside it ox, the cell ((ix+ox) % cx, (iy+oy) %
// cy, (iz+oz) % cz), inside a cell ascending list position -- and every lane adds in that order.  The arithmetic of one
// pair is the census kernel's d2 (pgsd.hoomd.pair_distance2), then rr = sqrt(d2), q = rr * inv_h and the polynomial of
// pgsd.hoomd.sph_weight, float64 without contraction; r2 = (2h)*(2h), inv_h = 1/h and sigma come from the host.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          CSR offsets; every kernel here reads the device flag first and does nothing where it is set,
//                          and clamps what it takes from the offsets to n
//   sph_compact_kernel<F64>   lane per entry: xs[k] = position[rows[k]] in the chunk's own element type, m[k] the mass
//                          and V[k] = m / rho (one float64 division of the stored values) as float64, so that the pair
//                          loop reads runs instead of gathering
//   sph_pair_kernel<F64, KERNEL, VOL>   lane per entry i: x_i and the three accumulators in registers, the candidates
//                          by traverse_candidates (pgsd_traverse.hpp) in the defined order, weighed by its sph_weight:
//                          the cells, the x-runs, the fold and the strict compare are written there, once for the pair
//                          units.  The counters
//                          (not_finite, surface) go through LDS counters and 64-bit integer atomics; the minima, maxima
//                          and the deviation leave as one partial per workgroup
//   sph_final_kernel       one workgroup: the partials in a fixed strided scan, then the words of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp; the launcher's host side: pgsd_scratch.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define SPH_WAVES (SEL_THREADS / 64)
// one workgroup's share of what is no count: per sum the smallest and largest value over its entries that have a cell
// (+inf / -inf: it has none, or NaNs only) and the deviation of the largest magnitude with its list position (SPH_NONE:
// it has none)
struct SphPartial
    {
    double lo[3], hi[3];
    double dev;
    uint32_t at, pad;
    };

// does the deviation (d, i) replace (e, k): the larger magnitude, then the smaller position; an empty slot never does
__device__ __forceinline__ bool sph_dev_before(double d, uint32_t i, double e, uint32_t k)
    {
    if (i == SPH_NONE)
        return false;
    if (k == SPH_NONE)
        return true;
    const double ad = __builtin_fabs(d), ae = __builtin_fabs(e);
    return ad > ae || (ad == ae && i < k);
    }

__device__ __forceinline__ void sph_merge(SphPartial& p, const SphPartial& o)
    {
#pragma unroll
    for (int s = 0; s < 3; s++)
        {
        p.lo[s] = o.lo[s] < p.lo[s] ? o.lo[s] : p.lo[s];
        p.hi[s] = o.hi[s] > p.hi[s] ? o.hi[s] : p.hi[s];
        }
    if (sph_dev_before(o.dev, o.at, p.dev, p.at))
        {
        p.dev = o.dev;
        p.at = o.at;
        }
    }

__device__ __forceinline__ SphPartial sph_nothing()
    {
    SphPartial p;
#pragma unroll
    for (int s = 0; s < 3; s++)
        {
        p.lo[s] = __builtin_huge_val();
        p.hi[s] = -__builtin_huge_val();
        }
    p.dev = 0.0;
    p.at = SPH_NONE;
    p.pad = 0;
    return p;
    }

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void sph_compact_kernel(const SphArgs a, const uint32_t* flag_dev, void* __restrict__ xs,
                                                                  double* __restrict__ ms, double* __restrict__ vs)
    {
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= a.n || *flag_dev != 0)
        return;
    const uint64_t row = a.rows[k];
    if (row >= a.N) // (the check kernel has refused such a list: nothing is loaded for it)
        return;
    compact_position<F64>(a.pos, row, xs, k);
    const double m = a.mass ? column_value(a.mass, a.mass_f64, row) : a.mass_default;
    ms[k] = m;
    if (a.volume)
        vs[k] = m / (a.density ? column_value(a.density, a.density_f64, row) : a.density_default);
    }

// words: the summary in device memory, zeroed by the launcher (words 2 and 3, not_finite and surface, are added to here)
template<bool F64, int KERNEL, bool VOL>
__global__ __launch_bounds__(SEL_THREADS) void sph_pair_kernel(const SphArgs a, const uint32_t* __restrict__ offs,
                                                               const uint32_t* flag_dev, const void* __restrict__ xs,
                                                               const double* __restrict__ ms, const double* __restrict__ vs,
                                                               double* __restrict__ out_number, double* __restrict__ out_density,
                                                               double* __restrict__ out_shepard,
                                                               unsigned long long* __restrict__ words,
                                                               SphPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_not_finite, s_surface;
    __shared__ SphPartial s_part[SPH_WAVES];
    if (*flag_dev != 0)
        return;
    if (threadIdx.x == 0)
        {
        s_not_finite = 0;
        s_surface = 0;
        }
    __syncthreads();
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    double a_n = 0.0, a_m = 0.0, a_v = 0.0;
    if (has)
        {
        const double inv_h = a.inv_h;
        traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                            [&](uint32_t j, double, double, double, double d2)
                            {
#pragma clang fp contract(off)
                                const double rr = __builtin_sqrt(d2);
                                const double q = rr * inv_h;
                                const double w = sph_weight<KERNEL>(q);
                                a_n = a_n + w;
                                a_m = a_m + ms[j] * w;
                                if constexpr (VOL)
                                    a_v = a_v + vs[j] * w;
                            });
        }
    // (an entry without a cell: the accumulators are +0.0, and so are the products)
    const double number = a.sigma * a_n, density = a.sigma * a_m, shepard = a.sigma * a_v;
    if (live)
        {
        if (out_number)
            out_number[k] = number;
        if (out_density)
            out_density[k] = density;
        if (VOL && out_shepard)
            out_shepard[k] = shepard;
        }
    SphPartial p = sph_nothing();
    if (has)
        {
        // (a NaN passes no compare: it replaces neither bound)
        p.lo[0] = number < p.lo[0] ? number : p.lo[0];
        p.hi[0] = number > p.hi[0] ? number : p.hi[0];
        p.lo[1] = density < p.lo[1] ? density : p.lo[1];
        p.hi[1] = density > p.hi[1] ? density : p.hi[1];
        if (!(__builtin_fabs(density) < __builtin_huge_val()))
            atomicAdd(&s_not_finite, 1u);
        if constexpr (VOL)
            {
            p.lo[2] = shepard < p.lo[2] ? shepard : p.lo[2];
            p.hi[2] = shepard > p.hi[2] ? shepard : p.hi[2];
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
        SphPartial o;
#pragma unroll
        for (int s = 0; s < 3; s++)
            {
            o.lo[s] = __shfl_xor(p.lo[s], h, 64);
            o.hi[s] = __shfl_xor(p.hi[s], h, 64);
            }
        o.dev = __shfl_xor(p.dev, h, 64);
        o.at = __shfl_xor(p.at, h, 64);
        sph_merge(p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SphPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < SPH_WAVES; w++)
            sph_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        if (s_not_finite)
            atomicAdd(&words[2], (unsigned long long)s_not_finite);
        if (s_surface)
            atomicAdd(&words[3], (unsigned long long)s_surface);
        }
    }

// One workgroup.  The words: n, nowhere, not_finite, surface, deviation_at, deviation_row, then as bit patterns the
// minimum and maximum of number, density and shepard and the deviation.
__global__ __launch_bounds__(SEL_THREADS) void sph_final_kernel(const SphArgs a, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const SphPartial* __restrict__ part,
                                                                uint32_t n_parts, unsigned long long* __restrict__ words)
    {
    __shared__ SphPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SphPartial p = sph_nothing();
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        sph_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        sph_merge(p, s_part[t]);
    const uint64_t n = a.n;
    const uint64_t somewhere = min((uint64_t)offs[a.n_cells], n);
    const bool any = p.at != SPH_NONE && p.at < n;
    words[0] = n;
    words[1] = n - somewhere;
    words[4] = any ? p.at : SPH_NONE;
    words[5] = any ? a.rows[p.at] : SPH_NONE;
#pragma unroll
    for (int s = 0; s < 3; s++)
        {
        words[6 + 2 * s] = (unsigned long long)__double_as_longlong(p.lo[s]);
        words[7 + 2 * s] = (unsigned long long)__double_as_longlong(p.hi[s]);
        }
    words[12] = (unsigned long long)__double_as_longlong(any ? p.dev : 0.0);
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), masses and volumes (n doubles each), the
// partials (one per workgroup) and the summary; the pinned flag word is the host's view of a refused list, the pinned
// host block the landing place of the summary.
constexpr size_t SPH_SUMMARY_BYTES = (size_t)SPH_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_sph_scratch("SPH kernel sums", 1.25, 1u << 16, SPH_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_sph_lock;

template<bool F64, int KERNEL>
void sph_launch_pair(bool vol, dim3 grid, dim3 block, hipStream_t stream, const SphArgs& a, const uint32_t* offs,
                     const uint32_t* flag_dev, const void* xs, const double* ms, const double* vs, double* out_number,
                     double* out_density, double* out_shepard, unsigned long long* words, SphPartial* part)
    {
    if (vol)
        hipLaunchKernelGGL((sph_pair_kernel<F64, KERNEL, true>), grid, block, 0, stream, a, offs, flag_dev, xs, ms, vs,
                           out_number, out_density, out_shepard, words, part);
    else
        hipLaunchKernelGGL((sph_pair_kernel<F64, KERNEL, false>), grid, block, 0, stream, a, offs, flag_dev, xs, ms, vs,
                           out_number, out_density, out_shepard, words, part);
    }
    } // namespace

void warm_sph_kernels()
    {
    warm_kernel((const void*)sph_pair_kernel<false, SPH_WENDLAND_C2, true>);
    }

int launch_sph_sums(const SphArgs& a, double* out_number, double* out_density, double* out_shepard, uint64_t* out_summary,
                    hipStream_t stream, std::string* err)
    {
    static const char* what = "SPH kernel sums";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.kernel != SPH_WENDLAND_C2 && a.kernel != SPH_CUBIC_SPLINE)
        return fail("the kernel is 0 (Wendland C2) or 1 (cubic spline)");
    const uint64_t n = a.n;
    if (n == 0)
        {
        sph_sums_of_nothing(out_summary);
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
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(SphPartial));
    const size_t words_bytes = SPH_SUMMARY_BYTES;
    LaunchScope scope(g_sph_lock, g_sph_scratch, 16 + offs_bytes + xs_bytes + 2 * col_bytes + part_bytes + words_bytes, stream,
                      err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    double* ms = (double*)((char*)xs + xs_bytes);
    double* vs = (double*)((char*)ms + col_bytes);
    SphPartial* part = (SphPartial*)((char*)vs + col_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    const bool vol = a.volume != 0;
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   words, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(sph_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs, ms, vs);
            if (a.kernel == SPH_WENDLAND_C2)
                sph_launch_pair<true, SPH_WENDLAND_C2>(vol, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, out_number,
                                                       out_density, out_shepard, words, part);
            else
                sph_launch_pair<true, SPH_CUBIC_SPLINE>(vol, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, out_number,
                                                        out_density, out_shepard, words, part);
            }
        else
            {
            hipLaunchKernelGGL(sph_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs, ms, vs);
            if (a.kernel == SPH_WENDLAND_C2)
                sph_launch_pair<false, SPH_WENDLAND_C2>(vol, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, out_number,
                                                        out_density, out_shepard, words, part);
            else
                sph_launch_pair<false, SPH_CUBIC_SPLINE>(vol, per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, out_number,
                                                         out_density, out_shepard, words, part);
            }
        hipLaunchKernelGGL(sph_final_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, part, n_blocks, words);
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
    std::copy(landed, landed + SPH_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
