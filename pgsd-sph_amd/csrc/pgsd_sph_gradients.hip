// pgsd_sph_gradients.hip -- the SPH kernel gradients on gfx950: per entry i of a row list in cell order the four
// gradient-weighted pair sums over the entries j of the periodically adjacent cells that lie strictly inside the kernel
// support 2h -- the density rate sum_j m_j (v_i - v_j) . grad_i W_ij of the continuity equation, the velocity divergence
// and curl sum_j V_j (v_j - v_i) {. , x} grad_i W_ij and the colour gradient sum_j V_j grad_i W_ij (the surface normal),
// V_j = m_j / rho_j -- and over the list the ranges of the two scalars and the largest curl and normal with their rows.
// pgsd.hoomd.sph_kernel_gradients is the definition and this file equals it exactly, the floats bit for bit: the grid, the
// support, the list and the ORDER of the candidates are the SPH kernel sums' (pgsd_sph.hip, pgsd_traverse.hpp); the
// arithmetic of one pair is d = pgsd.hoomd.pair_displacement, d2, rr = sqrt(d2), q = rr * inv_h, F(q) = (1/q) dw/dq of
// pgsd.hoomd.sph_gradient_factor, e = F * d, u = v_j - v_i, dot = (u0*e0 + u1*e1) + u2*e2 and c = e x u, float64 without
// contraction; r2 = (2h)*(2h), inv_h = 1/h and G = -((sigma*inv_h)*inv_h) come from the host, and G multiplies a sum once,
// after its last candidate.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          CSR offsets; every kernel here reads the device flag first and does nothing where it is set
//   sphg_compact_kernel<F64>   (pgsd_sph_compact.hpp, shared with pgsd_sph_tensors.hip) lane per entry: xs[k] = position[rows[k]] in the chunk's own element type, m[k] the mass,
//                          V[k] = m / rho (one float64 division of the stored values) and the velocity as three float64
//                          values (an exact conversion, so that the velocity chunk's element type stays out of the pair
//                          kernel's template list; the zero vector where no velocity is stored)
//   sphg_pair_kernel<F64, KERNEL, VOL>   lane per entry i: x_i, v_i and the eight accumulators in registers, the
//                          candidates by traverse_candidates (pgsd_traverse.hpp) in the defined order.  not_finite goes
//                          through an LDS counter and one 64-bit integer atomic; the ranges and the two largest norms,
//                          each with its list position, leave as one partial per workgroup
//   sphg_final_kernel      one workgroup: the partials in a fixed strided scan, then the words of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp, pgsd_traverse.hpp (the position copy and the column read of the compact kernel as well); the
// launcher's host side: pgsd_scratch.hpp and pgsd_cells.hpp (the argument checks and the opening sequence).  F(q) is
// pgsd_traverse.hpp's sphg_factor, which the SPH accelerations (pgsd_sph_forces.hip) take as well.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_sph_compact.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define SPHG_WAVES (SEL_THREADS / 64)
// one workgroup's share of what is no count: the smallest and largest divergence (0) and density rate (1) over its
// entries that have a cell (+inf / -inf: it has none, or NaNs only) and the largest squared curl (0) and normal (1) with
// their list positions (SPH_NONE: it has none)
struct SphgPartial
    {
    double lo[2], hi[2];
    double big[2];
    uint32_t at[2];
    };

// does the norm (v, i) replace (e, k): the larger value, then the smaller position; an empty slot never does
__device__ __forceinline__ bool sphg_before(double v, uint32_t i, double e, uint32_t k)
    {
    if (i == SPH_NONE)
        return false;
    if (k == SPH_NONE)
        return true;
    return v > e || (v == e && i < k);
    }

__device__ __forceinline__ void sphg_merge(SphgPartial& p, const SphgPartial& o)
    {
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        p.lo[s] = o.lo[s] < p.lo[s] ? o.lo[s] : p.lo[s];
        p.hi[s] = o.hi[s] > p.hi[s] ? o.hi[s] : p.hi[s];
        if (sphg_before(o.big[s], o.at[s], p.big[s], p.at[s]))
            {
            p.big[s] = o.big[s];
            p.at[s] = o.at[s];
            }
        }
    }

__device__ __forceinline__ SphgPartial sphg_nothing()
    {
    SphgPartial p;
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        p.lo[s] = __builtin_huge_val();
        p.hi[s] = -__builtin_huge_val();
        p.big[s] = 0.0;
        p.at[s] = SPH_NONE;
        }
    return p;
    }

// words: the summary in device memory, zeroed by the launcher (word 2, not_finite, is added to here)
template<bool F64, int KERNEL, bool VOL>
__global__ __launch_bounds__(SEL_THREADS) void sphg_pair_kernel(const SphGradientsArgs a, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                const double* __restrict__ ms, const double* __restrict__ vs,
                                                                const double* __restrict__ ws, double* __restrict__ out_rate,
                                                                double* __restrict__ out_divergence, double* __restrict__ out_curl,
                                                                double* __restrict__ out_normal,
                                                                unsigned long long* __restrict__ words,
                                                                SphgPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_not_finite;
    __shared__ SphgPartial s_part[SPHG_WAVES];
    if (*flag_dev != 0)
        return;
    if (threadIdx.x == 0)
        s_not_finite = 0;
    __syncthreads();
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    double a_r = 0.0, a_d = 0.0, a_w0 = 0.0, a_w1 = 0.0, a_w2 = 0.0, a_c0 = 0.0, a_c1 = 0.0, a_c2 = 0.0;
    if (has)
        {
        const double inv_h = a.inv_h;
        const double vi0 = ws[(size_t)k * 3 + 0], vi1 = ws[(size_t)k * 3 + 1], vi2 = ws[(size_t)k * 3 + 2];
        traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                            [&](uint32_t j, double dx, double dy, double dz, double d2)
                            {
#pragma clang fp contract(off)
                                const double rr = __builtin_sqrt(d2);
                                const double q = rr * inv_h;
                                const double F = sphg_factor<KERNEL>(q);
                                const double e0 = F * dx, e1 = F * dy, e2 = F * dz;
                                const double u0 = ws[(size_t)j * 3 + 0] - vi0, u1 = ws[(size_t)j * 3 + 1] - vi1;
                                const double u2 = ws[(size_t)j * 3 + 2] - vi2;
                                const double dot = (u0 * e0 + u1 * e1) + u2 * e2;
                                a_r = a_r + ms[j] * dot;
                                if constexpr (VOL)
                                    {
                                    const double V = vs[j];
                                    const double c0 = e1 * u2 - e2 * u1, c1 = e2 * u0 - e0 * u2, c2 = e0 * u1 - e1 * u0;
                                    a_d = a_d + V * dot;
                                    a_w0 = a_w0 + V * c0;
                                    a_w1 = a_w1 + V * c1;
                                    a_w2 = a_w2 + V * c2;
                                    a_c0 = a_c0 + V * e0;
                                    a_c1 = a_c1 + V * e1;
                                    a_c2 = a_c2 + V * e2;
                                    }
                            });
        }
    // (an entry without a cell: every value is +0.0, whatever the sign of G)
    const double G = a.G;
    const double rate = has ? -(G * a_r) : 0.0, divergence = has ? G * a_d : 0.0;
    const double w0 = has ? G * a_w0 : 0.0, w1 = has ? G * a_w1 : 0.0, w2 = has ? G * a_w2 : 0.0;
    const double n0 = has ? G * a_c0 : 0.0, n1 = has ? G * a_c1 : 0.0, n2 = has ? G * a_c2 : 0.0;
    if (live)
        {
        if (out_rate)
            out_rate[k] = rate;
        if constexpr (VOL)
            {
            if (out_divergence)
                out_divergence[k] = divergence;
            if (out_curl)
                {
                out_curl[(size_t)k * 3 + 0] = w0;
                out_curl[(size_t)k * 3 + 1] = w1;
                out_curl[(size_t)k * 3 + 2] = w2;
                }
            if (out_normal)
                {
                out_normal[(size_t)k * 3 + 0] = n0;
                out_normal[(size_t)k * 3 + 1] = n1;
                out_normal[(size_t)k * 3 + 2] = n2;
                }
            }
        }
    SphgPartial p = sphg_nothing();
    if (has)
        {
        // (a NaN passes no compare: it replaces neither bound and is no largest norm)
        p.lo[1] = rate < p.lo[1] ? rate : p.lo[1];
        p.hi[1] = rate > p.hi[1] ? rate : p.hi[1];
        if (!(__builtin_fabs(rate) < __builtin_huge_val()))
            atomicAdd(&s_not_finite, 1u);
        if constexpr (VOL)
            {
            p.lo[0] = divergence < p.lo[0] ? divergence : p.lo[0];
            p.hi[0] = divergence > p.hi[0] ? divergence : p.hi[0];
            const double curl2 = (w0 * w0 + w1 * w1) + w2 * w2;
            const double normal2 = (n0 * n0 + n1 * n1) + n2 * n2;
            if (curl2 == curl2)
                {
                p.big[0] = curl2;
                p.at[0] = k;
                }
            if (normal2 == normal2)
                {
                p.big[1] = normal2;
                p.at[1] = k;
                }
            }
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        SphgPartial o;
#pragma unroll
        for (int s = 0; s < 2; s++)
            {
            o.lo[s] = __shfl_xor(p.lo[s], h, 64);
            o.hi[s] = __shfl_xor(p.hi[s], h, 64);
            o.big[s] = __shfl_xor(p.big[s], h, 64);
            o.at[s] = __shfl_xor(p.at[s], h, 64);
            }
        sphg_merge(p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SphgPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < SPHG_WAVES; w++)
            sphg_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        if (s_not_finite)
            atomicAdd(&words[2], (unsigned long long)s_not_finite);
        }
    }

// One workgroup.  The words: n, nowhere, not_finite, curl_at, curl_row, normal_at, normal_row, then as bit patterns the
// minimum and maximum of the divergence and of the density rate and the largest squared curl and normal.
__global__ __launch_bounds__(SEL_THREADS) void sphg_final_kernel(const SphGradientsArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const SphgPartial* __restrict__ part,
                                                                 uint32_t n_parts, unsigned long long* __restrict__ words)
    {
    __shared__ SphgPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SphgPartial p = sphg_nothing();
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        sphg_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        sphg_merge(p, s_part[t]);
    const uint64_t n = a.n;
    const uint64_t somewhere = min((uint64_t)offs[a.n_cells], n);
    words[0] = n;
    words[1] = n - somewhere;
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        const bool any = p.at[s] != SPH_NONE && p.at[s] < n;
        words[3 + 2 * s] = any ? p.at[s] : SPH_NONE;
        words[4 + 2 * s] = any ? a.rows[p.at[s]] : SPH_NONE;
        words[11 + s] = (unsigned long long)__double_as_longlong(any ? p.big[s] : 0.0);
        words[7 + 2 * s] = (unsigned long long)__double_as_longlong(p.lo[s]);
        words[8 + 2 * s] = (unsigned long long)__double_as_longlong(p.hi[s]);
        }
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), masses and volumes (n doubles each), velocities
// (n x 3 doubles), the partials (one per workgroup) and the summary; the pinned flag word is the host's view of a refused
// list, the pinned host block the landing place of the summary.
constexpr size_t SPHG_SUMMARY_BYTES = (size_t)SPHG_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_sphg_scratch("SPH kernel gradients", 1.25, 1u << 16, SPHG_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_sphg_lock;

struct SphgBuffers
    {
    const uint32_t* offs;
    const uint32_t* flag_dev;
    const void* xs;
    const double *ms, *vs, *ws;
    double *out_rate, *out_divergence, *out_curl, *out_normal;
    unsigned long long* words;
    SphgPartial* part;
    };

template<bool F64, int KERNEL>
void sphg_launch_pair(bool vol, dim3 grid, dim3 block, hipStream_t stream, const SphGradientsArgs& a, const SphgBuffers& b)
    {
    if (vol)
        hipLaunchKernelGGL((sphg_pair_kernel<F64, KERNEL, true>), grid, block, 0, stream, a, b.offs, b.flag_dev, b.xs, b.ms, b.vs,
                           b.ws, b.out_rate, b.out_divergence, b.out_curl, b.out_normal, b.words, b.part);
    else
        hipLaunchKernelGGL((sphg_pair_kernel<F64, KERNEL, false>), grid, block, 0, stream, a, b.offs, b.flag_dev, b.xs, b.ms, b.vs,
                           b.ws, b.out_rate, b.out_divergence, b.out_curl, b.out_normal, b.words, b.part);
    }
    } // namespace

void warm_sph_gradients_kernels()
    {
    warm_kernel((const void*)sphg_pair_kernel<false, SPH_WENDLAND_C2, true>);
    }

int launch_sph_gradients(const SphGradientsArgs& a, double* out_rate, double* out_divergence, double* out_curl,
                         double* out_normal, uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "SPH kernel gradients";
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
        sph_gradients_of_nothing(out_summary);
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
    const size_t vel_bytes = round16((size_t)n * 3 * sizeof(double));
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(SphgPartial));
    const size_t words_bytes = SPHG_SUMMARY_BYTES;
    LaunchScope scope(g_sphg_lock, g_sphg_scratch,
                      16 + offs_bytes + xs_bytes + 2 * col_bytes + vel_bytes + part_bytes + words_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    double* ms = (double*)((char*)xs + xs_bytes);
    double* vs = (double*)((char*)ms + col_bytes);
    double* ws = (double*)((char*)vs + col_bytes);
    SphgPartial* part = (SphgPartial*)((char*)ws + vel_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    const bool vol = a.volume != 0;
    const SphgBuffers b = {offs, flag_dev, xs, ms, vs, ws, out_rate, out_divergence, out_curl, out_normal, words, part};
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   words, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(sphg_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs, ms, vs, ws);
            if (a.kernel == SPH_WENDLAND_C2)
                sphg_launch_pair<true, SPH_WENDLAND_C2>(vol, per_entry, block, stream, a, b);
            else
                sphg_launch_pair<true, SPH_CUBIC_SPLINE>(vol, per_entry, block, stream, a, b);
            }
        else
            {
            hipLaunchKernelGGL(sphg_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs, ms, vs, ws);
            if (a.kernel == SPH_WENDLAND_C2)
                sphg_launch_pair<false, SPH_WENDLAND_C2>(vol, per_entry, block, stream, a, b);
            else
                sphg_launch_pair<false, SPH_CUBIC_SPLINE>(vol, per_entry, block, stream, a, b);
            }
        hipLaunchKernelGGL(sphg_final_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, part, n_blocks, words);
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
    std::copy(landed, landed + SPHG_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
