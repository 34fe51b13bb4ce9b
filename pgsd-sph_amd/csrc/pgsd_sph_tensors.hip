// pgsd_sph_tensors.hip -- the SPH gradient tensors on gfx950: per entry i of a row list in cell order the kernel-gradient
// correction (renormalisation) matrix L_i = B_i^-1 with B_i = sum_j V_j d (x) grad_i W_ij, its determinant, the corrected
// velocity-gradient tensor D_i = (sum_j V_j (v_j - v_i) (x) grad_i W_ij) L_i and the shear rate sqrt(2 S:S) of its symmetric
// part, over the entries j of the periodically adjacent cells that lie strictly inside the kernel support 2h -- and over
// the list the entries that stayed uncorrected, the ranges of the determinant and of the trace and the largest shear rate
// with its row.  pgsd.hoomd.sph_gradient_tensors is the definition and this file equals it exactly, the floats bit for
// bit: the grid, the support, the list and the ORDER of the candidates are the SPH kernel sums' (pgsd_sph.hip,
// pgsd_traverse.hpp); the arithmetic of one pair is the SPH kernel gradients' (d, d2, rr = sqrt(d2), q = rr * inv_h, F(q),
// e = F * d, u = v_j - v_i), then b_ab += V_j * (d_a * e_b) for the upper triangle and g_ab += V_j * (u_a * e_b) for all
// nine, float64 without contraction; G multiplies a sum once, after its last candidate, and the inverse, the product and
// the shear rate follow in the association pgsd_private.h writes out.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          CSR offsets; every kernel here reads the device flag first and does nothing where it is set
//   sphg_compact_kernel<F64>   pgsd_sph_compact.hpp's, shared with pgsd_sph_gradients.hip: xs, m, V and the velocity as
//                          three float64 values
//   spht_pair_kernel<F64, KERNEL>   lane per entry i: x_i, v_i and the fifteen accumulators in registers, the candidates
//                          by traverse_candidates (pgsd_traverse.hpp) in the defined order; the 3x3 symmetric inverse and
//                          the epilogue in the same kernel, 2-D / 3-D a run-time branch of the epilogue.  not_finite and
//                          uncorrected go through LDS counters and one 64-bit integer atomic each per workgroup; the
//                          ranges, the smallest determinant and the largest shear rate, each with its list position,
//                          leave as one partial per workgroup (wave shuffles, then LDS)
//   spht_final_kernel      one workgroup: the partials in a fixed strided scan, then the words of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp, pgsd_traverse.hpp, pgsd_sph_compact.hpp; the launcher's host side: pgsd_scratch.hpp and pgsd_cells.hpp
// (the argument checks and the opening sequence).
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_sph_compact.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define SPHT_WAVES (SEL_THREADS / 64)
// one workgroup's share of what is no count: the smallest and largest determinant (0) and trace (1) over its entries that
// have a cell (+inf / -inf: it has none, or NaNs only), the smallest determinant below +inf and the largest shear rate
// with their list positions (SPH_NONE: it has none)
struct SphtPartial
    {
    double lo[2], hi[2];
    double small, big;
    uint32_t small_at, big_at;
    };

// does (v, i) replace (e, k) as the smallest (LARGEST false) or the largest value: the better value, then the smaller
// position; an empty slot never does
template<bool LARGEST> __device__ __forceinline__ bool spht_before(double v, uint32_t i, double e, uint32_t k)
    {
    if (i == SPH_NONE)
        return false;
    if (k == SPH_NONE)
        return true;
    return (LARGEST ? v > e : v < e) || (v == e && i < k);
    }

// is a below b, with -0.0 below +0.0: a determinant and a trace are often a zero of either sign, and a bound must not
// depend on the order in which the partials meet (a NaN is below nothing and nothing is below it)
__device__ __forceinline__ bool spht_below(double a, double b)
    {
    return a < b || (a == b && __double_as_longlong(a) < 0 && __double_as_longlong(b) >= 0);
    }

__device__ __forceinline__ void spht_merge(SphtPartial& p, const SphtPartial& o)
    {
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        p.lo[s] = spht_below(o.lo[s], p.lo[s]) ? o.lo[s] : p.lo[s];
        p.hi[s] = spht_below(p.hi[s], o.hi[s]) ? o.hi[s] : p.hi[s];
        }
    if (spht_before<false>(o.small, o.small_at, p.small, p.small_at))
        {
        p.small = o.small;
        p.small_at = o.small_at;
        }
    if (spht_before<true>(o.big, o.big_at, p.big, p.big_at))
        {
        p.big = o.big;
        p.big_at = o.big_at;
        }
    }

__device__ __forceinline__ SphtPartial spht_nothing()
    {
    SphtPartial p;
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        p.lo[s] = __builtin_huge_val();
        p.hi[s] = -__builtin_huge_val();
        }
    p.small = __builtin_huge_val();
    p.big = 0.0;
    p.small_at = p.big_at = SPH_NONE;
    return p;
    }

// words: the summary in device memory, zeroed by the launcher (words 2 and 3, not_finite and uncorrected, are added to
// here)
template<bool F64, int KERNEL>
__global__ __launch_bounds__(SEL_THREADS) void spht_pair_kernel(const SphTensorsArgs a, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                const double* __restrict__ vs, const double* __restrict__ ws,
                                                                double* __restrict__ out_correction,
                                                                double* __restrict__ out_determinant,
                                                                double* __restrict__ out_gradient, double* __restrict__ out_shear,
                                                                unsigned long long* __restrict__ words,
                                                                SphtPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_count[2]; // not_finite, uncorrected
    __shared__ SphtPartial s_part[SPHT_WAVES];
    if (*flag_dev != 0)
        return;
    if (threadIdx.x < 2)
        s_count[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    double b00 = 0.0, b01 = 0.0, b02 = 0.0, b11 = 0.0, b12 = 0.0, b22 = 0.0;
    double g00 = 0.0, g01 = 0.0, g02 = 0.0, g10 = 0.0, g11 = 0.0, g12 = 0.0, g20 = 0.0, g21 = 0.0, g22 = 0.0;
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
                                const double V = vs[j];
                                b00 = b00 + V * (dx * e0);
                                b01 = b01 + V * (dx * e1);
                                b02 = b02 + V * (dx * e2);
                                b11 = b11 + V * (dy * e1);
                                b12 = b12 + V * (dy * e2);
                                b22 = b22 + V * (dz * e2);
                                g00 = g00 + V * (u0 * e0);
                                g01 = g01 + V * (u0 * e1);
                                g02 = g02 + V * (u0 * e2);
                                g10 = g10 + V * (u1 * e0);
                                g11 = g11 + V * (u1 * e1);
                                g12 = g12 + V * (u1 * e2);
                                g20 = g20 + V * (u2 * e0);
                                g21 = g21 + V * (u2 * e1);
                                g22 = g22 + V * (u2 * e2);
                            });
        }
    // (an entry without a cell: every value is +0.0, written)
    double L00 = 0.0, L01 = 0.0, L02 = 0.0, L11 = 0.0, L12 = 0.0, L22 = 0.0, det = 0.0;
    double D00 = 0.0, D01 = 0.0, D02 = 0.0, D10 = 0.0, D11 = 0.0, D12 = 0.0, D20 = 0.0, D21 = 0.0, D22 = 0.0;
    double trace = 0.0, shear = 0.0;
    bool ok = false;
    if (has)
        {
        const double G = a.G;
        const double B00 = G * b00, B01 = G * b01, B02 = G * b02, B11 = G * b11, B12 = G * b12, B22 = G * b22;
        const double R00 = G * g00, R01 = G * g01, R02 = G * g02, R10 = G * g10, R11 = G * g11, R12 = G * g12;
        const double R20 = G * g20, R21 = G * g21, R22 = G * g22;
        const bool three = a.dims != 2;
        double c00, c01, c02 = 0.0, c11, c12 = 0.0, c22 = 0.0;
        if (three)
            {
            c00 = B11 * B22 - B12 * B12;
            c01 = B02 * B12 - B01 * B22;
            c02 = B01 * B12 - B02 * B11;
            c11 = B00 * B22 - B02 * B02;
            c12 = B01 * B02 - B00 * B12;
            c22 = B00 * B11 - B01 * B01;
            det = (B00 * c00 + B01 * c01) + B02 * c02;
            }
        else
            {
            det = B00 * B11 - B01 * B01;
            c00 = B11;
            c01 = -B01;
            c11 = B00;
            }
        ok = det > a.det_min && det < __builtin_huge_val();
        if (ok)
            {
            L00 = c00 / det;
            L01 = c01 / det;
            L11 = c11 / det;
            if (three)
                {
                L02 = c02 / det;
                L12 = c12 / det;
                L22 = c22 / det;
                D00 = (R00 * L00 + R01 * L01) + R02 * L02;
                D01 = (R00 * L01 + R01 * L11) + R02 * L12;
                D02 = (R00 * L02 + R01 * L12) + R02 * L22;
                D10 = (R10 * L00 + R11 * L01) + R12 * L02;
                D11 = (R10 * L01 + R11 * L11) + R12 * L12;
                D12 = (R10 * L02 + R11 * L12) + R12 * L22;
                D20 = (R20 * L00 + R21 * L01) + R22 * L02;
                D21 = (R20 * L01 + R21 * L11) + R22 * L12;
                D22 = (R20 * L02 + R21 * L12) + R22 * L22;
                }
            else
                {
                // (L02, L12, L22 and the third column of D stay the +0.0 they were written as)
                D00 = R00 * L00 + R01 * L01;
                D01 = R00 * L01 + R01 * L11;
                D10 = R10 * L00 + R11 * L01;
                D11 = R10 * L01 + R11 * L11;
                D20 = R20 * L00 + R21 * L01;
                D21 = R20 * L01 + R21 * L11;
                }
            }
        else
            {
            // (the identity and the uncorrected gradient, written, not computed)
            L00 = 1.0;
            L11 = 1.0;
            L22 = three ? 1.0 : 0.0;
            D00 = R00, D01 = R01, D02 = R02;
            D10 = R10, D11 = R11, D12 = R12;
            D20 = R20, D21 = R21, D22 = R22;
            }
        trace = (D00 + D11) + D22;
        const double s01 = 0.5 * (D01 + D10), s02 = 0.5 * (D02 + D20), s12 = 0.5 * (D12 + D21);
        const double ss = ((D00 * D00 + D11 * D11) + D22 * D22) + 2.0 * ((s01 * s01 + s02 * s02) + s12 * s12);
        shear = __builtin_sqrt(2.0 * ss);
        }
    if (live)
        {
        if (out_correction)
            {
            double* o = out_correction + (size_t)k * 6;
            o[0] = L00, o[1] = L01, o[2] = L02, o[3] = L11, o[4] = L12, o[5] = L22;
            }
        if (out_determinant)
            out_determinant[k] = det;
        if (out_gradient)
            {
            double* o = out_gradient + (size_t)k * 9;
            o[0] = D00, o[1] = D01, o[2] = D02, o[3] = D10, o[4] = D11, o[5] = D12, o[6] = D20, o[7] = D21, o[8] = D22;
            }
        if (out_shear)
            out_shear[k] = shear;
        }
    SphtPartial p = spht_nothing();
    if (has)
        {
        // (a NaN passes no compare: it replaces neither bound and is neither the smallest nor the largest)
        p.lo[0] = spht_below(det, p.lo[0]) ? det : p.lo[0];
        p.hi[0] = spht_below(p.hi[0], det) ? det : p.hi[0];
        p.lo[1] = spht_below(trace, p.lo[1]) ? trace : p.lo[1];
        p.hi[1] = spht_below(p.hi[1], trace) ? trace : p.hi[1];
        if (det < __builtin_huge_val())
            {
            p.small = det;
            p.small_at = k;
            }
        if (shear == shear)
            {
            p.big = shear;
            p.big_at = k;
            }
        if (!(__builtin_fabs(shear) < __builtin_huge_val()))
            atomicAdd(&s_count[0], 1u);
        if (!ok)
            atomicAdd(&s_count[1], 1u);
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        SphtPartial o;
#pragma unroll
        for (int s = 0; s < 2; s++)
            {
            o.lo[s] = __shfl_xor(p.lo[s], h, 64);
            o.hi[s] = __shfl_xor(p.hi[s], h, 64);
            }
        o.small = __shfl_xor(p.small, h, 64);
        o.big = __shfl_xor(p.big, h, 64);
        o.small_at = __shfl_xor(p.small_at, h, 64);
        o.big_at = __shfl_xor(p.big_at, h, 64);
        spht_merge(p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SphtPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < SPHT_WAVES; w++)
            spht_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        if (s_count[0])
            atomicAdd(&words[2], (unsigned long long)s_count[0]);
        if (s_count[1])
            atomicAdd(&words[3], (unsigned long long)s_count[1]);
        }
    }

// One workgroup.  The words: n, nowhere, not_finite, uncorrected, det_at, det_row, shear_at, shear_row, then as bit
// patterns the minimum and maximum of the determinant and of the trace and the largest shear rate; the last word is 0.
__global__ __launch_bounds__(SEL_THREADS) void spht_final_kernel(const SphTensorsArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const SphtPartial* __restrict__ part,
                                                                 uint32_t n_parts, unsigned long long* __restrict__ words)
    {
    __shared__ SphtPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SphtPartial p = spht_nothing();
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        spht_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        spht_merge(p, s_part[t]);
    const uint64_t n = a.n;
    const uint64_t somewhere = min((uint64_t)offs[a.n_cells], n);
    words[0] = n;
    words[1] = n - somewhere;
    const bool any_small = p.small_at != SPH_NONE && p.small_at < n;
    const bool any_big = p.big_at != SPH_NONE && p.big_at < n;
    words[4] = any_small ? p.small_at : SPH_NONE;
    words[5] = any_small ? a.rows[p.small_at] : SPH_NONE;
    words[6] = any_big ? p.big_at : SPH_NONE;
    words[7] = any_big ? a.rows[p.big_at] : SPH_NONE;
#pragma unroll
    for (int s = 0; s < 2; s++)
        {
        words[8 + 2 * s] = (unsigned long long)__double_as_longlong(p.lo[s]);
        words[9 + 2 * s] = (unsigned long long)__double_as_longlong(p.hi[s]);
        }
    words[12] = (unsigned long long)__double_as_longlong(any_big ? p.big : 0.0);
    words[13] = 0;
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), masses and volumes (n doubles each), velocities
// (n x 3 doubles), the partials (one per workgroup) and the summary; the pinned flag word is the host's view of a refused
// list, the pinned host block the landing place of the summary.
constexpr size_t SPHT_SUMMARY_BYTES = (size_t)SPHT_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_spht_scratch("SPH gradient tensors", 1.25, 1u << 16, SPHT_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_spht_lock;

template<bool F64>
void spht_launch(dim3 grid, dim3 block, hipStream_t stream, const SphTensorsArgs& a, const uint32_t* offs,
                 const uint32_t* flag_dev, void* xs, double* ms, double* vs, double* ws, double* out_correction,
                 double* out_determinant, double* out_gradient, double* out_shear, unsigned long long* words, SphtPartial* part)
    {
    const SphGradientsArgs& g = a;
    hipLaunchKernelGGL(sphg_compact_kernel<F64>, grid, block, 0, stream, g, flag_dev, xs, ms, vs, ws);
    if (a.kernel == SPH_WENDLAND_C2)
        hipLaunchKernelGGL((spht_pair_kernel<F64, SPH_WENDLAND_C2>), grid, block, 0, stream, a, offs, flag_dev, xs, vs, ws,
                           out_correction, out_determinant, out_gradient, out_shear, words, part);
    else
        hipLaunchKernelGGL((spht_pair_kernel<F64, SPH_CUBIC_SPLINE>), grid, block, 0, stream, a, offs, flag_dev, xs, vs, ws,
                           out_correction, out_determinant, out_gradient, out_shear, words, part);
    }
    } // namespace

void warm_sph_tensors_kernels()
    {
    warm_kernel((const void*)spht_pair_kernel<false, SPH_WENDLAND_C2>);
    }

int launch_sph_tensors(const SphTensorsArgs& a, double* out_correction, double* out_determinant, double* out_gradient,
                       double* out_shear, uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "SPH gradient tensors";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.kernel != SPH_WENDLAND_C2 && a.kernel != SPH_CUBIC_SPLINE)
        return fail("the kernel is 0 (Wendland C2) or 1 (cubic spline)");
    if (!(a.det_min >= 0.0))
        return fail("det_min is a number, at least 0");
    if (!a.volume)
        return fail("the volumes need a density: a chunk or a default that is a number");
    const uint64_t n = a.n;
    if (n == 0)
        {
        sph_tensors_of_nothing(out_summary);
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
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(SphtPartial));
    const size_t words_bytes = SPHT_SUMMARY_BYTES;
    LaunchScope scope(g_spht_lock, g_spht_scratch,
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
    SphtPartial* part = (SphtPartial*)((char*)ws + vel_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   words, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            spht_launch<true>(per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, ws, out_correction, out_determinant,
                              out_gradient, out_shear, words, part);
        else
            spht_launch<false>(per_entry, block, stream, a, offs, flag_dev, xs, ms, vs, ws, out_correction, out_determinant,
                               out_gradient, out_shear, words, part);
        hipLaunchKernelGGL(spht_final_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, part, n_blocks, words);
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
    std::copy(landed, landed + SPHT_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
