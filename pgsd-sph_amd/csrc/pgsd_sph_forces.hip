// pgsd_sph_forces.hip -- the SPH accelerations on gfx950: per entry i of a row list in cell order the right-hand side of
// the momentum equation over the entries j of the periodically adjacent cells that lie strictly inside the kernel support
// 2h -- the pressure acceleration -sum_j m_j (p_i/rho_i^2 + p_j/rho_j^2) grad_i W_ij, Morris' laminar viscous acceleration
// (1/rho_i) sum_j V_j 2 mu (v_i - v_j) (d . grad_i W_ij) / (|d|^2 + eta^2) written with u = v_j - v_i, and their sum with
// gravity -- and over the list the largest of the three with their rows.
// pgsd.hoomd.sph_accelerations is the definition and this file equals it exactly, the floats bit for bit: the grid, the
// support, the list and the ORDER of the candidates are the SPH kernel sums' (pgsd_sph.hip, pgsd_traverse.hpp); d, d2,
// rr = sqrt(d2), q = rr * inv_h, F(q) and e = F * d are the SPH kernel gradients' (sphg_factor); then S = A_i + A_j with
// the stored A_k = p_k / (rho_k*rho_k), a_p[k] += m_j * (S * e_k) and, with a viscosity, K = (F * d2) / (d2 + eta2),
// u_k = v_j[k] - v_i[k], a_v[k] += V_j * (K * u_k) with the stored V_k = m_k / rho_k -- float64 without contraction.
// r2, inv_h, G = -((sigma*inv_h)*inv_h), eta2 = (0.01*h)*h and Gv = G * (2.0*mu) come from the host; after the last
// candidate pressure_acc = -(G*a_p), viscous_acc = (Gv*a_v) / rho_i, total = (pressure_acc + viscous_acc) + g.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged (pgsd_cells.hpp): the refusal protocol and the
//                          CSR offsets; every kernel here reads the device flag first and does nothing where it is set
//   sphf_compact_kernel<F64>   lane per entry: xs[k] = position[rows[k]] in the chunk's own element type, m[k], A[k] =
//                          p / (rho*rho), V[k] = m / rho, rho[k] and the velocity as three float64 values (exact
//                          conversions; one multiplication and two divisions of the stored values)
//   sphf_pair_kernel<F64, KERNEL, VISC>   lane per entry i: x_i, v_i, A_i and the three or six accumulators in registers,
//                          the candidates by traverse_candidates (pgsd_traverse.hpp) in the defined order.  not_finite
//                          goes through an LDS counter and one 64-bit integer atomic; the three largest norms, each with
//                          its list position, leave as one partial per workgroup
//   sphf_final_kernel      one workgroup: the partials in a fixed strided scan, then the words of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp, pgsd_traverse.hpp; the launcher's host side: pgsd_scratch.hpp and pgsd_cells.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define SPHF_WAVES (SEL_THREADS / 64)
// one workgroup's share of the summary: the largest squared total (0), pressure (1) and viscous (2) acceleration over its
// entries that have a cell, with their list positions (SPH_NONE: it has none)
struct SphfPartial
    {
    double big[3];
    uint32_t at[3];
    uint32_t pad;
    };

// does the norm (v, i) replace (e, k): the larger value, then the smaller position; an empty slot never does
__device__ __forceinline__ bool sphf_before(double v, uint32_t i, double e, uint32_t k)
    {
    if (i == SPH_NONE)
        return false;
    if (k == SPH_NONE)
        return true;
    return v > e || (v == e && i < k);
    }

__device__ __forceinline__ void sphf_merge(SphfPartial& p, const SphfPartial& o)
    {
#pragma unroll
    for (int s = 0; s < 3; s++)
        if (sphf_before(o.big[s], o.at[s], p.big[s], p.at[s]))
            {
            p.big[s] = o.big[s];
            p.at[s] = o.at[s];
            }
    }

__device__ __forceinline__ SphfPartial sphf_nothing()
    {
    SphfPartial p;
#pragma unroll
    for (int s = 0; s < 3; s++)
        {
        p.big[s] = 0.0;
        p.at[s] = SPH_NONE;
        }
    p.pad = 0;
    return p;
    }

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void sphf_compact_kernel(const SphForcesArgs a, const uint32_t* flag_dev,
                                                                   void* __restrict__ xs, double* __restrict__ ms,
                                                                   double* __restrict__ As, double* __restrict__ vs,
                                                                   double* __restrict__ rhos, double* __restrict__ ws)
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
    const double p = a.pressure ? column_value(a.pressure, a.pressure_f64, row) : a.pressure_default;
    ms[k] = m;
    As[k] = p / (rho * rho);
    vs[k] = m / rho;
    rhos[k] = rho;
#pragma unroll
    for (int c = 0; c < 3; c++)
        ws[k * 3 + c] = a.velocity ? column_value(a.velocity, a.velocity_f64, row * 3 + c) : 0.0;
    }

// words: the summary in device memory, zeroed by the launcher (word 2, not_finite, is added to here)
template<bool F64, int KERNEL, bool VISC>
__global__ __launch_bounds__(SEL_THREADS) void sphf_pair_kernel(const SphForcesArgs a, const uint32_t* __restrict__ offs,
                                                                const uint32_t* flag_dev, const void* __restrict__ xs,
                                                                const double* __restrict__ ms, const double* __restrict__ As,
                                                                const double* __restrict__ vs, const double* __restrict__ rhos,
                                                                const double* __restrict__ ws, double* __restrict__ out_pressure,
                                                                double* __restrict__ out_viscous, double* __restrict__ out_total,
                                                                unsigned long long* __restrict__ words,
                                                                SphfPartial* __restrict__ part)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ uint32_t s_not_finite;
    __shared__ SphfPartial s_part[SPHF_WAVES];
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
    double a_p0 = 0.0, a_p1 = 0.0, a_p2 = 0.0, a_v0 = 0.0, a_v1 = 0.0, a_v2 = 0.0;
    if (has)
        {
        const double inv_h = a.inv_h, eta2 = a.eta2;
        const double Ai = As[k];
        double vi0 = 0.0, vi1 = 0.0, vi2 = 0.0;
        if constexpr (VISC)
            {
            vi0 = ws[(size_t)k * 3 + 0];
            vi1 = ws[(size_t)k * 3 + 1];
            vi2 = ws[(size_t)k * 3 + 2];
            }
        traverse_candidates((const elem_t*)xs, offs, n, k, (uint32_t)c, traverse_grid(a),
                            [&](uint32_t j, double dx, double dy, double dz, double d2)
                            {
#pragma clang fp contract(off)
                                const double rr = __builtin_sqrt(d2);
                                const double q = rr * inv_h;
                                const double F = sphg_factor<KERNEL>(q);
                                const double e0 = F * dx, e1 = F * dy, e2 = F * dz;
                                const double S = Ai + As[j];
                                const double m = ms[j];
                                a_p0 = a_p0 + m * (S * e0);
                                a_p1 = a_p1 + m * (S * e1);
                                a_p2 = a_p2 + m * (S * e2);
                                if constexpr (VISC)
                                    {
                                    const double K = (F * d2) / (d2 + eta2);
                                    const double V = vs[j];
                                    const double u0 = ws[(size_t)j * 3 + 0] - vi0, u1 = ws[(size_t)j * 3 + 1] - vi1;
                                    const double u2 = ws[(size_t)j * 3 + 2] - vi2;
                                    a_v0 = a_v0 + V * (K * u0);
                                    a_v1 = a_v1 + V * (K * u1);
                                    a_v2 = a_v2 + V * (K * u2);
                                    }
                            });
        }
    // (an entry without a cell: every value is +0.0, whatever the sign of G and whatever the gravity)
    const double G = a.G;
    const double p0 = has ? -(G * a_p0) : 0.0, p1 = has ? -(G * a_p1) : 0.0, p2 = has ? -(G * a_p2) : 0.0;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (has)
        {
        if constexpr (VISC)
            {
            const double Gv = a.Gv, rho = rhos[k];
            w0 = (Gv * a_v0) / rho;
            w1 = (Gv * a_v1) / rho;
            w2 = (Gv * a_v2) / rho;
            t0 = (p0 + w0) + a.gravity[0];
            t1 = (p1 + w1) + a.gravity[1];
            t2 = (p2 + w2) + a.gravity[2];
            }
        else
            {
            t0 = p0 + a.gravity[0];
            t1 = p1 + a.gravity[1];
            t2 = p2 + a.gravity[2];
            }
        }
    if (live)
        {
        if (out_pressure)
            {
            out_pressure[(size_t)k * 3 + 0] = p0;
            out_pressure[(size_t)k * 3 + 1] = p1;
            out_pressure[(size_t)k * 3 + 2] = p2;
            }
        if constexpr (VISC)
            {
            if (out_viscous)
                {
                out_viscous[(size_t)k * 3 + 0] = w0;
                out_viscous[(size_t)k * 3 + 1] = w1;
                out_viscous[(size_t)k * 3 + 2] = w2;
                }
            }
        if (out_total)
            {
            out_total[(size_t)k * 3 + 0] = t0;
            out_total[(size_t)k * 3 + 1] = t1;
            out_total[(size_t)k * 3 + 2] = t2;
            }
        }
    SphfPartial p = sphf_nothing();
    if (has)
        {
        const double inf = __builtin_huge_val();
        if (!(__builtin_fabs(t0) < inf) || !(__builtin_fabs(t1) < inf) || !(__builtin_fabs(t2) < inf))
            atomicAdd(&s_not_finite, 1u);
        // (a NaN passes no compare: it is no largest norm)
        const double total2 = (t0 * t0 + t1 * t1) + t2 * t2;
        const double pressure2 = (p0 * p0 + p1 * p1) + p2 * p2;
        if (total2 == total2)
            {
            p.big[0] = total2;
            p.at[0] = k;
            }
        if (pressure2 == pressure2)
            {
            p.big[1] = pressure2;
            p.at[1] = k;
            }
        if constexpr (VISC)
            {
            const double viscous2 = (w0 * w0 + w1 * w1) + w2 * w2;
            if (viscous2 == viscous2)
                {
                p.big[2] = viscous2;
                p.at[2] = k;
                }
            }
        }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        SphfPartial o;
#pragma unroll
        for (int s = 0; s < 3; s++)
            {
            o.big[s] = __shfl_xor(p.big[s], h, 64);
            o.at[s] = __shfl_xor(p.at[s], h, 64);
            }
        o.pad = 0;
        sphf_merge(p, o);
        }
    if ((threadIdx.x & 63) == 0)
        s_part[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        SphfPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < SPHF_WAVES; w++)
            sphf_merge(q, s_part[w]);
        part[blockIdx.x] = q;
        if (s_not_finite)
            atomicAdd(&words[2], (unsigned long long)s_not_finite);
        }
    }

// One workgroup.  The words: n, nowhere, not_finite, then the list position and the row of the largest total, pressure
// and viscous acceleration, then as bit patterns the three largest squared norms.
__global__ __launch_bounds__(SEL_THREADS) void sphf_final_kernel(const SphForcesArgs a, const uint32_t* __restrict__ offs,
                                                                 const uint32_t* flag_dev, const SphfPartial* __restrict__ part,
                                                                 uint32_t n_parts, unsigned long long* __restrict__ words)
    {
    __shared__ SphfPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    SphfPartial p = sphf_nothing();
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        sphf_merge(p, part[t]);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        sphf_merge(p, s_part[t]);
    const uint64_t n = a.n;
    const uint64_t somewhere = min((uint64_t)offs[a.n_cells], n);
    words[0] = n;
    words[1] = n - somewhere;
#pragma unroll
    for (int s = 0; s < 3; s++)
        {
        const bool any = p.at[s] != SPH_NONE && p.at[s] < n;
        words[3 + 2 * s] = any ? p.at[s] : SPH_NONE;
        words[4 + 2 * s] = any ? a.rows[p.at[s]] : SPH_NONE;
        words[9 + s] = (unsigned long long)__double_as_longlong(any ? p.big[s] : 0.0);
        }
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the
// offsets (n_cells + 2 words), the compacted positions (n x 3 elements), masses, A values, volumes and densities (n
// doubles each), velocities (n x 3 doubles), the partials (one per workgroup) and the summary; the pinned flag word is the
// host's view of a refused list, the pinned host block the landing place of the summary.
constexpr size_t SPHF_SUMMARY_BYTES = (size_t)SPHF_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_sphf_scratch("SPH accelerations", 1.25, 1u << 16, SPHF_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_sphf_lock;

struct SphfBuffers
    {
    const uint32_t* offs;
    const uint32_t* flag_dev;
    const void* xs;
    const double *ms, *As, *vs, *rhos, *ws;
    double *out_pressure, *out_viscous, *out_total;
    unsigned long long* words;
    SphfPartial* part;
    };

template<bool F64, int KERNEL>
void sphf_launch_pair(bool visc, dim3 grid, dim3 block, hipStream_t stream, const SphForcesArgs& a, const SphfBuffers& b)
    {
    if (visc)
        hipLaunchKernelGGL((sphf_pair_kernel<F64, KERNEL, true>), grid, block, 0, stream, a, b.offs, b.flag_dev, b.xs, b.ms, b.As,
                           b.vs, b.rhos, b.ws, b.out_pressure, b.out_viscous, b.out_total, b.words, b.part);
    else
        hipLaunchKernelGGL((sphf_pair_kernel<F64, KERNEL, false>), grid, block, 0, stream, a, b.offs, b.flag_dev, b.xs, b.ms, b.As,
                           b.vs, b.rhos, b.ws, b.out_pressure, b.out_viscous, b.out_total, b.words, b.part);
    }
    } // namespace

void warm_sph_forces_kernels()
    {
    warm_kernel((const void*)sphf_pair_kernel<false, SPH_WENDLAND_C2, true>);
    }

int launch_sph_accelerations(const SphForcesArgs& a, double* out_pressure_acc, double* out_viscous_acc, double* out_total,
                             uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "SPH accelerations";
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
        sph_forces_of_nothing(out_summary);
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
    const size_t part_bytes = round16((size_t)n_blocks * sizeof(SphfPartial));
    const size_t words_bytes = SPHF_SUMMARY_BYTES;
    LaunchScope scope(g_sphf_lock, g_sphf_scratch,
                      16 + offs_bytes + xs_bytes + 4 * col_bytes + vel_bytes + part_bytes + words_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs = (uint32_t*)(dev + 16);
    void* xs = dev + 16 + offs_bytes;
    double* ms = (double*)((char*)xs + xs_bytes);
    double* As = (double*)((char*)ms + col_bytes);
    double* vs = (double*)((char*)As + col_bytes);
    double* rhos = (double*)((char*)vs + col_bytes);
    double* ws = (double*)((char*)rhos + col_bytes);
    SphfPartial* part = (SphfPartial*)((char*)ws + vel_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    const dim3 block(SEL_THREADS), per_entry(n_blocks);
    const bool visc = a.viscous != 0;
    const SphfBuffers b = {offs, flag_dev, xs, ms, As, vs, rhos, ws, out_pressure_acc, out_viscous_acc, out_total, words, part};
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, (uint32_t*)scope.mem().mapped_dev, offs,
                                   words, words_bytes, stream);
    if (e == hipSuccess)
        {
        if (a.f64)
            {
            hipLaunchKernelGGL(sphf_compact_kernel<true>, per_entry, block, 0, stream, a, flag_dev, xs, ms, As, vs, rhos, ws);
            if (a.kernel == SPH_WENDLAND_C2)
                sphf_launch_pair<true, SPH_WENDLAND_C2>(visc, per_entry, block, stream, a, b);
            else
                sphf_launch_pair<true, SPH_CUBIC_SPLINE>(visc, per_entry, block, stream, a, b);
            }
        else
            {
            hipLaunchKernelGGL(sphf_compact_kernel<false>, per_entry, block, 0, stream, a, flag_dev, xs, ms, As, vs, rhos, ws);
            if (a.kernel == SPH_WENDLAND_C2)
                sphf_launch_pair<false, SPH_WENDLAND_C2>(visc, per_entry, block, stream, a, b);
            else
                sphf_launch_pair<false, SPH_CUBIC_SPLINE>(visc, per_entry, block, stream, a, b);
            }
        hipLaunchKernelGGL(sphf_final_kernel, dim3(1), block, 0, stream, a, offs, flag_dev, part, n_blocks, words);
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
    std::copy(landed, landed + SPHF_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
