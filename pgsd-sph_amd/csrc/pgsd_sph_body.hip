// pgsd_sph_body.hip -- the SPH body forces on gfx950: what force and torque does the fluid exert on a body?  The first pair
// pass between TWO row lists in cell order on one grid -- the targets b (the body) and the sources f (the fluid) -- and the
// first that sums floats over a list.  Per target the sources of the periodically adjacent cells that lie strictly inside
// the kernel support 2h give the pressure acceleration -sum_f m_f (A_b + A_f) grad_b W_bf and, with a viscosity, Morris'
// laminar viscous acceleration; the force terms m_b * acc and the torque terms r_b x them about a point go into a table,
// and the table's columns are summed in the order of pgsd.hoomd._ordered_sum.
// pgsd.hoomd.sph_body_force is the definition and this file equals it exactly, the floats bit for bit: the grid, the
// support and the ORDER of the candidates are the SPH kernel sums' (pgsd_traverse.hpp), with the sources' positions and
// offsets around the target's position and the target's cell; one pair is the accelerations' (pgsd_sph_forces.hip) with
// i = b from the targets' compaction and j = f from the sources'.
//   cells_check_kernel, cells_offsets_kernel   pgsd_cells.hip's, unchanged, once per list; the refusal flag is shared and
//                          every kernel here reads the device flag first and does nothing where it is set
//   body_compact_kernel<F64>   lane per entry of one list: sphf_compact_kernel's arithmetic -- xs in the chunk's own element
//                          type, m, A = p / (rho*rho), V = m / rho, rho and the velocity as three float64 values
//   body_pair_kernel<F64, KERNEL, VISC>   lane per target: x_b, v_b, A_b, the count and the three or six accumulators in
//                          registers, the candidates by traverse_candidates_around over the sources; then the six or
//                          twelve terms, column-major into the table (+0.0 for a bad target and for one nowhere).  wetted,
//                          pairs and bad go through LDS counters and one 64-bit integer atomic each per workgroup; the
//                          largest pressure force leaves as one partial per workgroup
//   body_tile_kernel       one workgroup per tile of 4096 entries and column: lane k % 256 adds its 16 steps in order, then
//                          stats_wave_sum and (w0 + w1) + (w2 + w3)
//   body_final_kernel      one workgroup per column: lane t adds tiles t, t + 256, ..., then the same tree; workgroup 0
//                          also scans the partials and writes the head of the summary
// No float atomic anywhere, no private (scratch) memory in any instance.  Shared device helpers: pgsd_stats.hpp,
// pgsd_kernels.hpp, pgsd_traverse.hpp; the launcher's host side: pgsd_scratch.hpp and pgsd_cells.hpp.
#include "pgsd_stats.hpp"
#include "pgsd_cells.hpp"
#include "pgsd_traverse.hpp"
#include "pgsd_scratch.hpp"

#include <type_traits>

namespace pgsd_amd
    {
#define BODY_WAVES (SEL_THREADS / 64)
#define BODY_STEPS (SPHB_TILE / SEL_THREADS)
static_assert(SEL_THREADS == 256 && BODY_STEPS == 16, "the tile of the ordered sum is 256 lanes x 16 steps");

// one workgroup's share of the summary: the largest squared pressure force over its targets that have a cell and are not
// bad, with its list position (SPH_NONE: it has none)
struct BodyPartial
    {
    double big;
    uint32_t at;
    uint32_t pad;
    };

// does the norm (v, i) replace (e, k): the larger value, then the smaller position; an empty slot never does
__device__ __forceinline__ bool body_before(double v, uint32_t i, double e, uint32_t k)
    {
    if (i == SPH_NONE)
        return false;
    if (k == SPH_NONE)
        return true;
    return v > e || (v == e && i < k);
    }

__device__ __forceinline__ void body_merge(BodyPartial& p, double big, uint32_t at)
    {
    if (body_before(big, at, p.big, p.at))
        {
        p.big = big;
        p.at = at;
        }
    }

// the rest of the block tree: the four waves' sums
__device__ __forceinline__ double body_block_sum(const double* w)
    {
#pragma clang fp contract(off)
    return (w[0] + w[1]) + (w[2] + w[3]);
    }

// the compacted columns of one list
struct BodyColumns
    {
    void* xs;
    double *ms, *As, *vs, *rhos, *ws;
    };

template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void body_compact_kernel(const SphBodyArgs a, const uint32_t* __restrict__ rows,
                                                                   uint64_t n, const uint32_t* flag_dev, const BodyColumns o)
    {
#pragma clang fp contract(off)
    const uint64_t k = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (k >= n || *flag_dev != 0)
        return;
    const uint64_t row = rows[k];
    if (row >= a.N) // (the check kernel has refused such a list: nothing is loaded for it)
        return;
    compact_position<F64>(a.pos, row, o.xs, k);
    const double m = a.mass ? column_value(a.mass, a.mass_f64, row) : a.mass_default;
    const double rho = a.density ? column_value(a.density, a.density_f64, row) : a.density_default;
    const double p = a.pressure ? column_value(a.pressure, a.pressure_f64, row) : a.pressure_default;
    o.ms[k] = m;
    o.As[k] = p / (rho * rho);
    o.vs[k] = m / rho;
    o.rhos[k] = rho;
#pragma unroll
    for (int c = 0; c < 3; c++)
        o.ws[k * 3 + c] = a.velocity ? column_value(a.velocity, a.velocity_f64, row * 3 + c) : 0.0;
    }

// what the pair kernel reads and writes besides its arguments
struct BodyBuffers
    {
    const uint32_t* offs_s; // the sources' offsets
    const uint32_t* flag_dev;
    BodyColumns t, s;       // the targets' and the sources' compaction
    uint32_t* out_contacts;
    double *out_pressure, *out_viscous;
    double* table;          // 6 or 12 columns of a.n doubles
    unsigned long long* words;
    BodyPartial* part;
    };

// words: the summary in device memory, zeroed by the launcher (words 4 .. 6, wetted, pairs and bad, are added to here)
template<bool F64, int KERNEL, bool VISC>
__global__ __launch_bounds__(SEL_THREADS) void body_pair_kernel(const SphBodyArgs a, const BodyBuffers b)
    {
#pragma clang fp contract(off)
    typedef typename std::conditional<F64, double, float>::type elem_t;
    __shared__ unsigned long long s_count[3];
    __shared__ BodyPartial s_part[BODY_WAVES];
    if (*b.flag_dev != 0)
        return;
    if (threadIdx.x < 3)
        s_count[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t n = a.n;
    const uint64_t k64 = (uint64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t k = (uint32_t)k64; // (n < 2^32)
    const bool live = k64 < n;
    const int32_t c = live ? a.cell[k] : (int32_t)a.n_cells;
    const bool has = live && c >= 0 && (uint32_t)c < a.n_cells;
    const elem_t* xt = (const elem_t*)b.t.xs;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    double a_p0 = 0.0, a_p1 = 0.0, a_p2 = 0.0, a_v0 = 0.0, a_v1 = 0.0, a_v2 = 0.0;
    uint32_t contacts = 0;
    if (has)
        {
        const double inv_h = a.inv_h, eta2 = a.eta2;
        const double Ab = b.t.As[k];
        x0 = (double)xt[(size_t)k * 3 + 0];
        x1 = (double)xt[(size_t)k * 3 + 1];
        x2 = (double)xt[(size_t)k * 3 + 2];
        double vb0 = 0.0, vb1 = 0.0, vb2 = 0.0;
        if constexpr (VISC)
            {
            vb0 = b.t.ws[(size_t)k * 3 + 0];
            vb1 = b.t.ws[(size_t)k * 3 + 1];
            vb2 = b.t.ws[(size_t)k * 3 + 2];
            }
        const double* __restrict__ As = b.s.As;
        const double* __restrict__ ms = b.s.ms;
        const double* __restrict__ vs = b.s.vs;
        const double* __restrict__ ws = b.s.ws;
        traverse_candidates_around((const elem_t*)b.s.xs, b.offs_s, a.n_fluid, x0, x1, x2, (uint32_t)c, traverse_grid(a),
                                   [&](uint32_t j, double dx, double dy, double dz, double d2)
                                   {
#pragma clang fp contract(off)
                                       const double rr = __builtin_sqrt(d2);
                                       const double q = rr * inv_h;
                                       const double F = sphg_factor<KERNEL>(q);
                                       const double e0 = F * dx, e1 = F * dy, e2 = F * dz;
                                       const double S = Ab + As[j];
                                       const double m = ms[j];
                                       contacts = contacts + 1u;
                                       a_p0 = a_p0 + m * (S * e0);
                                       a_p1 = a_p1 + m * (S * e1);
                                       a_p2 = a_p2 + m * (S * e2);
                                       if constexpr (VISC)
                                           {
                                           const double K = (F * d2) / (d2 + eta2);
                                           const double V = vs[j];
                                           const double u0 = ws[(size_t)j * 3 + 0] - vb0, u1 = ws[(size_t)j * 3 + 1] - vb1;
                                           const double u2 = ws[(size_t)j * 3 + 2] - vb2;
                                           a_v0 = a_v0 + V * (K * u0);
                                           a_v1 = a_v1 + V * (K * u1);
                                           a_v2 = a_v2 + V * (K * u2);
                                           }
                                   });
        }
    // (a target without a cell: every value is +0.0, whatever the sign of G)
    const double G = a.G;
    const double p0 = has ? -(G * a_p0) : 0.0, p1 = has ? -(G * a_p1) : 0.0, p2 = has ? -(G * a_p2) : 0.0;
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
    if constexpr (VISC)
        {
        if (has)
            {
            const double Gv = a.Gv, rho = b.t.rhos[k];
            w0 = (Gv * a_v0) / rho;
            w1 = (Gv * a_v1) / rho;
            w2 = (Gv * a_v2) / rho;
            }
        }
    if (live)
        {
        if (b.out_contacts)
            b.out_contacts[k] = contacts;
        if (b.out_pressure)
            {
            b.out_pressure[(size_t)k * 3 + 0] = p0;
            b.out_pressure[(size_t)k * 3 + 1] = p1;
            b.out_pressure[(size_t)k * 3 + 2] = p2;
            }
        if constexpr (VISC)
            {
            if (b.out_viscous)
                {
                b.out_viscous[(size_t)k * 3 + 0] = w0;
                b.out_viscous[(size_t)k * 3 + 1] = w1;
                b.out_viscous[(size_t)k * 3 + 2] = w2;
                }
            }
        }
    // the force and torque terms of this target: fp, [fv,] tp, [tv]
    constexpr int C = VISC ? 12 : 6;
    double term[C];
#pragma unroll
    for (int t = 0; t < C; t++)
        term[t] = 0.0;
    bool bad = false;
    BodyPartial p = {0.0, SPH_NONE, 0};
    if (has)
        {
        // the arm: the single-shift minimum image of x_b - about (pgsd.hoomd.pair_displacement(about, x_b)), z first
        const double Lx = a.vectors[0], Ly = a.vectors[1], Lz = a.vectors[2];
        double r0 = x0 - a.about[0], r1 = x1 - a.about[1], r2 = 0.0;
        if (a.dims != 2)
            {
            r2 = x2 - a.about[2];
            const bool up = r2 >= Lz * 0.5, down = r2 < -(Lz * 0.5);
            r0 = up ? r0 - a.vectors[4] : (down ? r0 + a.vectors[4] : r0);
            r1 = up ? r1 - a.vectors[5] : (down ? r1 + a.vectors[5] : r1);
            r2 = up ? r2 - Lz : (down ? r2 + Lz : r2);
            }
            {
            const bool up = r1 >= Ly * 0.5, down = r1 < -(Ly * 0.5);
            r0 = up ? r0 - a.vectors[3] : (down ? r0 + a.vectors[3] : r0);
            r1 = up ? r1 - Ly : (down ? r1 + Ly : r1);
            }
            {
            const bool up = r0 >= Lx * 0.5, down = r0 < -(Lx * 0.5);
            r0 = up ? r0 - Lx : (down ? r0 + Lx : r0);
            }
        const double mb = b.t.ms[k];
        const double fp0 = mb * p0, fp1 = mb * p1, fp2 = mb * p2;
        constexpr int TP = VISC ? 6 : 3;
        term[0] = fp0;
        term[1] = fp1;
        term[2] = fp2;
        term[TP + 0] = r1 * fp2 - r2 * fp1;
        term[TP + 1] = r2 * fp0 - r0 * fp2;
        term[TP + 2] = r0 * fp1 - r1 * fp0;
        if constexpr (VISC)
            {
            const double fv0 = mb * w0, fv1 = mb * w1, fv2 = mb * w2;
            term[3] = fv0;
            term[4] = fv1;
            term[5] = fv2;
            term[9] = r1 * fv2 - r2 * fv1;
            term[10] = r2 * fv0 - r0 * fv2;
            term[11] = r0 * fv1 - r1 * fv0;
            }
        const double inf = __builtin_huge_val();
#pragma unroll
        for (int t = 0; t < C; t++)
            bad = bad || !(__builtin_fabs(term[t]) < inf);
        // (a NaN passes no compare: it is no largest norm -- and a bad target is none either)
        const double norm2 = (fp0 * fp0 + fp1 * fp1) + fp2 * fp2;
        if (!bad && norm2 == norm2)
            {
            p.big = norm2;
            p.at = k;
            }
        }
    if (live)
        {
#pragma unroll
        for (int t = 0; t < C; t++)
            b.table[(size_t)t * n + k] = bad ? 0.0 : term[t];
        }
    const uint64_t wetted = stats_wave_count(has && contacts >= 1u ? 1u : 0u);
    const uint64_t pairs = stats_wave_count(has ? (uint64_t)contacts : 0u);
    const uint64_t n_bad = stats_wave_count(bad ? 1u : 0u);
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1)
        {
        const double big = __shfl_xor(p.big, h, 64);
        const uint32_t at = __shfl_xor(p.at, h, 64);
        body_merge(p, big, at);
        }
    if ((threadIdx.x & 63) == 0)
        {
        s_part[threadIdx.x >> 6] = p;
        if (wetted)
            atomicAdd(&s_count[0], (unsigned long long)wetted);
        if (pairs)
            atomicAdd(&s_count[1], (unsigned long long)pairs);
        if (n_bad)
            atomicAdd(&s_count[2], (unsigned long long)n_bad);
        }
    __syncthreads();
    if (threadIdx.x == 0)
        {
        BodyPartial q = s_part[0];
#pragma unroll
        for (int w = 1; w < BODY_WAVES; w++)
            body_merge(q, s_part[w].big, s_part[w].at);
        b.part[blockIdx.x] = q;
        }
    if (threadIdx.x < 3 && s_count[threadIdx.x])
        atomicAdd(&b.words[4 + threadIdx.x], s_count[threadIdx.x]);
    }

// One workgroup per (tile, column): sums[column * n_tiles + tile] = the tile's sum in the order of _ordered_sum; entries
// behind the list's end count as +0.0
__global__ __launch_bounds__(SEL_THREADS) void body_tile_kernel(const double* __restrict__ table, uint64_t n, uint32_t n_tiles,
                                                                const uint32_t* flag_dev, double* __restrict__ sums)
    {
#pragma clang fp contract(off)
    __shared__ double s_wave[BODY_WAVES];
    if (*flag_dev != 0)
        return;
    const uint32_t tile = blockIdx.x, column = blockIdx.y;
    const double* __restrict__ v = table + (size_t)column * n;
    const uint64_t base = (uint64_t)tile * SPHB_TILE + threadIdx.x;
    double sum = 0.0;
#pragma unroll
    for (int s = 0; s < BODY_STEPS; s++)
        {
        const uint64_t at = base + (uint64_t)s * SEL_THREADS;
        sum = sum + (at < n ? v[at] : 0.0);
        }
    sum = stats_wave_sum(sum);
    if ((threadIdx.x & 63) == 0)
        s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        sums[(size_t)column * n_tiles + tile] = body_block_sum(s_wave);
    }

// One workgroup per column of the table.  The words: the targets, those nowhere, the sources, those nowhere, (wetted,
// pairs, bad: the pair kernel's), the list position, the row and as a bit pattern the squared norm of the largest pressure
// force, then as bit patterns the twelve sums -- without a viscosity the table's six columns are words 10 .. 12 and
// 16 .. 18 and the launcher's zeros stand in the other six.
__global__ __launch_bounds__(SEL_THREADS) void body_final_kernel(const SphBodyArgs a, const uint32_t* __restrict__ offs_t,
                                                                 const uint32_t* __restrict__ offs_s, const uint32_t* flag_dev,
                                                                 const double* __restrict__ sums, uint32_t n_tiles,
                                                                 const BodyPartial* __restrict__ part, uint32_t n_parts,
                                                                 unsigned long long* __restrict__ words)
    {
#pragma clang fp contract(off)
    __shared__ double s_wave[BODY_WAVES];
    __shared__ BodyPartial s_part[SEL_THREADS];
    if (*flag_dev != 0)
        return;
    const uint32_t column = blockIdx.x;
    const double* __restrict__ t_sum = sums + (size_t)column * n_tiles;
    double sum = 0.0;
#pragma unroll 8
    for (uint32_t t = threadIdx.x; t < n_tiles; t += SEL_THREADS)
        sum = sum + t_sum[t];
    sum = stats_wave_sum(sum);
    if ((threadIdx.x & 63) == 0)
        s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
        {
        const uint32_t slot = a.viscous ? column : (column < 3 ? column : column + 3);
        words[10 + slot] = (unsigned long long)__double_as_longlong(body_block_sum(s_wave));
        }
    if (column != 0)
        return;
    BodyPartial p = {0.0, SPH_NONE, 0};
    for (uint32_t t = threadIdx.x; t < n_parts; t += SEL_THREADS)
        body_merge(p, part[t].big, part[t].at);
    s_part[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    for (uint32_t t = 1; t < SEL_THREADS; t++)
        body_merge(p, s_part[t].big, s_part[t].at);
    const uint64_t n = a.n, n_s = a.n_fluid;
    words[0] = n;
    words[1] = n - min((uint64_t)offs_t[a.n_cells], n);
    words[2] = n_s;
    words[3] = n_s - min((uint64_t)offs_s[a.n_cells], n_s);
    const bool any = p.at != SPH_NONE && p.at < n;
    words[7] = any ? p.at : SPH_NONE;
    words[8] = any ? a.rows[p.at] : SPH_NONE;
    words[9] = (unsigned long long)__double_as_longlong(any ? p.big : 0.0);
    }

// ------------------------------------------------------------------ host side
namespace
    {
// The family's scratch space (grow-only, per device, its own lock held), in bytes: the device flag word (16), the offsets
// of both lists (n_cells + 2 words each), per list the compacted positions (3 elements per entry), masses, A values,
// volumes and densities (one double each) and velocities (3 doubles), the table (6 or 12 doubles per target), the tiles'
// sums, the partials (one per workgroup) and the summary; the pinned flag word is the host's view of a refused list, the
// pinned host block the landing place of the summary.
constexpr size_t BODY_SUMMARY_BYTES = (size_t)SPHB_SUMMARY_WORDS * sizeof(uint64_t);
Scratch g_body_scratch("SPH body forces", 1.25, 1u << 16, BODY_SUMMARY_BYTES, sizeof(uint64_t));
std::mutex g_body_lock;

// what the compaction of a list of n entries occupies
size_t body_list_bytes(uint64_t n, bool f64)
    {
    return round16((size_t)n * 3 * (f64 ? sizeof(double) : sizeof(float))) + 4 * round16((size_t)n * sizeof(double))
           + round16((size_t)n * 3 * sizeof(double));
    }

// the compaction of a list of n entries from `at` on; *bytes: what it occupies (body_list_bytes)
BodyColumns body_columns(char* at, uint64_t n, bool f64, size_t* bytes)
    {
    const size_t xs_bytes = round16((size_t)n * 3 * (f64 ? sizeof(double) : sizeof(float)));
    const size_t col_bytes = round16((size_t)n * sizeof(double));
    const size_t vel_bytes = round16((size_t)n * 3 * sizeof(double));
    BodyColumns c;
    c.xs = at;
    c.ms = (double*)(at + xs_bytes);
    c.As = (double*)(at + xs_bytes + col_bytes);
    c.vs = (double*)(at + xs_bytes + 2 * col_bytes);
    c.rhos = (double*)(at + xs_bytes + 3 * col_bytes);
    c.ws = (double*)(at + xs_bytes + 4 * col_bytes);
    *bytes = xs_bytes + 4 * col_bytes + vel_bytes;
    return c;
    }

template<bool F64, int KERNEL>
void body_launch_pair(bool visc, dim3 grid, dim3 block, hipStream_t stream, const SphBodyArgs& a, const BodyBuffers& b)
    {
    if (visc)
        hipLaunchKernelGGL((body_pair_kernel<F64, KERNEL, true>), grid, block, 0, stream, a, b);
    else
        hipLaunchKernelGGL((body_pair_kernel<F64, KERNEL, false>), grid, block, 0, stream, a, b);
    }
    } // namespace

void warm_sph_body_kernels()
    {
    warm_kernel((const void*)body_pair_kernel<false, SPH_WENDLAND_C2, true>);
    }

int launch_sph_body_force(const SphBodyArgs& a, uint32_t* out_contacts, double* out_pressure_acc, double* out_viscous_acc,
                          uint64_t* out_summary, hipStream_t stream, std::string* err)
    {
    static const char* what = "SPH body forces";
    const auto fail = [err](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (!out_summary)
        return PGSD_ERROR_INVALID_ARGUMENT;
    int rc = cells_refuse_grid(a.n, a.N, a.cells, a.n_cells, what, err);
    if (rc == PGSD_SUCCESS)
        rc = cells_refuse_grid(a.n_fluid, a.N, a.cells, a.n_cells, what, err);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (a.kernel != SPH_WENDLAND_C2 && a.kernel != SPH_CUBIC_SPLINE)
        return fail("the kernel is 0 (Wendland C2) or 1 (cubic spline)");
    const uint64_t n = a.n, n_s = a.n_fluid;
    if (n == 0)
        {
        sph_body_force_of_nothing(n_s, out_summary);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return fail(cells_refused);
    if (!a.rows || !a.cell || !a.pos || (n_s > 0 && (!a.fluid_rows || !a.fluid_cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const uint32_t C = a.viscous ? 12u : 6u;
    const uint32_t t_blocks = (uint32_t)((n + SEL_THREADS - 1) / SEL_THREADS);
    const uint32_t s_blocks = (uint32_t)((n_s + SEL_THREADS - 1) / SEL_THREADS);
    const uint32_t n_tiles = (uint32_t)((n + SPHB_TILE - 1) / SPHB_TILE);
    const size_t offs_bytes = round16(((size_t)a.n_cells + 2) * sizeof(uint32_t));
    size_t t_bytes = body_list_bytes(n, a.f64 != 0), s_bytes = body_list_bytes(n_s, a.f64 != 0);
    const size_t table_bytes = round16((size_t)n * C * sizeof(double));
    const size_t sums_bytes = round16((size_t)n_tiles * C * sizeof(double));
    const size_t part_bytes = round16((size_t)t_blocks * sizeof(BodyPartial));
    const size_t words_bytes = BODY_SUMMARY_BYTES;
    LaunchScope scope(g_body_lock, g_body_scratch,
                      16 + 2 * offs_bytes + t_bytes + s_bytes + table_bytes + sums_bytes + part_bytes + words_bytes, stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    char* dev = scope.mem().dev;
    uint32_t* flag_dev = (uint32_t*)dev;
    uint32_t* offs_t = (uint32_t*)(dev + 16);
    uint32_t* offs_s = (uint32_t*)(dev + 16 + offs_bytes);
    char* at = dev + 16 + 2 * offs_bytes;
    const BodyColumns ct = body_columns(at, n, a.f64 != 0, &t_bytes);
    const BodyColumns cs = body_columns(at + t_bytes, n_s, a.f64 != 0, &s_bytes);
    double* table = (double*)(at + t_bytes + s_bytes);
    double* sums = (double*)((char*)table + table_bytes);
    BodyPartial* part = (BodyPartial*)((char*)sums + sums_bytes);
    unsigned long long* words = (unsigned long long*)((char*)part + part_bytes);
    uint32_t* host_flag = (uint32_t*)scope.mem().mapped;
    uint32_t* host_flag_dev = (uint32_t*)scope.mem().mapped_dev;
    const dim3 block(SEL_THREADS), per_target(t_blocks), per_source(s_blocks);
    const bool visc = a.viscous != 0;
    const BodyBuffers b = {offs_s, flag_dev, ct, cs, out_contacts, out_pressure_acc, out_viscous_acc, table, words, part};
    // the targets open the pass; the sources' check and offsets follow under the same flag words
    hipError_t e = cells_open_pass(a.rows, a.cell, n, a.N, a.n_cells, flag_dev, host_flag, host_flag_dev, offs_t, words, words_bytes,
                                   stream);
    if (e == hipSuccess)
        {
        if (n_s > 0)
            hipLaunchKernelGGL(cells_check_kernel, per_source, block, 0, stream, a.fluid_rows, a.fluid_cell, n_s, a.N, a.n_cells,
                               flag_dev, host_flag_dev);
        // (a list of no entry: every offset is 0 and every target is dry)
        hipLaunchKernelGGL(cells_offsets_kernel, dim3((a.n_cells + 2 + SEL_THREADS - 1) / SEL_THREADS), block, 0, stream,
                           a.fluid_cell, n_s, a.n_cells, flag_dev, offs_s);
        if (a.f64)
            {
            hipLaunchKernelGGL(body_compact_kernel<true>, per_target, block, 0, stream, a, a.rows, n, flag_dev, ct);
            if (n_s > 0)
                hipLaunchKernelGGL(body_compact_kernel<true>, per_source, block, 0, stream, a, a.fluid_rows, n_s, flag_dev, cs);
            if (a.kernel == SPH_WENDLAND_C2)
                body_launch_pair<true, SPH_WENDLAND_C2>(visc, per_target, block, stream, a, b);
            else
                body_launch_pair<true, SPH_CUBIC_SPLINE>(visc, per_target, block, stream, a, b);
            }
        else
            {
            hipLaunchKernelGGL(body_compact_kernel<false>, per_target, block, 0, stream, a, a.rows, n, flag_dev, ct);
            if (n_s > 0)
                hipLaunchKernelGGL(body_compact_kernel<false>, per_source, block, 0, stream, a, a.fluid_rows, n_s, flag_dev, cs);
            if (a.kernel == SPH_WENDLAND_C2)
                body_launch_pair<false, SPH_WENDLAND_C2>(visc, per_target, block, stream, a, b);
            else
                body_launch_pair<false, SPH_CUBIC_SPLINE>(visc, per_target, block, stream, a, b);
            }
        hipLaunchKernelGGL(body_tile_kernel, dim3(n_tiles, C), block, 0, stream, table, n, n_tiles, flag_dev, sums);
        hipLaunchKernelGGL(body_final_kernel, dim3(C), block, 0, stream, a, offs_t, offs_s, flag_dev, sums, n_tiles, part, t_blocks,
                           words);
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
    std::copy(landed, landed + SPHB_SUMMARY_WORDS, out_summary);
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
