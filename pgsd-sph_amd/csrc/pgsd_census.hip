// pgsd_census.hip -- the domain census on gfx950 (which decomposition to ask for):
//   axis_hist_kernel / cell_count_kernel   the selections' fractions binned per axis / counted per cell of a rectilinear
//                          grid, in LDS counters flushed with integer atomics
// Shared device helpers: pgsd_select.hpp (the fraction, the rows of a lane), pgsd_kernels.hpp; the launchers' host side:
// pgsd_scratch.hpp.
#include "pgsd_select.hpp"
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
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

    } // namespace pgsd_amd

using namespace pgsd_amd;

namespace
    {
// per device (g_select_lock held): the global counters (3 x CENSUS_MAX_BINS words, which also hold CENSUS_MAX_CELLS + 1)
// and their pinned landing place on the host -- one size for every call, so the allocation never grows
constexpr size_t CENSUS_WORDS = 3 * CENSUS_MAX_BINS;
static_assert(CENSUS_MAX_CELLS + 1 <= CENSUS_WORDS, "the cell counters share the histogram's room");
Scratch g_census_scratch("domain census", 1.0, 0, CENSUS_WORDS * sizeof(uint32_t), 0, "the counters");

// the grid cap of a pass on `device`: 2 x compute units, remembered for the device of the last call (g_select_lock held)
unsigned census_max_blocks(int device)
    {
    static int known = -1;
    static unsigned max_blocks = 0;
    if (device != known)
        {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1)
            cus = 256;
        max_blocks = 2u * (unsigned)cus;
        known = device;
        }
    return max_blocks;
    }
    } // namespace

namespace pgsd_amd
    {
void warm_census_kernels()
    {
    warm_kernel((const void*)axis_hist_kernel<false>);
    }

// One census pass over N rows (0 < N < 2^32) on `stream`: `words` global counters zeroed, `launch(blocks, tiles,
// counters)` enqueues the kernel over min(tiles, 2 x compute units) workgroups, the counters land in pinned memory and
// -- after the one stream wait -- in out[0 .. words) as 64-bit counts.
template<class Launch>
static int census_pass(uint64_t N, size_t words, const char* what, uint64_t* out, hipStream_t stream, std::string* err,
                       Launch launch)
    {
    LaunchScope scope(g_select_lock, g_census_scratch, CENSUS_WORDS * sizeof(uint32_t), stream, err);
    if (scope.rc() != PGSD_SUCCESS)
        return scope.rc();
    uint32_t* counters = (uint32_t*)scope.mem().dev;
    const uint32_t* landed = (const uint32_t*)scope.mem().host;
    const uint64_t n_tiles = (N + SEL_PER_BLOCK - 1) / SEL_PER_BLOCK;
    const dim3 grid((unsigned)std::min<uint64_t>(n_tiles, census_max_blocks(scope.device())));
    hipError_t e = hipMemsetAsync(counters, 0, words * sizeof(uint32_t), stream);
    if (e == hipSuccess)
        {
        launch(grid, n_tiles, counters);
        e = hipGetLastError();
        }
    if (e == hipSuccess)
        e = hipMemcpyAsync(scope.mem().host, counters, words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    const int rc = scope.finish(what, e);
    if (rc != PGSD_SUCCESS)
        return rc;
    for (size_t i = 0; i < words; i++)
        out[i] = landed[i];
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
                       [&](dim3 grid, uint64_t n_tiles, uint32_t* hist)
                       { PGSD_LAUNCH_BY_F64(d.f64, axis_hist_kernel, grid, stream, d, bins, n_tiles, hist); });
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
                         [&](dim3 grid, uint64_t n_tiles, uint32_t* counts)
                         { PGSD_LAUNCH_BY_F64(c.d.f64, cell_count_kernel, grid, stream, c, n_tiles, counts); });
    if (rc != PGSD_SUCCESS)
        return rc;
    std::copy(all.begin(), all.begin() + n_cells, out_counts);
    *out_nowhere = all[n_cells];
    return PGSD_SUCCESS;
    }
    } // namespace pgsd_amd
