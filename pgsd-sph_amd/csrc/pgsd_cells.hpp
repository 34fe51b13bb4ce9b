// pgsd_cells.hpp -- what every pass over a row list in cell order begins with (pgsd_cells.hip, pgsd_neighbours.hip,
// pgsd_neighbour_list.hip, pgsd_components.hip, pgsd_sph.hip, pgsd_sph_adaptive.hip, pgsd_sph_gradients.hip, pgsd_sph_tensors.hip, pgsd_sph_forces.hip, pgsd_sph_samples.hip): the two kernels, defined in pgsd_cells.hip -- the check of the lists and the CSR
// offsets --, and on the host the refusal of a list, chunk or grid before anything is launched (cells_refuse_grid) and the
// opening sequence on the stream (cells_open_pass), written once for all their launchers.  The refusal protocol is
// order_key_kernel's: a device flag word and a pinned one; every later kernel reads the device flag first and does
// nothing where it is set, and clamps what it derives from the offsets to n.  Seen by the HIP compiler alone.
#ifndef PGSD_CELLS_HPP
#define PGSD_CELLS_HPP

#include "pgsd_kernels.hpp"

namespace pgsd_amd
    {
// lane per entry: a row >= N, an id outside [0, n_cells] or below its predecessor raises both flag words.  rows: null
// where there are no rows to check
__global__ __launch_bounds__(SEL_THREADS) void cells_check_kernel(const uint32_t* rows, const int32_t* cell, uint64_t n,
                                                                  uint64_t N, uint32_t n_cells, uint32_t* flag_dev,
                                                                  uint32_t* flag_host);
// lane per c in [0, n_cells + 1]: offs[c] = the lower bound of c in cell[0 .. n), by binary search
__global__ __launch_bounds__(SEL_THREADS) void cells_offsets_kernel(const int32_t* cell, uint64_t n, uint32_t n_cells,
                                                                    const uint32_t* flag_dev, uint32_t* offs);

// what a pass over several chunks says of a list the check kernel has refused
inline const char* const cells_refused = "a cell id descends or lies outside [0, n_cells], or an entry of the row list lies outside "
                                         "the chunks (nothing was computed)";

// What a pass over a list of n entries into a chunk of N rows on a grid refuses before it launches anything, with the
// message behind "<what>: "; PGSD_SUCCESS otherwise.
inline int cells_refuse_grid(uint64_t n, uint64_t N, const uint32_t cells[3], uint32_t n_cells, const char* what, std::string* err)
    {
    const auto fail = [=](const char* why) { return launch_fail(err, PGSD_ERROR_INVALID_ARGUMENT, std::string(what) + ": " + why); };
    if (n >= (1ull << 32))
        return fail("a list holds fewer than 2^32 entries");
    if (N >= (1ull << 32))
        return fail("chunks of 2^32 rows or more have no 32-bit row list");
    uint64_t product = 1;
    for (int i = 0; i < 3; i++)
        {
        if (cells[i] < 1 || cells[i] > ORDER_MAX_AXIS_CELLS)
            return fail("every axis takes 1 to 1024 cells");
        product *= cells[i];
        }
    if (product > CELLS_MAX_CELLS || product != n_cells)
        return fail("a grid holds 1 to 2^20 cells");
    return PGSD_SUCCESS;
    }

// How such a pass opens on its stream: the pinned flag cleared, the device flag and `zeroed` (the words the pass adds
// into) set to zero, the check of the lists, the offsets.  Anything else the pass copies in ahead of its first kernel is
// enqueued before this.  The memsets' verdict, or what hipGetLastError() says behind the two launches.
inline hipError_t cells_open_pass(const uint32_t* rows, const int32_t* cell, uint64_t n, uint64_t N, uint32_t n_cells,
                                  uint32_t* flag_dev, uint32_t* host_flag, uint32_t* host_flag_dev, uint32_t* offs, void* zeroed,
                                  size_t zeroed_bytes, hipStream_t stream)
    {
    __atomic_store_n(host_flag, 0u, __ATOMIC_RELEASE);
    hipError_t e = hipMemsetAsync(flag_dev, 0, sizeof(uint32_t), stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(zeroed, 0, zeroed_bytes, stream);
    if (e != hipSuccess)
        return e;
    const dim3 block(SEL_THREADS);
    hipLaunchKernelGGL(cells_check_kernel, dim3((unsigned)((n + SEL_THREADS - 1) / SEL_THREADS)), block, 0, stream, rows, cell, n, N,
                       n_cells, flag_dev, host_flag_dev);
    hipLaunchKernelGGL(cells_offsets_kernel, dim3((n_cells + 2 + SEL_THREADS - 1) / SEL_THREADS), block, 0, stream, cell, n, n_cells,
                       flag_dev, offs);
    return hipGetLastError();
    }
    } // namespace pgsd_amd

#endif
