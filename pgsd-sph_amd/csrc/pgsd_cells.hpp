// pgsd_cells.hpp -- the two kernels every pass over a row list in cell order begins with (defined in pgsd_cells.hip,
// launched from there, from pgsd_neighbours.hip, from pgsd_sph.hip and from pgsd_sph_gradients.hip): the check of the lists
// and the CSR offsets.  The refusal protocol is
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
    } // namespace pgsd_amd

#endif
