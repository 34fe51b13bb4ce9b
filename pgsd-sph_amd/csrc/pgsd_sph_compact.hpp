// pgsd_sph_compact.hpp -- the compaction the SPH kernel gradients (pgsd_sph_gradients.hip) and the SPH gradient tensors
// (pgsd_sph_tensors.hip) share ahead of their pair kernels: one kernel template, instantiated in each unit's own code
// object, so that neither carries a copy of its text.  Seen by the HIP compiler alone.
#ifndef PGSD_SPH_COMPACT_HPP
#define PGSD_SPH_COMPACT_HPP

#include "pgsd_internal.hpp"
#include "pgsd_traverse.hpp"

namespace pgsd_amd
    {
// lane per entry: xs[k] = position[rows[k]] in the chunk's own element type, ms[k] the mass, with a.volume vs[k] = m / rho
// (one float64 division of the stored values) and the velocity as three float64 values (an exact conversion, so that the
// velocity chunk's element type stays out of the pair kernels' template lists; the zero vector where no velocity is
// stored).  Reads the device refusal flag first.
template<bool F64>
__global__ __launch_bounds__(SEL_THREADS) void sphg_compact_kernel(const SphGradientsArgs a, const uint32_t* flag_dev,
                                                                   void* __restrict__ xs, double* __restrict__ ms,
                                                                   double* __restrict__ vs, double* __restrict__ ws)
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
#pragma unroll
    for (int c = 0; c < 3; c++)
        ws[k * 3 + c] = a.velocity ? column_value(a.velocity, a.velocity_f64, row * 3 + c) : 0.0;
    }
    } // namespace pgsd_amd

#endif
