// pgsd_select.hpp -- the device helpers the units of the selection family share, and the map of those units.  (The
// file-map comment at the top of pgsd_kernels.hpp predates the split and is left alone: that header's bytes tell the
// benchmark whether its recorded pack traffic still describes the pack kernels.)
//   pgsd_pack.hip / pgsd_unpack.hip   the write path's pack kernels, the read path's inverse kernels, their planners
//   pgsd_compare.hip   packed chunk == reference rows?  the write path's elision (compare_bytes_kernel)
//   pgsd_select.hip    stream compaction: the flag compaction of pgsd_select_rows, the predicate selections (domain,
//                      ghost layer, particle group) and the row plan of sparse indexed reads -- everything that ends
//                      in the one-block scan and lives in the compaction scratch
//   pgsd_census.hip    the domain census: axis histograms and cell counts
//   pgsd_order.hip     cell order: keys, a stable radix sort, the pass that applies the permutation
//   pgsd_stats.hip     frame statistics; conservation sums and frame displacements on one final kernel and launcher
//   pgsd_cells.hip     cell fields: the conservation sums' values per grid cell of a list in cell order, CSR offsets
//   pgsd_neighbours.hip   the neighbour census: counts, nearest pair and pair histogram inside a range, over the runs
//                      of adjacent cells of a list in cell order (pgsd_cells.hpp: the check and offsets kernels it shares)
//   pgsd_neighbour_list.hip   neighbour lists: the census' neighbours as a CSR pair list -- count over the same traversal,
//                      one-workgroup scan, offsets, fill inside the segments
//   pgsd_components.hip   components: the connected components of the half list's pairs -- a lock-free union-find over
//                      the same traversal, a flatten pass, the roots numbered by the same scan (pgsd_scan.hpp)
//   pgsd_component_moments.hip   component fields: the cell fields' segmented sums per component -- the entries sorted by
//                      dense id with the cell order's radix sort, the position as the displacement from the component's root
//   pgsd_sph.hip       the SPH kernel sums: summation density, number density and Shepard sum inside the support 2h, in
//                      a defined order of the candidates (the same check and offsets kernels)
//   pgsd_sph_gradients.hip   the SPH kernel gradients: density rate, velocity divergence and curl and the colour gradient
//                      over the same support in the same order (pgsd_traverse.hpp: the traversal as an inlined template,
//                      which the pair units walk their candidates through)
//   pgsd_sph_adaptive.hip   the SPH sums with a per-particle smoothing length: the neighbour count, the three sums and the
//                      grad-h factor over the support 2 h_i or h_i + h_j, on the grid of the declared bound 2 h_max
//   pgsd_sph_tensors.hip   the SPH gradient tensors: the kernel-gradient correction matrix, the corrected velocity gradient
//                      and the shear rate over the same support in the same order (pgsd_sph_compact.hpp: the compaction
//                      kernel it shares with the gradients)
//   pgsd_sph_forces.hip   the SPH accelerations: pressure and laminar viscous acceleration and their sum with gravity
//                      over the same support in the same order, the largest of each with its row
//   pgsd_sph_samples.hip   the SPH samples: the interpolant of the list at points of the caller's choosing, the same
//                      candidates in the same order around the point's cell
//   pgsd_stats.hpp     what the two reduction units share: an element as a double, the wave tree, the wave counter
//   pgsd_device_memory.cpp   pgsd_device_alloc / _free / _copy: device memory owned by the library (no kernel)
//   pgsd_scratch.hpp / .cpp  the host side all of them stand on: scratch space, launch scope, device scope
//   pgsd_kernels.hpp / .cpp  row layout (SEL_THREADS ...), vector types, tuning, what the pack and unpack kernels share
// Here: the 64-lane scan of the compactions and the radix sort; and the fractional coordinate every spatial kernel
// derives from a position row -- domain_skew(), then domain_wrap() per axis, in float64 without contraction, in the
// operation order of pgsd.hoomd.domain_rows.  The selections compare the wrapped fraction f with a cell's bounds
// (domain_inside()); the census and the ordering kernels bin it instead and restate two rules: f * bins (or cells) is
// converted to an integer only after the test f == f, and a row with a NaN fraction on any axis belongs to no bin
// ("nowhere").  Seen by the HIP compiler alone.
#ifndef PGSD_SELECT_HPP
#define PGSD_SELECT_HPP

#include "pgsd_kernels.hpp"

#ifdef __HIP__
namespace pgsd_amd
    {
// kernel<true> where the positions are float64, kernel<false> where they are float32; workgroups of SEL_THREADS lanes
#define PGSD_LAUNCH_BY_F64(f64, kernel, grid, stream, ...)                                      \
    do                                                                                          \
        {                                                                                       \
        if (f64)                                                                                \
            hipLaunchKernelGGL(kernel<true>, grid, dim3(SEL_THREADS), 0, stream, __VA_ARGS__);  \
        else                                                                                    \
            hipLaunchKernelGGL(kernel<false>, grid, dim3(SEL_THREADS), 0, stream, __VA_ARGS__); \
        }                                                                                       \
    while (0)

// inclusive scan of one value per lane across the 64-lane wavefront
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x)
    {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
        {
        uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d)
            x += y;
        }
    return x;
    }

// (the two halves of the fraction, shared with the ghost layer's halo_class())
__device__ __forceinline__ void domain_skew(const DomainArgs& d, double x, double y, double z, double s[3])
    {
#pragma clang fp contract(off)
    s[0] = ((x + d.L[0] / 2.0) - ((d.xz - d.yz * d.xy) * z + d.xy * y)) / d.L[0];
    s[1] = ((y + d.L[1] / 2.0) - d.yz * z) / d.L[1];
    s[2] = (z + d.L[2] / 2.0) / d.L[2];
    }

__device__ __forceinline__ double domain_wrap(double s)
    {
#pragma clang fp contract(off)
    double f = s - floor(s);
    if (f >= 1.0)
        f = 0.0;
    return f;
    }

__device__ __forceinline__ bool domain_inside(const DomainArgs& d, double x, double y, double z)
    {
#pragma clang fp contract(off)
    double s[3];
    domain_skew(d, x, y, z, s);
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; a++)
        {
        if (a == 2 && d.dims == 2)
            break;
        const double f = domain_wrap(s[a]);
        in = in && d.lo[a] <= f && f < d.hi[a];
        }
    return in;
    }

// the SEL_PER_THREAD rows of this lane as doubles (zeros past the end): rows base + k * SEL_THREADS + threadIdx.x
template<bool F64>
__device__ __forceinline__ void domain_load_rows(const void* pos, uint64_t N, uint64_t base, double p[SEL_PER_THREAD][3])
    {
#pragma unroll
    for (int k = 0; k < SEL_PER_THREAD; k++)
        {
        const uint64_t i = base + (uint64_t)k * SEL_THREADS + threadIdx.x;
        p[k][0] = p[k][1] = p[k][2] = 0.0;
        if (i < N)
            {
            if constexpr (F64)
                {
                const double* q = (const double*)pos + i * 3;
                p[k][0] = __builtin_nontemporal_load(q);
                p[k][1] = __builtin_nontemporal_load(q + 1);
                p[k][2] = __builtin_nontemporal_load(q + 2);
                }
            else
                {
                const u32x3 v = __builtin_nontemporal_load((const u32x3_a4*)((const uint32_t*)pos + i * 3));
                p[k][0] = (double)__uint_as_float(v.x);
                p[k][1] = (double)__uint_as_float(v.y);
                p[k][2] = (double)__uint_as_float(v.z);
                }
            }
        }
    }
    } // namespace pgsd_amd
#endif // __HIP__

#endif
