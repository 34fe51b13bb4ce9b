// pgsd_traverse.hpp -- the traversal of the candidates of one entry of a row list in cell order, as one inlined device
// template over a per-candidate functor: the cells of pgsd.hoomd.sph_kernel_sums' defined order (oz over the offsets of
// the z axis -- {0} at one cell, {0, +1} at two, {-1, 0, +1} otherwise --, inside it oy, inside it ox, the cell ((ix+ox) %
// cx, (iy+oy) % cy, (iz+oz) % cz), inside a cell ascending list position), taken as at most two cyclic x-runs per (y, z)
// row of the grid; the clamping of what comes from the offsets to n; HOOMD's single-shift minimum image in float64
// without contraction (pgsd.hoomd.pair_displacement) and the strict test d2 < r2.  The functor receives (j, dx, dy, dz, d2)
// of every candidate that passes, in the defined order, and is inlined with what it captures: accumulators it holds by
// reference stay in registers.  With it what the compact kernels of the same units share: the copy of one position row
// into xs and the read of one column value -- and what the weighted units share, the weight w(q) and the factor F(q).
// traverse_candidates_around takes the centre from its caller -- a point that is no entry of the list (pgsd_sph_samples.hip)
// --, traverse_candidates loads entry k's position and forwards to it.  Used by pgsd_neighbours.hip,
// pgsd_neighbour_list.hip, pgsd_components.hip, pgsd_sph.hip, pgsd_sph_adaptive.hip, pgsd_sph_gradients.hip, pgsd_sph_tensors.hip, pgsd_sph_forces.hip and pgsd_sph_samples.hip, which carry
// no copy of any of it.  Seen by the HIP compiler alone.
#ifndef PGSD_TRAVERSE_HPP
#define PGSD_TRAVERSE_HPP

#include "pgsd_kernels.hpp"

namespace pgsd_amd
    {
// what the traversal reads besides the compacted positions and the offsets
struct TraverseGrid
    {
    double vectors[6]; // Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz
    double r2;
    uint32_t cells[3];
    uint32_t dims;
    };

// the grid of a family's argument struct (NeighboursArgs, SphArgs, SphAdaptiveArgs, SphGradientsArgs, SphTensorsArgs, SphForcesArgs, SphSamplesArgs)
template<typename Args> __device__ __forceinline__ TraverseGrid traverse_grid(const Args& a)
    {
    TraverseGrid g;
#pragma unroll
    for (int i = 0; i < 6; i++)
        g.vectors[i] = a.vectors[i];
    g.r2 = a.r2;
#pragma unroll
    for (int i = 0; i < 3; i++)
        g.cells[i] = a.cells[i];
    g.dims = a.dims;
    return g;
    }

// xs[k] = pos[row], three elements of the chunk's own type (float32 as one 12-byte word triple)
template<bool F64> __device__ __forceinline__ void compact_position(const void* pos, uint64_t row, void* __restrict__ xs, uint64_t k)
    {
    if constexpr (F64)
        {
        const double* q = (const double*)pos + row * 3;
        double* o = (double*)xs + k * 3;
        o[0] = q[0];
        o[1] = q[1];
        o[2] = q[2];
        }
    else
        {
        const u32x3 v = *(const u32x3_a4*)((const uint32_t*)pos + row * 3);
        *(u32x3_a4*)((uint32_t*)xs + k * 3) = v;
        }
    }

// one value of a float32 or float64 column as a double (exact)
__device__ __forceinline__ double column_value(const void* base, uint32_t f64, uint64_t at)
    {
    return f64 ? ((const double*)base)[at] : (double)((const float*)base)[at];
    }

// F(q) = (1/q) dw/dq of pgsd.hoomd.sph_gradient_factor: the operations as written there, one rounding each; only the
// spline's outer branch divides.  What the functors of pgsd_sph_gradients.hip and pgsd_sph_forces.hip form e = F * d with.
template<int KERNEL> __device__ __forceinline__ double sphg_factor(double q)
    {
#pragma clang fp contract(off)
    if constexpr (KERNEL == SPH_WENDLAND_C2)
        {
        const double t = 1.0 - 0.5 * q;
        return -5.0 * ((t * t) * t);
        }
    else
        {
        if (q < 1.0)
            return 2.25 * q - 3.0;
        const double u = 2.0 - q;
        return (-0.75 * (u * u)) / q;
        }
    }

// w(q) of pgsd.hoomd.sph_weight: the operations as written there, one rounding each.  What the functors of pgsd_sph.hip
// and pgsd_sph_samples.hip weigh a candidate with.
template<int KERNEL> __device__ __forceinline__ double sph_weight(double q)
    {
#pragma clang fp contract(off)
    if constexpr (KERNEL == SPH_WENDLAND_C2)
        {
        const double t = 1.0 - 0.5 * q;
        const double t2 = t * t;
        return (t2 * t2) * (2.0 * q + 1.0);
        }
    else
        {
        const double q2 = q * q;
        if (q < 1.0)
            return (1.0 - 1.5 * q2) + 0.75 * (q2 * q);
        const double u = 2.0 - q;
        return 0.25 * ((u * u) * u);
        }
    }

// The traversal with the centre handed in: xs: n x 3 compacted positions of element type elem_t; offs: n_cells + 1 CSR
// offsets; (xi0, xi1, xi2): the centre, a list entry's position or a point of the caller's; c: its cell id, inside
// [0, n_cells)
template<typename elem_t, typename Functor>
__device__ __forceinline__ void traverse_candidates_around(const elem_t* __restrict__ x, const uint32_t* __restrict__ offs,
                                                           uint64_t n, const double xi0, const double xi1, const double xi2,
                                                           uint32_t c, const TraverseGrid& g, Functor&& each)
    {
#pragma clang fp contract(off)
    const double Lx = g.vectors[0], Ly = g.vectors[1], Lz = g.vectors[2];
    const double xyLy = g.vectors[3], xzLz = g.vectors[4], yzLz = g.vectors[5];
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5; // (exact halves)
    const double r2 = g.r2;
    const bool three = g.dims != 2;
    const int cx = (int)g.cells[0], cy = (int)g.cells[1], cz = (int)g.cells[2];
    const int ix = (int)(c % (uint32_t)cx), iy = (int)((c / (uint32_t)cx) % (uint32_t)cy);
    const int iz = (int)(c / ((uint32_t)cx * (uint32_t)cy));
    // the x cells in the defined order: `take` cells cyclically from `from`, as run 0 [from, b0) and run 1 [0, b1)
    const int take = min(3, cx);
    const int from = cx == 1 ? 0 : (cx == 2 ? ix : (ix == 0 ? cx - 1 : ix - 1));
    const int b0 = min(from + take, cx), b1 = max(from + take - cx, 0);
    const int ylo = cy >= 3 ? -1 : 0, yhi = cy >= 2 ? 1 : 0;
    const int zlo = cz >= 3 ? -1 : 0, zhi = cz >= 2 ? 1 : 0;
    for (int oz = zlo; oz <= zhi; oz++)
        {
        int wz = iz + oz;
        wz = wz < 0 ? wz + cz : (wz >= cz ? wz - cz : wz);
        for (int oy = ylo; oy <= yhi; oy++)
            {
            int wy = iy + oy;
            wy = wy < 0 ? wy + cy : (wy >= cy ? wy - cy : wy);
            const uint32_t row0 = (uint32_t)cx * ((uint32_t)wy + (uint32_t)cy * (uint32_t)wz);
            for (int run = 0; run < 2; run++)
                {
                const int ra = run ? 0 : from, rb = run ? b1 : b0;
                if (rb <= ra)
                    continue;
                const uint32_t lo = (uint32_t)min((uint64_t)offs[row0 + (uint32_t)ra], n);
                const uint32_t hi = (uint32_t)min((uint64_t)offs[row0 + (uint32_t)rb], n);
                for (uint32_t j = lo; j < hi; j++)
                    {
                    const double xj0 = (double)x[(size_t)j * 3 + 0], xj1 = (double)x[(size_t)j * 3 + 1];
                    double dx = xj0 - xi0, dy = xj1 - xi1, dz = 0.0;
                    if (three)
                        {
                        dz = (double)x[(size_t)j * 3 + 2] - xi2;
                        const bool up = dz >= hz, down = dz < -hz;
                        dx = up ? dx - xzLz : (down ? dx + xzLz : dx);
                        dy = up ? dy - yzLz : (down ? dy + yzLz : dy);
                        dz = up ? dz - Lz : (down ? dz + Lz : dz);
                        }
                        {
                        const bool up = dy >= hy, down = dy < -hy;
                        dx = up ? dx - xyLy : (down ? dx + xyLy : dx);
                        dy = up ? dy - Ly : (down ? dy + Ly : dy);
                        }
                        {
                        const bool up = dx >= hx, down = dx < -hx;
                        dx = up ? dx - Lx : (down ? dx + Lx : dx);
                        }
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < r2)
                        each(j, dx, dy, dz, d2);
                    }
                }
            }
        }
    }

// the traversal around entry k of the list itself: its position is loaded and handed in
template<typename elem_t, typename Functor>
__device__ __forceinline__ void traverse_candidates(const elem_t* __restrict__ x, const uint32_t* __restrict__ offs, uint64_t n,
                                                    uint32_t k, uint32_t c, const TraverseGrid& g, Functor&& each)
    {
    traverse_candidates_around(x, offs, n, (double)x[(size_t)k * 3 + 0], (double)x[(size_t)k * 3 + 1],
                               (double)x[(size_t)k * 3 + 2], c, g, static_cast<Functor&&>(each));
    }
    } // namespace pgsd_amd

#endif
