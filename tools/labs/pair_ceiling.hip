// tools/labs/pair_ceiling.hip -- the arithmetic ceiling the neighbour census' pair kernel is judged against (DESIGN
// section 8, "Neighbour census").
//
// The per-candidate work of neighbours_pair_kernel on register values alone, with no memory traffic inside the loop:
// three float64 differences, the single-shift minimum image z, y, x as compares and selects, (dx*dx + dy*dy) + dz*dz
// without contraction, the strict compare against r*r, the count and the (d2, position) minimum.  The candidate is
// formed in registers: three float64 additions stand where the kernel converts three loaded elements, and nothing else
// is added.  Every lane runs ITER candidates; 256 lanes per workgroup and enough workgroups to fill the device eight
// waves deep.  Prints one JSON line: candidate pairs per second from the dispatch's own begin / end stamps, best and
// median of the repetitions.
//
//
// Variant `sph` ("SPH sums"): the per-candidate work of sph_pair_kernel<*, KERNEL, true> on register
// values -- the same differences, fold, d2 and strict compare, and under the compare rr = sqrt(d2), q = rr * inv_h, the
// kernel's polynomial and the three accumulations a_n += w, a_m += m_j * w, a_v += V_j * w, m_j and V_j formed in
// registers.  The candidate turns round at a step that differs per lane, so that the about 1.7 % of the candidates that
// lie inside the range are spread over the lanes' iterations as they are in a real list (a wave takes the branch in
// nearly every iteration), instead of all lanes taking it together.
//
// Variant `sph_grad` ("SPH gradients"): the per-candidate work of sphg_pair_kernel<*, KERNEL, true> on
// register values -- the same differences, fold, d2 and strict compare, and under the compare rr = sqrt(d2), q = rr *
// inv_h, the factor F(q) (the spline's outer branch divides), e = F * d, u = v_j - v_i, the dot, the cross product and
// the eight accumulations, m_j, V_j and v_j formed in registers.  The candidates are the `sph` variant's.
//
// Variant `sph_force` ("SPH accelerations"): the per-candidate work of sphf_pair_kernel<*, KERNEL, true>
// on register values -- the same differences, fold, d2 and strict compare, and under the compare rr = sqrt(d2), q = rr *
// inv_h, the factor F(q), e = F * d, S = A_i + A_j, the three accumulations a_p[k] += m_j * (S * e_k), and the viscous
// term's division K = (F * d2) / (d2 + eta2), u = v_j - v_i and a_v[k] += V_j * (K * u_k); m_j, A_j, V_j and v_j formed
// in registers.  The candidates are the `sph` variant's.
//
// Variant `sph_tensor` ("SPH gradient tensors"): the per-candidate work of spht_pair_kernel<*, KERNEL> on
// register values -- the same differences, fold, d2 and strict compare, and under the compare rr = sqrt(d2), q = rr *
// inv_h, the factor F(q), e = F * d, u = v_j - v_i and the fifteen accumulations b_ab += V_j * (d_a * e_b) (upper
// triangle) and g_ab += V_j * (u_a * e_b) (all nine), V_j and v_j formed in registers.  The inverse and the epilogue run
// once per entry and are left out.  The candidates are the `sph` variant's.
//
//   hipcc -O3 --offload-arch=gfx950 tools/labs/pair_ceiling.hip -o pair_ceiling
//   ./pair_ceiling [reps=20] [iter=4096]
//       [variant=census|sph_wendland|sph_spline|sph_grad_wendland|sph_grad_spline|sph_force_wendland|sph_force_spline|
//                sph_tensor_wendland|sph_tensor_spline]
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define CK(x)                                                                                 \
    do                                                                                        \
        {                                                                                     \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess)                                                                 \
            {                                                                                 \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                          \
            }                                                                                 \
        } while (0)

struct Box
    {
    double v[6]; // Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz
    double r2;
    };

__global__ __launch_bounds__(256) void pair_ceiling_kernel(const Box b, uint32_t iter, uint32_t* __restrict__ out_count,
                                                           double* __restrict__ out_best2, uint32_t* __restrict__ out_best)
    {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const double Lx = b.v[0], Ly = b.v[1], Lz = b.v[2], xyLy = b.v[3], xzLz = b.v[4], yzLz = b.v[5];
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5, r2 = b.r2;
    // the lane's own position, and a candidate that walks away from it in steps that differ per lane and turns round every
    // 512 candidates, so that the differences stay within a box length or two and every branch of the fold is taken
    const double xi0 = -hx + (double)(k & 1023) * (Lx / 1024.0), xi1 = -hy + (double)((k >> 10) & 1023) * (Ly / 1024.0);
    const double xi2 = -hz + (double)(k >> 20) * (Lz / 4096.0);
    double s0 = Lx / 977.0 + (double)(k & 63) * 1e-3, s1 = -Ly / 1931.0, s2 = Lz / 2953.0;
    double xj0 = xi0, xj1 = xi1, xj2 = xi2;
    uint32_t count = 0, best = 0xFFFFFFFFu;
    double best2 = __builtin_huge_val();
    for (uint32_t j = 0; j < iter; j++)
        {
        if ((j & 511) == 511) // (wave-uniform, once per 512 candidates)
            {
            s0 = -s0;
            s1 = -s1;
            s2 = -s2;
            }
        xj0 = xj0 + s0;
        xj1 = xj1 + s1;
        xj2 = xj2 + s2;
        double dx = xj0 - xi0, dy = xj1 - xi1, dz = xj2 - xi2;
            {
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
        const bool near = d2 < r2 && j != k;
        count += near ? 1u : 0u;
        if (near && (d2 < best2 || (d2 == best2 && j < best)))
            {
            best2 = d2;
            best = j;
            }
        }
    out_count[k] = count;
    out_best2[k] = best2;
    out_best[k] = best;
    }

template<int KERNEL>
__global__ __launch_bounds__(256) void sph_ceiling_kernel(const Box b, double inv_h, uint32_t iter, uint32_t* __restrict__ out_count,
                                                          double* __restrict__ out_sums)
    {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const double Lx = b.v[0], Ly = b.v[1], Lz = b.v[2], xyLy = b.v[3], xzLz = b.v[4], yzLz = b.v[5];
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5, r2 = b.r2;
    const double xi0 = -hx + (double)(k & 1023) * (Lx / 1024.0), xi1 = -hy + (double)((k >> 10) & 1023) * (Ly / 1024.0);
    const double xi2 = -hz + (double)(k >> 20) * (Lz / 4096.0);
    double s0 = Lx / 977.0 + (double)(k & 63) * 1e-3, s1 = -Ly / 1931.0, s2 = Lz / 2953.0;
    double xj0 = xi0, xj1 = xi1, xj2 = xi2;
    const uint32_t phase = (k & 63) * 8; // the lane's own turning step
    uint32_t count = 0;
    double a_n = 0.0, a_m = 0.0, a_v = 0.0;
    for (uint32_t j = 0; j < iter; j++)
        {
        const bool turn = ((j + phase) & 511) == 511;
        s0 = turn ? -s0 : s0;
        s1 = turn ? -s1 : s1;
        s2 = turn ? -s2 : s2;
        xj0 = xj0 + s0;
        xj1 = xj1 + s1;
        xj2 = xj2 + s2;
        double dx = xj0 - xi0, dy = xj1 - xi1, dz = xj2 - xi2;
            {
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
            {
            const double rr = __builtin_sqrt(d2);
            const double q = rr * inv_h;
            double w;
            if constexpr (KERNEL == 0)
                {
                const double t = 1.0 - 0.5 * q;
                const double t2 = t * t;
                w = (t2 * t2) * (2.0 * q + 1.0);
                }
            else
                {
                const double q2 = q * q;
                const double u = 2.0 - q;
                w = q < 1.0 ? (1.0 - 1.5 * q2) + 0.75 * (q2 * q) : 0.25 * ((u * u) * u);
                }
            const double mj = 1.0 + (double)(j & 7u), vj = mj * 0.5;
            a_n = a_n + w;
            a_m = a_m + mj * w;
            a_v = a_v + vj * w;
            count++;
            }
        }
    out_count[k] = count;
    out_sums[(size_t)k * 3 + 0] = a_n;
    out_sums[(size_t)k * 3 + 1] = a_m;
    out_sums[(size_t)k * 3 + 2] = a_v;
    }

template<int KERNEL>
__global__ __launch_bounds__(256) void sph_grad_ceiling_kernel(const Box b, double inv_h, uint32_t iter, uint32_t* __restrict__ out_count,
                                                               double* __restrict__ out_sums)
    {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const double Lx = b.v[0], Ly = b.v[1], Lz = b.v[2], xyLy = b.v[3], xzLz = b.v[4], yzLz = b.v[5];
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5, r2 = b.r2;
    const double xi0 = -hx + (double)(k & 1023) * (Lx / 1024.0), xi1 = -hy + (double)((k >> 10) & 1023) * (Ly / 1024.0);
    const double xi2 = -hz + (double)(k >> 20) * (Lz / 4096.0);
    const double vi0 = (double)(k & 15) * 0.125, vi1 = -(double)(k & 7) * 0.25, vi2 = 0.5;
    double s0 = Lx / 977.0 + (double)(k & 63) * 1e-3, s1 = -Ly / 1931.0, s2 = Lz / 2953.0;
    double xj0 = xi0, xj1 = xi1, xj2 = xi2;
    const uint32_t phase = (k & 63) * 8; // the lane's own turning step
    uint32_t count = 0;
    double a_r = 0.0, a_d = 0.0, a_w0 = 0.0, a_w1 = 0.0, a_w2 = 0.0, a_c0 = 0.0, a_c1 = 0.0, a_c2 = 0.0;
    for (uint32_t j = 0; j < iter; j++)
        {
        const bool turn = ((j + phase) & 511) == 511;
        s0 = turn ? -s0 : s0;
        s1 = turn ? -s1 : s1;
        s2 = turn ? -s2 : s2;
        xj0 = xj0 + s0;
        xj1 = xj1 + s1;
        xj2 = xj2 + s2;
        double dx = xj0 - xi0, dy = xj1 - xi1, dz = xj2 - xi2;
            {
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
            {
            const double rr = __builtin_sqrt(d2);
            const double q = rr * inv_h;
            double F;
            if constexpr (KERNEL == 0)
                {
                const double t = 1.0 - 0.5 * q;
                F = -5.0 * ((t * t) * t);
                }
            else
                {
                const double u = 2.0 - q;
                F = q < 1.0 ? 2.25 * q - 3.0 : (-0.75 * (u * u)) / q;
                }
            const double mj = 1.0 + (double)(j & 7u), vj = mj * 0.5;
            const double e0 = F * dx, e1 = F * dy, e2 = F * dz;
            const double u0 = (double)(j & 3u) - vi0, u1 = (double)(j & 5u) - vi1, u2 = (double)(j & 9u) - vi2;
            const double dot = (u0 * e0 + u1 * e1) + u2 * e2;
            const double c0 = e1 * u2 - e2 * u1, c1 = e2 * u0 - e0 * u2, c2 = e0 * u1 - e1 * u0;
            a_r = a_r + mj * dot;
            a_d = a_d + vj * dot;
            a_w0 = a_w0 + vj * c0;
            a_w1 = a_w1 + vj * c1;
            a_w2 = a_w2 + vj * c2;
            a_c0 = a_c0 + vj * e0;
            a_c1 = a_c1 + vj * e1;
            a_c2 = a_c2 + vj * e2;
            count++;
            }
        }
    out_count[k] = count;
    double* o = out_sums + (size_t)k * 8;
    o[0] = a_r;
    o[1] = a_d;
    o[2] = a_w0;
    o[3] = a_w1;
    o[4] = a_w2;
    o[5] = a_c0;
    o[6] = a_c1;
    o[7] = a_c2;
    }

template<int KERNEL>
__global__ __launch_bounds__(256) void sph_force_ceiling_kernel(const Box b, double inv_h, uint32_t iter, uint32_t* __restrict__ out_count,
                                                                double* __restrict__ out_sums)
    {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const double Lx = b.v[0], Ly = b.v[1], Lz = b.v[2], xyLy = b.v[3], xzLz = b.v[4], yzLz = b.v[5];
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5, r2 = b.r2;
    const double xi0 = -hx + (double)(k & 1023) * (Lx / 1024.0), xi1 = -hy + (double)((k >> 10) & 1023) * (Ly / 1024.0);
    const double xi2 = -hz + (double)(k >> 20) * (Lz / 4096.0);
    const double vi0 = (double)(k & 15) * 0.125, vi1 = -(double)(k & 7) * 0.25, vi2 = 0.5;
    const double Ai = 0.1 + (double)(k & 31) * 0.001, eta2 = (0.01 / inv_h) / inv_h;
    double s0 = Lx / 977.0 + (double)(k & 63) * 1e-3, s1 = -Ly / 1931.0, s2 = Lz / 2953.0;
    double xj0 = xi0, xj1 = xi1, xj2 = xi2;
    const uint32_t phase = (k & 63) * 8; // the lane's own turning step
    uint32_t count = 0;
    double a_p0 = 0.0, a_p1 = 0.0, a_p2 = 0.0, a_v0 = 0.0, a_v1 = 0.0, a_v2 = 0.0;
    for (uint32_t j = 0; j < iter; j++)
        {
        const bool turn = ((j + phase) & 511) == 511;
        s0 = turn ? -s0 : s0;
        s1 = turn ? -s1 : s1;
        s2 = turn ? -s2 : s2;
        xj0 = xj0 + s0;
        xj1 = xj1 + s1;
        xj2 = xj2 + s2;
        double dx = xj0 - xi0, dy = xj1 - xi1, dz = xj2 - xi2;
            {
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
            {
            const double rr = __builtin_sqrt(d2);
            const double q = rr * inv_h;
            double F;
            if constexpr (KERNEL == 0)
                {
                const double t = 1.0 - 0.5 * q;
                F = -5.0 * ((t * t) * t);
                }
            else
                {
                const double u = 2.0 - q;
                F = q < 1.0 ? 2.25 * q - 3.0 : (-0.75 * (u * u)) / q;
                }
            const double mj = 1.0 + (double)(j & 7u), vj = mj * 0.5, Aj = 0.1 + (double)(j & 15u) * 0.002;
            const double e0 = F * dx, e1 = F * dy, e2 = F * dz;
            const double S = Ai + Aj;
            a_p0 = a_p0 + mj * (S * e0);
            a_p1 = a_p1 + mj * (S * e1);
            a_p2 = a_p2 + mj * (S * e2);
            const double K = (F * d2) / (d2 + eta2);
            const double u0 = (double)(j & 3u) - vi0, u1 = (double)(j & 5u) - vi1, u2 = (double)(j & 9u) - vi2;
            a_v0 = a_v0 + vj * (K * u0);
            a_v1 = a_v1 + vj * (K * u1);
            a_v2 = a_v2 + vj * (K * u2);
            count++;
            }
        }
    out_count[k] = count;
    double* o = out_sums + (size_t)k * 8;
    o[0] = a_p0;
    o[1] = a_p1;
    o[2] = a_p2;
    o[3] = a_v0;
    o[4] = a_v1;
    o[5] = a_v2;
    }

template<int KERNEL>
__global__ __launch_bounds__(256) void sph_tensor_ceiling_kernel(const Box b, double inv_h, uint32_t iter, uint32_t* __restrict__ out_count,
                                                                 double* __restrict__ out_sums)
    {
#pragma clang fp contract(off)
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    const double Lx = b.v[0], Ly = b.v[1], Lz = b.v[2], xyLy = b.v[3], xzLz = b.v[4], yzLz = b.v[5];
    const double hx = Lx * 0.5, hy = Ly * 0.5, hz = Lz * 0.5, r2 = b.r2;
    const double xi0 = -hx + (double)(k & 1023) * (Lx / 1024.0), xi1 = -hy + (double)((k >> 10) & 1023) * (Ly / 1024.0);
    const double xi2 = -hz + (double)(k >> 20) * (Lz / 4096.0);
    const double vi0 = (double)(k & 15) * 0.125, vi1 = -(double)(k & 7) * 0.25, vi2 = 0.5;
    double s0 = Lx / 977.0 + (double)(k & 63) * 1e-3, s1 = -Ly / 1931.0, s2 = Lz / 2953.0;
    double xj0 = xi0, xj1 = xi1, xj2 = xi2;
    const uint32_t phase = (k & 63) * 8; // the lane's own turning step
    uint32_t count = 0;
    double b00 = 0.0, b01 = 0.0, b02 = 0.0, b11 = 0.0, b12 = 0.0, b22 = 0.0;
    double g00 = 0.0, g01 = 0.0, g02 = 0.0, g10 = 0.0, g11 = 0.0, g12 = 0.0, g20 = 0.0, g21 = 0.0, g22 = 0.0;
    for (uint32_t j = 0; j < iter; j++)
        {
        const bool turn = ((j + phase) & 511) == 511;
        s0 = turn ? -s0 : s0;
        s1 = turn ? -s1 : s1;
        s2 = turn ? -s2 : s2;
        xj0 = xj0 + s0;
        xj1 = xj1 + s1;
        xj2 = xj2 + s2;
        double dx = xj0 - xi0, dy = xj1 - xi1, dz = xj2 - xi2;
            {
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
            {
            const double rr = __builtin_sqrt(d2);
            const double q = rr * inv_h;
            double F;
            if constexpr (KERNEL == 0)
                {
                const double t = 1.0 - 0.5 * q;
                F = -5.0 * ((t * t) * t);
                }
            else
                {
                const double u = 2.0 - q;
                F = q < 1.0 ? 2.25 * q - 3.0 : (-0.75 * (u * u)) / q;
                }
            const double vj = (1.0 + (double)(j & 7u)) * 0.5;
            const double e0 = F * dx, e1 = F * dy, e2 = F * dz;
            const double u0 = (double)(j & 3u) - vi0, u1 = (double)(j & 5u) - vi1, u2 = (double)(j & 9u) - vi2;
            b00 = b00 + vj * (dx * e0);
            b01 = b01 + vj * (dx * e1);
            b02 = b02 + vj * (dx * e2);
            b11 = b11 + vj * (dy * e1);
            b12 = b12 + vj * (dy * e2);
            b22 = b22 + vj * (dz * e2);
            g00 = g00 + vj * (u0 * e0);
            g01 = g01 + vj * (u0 * e1);
            g02 = g02 + vj * (u0 * e2);
            g10 = g10 + vj * (u1 * e0);
            g11 = g11 + vj * (u1 * e1);
            g12 = g12 + vj * (u1 * e2);
            g20 = g20 + vj * (u2 * e0);
            g21 = g21 + vj * (u2 * e1);
            g22 = g22 + vj * (u2 * e2);
            count++;
            }
        }
    out_count[k] = count;
    double* o = out_sums + (size_t)k * 16;
    o[0] = b00, o[1] = b01, o[2] = b02, o[3] = b11, o[4] = b12, o[5] = b22;
    o[6] = g00, o[7] = g01, o[8] = g02, o[9] = g10, o[10] = g11, o[11] = g12, o[12] = g20, o[13] = g21, o[14] = g22;
    }

// kernel: 0 sph_wendland, 1 sph_spline, 2 sph_grad_wendland, 3 sph_grad_spline, 4 sph_force_wendland, 5 sph_force_spline,
// 6 sph_tensor_wendland, 7 sph_tensor_spline
static int run_sph(int reps, uint32_t iter, int kernel)
    {
    int cus = 256;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const uint32_t blocks = (uint32_t)cus * 8u;
    const size_t lanes = (size_t)blocks * 256;
    uint32_t* count;
    double* sums;
    CK(hipMalloc(&count, lanes * sizeof(uint32_t)));
    // (three per lane for the sums, eight for the gradients, six for the forces, fifteen for the tensors)
    CK(hipMalloc(&sums, lanes * 16 * sizeof(double)));
    const Box b = {{40.0, 40.0, 40.0, 0.25 * 40.0, 0.125 * 40.0, -0.0625 * 40.0}, 0.197 * 0.197};
    const double inv_h = 1.0 / (0.197 / 2);
    hipEvent_t t0, t1;
    CK(hipEventCreate(&t0));
    CK(hipEventCreate(&t1));
    std::vector<double> ms;
    for (int r = 0; r < reps + 2; r++)
        {
        if (kernel == 0)
            hipExtLaunchKernelGGL(sph_ceiling_kernel<0>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else if (kernel == 1)
            hipExtLaunchKernelGGL(sph_ceiling_kernel<1>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else if (kernel == 2)
            hipExtLaunchKernelGGL(sph_grad_ceiling_kernel<0>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else if (kernel == 3)
            hipExtLaunchKernelGGL(sph_grad_ceiling_kernel<1>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else if (kernel == 4)
            hipExtLaunchKernelGGL(sph_force_ceiling_kernel<0>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else if (kernel == 5)
            hipExtLaunchKernelGGL(sph_force_ceiling_kernel<1>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else if (kernel == 6)
            hipExtLaunchKernelGGL(sph_tensor_ceiling_kernel<0>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        else
            hipExtLaunchKernelGGL(sph_tensor_ceiling_kernel<1>, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, inv_h, iter, count, sums);
        CK(hipGetLastError());
        CK(hipEventSynchronize(t1));
        float t = 0;
        CK(hipEventElapsedTime(&t, t0, t1));
        if (r >= 2) // (two warm-up launches)
            ms.push_back(t);
        }
    std::vector<uint32_t> h(lanes);
    CK(hipMemcpy(h.data(), count, lanes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t near = 0;
    for (uint32_t c : h)
        near += c;
    std::sort(ms.begin(), ms.end());
    const double pairs = (double)lanes * iter;
    static const char* variants[8] = {"sph_wendland",    "sph_spline",         "sph_grad_wendland", "sph_grad_spline",
                                      "sph_force_wendland", "sph_force_spline", "sph_tensor_wendland", "sph_tensor_spline"};
    printf("{\"kind\": \"pair_ceiling\", \"variant\": \"%s\", \"lanes\": %zu, \"iter\": %u, \"pairs\": %.0f, \"near\": %llu, "
           "\"best_ms\": %.4f, \"median_ms\": %.4f, \"worst_ms\": %.4f, \"pairs_per_s_best\": %.4g, \"pairs_per_s_median\": %.4g}\n",
           variants[kernel], lanes, iter, pairs, (unsigned long long)near, ms.front(),
           ms[ms.size() / 2], ms.back(), pairs / (ms.front() * 1e-3), pairs / (ms[ms.size() / 2] * 1e-3));
    CK(hipFree(count));
    CK(hipFree(sums));
    return 0;
    }

int main(int argc, char** argv)
    {
    const int reps = argc > 1 ? atoi(argv[1]) : 20;
    const uint32_t iter = argc > 2 ? (uint32_t)atoi(argv[2]) : 4096u;
    if (argc > 3 && std::string(argv[3]) != "census")
        {
        const std::string v = argv[3];
        static const char* names[8] = {"sph_wendland",    "sph_spline",         "sph_grad_wendland", "sph_grad_spline",
                                       "sph_force_wendland", "sph_force_spline", "sph_tensor_wendland", "sph_tensor_spline"};
        int kernel = 0;
        for (int i = 0; i < 8; i++)
            if (v == names[i])
                kernel = i;
        return run_sph(reps, iter, kernel);
        }
    int cus = 256;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const uint32_t blocks = (uint32_t)cus * 8u; // 32 waves per compute unit: eight per SIMD
    const size_t lanes = (size_t)blocks * 256;
    uint32_t *count, *best;
    double* best2;
    CK(hipMalloc(&count, lanes * sizeof(uint32_t)));
    CK(hipMalloc(&best, lanes * sizeof(uint32_t)));
    CK(hipMalloc(&best2, lanes * sizeof(double)));
    const Box b = {{40.0, 40.0, 40.0, 0.25 * 40.0, 0.125 * 40.0, -0.0625 * 40.0}, 0.197 * 0.197};
    hipEvent_t t0, t1;
    CK(hipEventCreate(&t0));
    CK(hipEventCreate(&t1));
    std::vector<double> ms;
    for (int r = 0; r < reps + 2; r++)
        {
        hipExtLaunchKernelGGL(pair_ceiling_kernel, dim3(blocks), dim3(256), 0, 0, t0, t1, 0, b, iter, count, best2, best);
        CK(hipGetLastError());
        CK(hipEventSynchronize(t1));
        float t = 0;
        CK(hipEventElapsedTime(&t, t0, t1));
        if (r >= 2) // (two warm-up launches)
            ms.push_back(t);
        }
    std::vector<uint32_t> h(lanes);
    CK(hipMemcpy(h.data(), count, lanes * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint64_t near = 0;
    for (uint32_t c : h)
        near += c;
    std::sort(ms.begin(), ms.end());
    const double pairs = (double)lanes * iter;
    printf("{\"kind\": \"pair_ceiling\", \"lanes\": %zu, \"iter\": %u, \"pairs\": %.0f, \"near\": %llu, \"best_ms\": %.4f, "
           "\"median_ms\": %.4f, \"pairs_per_s_best\": %.4g, \"pairs_per_s_median\": %.4g}\n",
           lanes, iter, pairs, (unsigned long long)near, ms.front(), ms[ms.size() / 2], pairs / (ms.front() * 1e-3),
           pairs / (ms[ms.size() / 2] * 1e-3));
    CK(hipFree(count));
    CK(hipFree(best));
    CK(hipFree(best2));
    return 0;
    }
