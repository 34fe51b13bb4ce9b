// pgsd_pieces.hpp -- the ORDER of a segmented sum over a sorted list, written once for the cell fields (pgsd_cells.hip:
// the segments are grid cells) and the component fields (pgsd_component_moments.hip: the segments are components):
//   a segment's entries, in sorted order, are cut into PIECES of 1024 counted from the segment's first entry; in a piece
//   lane l of 64 adds entries l, l + 64, ... to +0.0 (an entry past the end and a value that is not finite add +0.0); the
//   64 lane sums go through the wave tree of the statistics; the piece sums are added to +0.0 in ascending order.
// pieces_walk_slab is the body of a kernel with one WAVE per slab of 1024 consecutive sorted entries: the wave owns the
// pieces that START in its slab (p is a start iff its segment id s is below the number of segments and (p - offs[s]) %
// 1024 == 0), found by ballot and handled in ascending order; per piece ceil(len / 64) wave-uniform steps of gathered
// loads of the four moments chunks, nine trees and one counter.  The piece of a segment of at most 1024 entries is the
// segment; a longer segment's pieces go to a partials table of TWO slots per slab, and pieces_long_slots walks them in
// sequence for the kernel that adds them up.
//
// Why two slots per slab suffice for the pieces of long segments (segments of more than 1024 entries):
//   * piece j of a segment whose first entry is s starts at s + 1024 j; with s in slab w that lies in slab w + j, so the
//     long kernel finds a segment's pieces without a list;
//   * a slab holds at most one piece of number >= 1: the 1024 entries before such a piece's start belong to its segment,
//     so a second start of number >= 1 in the same slab would lie in the same segment less than 1024 entries away -- but
//     a segment's starts are 1024 apart;
//   * a slab holds at most one FIRST piece of a long segment: the 1024 entries behind its start belong to that segment,
//     so no other segment starts in the rest of the slab.
// Slot 0 takes the piece of number >= 1, slot 1 the first piece of a long segment; first[w] is that piece's start, or
// PIECES_NONE (every slab's wave writes it: one writer per word, nothing to clear).
//
// What differs between the two units is a POLICY object handed to the walk:
//   static constexpr int BATCH   steps a lane has in flight
//   uint32_t segments            the number of segments; an id >= segments is summed nowhere
//   uint32_t id(uint64_t p)      the segment id at sorted position p < n
//   bool summed(uint32_t id)     does the id name a segment (below `segments`, and whatever else the unit asks)
//   void open(uint32_t c, uint64_t c_lo)                     a piece of segment c begins (wave-uniform)
//   uint64_t row(uint64_t p, bool ok, int i)                 the chunk row of sorted position p for step i of the batch
//                                                            (ok: p lies in the piece; otherwise anything below 2^64)
//   void place(double x[3], bool ok, int i)                  the entry's position -> what is summed in its place
//   void close(c, w, is_long, is_first, sum, n_bad, lane)    the piece's nine sums (lane 0 holds them) and its bad entries
// Seen by the HIP compiler alone.
#ifndef PGSD_PIECES_HPP
#define PGSD_PIECES_HPP

#include "pgsd_stats.hpp"

namespace pgsd_amd
    {
#define PIECES_STEPS (CELLS_PIECE / 64)
enum
    {
    PIECES_Q = MOMENTS_QUANTITIES,
    PIECES_NONE = 0xFFFFFFFFu
    };
static_assert(PIECES_STEPS == SEL_PER_THREAD, "a slab is 16 steps of a wave");

// s: the four chunks (s.chunk[1 .. 4]: mass, velocity, energy, position; null: s.defaults stands for every row), s.n,
// s.N; offs: segments + 1 offsets into the sorted list; first: one word per slab
template<bool F64, class Args, class Policy>
__device__ __forceinline__ void pieces_walk_slab(const Args& s, Policy& P, const uint32_t* __restrict__ offs, uint32_t w,
                                                 uint32_t lane, uint32_t* __restrict__ first)
    {
#pragma clang fp contract(off)
    constexpr int T = F64 ? STATS_F64 : STATS_F32;
    constexpr int W1 = F64 ? 2 : 1, W3 = 3 * W1; // 32-bit words of a scalar and of a three-column row
    constexpr int BATCH = Policy::BATCH;
    constexpr int Q = PIECES_Q;
    const uint64_t n = s.n;
    const uint32_t segments = P.segments;
    const uint64_t base = (uint64_t)w * CELLS_PIECE;
    const uint32_t* c_mass = (const uint32_t*)s.chunk[1];
    const uint32_t* c_vel = (const uint32_t*)s.chunk[2];
    const uint32_t* c_energy = (const uint32_t*)s.chunk[3];
    const uint32_t* c_pos = (const uint32_t*)s.chunk[4];
    // the slab's ids, 16 per lane and coalesced; bit j of `starts`: entry base + 64 j + lane starts a piece
    uint32_t id[PIECES_STEPS];
#pragma unroll
    for (int j = 0; j < PIECES_STEPS; j++)
        {
        const uint64_t p = base + (uint64_t)j * 64 + lane;
        id[j] = p < n ? P.id(p) : segments;
        }
    uint32_t starts = 0;
#pragma unroll
    for (int j = 0; j < PIECES_STEPS; j++)
        {
        const uint64_t p = base + (uint64_t)j * 64 + lane;
        if (P.summed(id[j]))
            {
            const uint64_t o = min((uint64_t)offs[id[j]], n);
            if (o <= p && ((p - o) & (CELLS_PIECE - 1)) == 0)
                starts |= 1u << j;
            }
        }
    uint32_t first_long = PIECES_NONE;
    for (int j = 0; j < PIECES_STEPS; j++)
        {
        uint64_t mask = __ballot((starts >> j) & 1u);
        while (mask != 0)
            {
            const uint32_t b = (uint32_t)__builtin_ctzll(mask);
            mask &= mask - 1;
            const uint64_t at = base + (uint64_t)j * 64 + b; // (wave-uniform, < n: only an entry of the list starts a piece)
            const uint32_t c = min((uint32_t)__builtin_amdgcn_readfirstlane(P.id(at)), segments - 1u);
            const uint64_t c_lo = min((uint64_t)offs[c], n), c_hi = min((uint64_t)offs[c + 1], n);
            const uint64_t end = min(at + CELLS_PIECE, c_hi);
            const bool is_long = c_hi > c_lo && c_hi - c_lo > CELLS_PIECE;
            const bool is_first = at == c_lo;
            const uint32_t steps = end > at ? (uint32_t)((end - at + 63) >> 6) : 0u;
            P.open(c, c_lo);
            double acc[Q];
            uint32_t bad = 0;
#pragma unroll
            for (int q = 0; q < Q; q++)
                acc[q] = 0.0;
            for (uint32_t t0 = 0; t0 < steps; t0 += BATCH)
                {
                RowRegs r_mass[BATCH], r_vel[BATCH], r_energy[BATCH], r_pos[BATCH];
                bool ok[BATCH];
#pragma unroll
                for (int i = 0; i < BATCH; i++)
                    {
                    const uint64_t p = at + (uint64_t)(t0 + i) * 64 + lane;
                    ok[i] = p < end;
                    const u32x4 zero = {0u, 0u, 0u, 0u};
                    r_mass[i].lo = r_vel[i].lo = r_vel[i].hi = r_energy[i].lo = r_pos[i].lo = r_pos[i].hi = zero;
                    const uint64_t row = P.row(p, ok[i], i);
                    ok[i] = ok[i] && row < s.N; // (the check kernel has refused such a list: nothing is loaded for it)
                    if (ok[i])
                        {
                        if (c_mass)
                            row_load<W1>(c_mass + row * W1, r_mass[i]);
                        if (c_vel)
                            row_load<W3>(c_vel + row * W3, r_vel[i]);
                        if (c_energy)
                            row_load<W1>(c_energy + row * W1, r_energy[i]);
                        if (c_pos)
                            row_load<W3>(c_pos + row * W3, r_pos[i]);
                        }
                    }
#pragma unroll
                for (int i = 0; i < BATCH; i++)
                    {
                    // the nine values of the conservation sums (moments_tile_kernel), in the same association
                    const double m = c_mass ? stats_elem<T>(r_mass[i], 0) : s.defaults[0];
                    const double e = c_energy ? stats_elem<T>(r_energy[i], 0) : s.defaults[4];
                    double v[3], x[3], val[Q];
#pragma unroll
                    for (int a = 0; a < 3; a++)
                        {
                        v[a] = c_vel ? stats_elem<T>(r_vel[i], a) : s.defaults[1 + a];
                        x[a] = c_pos ? stats_elem<T>(r_pos[i], a) : s.defaults[5 + a];
                        }
                    P.place(x, ok[i], i);
                    val[0] = m;
                    val[4] = (0.5 * m) * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
                    val[5] = m * e;
#pragma unroll
                    for (int a = 0; a < 3; a++)
                        {
                        val[1 + a] = m * v[a];
                        val[6 + a] = m * x[a];
                        }
                    bool all_fin = true;
#pragma unroll
                    for (int q = 0; q < Q; q++)
                        {
                        const bool fin = __builtin_fabs(val[q]) < __builtin_huge_val(); // (false for a NaN as well)
                        all_fin = all_fin && fin;
                        acc[q] = acc[q] + ((ok[i] && fin) ? val[q] : 0.0);
                        }
                    bad += (ok[i] && !all_fin) ? 1u : 0u;
                    }
                }
            double sum[Q];
#pragma unroll
            for (int q = 0; q < Q; q++)
                sum[q] = stats_wave_sum(acc[q]);
            const uint64_t n_bad = stats_wave_count(bad);
            if (is_long && is_first)
                first_long = (uint32_t)at;
            P.close(c, w, is_long, is_first, sum, n_bad, lane);
            }
        }
    if (lane == 0)
        first[w] = first_long;
    }

// The slots of the long segment whose first piece starts at sorted position `at` of slab w, in ascending piece order:
// each(slot) for piece 0 (slot 1 of slab w), piece 1 (slot 0 of slab w + 1), ...  c_lo, c_hi: the segment's bounds,
// clamped to n by the caller; SLOT_WORDS: 64-bit words of a slot
template<int SLOT_WORDS, class Each>
__device__ __forceinline__ void pieces_long_slots(const double* __restrict__ part, uint32_t w, uint64_t c_lo, uint64_t c_hi,
                                                  uint32_t n_slabs, Each&& each)
    {
    const uint64_t pieces = c_hi > c_lo ? (c_hi - c_lo + CELLS_PIECE - 1) / CELLS_PIECE : 0;
    for (uint64_t j = 0; j < pieces && w + j < n_slabs; j++)
        each(part + ((size_t)2 * (w + j) + (j == 0 ? 1 : 0)) * SLOT_WORDS);
    }
    } // namespace pgsd_amd

#endif
