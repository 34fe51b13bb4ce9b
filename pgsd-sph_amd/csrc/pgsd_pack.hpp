// pgsd_pack.hpp -- kernel argument blocks of the pack, unpack and select kernels (pgsd_*.hip) and the
// host-side launchers shared with the device pipeline (pgsd_device_write.cpp, pgsd_device_read.cpp).
#ifndef PGSD_PACK_HPP
#define PGSD_PACK_HPP

#include "pgsd.h"
#include "pgsd_internal.hpp"
#include "pgsd_private.h"

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>

namespace pgsd_amd
    {
enum
    {
    PACK_MAX_GROUPS = 8,       // distinct source arrays per launch
    PACK_MAX_OUT = 6,          // chunks fed from one source array
    PACK_LDS_BYTES = 49152,    // LDS budget per workgroup of the workgroup-tiled kernel (3 workgroups per CU)
    PACK_MAX_ROWBYTES = 2048,  // wider source rows take the generic kernel
    PACK_MAX_M = 1024
    };

// element conversions (wave-uniform per output)
enum
    {
    PACK_BITS = 0, // copy the low destination-size bytes (same type, narrowing, zero-extension, bitcast)
    PACK_SEXT = 1, // sign-extend a narrower signed integer
    PACK_F2F = 2,  // f64 -> f32 (round to nearest even) or f32 -> f64
    PACK_U2F = 3,  // unsigned integer (<= 32 bit) -> f32 / f64
    PACK_S2F = 4   // signed integer (<= 32 bit) -> f32 / f64
    };

// compile-time specialisations of the LDS-tiled kernels
enum
    {
    PACK_MODE_GENERIC = 0, // any element sizes / conversions, decided at run time per output
    PACK_MODE_W32 = 1,     // 4-byte source and chunk elements, bits unchanged
    PACK_MODE_F64_F32 = 2  // f64 sources, f32 chunks
    };

struct PackOut
    {
    void* dst;      // chunk buffer, 16-byte aligned
    uint32_t M;     // columns of the chunk
    uint32_t col0;  // first source column
    uint32_t dsz;   // bytes per chunk element
    uint32_t kind;  // PACK_*
    uint32_t magic; // ceil(2^32 / M) for row = e / M (0 when M == 1)
    uint32_t pad;
    };

struct PackGroup
    {
    const void* src;       // source array, 16-byte aligned
    const uint32_t* order; // gather index or nullptr
    uint32_t rowbytes;     // stride * ssz
    uint32_t ssz;          // bytes per source element
    uint32_t stride;       // elements per source row
    uint32_t n_out;
    uint32_t pad0[2];
    uint32_t lds_off;      // byte offset of this group's tile inside the workgroup's LDS (tiles kernel)
    uint32_t pad;
    PackOut out[PACK_MAX_OUT];
    };

struct PackArgs
    {
    uint64_t N;
    uint64_t n_tiles;
    uint32_t tile_rows;
    uint32_t n_groups;
    // groups [batch_start[b], batch_start[b+1]) are staged together, then emitted together
    uint32_t n_batches;
    uint32_t pad;
    uint8_t batch_start[PACK_MAX_GROUPS + 8];
    PackGroup g[PACK_MAX_GROUPS];
    };

// ---- row-per-lane kernel (pack_rows_kernel): the default for 4- and 8-byte elements
enum
    {
    ROWS_MAX_WORDS = 8, // a source row / a chunk row is at most 8 dwords (double4, N x 4 doubles)
    ROWS_MAX_GROUPS = 16, // source arrays per launch (16 x 184 B of descriptors: inside the 4 KiB of kernel arguments)
    ROWS_BITS = 0,      // dwords moved unchanged (equal element sizes; 8-byte elements are dword pairs)
    ROWS_F64_F32 = 1,   // f64 -> f32, round to nearest even
    ROWS_F32_F64 = 2    // f32 -> f64
    };

struct RowsOut
    {
    void* dst;       // chunk buffer
    uint32_t col0;   // first source ELEMENT (not dword)
    uint32_t M;      // chunk columns
    uint32_t kind;   // ROWS_*
    uint32_t nw_out; // dwords per chunk row = M * dsz / 4
    };

struct RowsGroup
    {
    const void* src;
    uint64_t copy_vecs;    // dense same-type copy: 16-byte vectors to move (0 = row mode)
    uint32_t copy_tail;    // ... and bytes behind the last whole vector
    uint32_t row_words;    // dwords per source row
    uint32_t n_out;
    uint32_t pad;
    RowsOut out[PACK_MAX_OUT];
    };

struct RowsArgs
    {
    uint64_t N;
    uint64_t n_blocks;     // gridDim.x: blocks of T*U rows (or 16-byte vectors); gridDim.y = n_groups
    uint32_t n_groups;
    uint32_t pad;
    RowsGroup g[ROWS_MAX_GROUPS];
    };
static_assert(sizeof(RowsArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// columns of destination rows that no chunk of a launch writes, set to one element value
// (pgsd_field_dst.fill_rest on the paths that do not assemble whole rows)
struct FillArgs
    {
    void* dst;
    const uint32_t* order;
    uint64_t N;
    uint64_t bits;
    uint32_t stride, dsz, colmask, pad;
    // indexed read: row k < rows_n whose entry rows[k] lies outside the chunk (>= src_N) is left alone, as the gathers
    // leave it (nullptr: every row is filled)
    const uint32_t* rows;
    uint64_t src_N, rows_n;
    };

struct PackGenericArgs
    {
    void* dst;
    const void* src;
    const uint32_t* order;
    uint64_t N;
    uint32_t M, stride, col0, ssz, dsz, kind;
    };

enum
    {
    UNPACK_MAX_JOBS = 12,     // chunks per launch
    UNPACK_MAX_GROUPS = 6,    // destination arrays assembled row-wise per launch
    UNPACK_MAX_ROW_COLS = 16, // columns of such a destination row
    UNPACK_LDS_BYTES = 49152, // LDS budget per workgroup
    UNPACK_MAX_SUM_ROWBYTES = UNPACK_LDS_BYTES / 16 // chunk row bytes one launch can stage at the smallest tile
    };

struct UnpackJob
    {
    const void* src;       // dense chunk rows
    void* dst;             // destination array
    const uint32_t* order; // scatter index or nullptr
    uint32_t M, ssz, dsz, kind;
    uint32_t dst_stride, dst_col0, magic, rowbytes; // rowbytes = M * ssz
    uint32_t lds_off;      // where this chunk's tile sits in the workgroup's LDS
    uint32_t in_group;     // 1: written by the row assembly of its destination array
    uint32_t fill_rest;    // host side only: the job asked for the untouched columns to be filled ...
    uint32_t pad;
    uint64_t fill_bits;    // ... with this element
    };

// A destination array every column of which is restored by chunks of the same launch (position.xyz
// + type id into a Scalar4 array): its rows are assembled in registers and written with 16-byte stores.
struct UnpackGroup
    {
    void* dst;
    const uint32_t* order;
    uint32_t stride, dsz;
    uint32_t vec_shift; // log2(16-byte vectors per destination row)
    uint32_t pad;
    uint8_t col_job[UNPACK_MAX_ROW_COLS]; // per destination column: the chunk it comes from ...
    uint8_t col_off[UNPACK_MAX_ROW_COLS]; // ... and the column inside that chunk
    };

struct UnpackArgs
    {
    uint64_t N;
    uint64_t n_tiles;
    uint32_t tile_rows;
    uint32_t n_jobs;
    uint32_t n_groups;
    uint32_t pad;
    UnpackJob j[UNPACK_MAX_JOBS];
    UnpackGroup g[UNPACK_MAX_GROUPS];
    };

// ---- row-per-lane unpack (unpack_rows_kernel): Scalar4 / double4 destination arrays fed by one or two chunks
struct UnrowsGroup
    {
    void* dst;          // destination array: rows of 4 elements (float4-like; double4 when converting f32 -> f64)
    const void* a;      // first chunk (dense rows of a_nw dwords), never null
    const void* b;      // second chunk or nullptr
    uint32_t a_nw, a_col0, b_nw, b_col0; // dwords per chunk row / first destination ELEMENT
    uint64_t copy_vecs; // dense same-type array riding along: 16-byte vectors to copy from `a` to `dst` (0 = row mode)
    uint32_t copy_tail;
    uint32_t fill_on;   // 1: columns no chunk feeds take the fill element, the row is stored whole
    uint32_t fill_lo, fill_hi; // bits of one destination element (hi: the upper half of a double)
    };

struct UnrowsArgs
    {
    uint64_t N;
    uint64_t n_blocks;
    uint32_t n_groups;
    uint32_t pad;
    // indexed read (gather): destination row i takes chunk row rows[i]; an entry >= src_N stores nothing and sets *bad
    const uint32_t* rows;
    uint64_t src_N;
    uint32_t* bad;
    UnrowsGroup g[ROWS_MAX_GROUPS];
    };

// the generic gather of an indexed read: element per lane, dst[k][col0 + c] = convert(chunk[rows[k]][c])
struct GatherArgs
    {
    const void* src;
    void* dst;
    const uint32_t* rows;
    uint32_t* bad;
    uint64_t n, src_N;
    uint32_t M, ssz, dsz, kind, dst_stride, dst_col0;
    };

// Enqueue the unpack of `n_jobs` chunks of N rows each on `stream`. Returns a pgsd_error.
// With `rows` (device memory, N entries in any order): an indexed read -- destination row i takes row rows[i] of every
// chunk, whose own height is src_N; an entry >= src_N writes nothing and sets the word *bad (device-visible) to 1.
int launch_unpack(uint32_t n_jobs, const pgsd_unpack_job* jobs, uint64_t N, hipStream_t stream, std::string* err,
                  const uint32_t* rows = nullptr, uint64_t src_N = 0, uint32_t* bad = nullptr);

// A fill pass of its own, for a destination array whose chunks are spread over several launches (each of which sees its
// own chunks only): the columns of rows [0, N) of `want`'s destination that are not in `covered` (bit c = column c) take
// want's fill element.  With `rows`: the rows k < rows_n whose entry is >= src_N are left alone.
int launch_fill_rest(const pgsd_unpack_job& want, uint32_t covered, uint64_t N, hipStream_t stream, std::string* err,
                     const uint32_t* rows = nullptr, uint64_t src_N = 0, uint64_t rows_n = 0);

// count -> one-block scan -> scatter of the rows inside the domain into out_rows (device, room for N), ascending;
// synchronises `stream` and leaves the count in *out_count (host)
int launch_select_domain(const DomainArgs& d, uint32_t* out_rows, uint64_t* out_count, hipStream_t stream, std::string* err);

// the same over a group predicate (WhereArgs, every base filled in): the rows that satisfy all of its terms and lie in
// its domain, if it has one
int launch_select_where(const WhereArgs& w, uint32_t* out_rows, uint64_t* out_count, hipStream_t stream, std::string* err);

// the ghost layer selection (HaloArgs, d.pos filled in): owned rows, then ghost rows, into out_rows (room for N), the ghosts'
// shifts into out_shift (room for 3 x N), the two counts into out_counts (host); synchronises `stream`
int launch_select_halo(const HaloArgs& h, uint32_t* out_rows, int32_t* out_shift, uint64_t out_counts[2], hipStream_t stream,
                       std::string* err);

// the domain census (d.pos / c.d.pos filled in): one pass over the position rows bins every wrapped fraction into `bins`
// bins per axis (out_hist, host: 3 x bins) / counts the rows of every cell (out_counts, host: n[0] * n[1] * n[2];
// *out_nowhere: rows with a NaN fraction); synchronises `stream`
int launch_axis_histograms(const DomainArgs& d, uint32_t bins, uint64_t* out_hist, hipStream_t stream, std::string* err);
int launch_cell_counts(const CellArgs& c, uint64_t* out_counts, uint64_t* out_nowhere, hipStream_t stream, std::string* err);

// cell order (OrderArgs, d.pos filled in): keys -> stable radix sort of (key, entry) pairs -> apply; rows (device, o.n
// entries) is sorted in place, shift (device, 3 x ghosts, or null) follows its ghosts, out_cell (device, o.n, or null)
// receives the sorted cell ids; synchronises `stream`.  PGSD_ERROR_INVALID_ARGUMENT, with nothing written, if an entry
// is >= o.d.N
int launch_order_rows(const OrderArgs& o, uint32_t* rows, int32_t* shift, int32_t* out_cell, hipStream_t stream,
                      std::string* err);
// the cell order's radix sort alone, for keys that are no grid cells (pgsd_component_moments.hip): the 8-bit passes that
// cover max_key over (key, value) pairs in the caller's memory -- keys[0] / vals[0] in, keys[1] / vals[1] their twins, table
// of sort_pairs_table_words(n) words, totals of 256 --, enqueued on `stream` without a synchronisation; the sorted pairs
// lie in keys[r] / vals[r] of the returned r.  Stable; no store at an index >= n whatever the keys hold
size_t sort_pairs_table_words(uint64_t n);
unsigned enqueue_sort_pairs(uint32_t* const keys[2], uint32_t* const vals[2], uint32_t* table, uint32_t* totals, uint64_t n,
                            uint64_t max_key, hipStream_t stream);

// chunk statistics (StatsArgs, base filled in): one pass of a workgroup per tile of 4096 entries, one workgroup over the
// tiles' partial results; out_counts / out_values (host, C x 3 each) are written on success only; synchronises `stream`.
// PGSD_ERROR_INVALID_ARGUMENT if an entry of the row list is >= s.N
int launch_chunk_stats(const StatsArgs& s, uint64_t* out_counts, double* out_values, hipStream_t stream, std::string* err);

// conservation sums (MomentsArgs, the addresses of the chunks that are present filled in): one pass of a workgroup per
// tile of 4096 entries over all chunks, one workgroup per (type, quantity) over the tiles' partial results; out_counts
// (host, n_types x 2, then the entries of no type) and out_sums (host, n_types x 9) are written on success only;
// synchronises `stream`.  PGSD_ERROR_INVALID_ARGUMENT if an entry of the row list is >= m.N
int launch_frame_moments(const MomentsArgs& m, uint64_t* out_counts, double* out_sums, hipStream_t stream, std::string* err);

// frame displacements (DisplacementArgs, the addresses of the chunks that are present filled in): one pass of a
// workgroup per tile of 4096 entries over the rows of both frames, one workgroup per (type, value) over the tiles'
// partial results; out_counts (host, n_types x 3, then the entries of no type) and out_values (host, n_types x 5) are
// written on success only; d.out (device, or null) receives every entry's displacement; synchronises `stream`.
// PGSD_ERROR_INVALID_ARGUMENT if an entry of the row list is >= d.N
int launch_frame_displacements(const DisplacementArgs& d, uint64_t* out_counts, double* out_values, hipStream_t stream,
                               std::string* err);

// cell fields (pgsd_cells.hip).  launch_cell_offsets: check and offsets kernels over a sorted cell list; out_offsets
// (device, n_cells + 2) is written on success only (zeros for n == 0).  launch_cell_moments (CellMomentsArgs, the
// addresses of the chunks that are present filled in): check, offsets, one wave per slab of 1024 sorted entries, one lane
// per slab and value for the cells of more than 1024 entries; out_counts (host, n_cells x 2, then the entries nowhere)
// and out_sums (host, n_cells x 9) are written on success only.  Both synchronise `stream`;
// PGSD_ERROR_INVALID_ARGUMENT for an id that descends or lies outside [0, n_cells] and for an entry >= c.N
int launch_cell_offsets(const int32_t* cell, uint64_t n, uint32_t n_cells, uint32_t* out_offsets, hipStream_t stream,
                        std::string* err);
int launch_cell_moments(const CellMomentsArgs& c, uint64_t* out_counts, double* out_sums, hipStream_t stream, std::string* err);

// component fields (pgsd_component_moments.hip; ComponentMomentsArgs, the addresses of the chunks that are present filled
// in): check, stable sort of the entries by component, offsets, a second check of the numbering, one wave per slab of 1024
// sorted entries, one lane per slab and word for the components of more than 1024 entries, two kernels for the flags and
// the summary.  out_sums (device, components x 9), out_extent (device, components x 6), out_origin (device, components x
// 3), out_flags (device, components x 2 uint32: bad, wide); out_summary (host, 6 words: n, components, bad, wide, heaviest,
// widest) is written on success only.  Synchronises `stream`; PGSD_ERROR_INVALID_ARGUMENT, with no output touched, for
// labels and ids that are not a components result of this list and for an entry >= c.N
int launch_component_moments(const ComponentMomentsArgs& c, double* out_sums, double* out_extent, double* out_origin,
                             uint32_t* out_flags, uint64_t* out_summary, hipStream_t stream, std::string* err);

// neighbour census (pgsd_neighbours.hip; NeighboursArgs, a.pos filled in): check, offsets, compaction of the listed
// positions, one lane per entry over the runs of the adjacent cells, one workgroup for the minima.  edges2 (host, a.bins
// + 1 doubles; null without bins); out_count, out_nearest2, out_nearest (device, a.n entries each, or null); out_summary
// (host, 8 + 257 + a.bins words) and out_closest2 (host) are written on success only.  Synchronises `stream`;
// PGSD_ERROR_INVALID_ARGUMENT for an id that descends or lies outside [0, n_cells] and for an entry >= a.N
int launch_neighbours(const NeighboursArgs& a, const double* edges2, uint32_t* out_count, double* out_nearest2,
                      uint32_t* out_nearest, uint64_t* out_summary, double* out_closest2, hipStream_t stream, std::string* err);

// neighbour lists (pgsd_neighbour_list.hip; NeighbourListArgs, a.pos filled in).  launch_neighbour_offsets: check,
// offsets, compaction, one lane per entry counting over the census's traversal, one workgroup scanning the workgroup sums,
// one pass writing out_offsets (device, a.n + 1 words); out_summary (host, 4 words: n, nowhere, pairs, longest); both are
// written on success only; a.n == 0 is one memset of out_offsets[0].  launch_neighbour_list: check, offsets, compaction,
// then the same traversal storing each neighbour (and its d2 where out_distance2 is given) inside the entry's segment of
// `offsets` (device, a.n + 1 words) and below `capacity`.  Both synchronise `stream`; PGSD_ERROR_INVALID_ARGUMENT for
// what the census refuses and, from the fill, for offsets that are not this list's or exceed the capacity
int launch_neighbour_offsets(const NeighbourListArgs& a, uint64_t* out_offsets, uint64_t* out_summary, hipStream_t stream,
                             std::string* err);
int launch_neighbour_list(const NeighbourListArgs& a, const uint64_t* offsets, uint64_t capacity, uint32_t* out_neighbours,
                          double* out_distance2, hipStream_t stream, std::string* err);

// components (pgsd_components.hip; NeighboursArgs, a.pos filled in): check, offsets, compaction, one lane per entry uniting
// itself with its later neighbours over the census's traversal in a lock-free union-find whose parent array is out_label
// (device, a.n words), a flatten pass, a count of the roots, one workgroup scanning the workgroups' counts, a numbering
// pass; out_component (device, a.n words, or null), out_sizes (device, a.n words of which the first `components` are
// written, or null); out_summary (host, 6 words: n, nowhere, components, singletons, largest, largest_label) is written on
// success only; a.n == 0 launches nothing.  Synchronises `stream`; PGSD_ERROR_INVALID_ARGUMENT for what the census
// refuses, PGSD_ERROR_DEVICE where a hook reached the cap of its retries (the pass gave up)
int launch_components(const NeighboursArgs& a, uint32_t* out_label, uint32_t* out_component, uint32_t* out_sizes,
                      uint64_t* out_summary, hipStream_t stream, std::string* err);

// SPH kernel sums (pgsd_sph.hip; SphArgs, a.pos, a.mass and a.density filled in): check, offsets, compaction of the listed
// positions, masses and volumes, one lane per entry over the runs of the adjacent cells in the defined order, one
// workgroup for the ranges and the deviation.  out_number, out_density, out_shepard (device, a.n entries each, or null);
// out_summary (host, 13 words) is written on success only.  Synchronises `stream`; PGSD_ERROR_INVALID_ARGUMENT for an id
// that descends or lies outside [0, n_cells] and for an entry >= a.N
int launch_sph_sums(const SphArgs& a, double* out_number, double* out_density, double* out_shepard, uint64_t* out_summary,
                    hipStream_t stream, std::string* err);

// SPH kernel gradients (pgsd_sph_gradients.hip; SphGradientsArgs, the chunk pointers filled in): check, offsets,
// compaction of the listed positions, masses, volumes and velocities, one lane per entry over the candidates in the sums'
// order (pgsd_traverse.hpp), one workgroup for the ranges and the largest norms.  out_rate, out_divergence (device, a.n
// entries), out_curl, out_normal (device, a.n x 3), each or null; out_summary (host, 13 words) is written on success only.
// Synchronises `stream`; PGSD_ERROR_INVALID_ARGUMENT for an id that descends or lies outside [0, n_cells] and for an
// entry >= a.N
// SPH sums with a per-particle smoothing length (pgsd_sph_adaptive.hip; SphAdaptiveArgs, the chunk pointers filled in):
// check, offsets, compaction with the float64 h column and the check of the declared bound h_max, one lane per entry over
// the candidates in the sums' order for the range 2 h_max (pgsd_traverse.hpp) with the per-pair support test, one workgroup
// for the summary.  out_count (device, a.n uint32), out_number, out_density, out_shepard (with a.volume), out_omega (gather
// mode) (device, a.n doubles), each or null; out_summary (host, 22 words) is written on success only.  Synchronises
// `stream`; PGSD_ERROR_INVALID_ARGUMENT for what launch_sph_sums refuses, an unknown mode, an h_max that is not valid and a
// listed valid smoothing length above h_max
int launch_sph_adaptive_sums(const SphAdaptiveArgs& a, uint32_t* out_count, double* out_number, double* out_density,
                             double* out_shepard, double* out_omega, uint64_t* out_summary, hipStream_t stream,
                             std::string* err);
// (n, bad, h_min, h_max) of a staged smoothing-length chunk (float32 or float64, N rows) over a row list (device, n
// entries; null: every row, n == N): out_words (host, 4 words: two counts, two float64 bit patterns) is written on success
// only.  Synchronises `stream`; PGSD_ERROR_INVALID_ARGUMENT for an entry >= N
int launch_sph_smoothing_range(const void* slength, uint32_t f64, const uint32_t* rows, uint64_t n, uint64_t N,
                               uint64_t* out_words, hipStream_t stream, std::string* err);

int launch_sph_gradients(const SphGradientsArgs& a, double* out_rate, double* out_divergence, double* out_curl,
                         double* out_normal, uint64_t* out_summary, hipStream_t stream, std::string* err);

// SPH gradient tensors (pgsd_sph_tensors.hip; SphTensorsArgs, the chunk pointers filled in): check, offsets, the
// gradients' compaction (pgsd_sph_compact.hpp), one lane per entry over the candidates in the sums' order
// (pgsd_traverse.hpp) with the inverse and the epilogue in the same kernel, one workgroup for the ranges, the smallest
// determinant and the largest shear rate.  out_correction (device, a.n x 6), out_determinant (a.n), out_gradient (a.n x 9),
// out_shear (a.n), each or null; out_summary (host, 14 words) is written on success only.  Synchronises `stream`;
// PGSD_ERROR_INVALID_ARGUMENT for an id that descends or lies outside [0, n_cells], for an entry >= a.N and for a det_min
// that is NaN or negative
int launch_sph_tensors(const SphTensorsArgs& a, double* out_correction, double* out_determinant, double* out_gradient,
                       double* out_shear, uint64_t* out_summary, hipStream_t stream, std::string* err);

// SPH accelerations (pgsd_sph_forces.hip; SphForcesArgs, the chunk pointers filled in): check, offsets, compaction of the
// listed positions, masses, A = p/rho^2, volumes, densities and velocities, one lane per entry over the candidates in the
// sums' order (pgsd_traverse.hpp), one workgroup for the largest norms.  out_pressure_acc, out_viscous_acc, out_total
// (device, a.n x 3), each or null; out_summary (host, 12 words) is written on success only.  Synchronises `stream`;
// PGSD_ERROR_INVALID_ARGUMENT for an id that descends or lies outside [0, n_cells] and for an entry >= a.N
int launch_sph_accelerations(const SphForcesArgs& a, double* out_pressure_acc, double* out_viscous_acc, double* out_total,
                             uint64_t* out_summary, hipStream_t stream, std::string* err);

// SPH samples (pgsd_sph_samples.hip; SphSamplesArgs, the chunk pointers filled in): check, offsets, compaction of the listed
// positions, masses, volumes and value columns, one lane per point of a.points (device, a.K x 3) over the candidates in the
// sums' order around the point's cell (pgsd_traverse.hpp), one workgroup for the ranges and the largest count.  out_count
// (device, a.K), out_density, out_shepard (device, a.K), out_values (device, a.K x a.C), each or null; out_summary (host, 11
// words) is written on success only.  a.K == 0 launches nothing; a.n == 0 still runs.  Synchronises `stream`;
// PGSD_ERROR_INVALID_ARGUMENT for an id that descends or lies outside [0, n_cells] and for an entry >= a.N
int launch_sph_samples(const SphSamplesArgs& a, uint32_t* out_count, double* out_density, double* out_shepard,
                       double* out_values, uint64_t* out_summary, hipStream_t stream, std::string* err);

// SPH body forces (pgsd_sph_body.hip; SphBodyArgs, the chunk pointers filled in): check and offsets of both lists, the
// accelerations' compaction of each, one lane per target over the sources in the sums' order around the target's cell
// (pgsd_traverse.hpp), the per-target force and torque terms into a table, the table's ordered sums (tiles of 4096, then
// one workgroup).  out_contacts (device, a.n), out_pressure_acc, out_viscous_acc (device, a.n x 3), each or null;
// out_summary (host, 22 words) is written on success only.  a.n == 0 launches nothing; a.n_fluid == 0 still runs.
// Synchronises `stream`; PGSD_ERROR_INVALID_ARGUMENT for an id of either list that descends or lies outside [0, n_cells]
// and for an entry >= a.N
int launch_sph_body_force(const SphBodyArgs& a, uint32_t* out_contacts, double* out_pressure_acc, double* out_viscous_acc,
                          uint64_t* out_summary, hipStream_t stream, std::string* err);

// mark -> one-block scan -> remap of a row plan (pgsd_internal.hpp) on `stream`; synchronises it and fills in the plan's
// host side (touched blocks, runs, staged_rows) and rows2 (device)
int launch_row_plan(RowPlan& plan, hipStream_t stream, std::string* err);

// Enqueue the pack of `n_jobs` fields of N rows each on `stream`. Returns a pgsd_error.
// ev_start / ev_stop (optional) receive the begin time of the first and the end time of the last kernel.
int launch_pack(uint32_t n_jobs, const pgsd_pack_job* jobs, uint64_t N, hipStream_t stream, std::string* err,
                hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// ---- comparison of packed chunks with reference rows (pgsd_compare_staged_chunks)
enum
    {
    CMP_MAX_JOBS = 64
    };

enum
    {
    CMP_BYTES = 0, // integers: equal bytes
    CMP_F32 = 1,   // float chunks are compared by VALUE, as numpy.array_equal compares them (hoomd.py:679-682):
    CMP_F64 = 2    // a NaN equals nothing (itself included), +0.0 equals -0.0
    };

struct CompareJob
    {
    const void* a;   // packed chunk (staging: HBM, or the pinned arena of the direct path)
    const void* b;   // reference in device memory
    uint64_t bytes;  // of the chunk
    uint64_t period; // 0: the reference holds `bytes` bytes; else it holds `period` bytes (a multiple of 16 and of the
                     // element size) and REPEATS: byte j of the chunk is compared with byte j % period of the reference
                     // (a few thousand rows of a default value stand for any number of rows)
    uint32_t mode;   // CMP_*
    uint32_t pad;
    };

struct CompareArgs
    {
    uint32_t* dflags; // device memory, one word per job: == gen once a difference was seen (early exit of the other workgroups)
    uint32_t* hflags; // pinned host memory (device-mapped), one word per job: the answer
    uint32_t gen;     // this launch's mark: the flag words are never cleared
    uint32_t n_jobs;
    uint64_t limit;   // compare at most this many bytes of every job (the probe launch); 0: all
    CompareJob j[CMP_MAX_JOBS];
    };

// Enqueue the comparison of `n_jobs` (<= CMP_MAX_JOBS) byte ranges on `stream`; hflags[i] == gen afterwards: they differ.
int launch_compare(uint32_t n_jobs, const CompareJob* jobs, uint32_t gen, uint32_t* dflags, uint32_t* hflags,
                   hipStream_t stream, std::string* err);

// The runtime loads a code object when one of its kernels is first used (about a millisecond each; every .hip unit is
// one object).  A caller who asked for everything up front (prealloc_mib) gets that over with in pgsd_device_configure:
// one attribute query per object -- pack, unpack, compare (warm_select_kernels), compaction, census and cell order.
void warm_pack_kernels();
void warm_unpack_kernels();
void warm_select_kernels();
void warm_compaction_kernels();
void warm_census_kernels();
void warm_order_kernels();
void warm_cells_kernels();
void warm_neighbours_kernels();
void warm_neighbour_list_kernels();
void warm_components_kernels();
void warm_component_moments_kernels();
void warm_sph_kernels();
void warm_sph_adaptive_kernels();
void warm_sph_gradients_kernels();
void warm_sph_tensors_kernels();
void warm_sph_forces_kernels();
void warm_sph_samples_kernels();
void warm_sph_body_kernels();

// algorithmic traffic of one job: bytes that must be read (needed columns only, plus the
// gather index) and chunk bytes written
uint64_t pack_algorithmic_bytes_in(const pgsd_pack_job& j, uint64_t N);
uint64_t pack_bytes_out(const pgsd_pack_job& j, uint64_t N);
    } // namespace pgsd_amd

#endif
