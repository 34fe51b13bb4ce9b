/* pgsd_private.h -- entry points of libpgsd_amd.so that are NOT part of the public C ABI (include/pgsd.h).
 *
 * They are exported from the library because the parity tests, bench.py's kernel legs, the tools under tools/ and the
 * Cython binding reach them across the shared-object boundary, but no caller of the file format needs them and they
 * may change without a PGSD_ABI_VERSION bump:
 *
 *   bare kernels      pgsd_pack_fields, pgsd_unpack_fields: the HIP kernels without a file (tests/test_gpu_pack.py,
 *                     bench_legs.py, tools/pack_bench.py, tools/unpack_bench.py)
 *   queue plumbing    pgsd_frame_exchange (the scenario driver's `dump`), pgsd_set_deferred_rows (pgsd.fl only: it
 *                     owns the host arrays it queues)
 *   housekeeping      pgsd_device_release_parked, pgsd_reload_tuning
 *   binding helpers   pgsd_device_of, pgsd_device_copy (pgsd.fl keeps library-owned device buffers on the pipeline's
 *                     device and clones them without a tensor library)
 *   restart helpers   pgsd_select_domain_device, pgsd_read_rows_device (pgsd.fl's select_domain_device and
 *                     read_chunk_device(rows=...), behind pgsd.hoomd's read_frame_device(domain=...): a rank of a
 *                     domain-decomposed run reads its own particles; the public header has no room for them)
 *                     pgsd_select_where_device (pgsd.fl's select_where_device, behind pgsd.hoomd's
 *                     read_frame_device(where=...): a particle group -- a set of types, ranges of per-particle values,
 *                     optionally inside a domain -- selected on the GPU from the staged chunks of its terms)
 *                     pgsd_select_halo_device (pgsd.fl's select_halo_device, behind pgsd.hoomd's
 *                     read_frame_device(domain=..., ghost=...): a cell plus the ghost layer its neighbours reach -- the
 *                     owned rows, the ghost rows and the periodic shift of each ghost -- from one staged position chunk)
 *                     pgsd_domain_histogram_device, pgsd_domain_counts_device (pgsd.fl's domain_histogram_device and
 *                     domain_counts_device, behind pgsd.hoomd's axis_histograms_device, domain_counts_device and
 *                     balanced_grid_device: per-axis histograms of the fractions and per-cell counts of a decomposition,
 *                     counted on the GPU from one staged position chunk, so that a restart can choose balanced splits)
 *                     pgsd_chunk_stats_device (pgsd.fl's chunk_stats_device, behind pgsd.hoomd's frame_stats_device:
 *                     per column of a staged chunk, or of a selection's row list over it, the NaN and infinite entries,
 *                     minimum, maximum and a sum in a fixed order, so that "did the run blow up, what is the largest
 *                     speed, what is the density range" cost one pass over rows that are in HBM already)
 *                     pgsd_frame_moments_device (pgsd.fl's frame_moments_device, behind pgsd.hoomd's
 *                     frame_moments_device: per particle type the mass, momentum, kinetic and internal energy and first
 *                     moment of a frame or of a selection, from the staged typeid, mass, velocity, energy and position
 *                     chunks in one pass, so that "did the run conserve what it must" costs no read to the host)
 *                     pgsd_frame_displacements_device (pgsd.fl's frame_displacements_device, behind pgsd.hoomd's
 *                     frame_displacements_device: per particle type the drift, the squared displacement and the largest
 *                     move between two frames, unwrapped through image flags and box vectors, from the staged position
 *                     and image chunks of both frames in one pass)
 *                     pgsd_cell_offsets_device, pgsd_cell_moments_device (pgsd.fl's cell_offsets_device and
 *                     cell_moments_device, behind pgsd.hoomd's cell_moments_device: the CSR offsets of a row list in
 *                     cell order, and per grid cell the mass, momentum, kinetic and internal energy and first moment of
 *                     its entries -- the coarse-grained density and velocity field -- from the staged chunks in one
 *                     segmented pass)
 *                     pgsd_neighbours_device (pgsd.fl's neighbours_device, behind pgsd.hoomd's frame_neighbours_device:
 *                     per entry of a row list in cell order the neighbours inside a range and the nearest of them, and
 *                     over the list the count histogram, the closest pair and the pair histogram of g(r))
 *                     pgsd_neighbour_offsets_device, pgsd_neighbour_list_device (pgsd.fl's neighbour_list_device, behind
 *                     pgsd.hoomd's frame_neighbour_list_device: the same neighbours handed over as a CSR pair list in a
 *                     defined order -- count and scan, then fill -- which is what a restarted solver builds first)
 *                     pgsd_components_device (pgsd.fl's components_device, behind pgsd.hoomd's frame_components_device:
 *                     the connected components of the half list's pairs -- which pieces has the fluid broken into, how
 *                     many droplets and stray particles are there -- as a label, a dense id and the sizes, by a lock-free
 *                     union-find over the same traversal)
 *                     pgsd_component_moments_device (pgsd.fl's component_moments_device, behind pgsd.hoomd's
 *                     frame_component_moments_device: what each of those pieces is -- mass, momentum, energies, centre
 *                     and extent per component, the cell fields' sums over the entries sorted by component, positions
 *                     as displacements from the component's root, and a flag for a piece that spans half the box)
 *                     pgsd_sph_sums_device (pgsd.fl's sph_sums_device, behind pgsd.hoomd's frame_kernel_sums_device: per
 *                     entry of a row list in cell order the SPH summation density, number density and Shepard sum over
 *                     the kernel support, in a defined order, and over the list their ranges, the largest deviation from
 *                     the stored density and the entries below a Shepard threshold)
 *                     pgsd_sph_smoothing_range_device, pgsd_sph_adaptive_sums_device (pgsd.fl's smoothing_range_device
 *                     and sph_adaptive_sums_device, behind pgsd.hoomd's frame_adaptive_sums_device: the sums with the
 *                     smoothing length stored per particle, the neighbour count and the grad-h factor)
 *                     pgsd_sph_gradients_device (pgsd.fl's sph_gradients_device, behind pgsd.hoomd's
 *                     frame_kernel_gradients_device: per entry of the same list, over the same support and in the same
 *                     order, the density rate of the continuity equation, the velocity divergence and curl and the
 *                     colour gradient, and over the list their ranges and the largest vorticity and surface normal)
 *                     pgsd_sph_tensors_device (pgsd.fl's sph_tensors_device, behind pgsd.hoomd's
 *                     frame_gradient_tensors_device: per entry of the same list, over the same support and in the same
 *                     order, the kernel-gradient correction matrix, the corrected velocity-gradient tensor and the shear
 *                     rate, and over the list the entries left uncorrected and the largest shear rate with its row)
 *                     pgsd_sph_accelerations_device (pgsd.fl's sph_accelerations_device, behind pgsd.hoomd's
 *                     frame_accelerations_device: per entry of the same list, over the same support and in the same
 *                     order, the pressure and the laminar viscous acceleration and their sum with gravity, and over the
 *                     list the largest of each with its row -- is the frame in equilibrium, and what time step does it
 *                     allow)
 *                     pgsd_sph_samples_device (pgsd.fl's sph_samples_device, behind pgsd.hoomd's frame_samples_device:
 *                     the SPH interpolant of the same list at points of the caller's choosing -- a gauge, a line, a
 *                     slice, a grid to render --, the same candidates in the same order around the point's cell)
 *                     pgsd_sph_body_force_device (pgsd.fl's sph_body_force_device, behind pgsd.hoomd's
 *                     frame_body_force_device: the force and the torque the fluid exerts on a body -- a pair pass
 *                     between two lists in cell order on one grid and the ordered sums over the targets)
 *                     pgsd_row_plan_create / _destroy / _query, pgsd_read_rows_planned_device,
 *                     pgsd_device_read_counters (pgsd.fl's plan_rows, read_chunk_device(rows=plan) and
 *                     device_read_stats, behind pgsd.hoomd's read_tracks_device: a few particles through many frames,
 *                     reading only the file blocks their rows touch)
 */
#ifndef PGSD_PRIVATE_H
#define PGSD_PRIVATE_H

#include "pgsd.h"

#ifdef __cplusplus
extern "C"
    {
#endif

    /* Bare kernels, no file: pack into caller-provided device buffers on `stream`
       (a hipStream_t passed as void*; NULL = the null stream). */
    struct pgsd_pack_job
        {
        void* dst;         /* device pointer, N*M elements of dst_type, 16-byte aligned */
        uint32_t dst_type; /* enum pgsd_type */
        uint32_t M;
        struct pgsd_field_desc src;
        };
    /* kernel_ms (may be NULL): receives the time from the begin of the first to the end of the last kernel of the call
       as the dispatches themselves stamp it (what rocprofv3 reports per kernel; no launch latency); the call then
       synchronises `stream`.  Measurement only. */
    int pgsd_pack_fields(uint32_t n_jobs, const struct pgsd_pack_job* jobs, uint64_t N, void* stream, float* kernel_ms);

    /* Bare unpack kernel: dense chunk rows already in device memory -> destination arrays. */
    struct pgsd_unpack_job
        {
        const void* src;   /* device pointer, N*M elements of src_type, 16-byte aligned */
        uint32_t src_type; /* enum pgsd_type of the chunk */
        uint32_t M;
        struct pgsd_field_dst dst;
        };
    int pgsd_unpack_fields(uint32_t n_jobs, const struct pgsd_unpack_job* jobs, uint64_t N, void* stream);

    /* Batched mode only: with `on`, the host rows of pgsd_write_chunk(..., all == true, data) are BORROWED UNTIL
       THE FRAME'S EXCHANGE instead of for the call -- the caller promises to leave them alone until the next
       pgsd_end_frame / pgsd_flush / pgsd_frame_exchange / pgsd_close (the contract device sources have anyway).
       Such a chunk then waits in the queue like every other instead of resolving it at once, and a frame costs
       ONE exchange whatever mix of host and device chunks it holds.  (The reference's contract -- rows borrowed
       for the call -- is the default; pgsd.fl turns this on where it holds the arrays itself.) */
    int pgsd_set_deferred_rows(struct pgsd_handle* handle, int on);

    /* Perform the batched frame exchange now (collective; nothing is flushed): afterwards the queue is empty and
       the handle's mirror is current.  No-op when nothing is queued. */
    int pgsd_frame_exchange(struct pgsd_handle* handle);

    /* Give every parked pipeline set (include/pgsd.h, end of part 3) back to the runtime now; returns the number of
       sets freed.  Not to be called while another thread opens or closes a handle. */
    int pgsd_device_release_parked(void);

    /* The PGSD_* tuning variables (launch shapes, kernel choices, direct-path threshold ...) are read ONCE, when the
       library first needs them.  Tools that A/B variants inside one process change the environment and call this to
       have it read again. */
    void pgsd_reload_tuning(void);

    /* The HIP device the handle's pipeline runs on (the pipeline is created if it does not exist yet: the device
       configured with pgsd_device_configure, else the current one at that moment); negative: a pgsd_error. */
    int pgsd_device_of(struct pgsd_handle* handle);

    /* `bytes` bytes from src to dst: device memory on `device` (-1: the current one) or host memory, either side
       (hipMemcpyDefault); complete on return. */
    int pgsd_device_copy(int device, void* dst, const void* src, size_t bytes);

    /* ---- restart helpers behind pgsd.fl / pgsd.hoomd ---- */

    /* The rows of a frame's position chunk (N x 3 float32 or float64, N < 2^32) that lie in one spatial domain, in
       ascending order.  The predicate is HOOMD's BoxDim::makeFraction in float64, operation for operation (no FMA
       contraction), box = {Lx, Ly, Lz, xy, xz, yz}:
           sx = ((x + Lx/2) - ((xz - yz*xy)*z + xy*y)) / Lx,  sy = ((y + Ly/2) - yz*z) / Ly,  sz = (z + Lz/2) / Lz
           s = s - floor(s), then 0 where s >= 1 (periodic wrap);  inside: lo[a] <= s[a] < hi[a] for x, y and -- unless
           dimensions == 2 -- z.
       Requires 0 <= lo < hi <= 1 per axis, Lx, Ly > 0 and Lz > 0 unless dimensions == 2 (dimensions is 2 or 3).
       out_rows: device memory with room for position->N entries; *out_count (host) receives their number.  The chunk is
       staged into HBM and the call synchronises; the staged rows are kept until the next pgsd_device_wait_read, so a
       pgsd_read_rows_device of the same chunk before it reads no file bytes again. */
    int pgsd_select_domain_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const float box[6],
                                  uint32_t dimensions, const double lo[3], const double hi[3], uint32_t* out_rows,
                                  uint64_t* out_count);

    /* A domain plus its ghost layer (pgsd.hoomd.halo_rows is the definition).  position, box, dimensions, lo, hi: as
       pgsd_select_domain_device's, and the OWNED rows are exactly its rows.  bands: per axis (x, y, z) eight bounds
       in [0, 1] -- four half-open intervals {lo, hi}: below, below wrapped, above, above wrapped; an empty one is {1, 0} --
       computed by the caller (pgsd.hoomd.halo_bands); divided[a] == 0: axis a has no bands and every fraction counts as
       inside on it (z is not looked at when dimensions == 2).  A row's state on a divided axis is the first match of:
       inside [lo, hi), the four bands in that order, else out.  A GHOST row is inside or in a band on every axis and in a
       band on at least one; its shift on an axis is -1 for the below-wrapped band, +1 for the above-wrapped band, else
       0: the number of box vectors to add along that axis so that the row lies next to the domain.
       out_rows: device memory with room for position->N entries: the owned rows at [0, out_counts[0]), the ghost rows at
       [out_counts[0], out_counts[0] + out_counts[1]), each ascending.  out_shift: device memory with room for 3 x
       position->N int32 entries (the number of ghosts is the call's result); entry 3 k + a is ghost k's shift on axis a.
       out_counts (host): owned, ghost.  Staging as pgsd_select_domain_device: the chunk is staged whole, the call
       synchronises, and the staged rows are kept until the next pgsd_device_wait_read.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): pgsd_select_domain_device's refusals, a band bound
       outside [0, 1]. */
    int pgsd_select_halo_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const float box[6],
                                uint32_t dimensions, const double lo[3], const double hi[3], const double bands[24],
                                const uint32_t divided[3], uint32_t* out_rows, int32_t* out_shift, uint64_t out_counts[2]);

    /* The rows of a frame that satisfy EVERY term of a predicate over per-particle chunks and -- with `position` -- lie
       in a domain, in ascending order (pgsd.hoomd.where_rows is the definition).  Term j -- entry j of the six parallel
       arrays chunks, columns, kinds, lo, hi, sets (n_terms entries each; the layout tests keep this header free of
       structs without a ctypes twin) -- looks at element (row, columns[j]) of chunks[j] (uint32, int32, float32 or
       float64 elements; all chunks of one N < 2^32):
           kind 0, range   with v = (double)x, exact for all four types: kept iff lo <= v < hi.  A NaN v is never kept;
                           a NaN bound leaves that side open (hi = +inf does not: it refuses v = +inf); lo >= hi
                           selects nothing.
           kind 1, set     integer chunks only: kept iff 0 <= x < 64 and bit x of sets[j] is set.
       position / box / dimensions / dlo / dhi: as pgsd_select_domain_device's position, box, dimensions, lo, hi; all NULL
       (dimensions ignored) for a predicate without a domain.  n_terms <= 4; n_terms == 0 needs a domain.
       out_rows: device memory with room for N entries; *out_count (host) receives their number.  Every chunk is staged
       whole into HBM (one that several terms name, once) and the call synchronises; the staged chunks are kept until the
       next pgsd_device_wait_read, so a pgsd_read_rows_device of one of them before it reads no file bytes again.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): another element type, a set on a float chunk,
       column >= M, n_terms > 4, chunks that differ in N, neither a term nor a domain. */
    int pgsd_select_where_device(struct pgsd_handle* handle, uint32_t n_terms, const struct pgsd_index_entry* chunks,
                                 const uint32_t* columns, const uint32_t* kinds, const double* lo, const double* hi,
                                 const uint64_t* sets, const struct pgsd_index_entry* position, const float box[6],
                                 uint32_t dimensions, const double dlo[3], const double dhi[3], uint32_t* out_rows,
                                 uint64_t* out_count);

    /* Domain census: which decomposition to ask for.  Both calls evaluate pgsd_select_domain_device's wrapped fractions
       f[a] of every row of a position chunk (position, box, dimensions: as there) and count instead of selecting; the
       results are host arrays.  A row whose fraction on an axis is NaN (NaN or infinite coordinates) is counted in no
       bin of that axis / in no cell; z takes no part when dimensions == 2.
       pgsd_domain_histogram_device (pgsd.hoomd.axis_histograms is the definition): out_hist[a * bins + k] is the number
       of rows with int(f[a] * bins) == k; bins is a power of two in [2, 4096], so every bin edge k / bins is an exact
       double and no clamp is involved.  The z row is zero when dimensions == 2.
       pgsd_domain_counts_device (pgsd.hoomd.domain_counts): the rows of every cell of an n[0] x n[1] x n[2] grid cut at
       interior_bounds -- the (n[0] - 1) + (n[1] - 1) + (n[2] - 1) interior boundaries, x's, then y's, then z's, each
       axis' strictly ascending inside (0, 1); NULL is allowed for a single cell --: a row's cell on an axis is the number
       of that axis' bounds b with b <= f, out_counts[x + n[0] * (y + n[1] * z)] is the cell's number of rows -- the count
       pgsd_select_domain_device returns for that cell -- and *out_nowhere the number of rows with a NaN fraction on an
       axis that takes part.  1 <= n[a] <= 64 and at most 4096 cells.
       The position chunk is staged whole and the call synchronises; the staged rows are kept until the next
       pgsd_device_wait_read, and both calls look there first: a histogram followed by a count (or by a selection's
       pgsd_read_rows_device) of the same chunk reads its file bytes once.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): pgsd_select_domain_device's refusals; bins not a
       power of two in [2, 4096]; an n[a] of 0 or above 64; more than 4096 cells; bounds that do not ascend strictly
       inside (0, 1); dimensions == 2 with n[2] != 1. */
    int pgsd_domain_histogram_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const float box[6],
                                     uint32_t dimensions, uint32_t bins, uint64_t* out_hist);
    int pgsd_domain_counts_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const float box[6],
                                  uint32_t dimensions, const uint32_t n[3], const double* interior_bounds,
                                  uint64_t* out_counts, uint64_t* out_nowhere);

    /* Cell order: sort a row list by the grid cell of its rows' positions (pgsd.hoomd.cell_ids and cell_order are the
       definitions).  position, box, dimensions: as pgsd_select_domain_device's.  With f[a] the wrapped fraction of a row
       on axis a, i_a = min(int(f[a] * cells[a]), cells[a] - 1) and the row's cell id is i_x + cells[0] * (i_y + cells[1] *
       i_z); a row with a NaN fraction on an axis that takes part gets cells[0] * cells[1] * cells[2], which sorts last;
       z takes no part when dimensions == 2.  1 <= cells[a] <= 1024.
       rows (device, n entries, any order, repeats allowed) is reordered IN PLACE by a stable sort on the cell id: entries
       of one cell keep their order.  Entries [0, n_owned) and [n_owned, n) -- the owned and the ghost run of
       pgsd_select_halo_device; n_owned == n without ghosts -- are sorted separately and stay where they are.  shift
       (device, 3 x (n - n_owned) int32, or NULL): the ghost run's rows of three, permuted like its entries.  out_cell
       (device, n int32, or NULL) receives the sorted cell ids, the ghost run's ascending on their own.
       The position chunk is staged whole unless an earlier selection or census of the same chunk left it staged (then no
       file byte is read), the sort runs on the handle's GPU and the call synchronises; the staged rows are kept until
       the next pgsd_device_wait_read.  n == 0 succeeds and touches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): pgsd_select_domain_device's refusals; a cells[a] of 0
       or above 1024; dimensions == 2 with cells[2] != 1; n_owned > n; n >= 2^32; an entry >= position->N -- found
       before anything of the caller's is written: rows, shift and out_cell are as they were. */
    int pgsd_order_rows_by_cell_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                       const float box[6], uint32_t dimensions, const uint32_t cells[3], uint32_t* rows,
                                       uint64_t n, uint64_t n_owned, int32_t* shift, int32_t* out_cell);

    /* Chunk statistics (pgsd.hoomd.column_stats is the definition, and the results equal it exactly, the sums bit for
       bit).  chunk: N x M elements of float32, float64, int32 or uint32, 1 <= M <= 4, N < 2^32.  rows (device memory, n
       entries, any order, repeats allowed) or NULL: the statistics are those of rows[0 .. n) in list order, or of all
       chunk->N rows (n is then not looked at).  Every element is converted to float64 first, which is exact.  With
       C = M + (with_norm2 ? 1 : 0) columns -- with_norm2 appends the column (x*x + y*y) + z*z in float64, no contraction,
       to a float chunk of three columns -- the results are HOST arrays:
           out_counts[3 c + 0 .. 2]   the entries, those that are NaN, those that are +-infinity
           out_values[3 c + 0 .. 2]   minimum and maximum over the entries that are no NaN (+inf / -inf when there is
                                      none; the sign of a zero is not specified) and the sum of the finite entries
       The sum's order is fixed: entry k belongs to tile k / 4096, lane k % 256, step (k % 4096) / 256; a lane adds its 16
       entries in step order to +0.0 (an entry that is not finite or lies past the end adds +0.0); the 256 lane sums are
       combined by the block tree -- inside each run of 64 lanes p[i] += p[i + h] for h = 32, 16, 8, 4, 2, 1, then
       (w0 + w1) + (w2 + w3) --; lane t of a last workgroup adds the sums of tiles t, t + 256, ... in that order to +0.0
       and the block tree gives the result.  It depends on neither the grid nor the device.
       The chunk is staged whole unless an earlier selection, census, ordering or statistics call of the same chunk left
       it staged (then no file byte is read), the reduction runs on the handle's GPU and the call synchronises; the
       staged rows are kept until the next pgsd_device_wait_read.  n == 0 (or chunk->N == 0 without a list) succeeds with
       zero counts, +inf, -inf and 0.0 and launches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): another element type; M == 0 or M > 4; with_norm2 on
       an integer chunk or with M != 3; chunk->N >= 2^32 or n >= 2^32; an entry >= chunk->N.  out_counts and out_values
       are written on success only. */
    int pgsd_chunk_stats_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk, const uint32_t* rows,
                                uint64_t n, uint32_t with_norm2, uint64_t* out_counts, double* out_values);

    /* Conservation sums (pgsd.hoomd.particle_moments is the definition, and the results equal it exactly, the sums bit
       for bit).  typeid_chunk: N x 1 uint32 or int32; mass, energy: N x 1; velocity, position: N x 3; the four float
       chunks hold float32 or float64, all the same; every chunk that is given has the same N < 2^32.  A chunk that is
       NULL is stored nowhere: defaults -- mass, v[3], energy, x[3] -- holds the row that stands for each of its rows, and
       a NULL typeid_chunk puts every entry into one group (n_types must be 1).  rows (device memory, n entries, any
       order, repeats allowed) or NULL: the entries are rows[0 .. n) in list order, or all N rows; when no chunk is given
       and rows is NULL, n is the number of entries.  Every element is converted to float64 first.  Per entry nine
       values, in this association and without a fused multiply-add:
           0 m   1..3 m * v[a]   4 (0.5 * m) * ((vx*vx + vy*vy) + vz*vz)   5 m * e   6..8 m * x[a]
       Per type t of [type0, type0 + n_types), 1 <= n_types <= 4, the results are HOST arrays:
           out_counts[2 t + 0 .. 1]   the entries of the type, those of them with a value that is not finite
           out_counts[2 n_types]      the entries of no type of the group (a negative int32 id is one)
           out_sums[9 t + q]          the sum, in pgsd_chunk_stats_device's order, of value q over the list's entries, an
                                      entry of another type or a value that is not finite counting as +0.0
       The chunks are staged whole unless an earlier selection, census, ordering, statistics or moments call left them
       staged (then no file byte is read), the reduction runs on the handle's GPU and the call synchronises; the staged
       rows are kept until the next pgsd_device_wait_read.  No entry succeeds with zeros and launches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): a float chunk of another element type, or of both;
       a typeid chunk that is neither uint32 nor int32; a wrong number of columns; chunks that differ in N; n_types of 0
       or above 4; a NULL typeid_chunk with n_types != 1; N or n >= 2^32; an entry >= N.  out_counts and out_sums are
       written on success only. */
    int pgsd_frame_moments_device(struct pgsd_handle* handle, const struct pgsd_index_entry* typeid_chunk,
                                  const struct pgsd_index_entry* mass, const struct pgsd_index_entry* velocity,
                                  const struct pgsd_index_entry* energy, const struct pgsd_index_entry* position,
                                  const double defaults[8], uint32_t type0, uint32_t n_types, const uint32_t* rows,
                                  uint64_t n, uint64_t* out_counts, double* out_sums);

    /* Frame displacements (pgsd.hoomd.particle_displacements is the definition, and the results equal it exactly, the
       sums bit for bit).  Row k of frame a and row k of frame b are one particle.  position_a, position_b: N x 3 float32
       or float64, both the same; image_a, image_b: N x 3 int32, or NULL: stored nowhere, (0, 0, 0) in every row;
       typeid_chunk: N x 1 uint32 or int32, or NULL: one group (n_types must be 1); every chunk has the same N < 2^32.
       vectors_a, vectors_b: Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz of each frame's box as float64 (pgsd.hoomd.box_vectors: the
       products are rounded once, by the caller).  rows (device memory, n entries, any order, repeats allowed) or NULL:
       the entries are rows[0 .. n) in list order, or all N rows.  Every element is converted to float64 first; no fused
       multiply-add.  Per entry and frame, with i the image:
           u[0] = x[0] + ((i[0]*Lx + i[1]*xyLy) + i[2]*xzLz)   u[1] = x[1] + (i[1]*Ly + i[2]*yzLz)   u[2] = x[2] + i[2]*Lz
       (u = x without an image chunk), d = u_b - u_a; with bit 0 of flags, the minimum image (no image chunk allowed), d
       is folded with frame b's vectors: n = rint(d[2] / Lz), d[2] -= n*Lz, d[1] -= n*yzLz, d[0] -= n*xzLz (dimensions
       == 3 only), n = rint(d[1] / Ly), d[1] -= n*Ly, d[0] -= n*xyLy, n = rint(d[0] / Lx), d[0] -= n*Lx, rint rounding
       half to even; s = (d[0]*d[0] + d[1]*d[1]) + d[2]*d[2].
       Per type t of [type0, type0 + n_types), 1 <= n_types <= 4, the results are HOST arrays:
           out_counts[3 t + 0 .. 2]   the entries of the type, those of them where a d[a] or s is not finite, and the
                                      smallest entry (a position in rows, else a row) that attains the largest s
                                      (UINT64_MAX when no entry of the type has an s that is a number)
           out_counts[3 n_types]      the entries of no type of the group (a negative int32 id is one)
           out_values[5 t + 0 .. 3]   the sums, in pgsd_chunk_stats_device's order, of d[0], d[1], d[2] and s over the
                                      list's entries, an entry of another type or a value that is not finite counting
                                      as +0.0
           out_values[5 t + 4]        the largest s over the entries of the type where s is no NaN; -inf without one
       out_rows (device memory, n x 3 float64, n the number of entries) or NULL: entry k's d at out_rows[3 k .. 3 k + 2].
       The chunks are staged whole unless an earlier call left them staged (then no file byte is read); two chunks that
       are one stored chunk -- an elided position both frames read from frame 0 -- are staged once.  The reduction runs
       on the handle's GPU and the call synchronises; the staged rows are kept until the next pgsd_device_wait_read.
       No entry succeeds with zero counts, +0.0, -inf and UINT64_MAX and launches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): positions of another element type, or of both; an
       image that is not int32; a typeid that is neither uint32 nor int32; a wrong number of columns; chunks that differ
       in N; n_types of 0 or above 4; a NULL typeid_chunk with n_types != 1; the minimum image together with an image
       chunk; another bit of flags; dimensions not 2 or 3; N or n >= 2^32; an entry >= N (out_rows beyond such an entry
       is unspecified).  out_counts and out_values are written on success only. */
    int pgsd_frame_displacements_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position_a,
                                        const struct pgsd_index_entry* image_a, const struct pgsd_index_entry* position_b,
                                        const struct pgsd_index_entry* image_b, const struct pgsd_index_entry* typeid_chunk,
                                        const double vectors_a[6], const double vectors_b[6], uint32_t flags,
                                        uint32_t dimensions, uint32_t type0, uint32_t n_types, const uint32_t* rows,
                                        uint64_t n, double* out_rows, uint64_t* out_counts, double* out_values);

    /* CSR offsets of a cell list in cell order (pgsd.hoomd.cell_offsets is the definition).  cell (device memory, n
       int32 entries, non-decreasing, in [0, n_cells]; n_cells is pgsd_order_rows_by_cell_device's "nowhere" id).
       out_offsets (device memory, n_cells + 2 words): out_offsets[c] is the first position whose id is not below c --
       the first entry of cell c --, out_offsets[n_cells + 1] == n.  Runs on the handle's GPU and synchronises.  n == 0
       writes zeros.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), out_offsets as it was: an id that is below its
       predecessor or outside [0, n_cells]; n >= 2^32; n_cells of 0 or above 2^20. */
    int pgsd_cell_offsets_device(struct pgsd_handle* handle, const int32_t* cell, uint64_t n, uint32_t n_cells,
                                 uint32_t* out_offsets);

    /* Cell fields (pgsd.hoomd.cell_moments is the definition, and the results equal it exactly, the sums bit for bit).
       mass, velocity, energy, position, defaults: as pgsd_frame_moments_device's, and so are the nine values per entry.
       rows (device memory, n entries) and cell (device memory, n int32 entries, non-decreasing, in [0, n_cells]) are a
       row list in cell order and the ids of its entries, as pgsd_order_rows_by_cell_device leaves them; an entry with
       id n_cells is nowhere and is summed nowhere.  The results are HOST arrays:
           out_counts[2 c + 0 .. 1]   the entries of cell c, those of them with a value that is not finite
           out_counts[2 n_cells]      the entries nowhere
           out_sums[9 c + q]          the sum of value q over the cell's entries, a value that is not finite counting as
                                      +0.0, in the cell's own order
       The order: the cell's entries in list order are cut into pieces of 1024 from the cell's first entry; in a piece lane
       l of 64 adds entries l, l + 64, ..., l + 960 in that order to +0.0 (an entry past the end adds +0.0); the 64 lane
       sums are combined by p[i] += p[i + h] for h = 32, 16, 8, 4, 2, 1; the piece sums are added to +0.0 in ascending
       order.  A cell without entries has sums of +0.0.  It depends on neither the grid of the launch nor the device.
       The chunks are staged whole unless an earlier call left them staged (then no file byte is read), the reduction runs
       on the handle's GPU and the call synchronises; the staged rows are kept until the next pgsd_device_wait_read.
       n == 0 succeeds with zeros and launches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(): pgsd_frame_moments_device's refusals for the chunks;
       pgsd_cell_offsets_device's; an entry >= N.  out_counts and out_sums are written on success only. */
    int pgsd_cell_moments_device(struct pgsd_handle* handle, const struct pgsd_index_entry* mass,
                                 const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* energy,
                                 const struct pgsd_index_entry* position, const double defaults[8], const uint32_t* rows,
                                 const int32_t* cell, uint64_t n, uint32_t n_cells, uint64_t* out_counts, double* out_sums);

    /* Neighbour census (pgsd.hoomd.particle_neighbours is the definition, and the results equal it exactly: every
       counter and index, the two distances bit for bit).  position: an N x 3 float32 or float64 chunk.  vectors:
       (Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz) of the box, r the range, cells the grid (cx, cy, cz; cz == 1 with dimensions ==
       2).  rows (device memory, n entries) and cell (device memory, n int32 entries, non-decreasing, in [0, n_cells]) are
       a row list in cell order and the ids of its entries, as pgsd_order_rows_by_cell_device leaves them for the same
       grid; an entry with id n_cells is nowhere and is nobody's neighbour.
       Entry j is a CANDIDATE of entry i when j != i as a list position (the same row listed twice is two entries), both
       have a cell and j's cell is periodically adjacent to i's: per axis the offsets {0} at one cell, {0, +1} at two and
       {-1, 0, +1} otherwise, indices wrapping.  The DISTANCE of i -> j, float64 from the stored values, no contraction:
       d = x_j - x_i; if d_z >= Lz/2 subtract (xz*Lz, yz*Lz, Lz), else if d_z < -(Lz/2) add it (dimensions == 3 only;
       otherwise d_z = 0); the same for y with Ly/2 and (xy*Ly, Ly), then for x with Lx/2 and Lx; d2 = (d_x*d_x +
       d_y*d_y) + d_z*d_z.  j is a NEIGHBOUR when d2 < r*r, strictly, r*r formed once.
       Device outputs, n entries each, each optional (NULL):
           out_count[k]      the neighbours of entry k
           out_nearest2[k]   the smallest d2 among them, +inf without one
           out_nearest[k]    the smallest list position that attains it, 0xFFFFFFFF without one
       Host outputs:
           out_summary[0 .. 7]       n; the entries nowhere; the sum of the counts (ordered pairs); the smallest and the
                                     largest count over the entries that have a cell (0 without one); the smallest list
                                     position whose nearest2 is the smallest; that entry's row and its nearest's row (the
                                     last three 0xFFFFFFFF where no entry has a neighbour)
           out_summary[8 + k]        k < 256: the entries that have a cell and k neighbours; k == 256: 256 or more
           out_summary[265 + b]      b < bins: the neighbour pairs with edges2[b] <= d2 < edges2[b + 1] -- the bin
                                     searchsorted(edges2, d2, 'right') - 1; a pair outside the edges is in no bin
           *out_closest2             the smallest nearest2, +inf where no entry has a neighbour
       edges2: a HOST array of bins + 1 doubles (pgsd.hoomd.neighbour_edges2), copied as it is: the GPU never recomputes
       an edge.  bins == 0: no pair histogram, edges2 may be NULL.
       The chunk is staged whole unless an earlier call (the ordering) left it staged, the search runs on the handle's GPU
       and the call synchronises; the staged rows are kept until the next pgsd_device_wait_read.  n == 0 succeeds with
       the summary of no entry and launches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: a chunk that is not float32
       or float64 or has another column count than 3; N or n >= 2^32; dimensions other than 2 or 3; r not finite or not
       positive; a box length that is not positive; a count outside 1 to 1024, cz != 1 with dimensions == 2, more than
       2^20 cells; r above half the nearest plane distance of an axis that takes part (an image would count twice); a
       count above floor(plane distance / r) (cells narrower than r); bins > 1024; edges that descend or are not numbers;
       an id that is below its predecessor or outside [0, n_cells]; an entry >= N. */
    int pgsd_neighbours_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const double vectors[6],
                               double r, uint32_t dimensions, const uint32_t cells[3], const uint32_t* rows,
                               const int32_t* cell, uint64_t n, uint32_t bins, const double* edges2, uint32_t* out_count,
                               double* out_nearest2, uint32_t* out_nearest, uint64_t* out_summary, double* out_closest2);

    /* Neighbour lists (pgsd.hoomd.neighbour_list is the definition, and the results equal it exactly: every offset and
       index, every distance bit for bit): the neighbours pgsd_neighbours_device counts, handed over as a CSR pair list.
       position, vectors, r, dimensions, cells, rows, cell and n are pgsd_neighbours_device's, and so are the candidates,
       the distance of one pair and the strict test d2 < r*r.  flags: bit 0 is the HALF list; every other bit is refused.
       The SEGMENT of entry i holds the list positions j of its neighbours, j != i as a list position (with the half list:
       j > i, the same filter of the same segment), in the order the SPH kernel sums define: oz over the offsets of the z
       axis, inside it oy, inside it ox, the cell ((ix+ox) % cx, (iy+oy) % cy, (iz+oz) % cz), inside a cell ascending list
       position.  An entry without a cell has an empty segment and is in nobody's.  The size of the list is not known
       before it is counted, so it is made in two calls.

       pgsd_neighbour_offsets_device counts and scans:
           out_offsets   device memory, n + 1 uint64: out_offsets[0] = 0, out_offsets[k + 1] - out_offsets[k] the length
                         of entry k's segment, out_offsets[n] the pairs
           out_summary   host, 4 uint64: n; the entries nowhere; the pairs; the longest segment (0 at n == 0)
       The chunk is staged whole unless an earlier call (the ordering) left it staged, the pass runs on the handle's GPU
       and the call synchronises; the staged rows are kept until the next pgsd_device_wait_read.  n == 0 stages nothing
       and launches no kernel: out_offsets[0] = 0 is one memset on the pipeline's stream, the summary is four zeros.

       pgsd_neighbour_list_device fills the segments:
           offsets         device memory, n + 1 uint64, as the call above left them for the SAME arguments
           capacity        the entries out_neighbours (and out_distance2) have room for
           out_neighbours  device memory, capacity uint32: the list positions j, segment after segment
           out_distance2   device memory, capacity doubles, or NULL: d2 of each pair
       No store lands at an index >= capacity or outside [offsets[k], offsets[k + 1]) of the entry k it belongs to.  Where
       an entry finds another number of neighbours than its segment holds, the offsets descend or do not begin at 0, or
       offsets[n] > capacity, the call is refused: PGSD_ERROR_INVALID_ARGUMENT, and the message says that the capacity is
       too small (naming it and offsets[n]) or that the offsets do not belong to this list.  After such a refusal the
       output arrays are unspecified inside the capacity and untouched outside it.  n == 0 fills nothing and launches
       nothing.  The chunk is taken from what the first call left staged (or staged again after a wait_read).

       Both calls refuse everything pgsd_neighbours_device refuses (but for the pair histogram, which they do not have),
       with its messages; out_offsets and out_summary are written on success only. */
    int pgsd_neighbour_offsets_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                      const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                      const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t flags,
                                      uint64_t* out_offsets, uint64_t* out_summary);
    int pgsd_neighbour_list_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                   const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                   const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t flags,
                                   const uint64_t* offsets, uint64_t capacity, uint32_t* out_neighbours,
                                   double* out_distance2);

    /* Components (pgsd.hoomd.neighbour_components is the definition, and the results equal it exactly: every word is an
       integer and none depends on an order of evaluation): the friends-of-friends grouping of a row list in cell order
       with the linking length r -- the connected components of the graph whose EDGES are the pairs of the half list of
       pgsd_neighbour_offsets_device / pgsd_neighbour_list_device for the same arguments: i and j, i < j by list position,
       are joined iff i -> j lies strictly inside the range (d2 < r*r).  A row listed twice is two entries at distance 0,
       and the two are joined; an entry without a cell has no edge and is a component of its own.  position, vectors, r,
       dimensions, cells, rows, cell and n are pgsd_neighbour_offsets_device's, and the call refuses everything that call
       refuses, with its messages and in its order.  flags must be 0: any set bit is refused.
           out_label      device memory, n uint32, required for n > 0: the smallest list position of the entry's
                          component (while the pass runs it is the parent array of a lock-free union-find)
           out_component  device memory, n uint32, or NULL: the dense id -- the number of components whose label is
                          smaller, so that components are numbered in ascending order of their smallest member
           out_sizes      device memory with room for n uint32, or NULL: the first `components` words are defined,
                          out_sizes[c] the entries of component c
           out_summary    host, 6 uint64, written on success only: n; the entries nowhere; the components; the
                          singletons (components of one entry, the nowhere entries among them); the largest size; the
                          label of the largest component, among equal sizes the smallest label
       No store lands at an index >= n of any output.  The chunk is staged whole unless an earlier call (the ordering)
       left it staged, the pass runs on the handle's GPU on the pipeline's stream and the call synchronises; the staged
       rows are kept until the next pgsd_device_wait_read.  n == 0 stages nothing and launches no kernel: the summary is
       six zeros.  Every loop on the GPU that depends on other lanes carries a hard cap; a pass that reaches it gives up:
       PGSD_ERROR_DEVICE, "the pass gave up: internal error", instead of a wrong result (the outputs are unspecified). */
    int pgsd_components_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const double vectors[6],
                               double r, uint32_t dimensions, const uint32_t cells[3], const uint32_t* rows,
                               const int32_t* cell, uint64_t n, uint32_t flags, uint32_t* out_label,
                               uint32_t* out_component, uint32_t* out_sizes, uint64_t* out_summary);

    /* Component fields (pgsd.hoomd.component_moments is the definition, and the results equal it exactly, every float bit
       for bit): what each piece of a pgsd_components_device result IS -- per component the nine sums of
       pgsd_cell_moments_device with the position replaced by the displacement d from the component's ROOT (the entry at
       list position `label`, its smallest member) to the entry under HOOMD's single-shift minimum image (the arithmetic
       of one pair of pgsd_neighbours_device; the root's own d is +0.0 by definition), the extent of those displacements
       and the root's position.  The order of a component's sum is the cell fields' over the component's entries in list
       order.  mass, velocity, energy, position and defaults are pgsd_cell_moments_device's; the position chunk is
       required (a position that is stored nowhere is refused).  vectors: Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz; dimensions: 2
       or 3 (2: z is never looked at and d_z is 0).  rows, label, component: device memory, n uint32 each, the list and
       what pgsd_components_device wrote for it; components: its summary's third word.  flags must be 0.
           out_sums     device memory, components x 9 float64: mass, momentum[3], kinetic, internal, sum of m d[3]
           out_extent   device memory, components x 6 float64: lo[3], hi[3] of the finite d of the component, from +0.0
                        (the root's) by strict comparisons: neither is ever -0.0
           out_origin   device memory, components x 3 float64: the root's position
           out_flags    device memory, components x 2 uint32: the entries with a value that is not finite, and `wide`:
                        1 if hi - lo >= L / 2 on an axis below `dimensions` -- the piece percolates or nearly does, and
                        its origin-relative centre and extent are reported but not meaningful; 0 guarantees that d is
                        the piece's one consistent unwrapping
           out_summary  host, 6 uint64, written on success only: n; components; the bad entries; the wide components;
                        the id of the largest mass sum and of the largest extent over the axes, among equals the smallest
                        id (a sum that is a NaN counts as -inf)
       No store lands at an index >= components of any output.  Refused, with no output touched: label[k] > k, a label
       that is no root, an id >= components, an id other than its root's, ids that are not the dense ascending numbering
       of the labels, rows[k] >= N.  The chunks are staged whole unless an earlier call left them staged; the pass runs on
       the pipeline's stream and the call synchronises; the staged rows are kept until the next pgsd_device_wait_read.
       n == 0 stages nothing and launches no kernel: the summary is six zeros. */
    int pgsd_component_moments_device(struct pgsd_handle* handle, const struct pgsd_index_entry* mass,
                                      const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* energy,
                                      const struct pgsd_index_entry* position, const double defaults[8],
                                      const double vectors[6], uint32_t dimensions, const uint32_t* rows, const uint32_t* label,
                                      const uint32_t* component, uint64_t n, uint64_t components, uint32_t flags,
                                      double* out_sums, double* out_extent, double* out_origin, uint32_t* out_flags,
                                      uint64_t* out_summary);

    /* SPH kernel sums (pgsd.hoomd.sph_kernel_sums is the definition, and the results equal it exactly: every counter and
       index, every float bit for bit -- a NaN is a NaN, its sign and payload are the processor's).  position: an N x 3
       float32 or float64 chunk; mass, density: N x 1 float32 or float64 chunks, each of its own element type, either may
       be NULL: defaults[0] then stands for every mass and defaults[1] for every density, and with density == NULL and
       defaults[1] a NaN there is NO VOLUME: no third sum, no deviation, no surface count.  vectors, dimensions, cells,
       rows, cell and n are pgsd_neighbours_device's; the range of the search is the support 2h, so the cells are no
       narrower than 2h.  kernel: 0 Wendland C2, 1 cubic spline.
       On the host, once, in float64: r2 = (2h)*(2h), inv_h = 1/h and sigma = 21/(16 pi h^3) (3-D) or 7/(4 pi h^2) (2-D)
       for Wendland C2, 1/(pi h^3) or 10/(7 pi h^2) for the cubic spline; the GPU receives them and never recomputes them.
       ONE PAIR i <- j, float64 from the stored values, no contraction: d2 as pgsd_neighbours_device forms it; j
       contributes when d2 < r2, strictly; i itself contributes (list position j == i: d2 = 0, w = 1) and the same row
       listed twice is two entries; rr = sqrt(d2), q = rr * inv_h;
           Wendland C2    t = 1.0 - 0.5*q, t2 = t*t, w = (t2*t2) * (2.0*q + 1.0)
           cubic spline   q2 = q*q; if q < 1.0: w = (1.0 - 1.5*q2) + 0.75*(q2*q), else u = 2.0 - q, w = 0.25*((u*u)*u)
       Three accumulators per entry start at +0.0: a_n += w, a_m += m_j * w, a_v += V_j * w with V_j = m_j / rho_j, one
       float64 division of the stored values taken as it is (rho_j == 0 gives what IEEE gives).
       THE ORDER of the candidates is part of the definition: the cells with oz over the offsets of the z axis ({0} at one
       cell, {0, +1} at two, {-1, 0, +1} otherwise, in that order), inside it oy, inside it ox, the cell ((ix+ox) % cx,
       (iy+oy) % cy, (iz+oz) % cz); inside a cell ascending list position.  After the last candidate number = sigma*a_n,
       density = sigma*a_m, shepard = sigma*a_v.  An entry with id n_cells is nowhere: it contributes to nobody and its
       three values are +0.0.
       Device outputs, n float64 entries each, each optional (NULL): out_number, out_density, out_shepard (the last is
       not written where there is no volume).
       Host output, 13 words:
           out_summary[0 .. 3]    n; the entries nowhere; the entries that have a cell and whose density sum is NaN or
                                  infinite; the entries that have a cell and shepard < surface_below, strictly (0 without
                                  a volume or with surface_below a NaN: none asked for)
           out_summary[4], [5]    the list position of the deviation and its row, 0xFFFFFFFF without one
           out_summary[6 .. 11]   as float64 bit patterns the minimum and the maximum of number, of density and of shepard
                                  over the entries that have a cell, kept by strict compares from +inf and -inf: a NaN
                                  never replaces a value (shepard without a volume: +inf, -inf)
           out_summary[12]        as a float64 bit pattern the deviation density_i - (double)rho_i of the largest
                                  magnitude over the entries that have a cell, its sign kept, the smaller list position
                                  on a tie, a NaN never; +0.0 without one
       No float is summed over the list, so the summary depends on no order.  The chunks are staged whole unless an
       earlier call (the ordering, a selection) left them staged, the pass runs on the handle's GPU and the call
       synchronises; the staged rows are kept until the next pgsd_device_wait_read.  n == 0 succeeds with the summary of
       no entry and launches nothing.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_neighbours_device refuses for the range 2h; a mass or density chunk that is not one float32 or float64
       column or has another N than position; h not finite or not positive; an unknown kernel. */
    int pgsd_sph_sums_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                             const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                             const double defaults[2], const double vectors[6], double h, uint32_t kernel,
                             uint32_t dimensions, const uint32_t cells[3], const uint32_t* rows, const int32_t* cell,
                             uint64_t n, double surface_below, double* out_number, double* out_density,
                             double* out_shepard, uint64_t* out_summary);

    /* The range of a smoothing-length chunk over a row list (pgsd.hoomd.smoothing_range is the definition): what a caller
       needs before it can choose the grid of pgsd_sph_adaptive_sums_device, without copying a row to the host.  slength:
       one float32 or float64 column of N rows, or NULL: h_default stands for every row (nothing is read).  rows: device,
       n entries < N, or NULL: every row.  h is valid when h > 0.0 and h < +inf.
       Host output, 4 words: the entries; those whose h is not valid; as float64 bit patterns the smallest and the largest
       valid h (+inf and -inf without one).  A minimum and a maximum: no order enters.  Staging and synchronisation are
       pgsd_chunk_stats_device's.  PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), out_words as it was: a
       chunk that is no such column, an entry >= N. */
    int pgsd_sph_smoothing_range_device(struct pgsd_handle* handle, const struct pgsd_index_entry* slength, double h_default,
                                        const uint32_t* rows, uint64_t n, uint64_t N, uint64_t* out_words);

    /* SPH sums with a per-particle smoothing length (pgsd.hoomd.sph_adaptive_sums is the definition, and the results equal
       it exactly: every counter and index, every float bit for bit -- a NaN is a NaN).  position, mass, density, vectors,
       kernel, dimensions, cells, rows, cell, n and surface_below are pgsd_sph_sums_device's.  slength: one float32 or
       float64 column of the position chunk's N rows, or NULL.  defaults: the mass, the density (NaN: no volume sum) and
       the smoothing length that stand for a chunk stored nowhere.  h_max: the declared bound of the listed valid
       smoothing lengths; the grid, every refusal and THE ORDER of the candidates are pgsd_sph_sums_device's for h = h_max.
       mode: 0 gather, 1 mean.
       h is VALID when h > 0.0 and h < +inf.  An entry whose h is not valid is treated like an entry nowhere: it contributes
       to nobody and every per-entry output of it is +0.0, written; it is counted in bad_h (if it has a cell), not in
       nowhere.  An entry is LIVE when it has a cell and a valid h.
       ONE PAIR i <- j, float64, no contraction, d2 as pgsd_sph_sums_device; i itself and coincident entries are candidates.
       gather: once per entry s_i = 2.0*h_i, r2_i = s_i*s_i, inv_i = 1.0/h_i; j contributes when d2 < r2_i, strictly; rr =
       sqrt(d2), q = rr*inv_i, w = w(q), F = F(q) of pgsd_sph_gradients_device; a_n += w, a_m += m_j*w, a_v += V_j*w (with a
       volume), a_o += m_j*(D*w + (q*q)*F) with D = 2.0 or 3.0, count += 1.  After the last candidate sigma_i = the sums'
       sigma for h_i, number = sigma_i*a_n, density = sigma_i*a_m, shepard = sigma_i*a_v, omega = 1.0 - a_o/(D*a_m).
       mean: s = h_i + h_j, j contributes when d2 < s*s; hij = 0.5*s, ih = 1.0/hij, q = sqrt(d2)*ih, w = w(q), p = ih*ih (2-D)
       or (ih*ih)*ih (3-D), wp = w*p; a_n += wp, a_m += m_j*wp, a_v += V_j*wp, count += 1; afterwards number = C*a_n and so
       on with C the sums' sigma for h = 1.0; out_omega is not written.
       Device outputs, each optional (NULL): out_count, n uint32; out_number, out_density, out_shepard (with a volume
       only), out_omega (gather only), n float64.
       Host output, 22 words:
           out_summary[0 .. 4]    n; the entries nowhere; bad_h; the live entries whose density is NaN or infinite; the
                                  live entries with shepard < surface_below
           out_summary[5], [6]    the list position of the deviation and its row, with pgsd_sph_sums_device's rule over the
                                  live entries; 0xFFFFFFFF without one
           out_summary[7 .. 9]    the smallest and the largest count over the live entries and the list position of the
                                  smallest (the smaller position on a tie); 0, 0, 0xFFFFFFFF without one
           out_summary[10 .. 19]  as float64 bit patterns the minimum and maximum of slength, number, density, shepard and
                                  omega over the live entries, by strict compares from +inf and -inf: a NaN never replaces a
                                  value (shepard without a volume and omega in mean mode: +inf, -inf)
           out_summary[20]        as a float64 bit pattern the deviation; +0.0 without one
           out_summary[21]        pairs, the exact sum of count
       No float is summed over the list.  Staging, synchronisation and n == 0 are pgsd_sph_sums_device's.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_sph_sums_device refuses for the range 2*h_max; an unknown mode; a slength chunk that is not one float32 or
       float64 column of N rows; an h_max that is not valid; a listed valid h above h_max (found on the device). */
    int pgsd_sph_adaptive_sums_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                      const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                                      const struct pgsd_index_entry* slength, const double defaults[3],
                                      const double vectors[6], double h_max, uint32_t kernel, uint32_t mode,
                                      uint32_t dimensions, const uint32_t cells[3], const uint32_t* rows, const int32_t* cell,
                                      uint64_t n, double surface_below, uint32_t* out_count, double* out_number,
                                      double* out_density, double* out_shepard, double* out_omega, uint64_t* out_summary);

    /* SPH kernel gradients (pgsd.hoomd.sph_kernel_gradients is the definition, and the results equal it exactly: every
       counter and index, every float bit for bit -- a NaN is a NaN).  position, mass, density, defaults, vectors, h,
       kernel, dimensions, cells, rows, cell and n are pgsd_sph_sums_device's, and so are the grid, the support 2h, r2,
       inv_h, sigma, V_j = m_j / rho_j, "no volume" and THE ORDER of the candidates.  velocity: an N x 3 float32 or float64
       chunk of its own element type, or NULL: the zero vector stands for every row.
       On the host, once, in float64: G = -((sigma*inv_h)*inv_h).
       ONE PAIR i <- j, float64 from the stored values (converted before any subtraction), no contraction: d = x_j - x_i
       under the minimum image and d2 as pgsd_neighbours_device forms them; j contributes when d2 < r2, strictly; i itself
       and coincident entries are candidates like any other (d = 0, so their terms are zero); rr = sqrt(d2), q = rr * inv_h;
           Wendland C2    t = 1.0 - 0.5*q, F = -5.0 * ((t*t)*t)
           cubic spline   if q < 1.0: F = 2.25*q - 3.0, else u = 2.0 - q, F = (-0.75*(u*u)) / q
       e_k = F * d_k (grad_i W_ij = G * e), u_k = v_j[k] - v_i[k], dot = (u0*e0 + u1*e1) + u2*e2, c0 = e1*u2 - e2*u1,
       c1 = e2*u0 - e0*u2, c2 = e0*u1 - e1*u0.  Eight accumulators per entry start at +0.0 and add in the defined order:
       a_r += m_j * dot, a_d += V_j * dot, a_w[k] += V_j * c_k, a_c[k] += V_j * e_k.  After the last candidate
       density_rate = -(G*a_r), divergence = G*a_d, curl[k] = G*a_w[k], normal[k] = G*a_c[k].  An entry with id n_cells is
       nowhere: it contributes to nobody and all its values are +0.0.  With dimensions == 2 d_z is 0 and nothing else
       differs.
       Device outputs, float64, each optional (NULL): out_density_rate and out_divergence, n entries; out_curl and
       out_normal, n x 3.  The last three are not written where there is no volume.
       Host output, 13 words:
           out_summary[0 .. 2]    n; the entries nowhere; the entries that have a cell and whose density_rate is NaN or
                                  infinite
           out_summary[3], [4]    the list position of the largest curl and its row; [5], [6] the same of the largest
                                  normal; 0xFFFFFFFF without one
           out_summary[7 .. 10]   as float64 bit patterns the minimum and the maximum of divergence and of density_rate
                                  over the entries that have a cell, kept by strict compares from +inf and -inf: a NaN
                                  never replaces a value (divergence without a volume: +inf, -inf)
           out_summary[11], [12]  as float64 bit patterns the largest curl2 = (c0*c0 + c1*c1) + c2*c2 of the outputs and
                                  the largest normal2 over the entries that have a cell, the smaller list position on a
                                  tie, a NaN never; +0.0 without one
       No float is summed over the list.  Staging, synchronisation and n == 0 are pgsd_sph_sums_device's.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_sph_sums_device refuses; a velocity chunk that is not three float32 or float64 columns or has another N than
       position. */
    int pgsd_sph_gradients_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                  const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                  const struct pgsd_index_entry* density, const double defaults[2], const double vectors[6],
                                  double h, uint32_t kernel, uint32_t dimensions, const uint32_t cells[3],
                                  const uint32_t* rows, const int32_t* cell, uint64_t n, double* out_density_rate,
                                  double* out_divergence, double* out_curl, double* out_normal, uint64_t* out_summary);

    /* SPH gradient tensors (pgsd.hoomd.sph_gradient_tensors is the definition, and the results equal it exactly: every
       counter and index, every float bit for bit -- a NaN is a NaN).  position, velocity, mass, density, vectors, h,
       kernel, dimensions, cells, rows, cell and n are pgsd_sph_gradients_device's, and so are the grid, the support 2h, r2,
       inv_h, sigma, G, F(q), V_j = m_j / rho_j and THE ORDER of the candidates.  defaults: the mass and the density that
       stand for a chunk stored nowhere (the density default is a number here: there is no "no volume").  det_min: an entry
       is corrected where det_min < det < +inf; a convention of the caller's, not a tuned figure (an interior particle has
       det near 1, a flat free surface about one half).
       ONE PAIR i <- j, float64, no contraction: d, d2, the strict test d2 < r2, rr, q, F, e_k = F * d_k and u_k = v_j[k] -
       v_i[k] as in the gradients; i itself and coincident entries are candidates like any other.  Fifteen accumulators
       per entry start at +0.0 and add in the defined order:
           b_ab += V_j * (d_a * e_b)   for ab in (00, 01, 02, 11, 12, 22)
           g_ab += V_j * (u_a * e_b)   for all nine ab: row a the velocity component, column b the derivative direction
       AFTER THE LAST CANDIDATE, every product and sum in the association shown: B_ab = G*b_ab, R_ab = G*g_ab (R is the
       uncorrected dv_a/dx_b); with dimensions == 3
           c00 = B11*B22 - B12*B12, c01 = B02*B12 - B01*B22, c02 = B01*B12 - B02*B11,
           c11 = B00*B22 - B02*B02, c12 = B01*B02 - B00*B12, c22 = B00*B11 - B01*B01,
           det = (B00*c00 + B01*c01) + B02*c02
       and with dimensions == 2 (d_z is 0, the z row and column of B vanish)
           det = B00*B11 - B01*B01, c00 = B11, c01 = -B01, c11 = B00, c02 = c12 = c22 = +0.0;
       ok = det > det_min and det < +inf (a NaN is never ok).  Where ok: L_ab = c_ab / det (2-D: the three z entries are
       +0.0, written) and D_ab = (R_a0*L_0b + R_a1*L_1b) + R_a2*L_2b (2-D: D_ab = R_a0*L_0b + R_a1*L_1b for b < 2 and D_a2 =
       +0.0, written).  Where not ok: L is the identity (2-D: diag(1, 1, 0)) and D_ab = R_ab, both written, not computed.
           trace = (D00 + D11) + D22, s01 = 0.5*(D01 + D10), s02 = 0.5*(D02 + D20), s12 = 0.5*(D12 + D21),
           ss = ((D00*D00 + D11*D11) + D22*D22) + 2.0*((s01*s01 + s02*s02) + s12*s12), shear_rate = sqrt(2.0*ss).
       An entry with id n_cells is nowhere: it contributes to nobody and all its values are +0.0, written.
       Device outputs, float64, each optional (NULL): out_correction, n x 6 (xx, xy, xz, yy, yz, zz); out_determinant, n;
       out_velocity_gradient, n x 9, row-major; out_shear_rate, n.
       Host output, 14 words:
           out_summary[0 .. 2]    n; the entries nowhere; the entries that have a cell and whose shear_rate is NaN or
                                  infinite
           out_summary[3]         the entries that have a cell and are not ok (uncorrected)
           out_summary[4], [5]    the list position of the smallest determinant and its row: a strict compare from +inf,
                                  the smaller list position on a tie, a NaN never; 0xFFFFFFFF without one
           out_summary[6], [7]    the same of the largest shear_rate (any value that is no NaN counts)
           out_summary[8 .. 11]   as float64 bit patterns the minimum and the maximum of the determinant and of the trace
                                  over the entries that have a cell, kept by strict compares from +inf and -inf in
                                  which -0.0 is below +0.0 (both occur, and no bound depends on an order): a NaN never
                                  replaces a value
           out_summary[12]        as a float64 bit pattern the largest shear_rate; +0.0 without one
           out_summary[13]        0
       No float is summed over the list.  Staging, synchronisation and n == 0 are pgsd_sph_sums_device's.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_sph_gradients_device refuses; a det_min that is NaN or negative. */
    int pgsd_sph_tensors_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                const struct pgsd_index_entry* density, const double defaults[2], const double vectors[6],
                                double h, uint32_t kernel, uint32_t dimensions, double det_min, const uint32_t cells[3],
                                const uint32_t* rows, const int32_t* cell, uint64_t n, double* out_correction,
                                double* out_determinant, double* out_velocity_gradient, double* out_shear_rate,
                                uint64_t* out_summary);

    /* SPH accelerations (pgsd.hoomd.sph_accelerations is the definition, and the results equal it exactly: every counter
       and index, every float bit for bit -- a NaN is a NaN).  position, velocity, mass, density, vectors, h, kernel,
       dimensions, cells, rows, cell and n are pgsd_sph_gradients_device's, and so are the grid, the support 2h, r2, inv_h,
       sigma, G, F(q) and THE ORDER of the candidates.  pressure: an N x 1 float32 or float64 chunk, or NULL.  defaults:
       the mass, the density and the pressure that stand for a chunk stored nowhere (the density default is a number
       here: there is no "no volume").  viscosity: mu >= 0, or any negative number: no viscous term.  gravity: g[3].
       On the host, once, in float64: eta2 = (0.01*h)*h and Gv = G * (2.0*mu).
       PER ENTRY k, once, float64 from the stored values: A_k = p_k / (rho_k*rho_k), V_k = m_k / rho_k (a density of 0
       gives what IEEE gives).
       ONE PAIR i <- j, float64, no contraction: d, d2, the strict test d2 < r2, rr = sqrt(d2), q = rr * inv_h and F as in
       the gradients; i itself and coincident entries are candidates like any other (their e is zero, so an infinite S
       gives a NaN there);
           e_k = F * d_k, S = A_i + A_j, a_p[k] += m_j * (S * e_k)
       and with a viscosity (Morris' laminar viscosity for one constant mu)
           K = (F * d2) / (d2 + eta2), u_k = v_j[k] - v_i[k], a_v[k] += V_j * (K * u_k).
       The three or six accumulators per entry start at +0.0 and add in the defined order.  After the last candidate
           pressure_acc[k] = -(G * a_p[k]), viscous_acc[k] = (Gv * a_v[k]) / rho_i,
           total[k] = (pressure_acc[k] + viscous_acc[k]) + g[k], or pressure_acc[k] + g[k] without a viscosity.
       An entry with id n_cells is nowhere: it contributes to nobody and all its values are +0.0, the total too.  With
       dimensions == 2 d_z is 0 and nothing else differs.
       Device outputs, n x 3 float64, each optional (NULL): out_pressure_acc, out_viscous_acc (not written without a
       viscosity), out_total.
       Host output, 12 words:
           out_summary[0 .. 2]    n; the entries nowhere; the entries that have a cell and whose total has a component
                                  that is NaN or infinite
           out_summary[3 .. 8]    the list position and the row of the largest total, of the largest pressure_acc and of
                                  the largest viscous_acc; 0xFFFFFFFF without one
           out_summary[9 .. 11]   as float64 bit patterns the largest total2 = (a0*a0 + a1*a1) + a2*a2 of the outputs,
                                  pressure2 and viscous2 over the entries that have a cell, the smaller list position on
                                  a tie, a NaN never; +0.0 without one
       No float is summed over the list.  Staging, synchronisation and n == 0 are pgsd_sph_sums_device's.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_sph_gradients_device refuses; a pressure chunk that is not one float32 or float64 column or has another N
       than position; a viscosity that is NaN or infinite; a gravity component that is not finite. */
    int pgsd_sph_accelerations_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                      const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                      const struct pgsd_index_entry* density, const struct pgsd_index_entry* pressure,
                                      const double defaults[3], const double vectors[6], double h, uint32_t kernel,
                                      uint32_t dimensions, const uint32_t cells[3], double viscosity,
                                      const double gravity[3], const uint32_t* rows, const int32_t* cell, uint64_t n,
                                      double* out_pressure_acc, double* out_viscous_acc, double* out_total,
                                      uint64_t* out_summary);

    /* SPH body forces: the force and the torque the fluid exerts on a body (pgsd.hoomd.sph_body_force is the definition,
       and the results equal it exactly: every counter and index, every float bit for bit -- a NaN is a NaN).  A pair pass
       between TWO row lists in cell order on one grid: the targets b (body_rows, body_cell, n_body) and the sources f
       (fluid_rows, fluid_cell, n_fluid), each checked and given offsets of its own; a row may occur in both, which is not
       detected.  position, velocity, mass, density, pressure, defaults, vectors, h, kernel, dimensions, cells and
       viscosity are pgsd_sph_accelerations_device's, and so are the grid, the support 2h, r2, inv_h, sigma, G, eta2, Gv,
       A_k, V_k and F(q).  about: the point the torque is taken about.
       THE CANDIDATES of target b: the sources in the cells of the sums' order around b's cell, looked up in the sources'
       offsets, inside a cell in ascending position in the sources' list; d = x_f - x_b under the single-shift minimum
       image, the test d2 < r2 is strict.  Entries of either list with id n_cells are nowhere and take no part.
       ONE PAIR b <- f, float64, no contraction: the accelerations' arithmetic with i = b and j = f;
           contacts[b] += 1, a_p[k] += m_f * ((A_b + A_f) * e_k), and with a viscosity a_v[k] += V_f * (K * (v_f[k] - v_b[k])).
       After the last candidate pressure_acc[k] = -(G * a_p[k]), viscous_acc[k] = (Gv * a_v[k]) / rho_b; no gravity enters.
       A target nowhere has every value +0.0.
       PER TARGET, one rounding per operation: fp[k] = m_b * pressure_acc[k], fv[k] = m_b * viscous_acc[k]; the arm r = x_b
       - about under the single-shift minimum image (z, then y, then x; r_z = 0 with dimensions == 2);
           tp = (r1*fp2 - r2*fp1, r2*fp0 - r0*fp2, r0*fp1 - r1*fp0), tv likewise.
       A target with a cell is BAD if any of its six or twelve terms is NaN or infinite: all its terms count as +0.0.
       THE SUMS: each column over the targets' list positions (nowhere: +0.0) in tiles of 4096 -- lane k % 256 adds its 16
       steps in order, then the halvings 32 .. 1 inside each run of 64 lanes and (w0 + w1) + (w2 + w3) --, over the
       tiles lane t adds tiles t, t + 256, ... and then the same tree (pgsd.hoomd._ordered_sum).
       Device outputs, each optional (NULL): out_contacts (n_body uint32), out_pressure_acc, out_viscous_acc (n_body x 3
       float64; the second is not written without a viscosity).
       Host output, 22 words:
           out_summary[0 .. 3]    n_body; the targets nowhere; n_fluid; the sources nowhere
           out_summary[4 .. 6]    wetted: the targets with a cell and contacts >= 1; pairs: the sum of contacts; bad
           out_summary[7 .. 9]    the list position, the row and as a float64 bit pattern the largest (fp0*fp0 + fp1*fp1) +
                                  fp2*fp2 over the targets with a cell that are not bad, the smaller position on a tie,
                                  a NaN never; 0xFFFFFFFF, 0xFFFFFFFF and +0.0 without one
           out_summary[10 .. 21]  as float64 bit patterns force_pressure[3], force_viscous[3], torque_pressure[3],
                                  torque_viscous[3]; the viscous six are +0.0 without a viscosity
       n_body == 0 launches nothing: the summary is n_fluid in word 2, 0xFFFFFFFF in words 7 and 8 and zeros (no source
       is looked at).  n_fluid == 0 still runs: every target is dry and every sum +0.0.  Staging and synchronisation are
       pgsd_sph_sums_device's; both lists read the same staged chunks.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_sph_accelerations_device refuses, for either list; an about component that is not finite. */
    int pgsd_sph_body_force_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                   const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                   const struct pgsd_index_entry* density, const struct pgsd_index_entry* pressure,
                                   const double defaults[3], const double vectors[6], double h, uint32_t kernel,
                                   uint32_t dimensions, const uint32_t cells[3], double viscosity, const double about[3],
                                   const uint32_t* body_rows, const int32_t* body_cell, uint64_t n_body,
                                   const uint32_t* fluid_rows, const int32_t* fluid_cell, uint64_t n_fluid,
                                   uint32_t* out_contacts, double* out_pressure_acc, double* out_viscous_acc,
                                   uint64_t* out_summary);

    /* SPH samples (pgsd.hoomd.sph_samples is the definition, and the results equal it exactly: every counter and index,
       every float bit for bit -- a NaN is a NaN): the SPH interpolant of a row list at K points of the caller's choosing,
       the first pass whose centre is no entry of the list.  position, mass, density, vectors, h, kernel, dimensions,
       cells, rows, cell and n are pgsd_sph_sums_device's, and so are the grid, the support 2h, r2, inv_h, sigma, w(q) and
       THE ORDER of the candidates.  defaults: the mass and the density that stand for a chunk stored nowhere (the
       density default is a number here: there is no "no volume").  values[k], k < 4: an N x value_columns[k] float32 or
       float64 chunk, or NULL: value_defaults[k] stands for every element of it; value_columns[k] == 0: the slot is
       unused (values may be NULL when every slot is).  The used slots come first; their C <= 8 columns are concatenated
       in the order given.  box: the float32 box pgsd_order_rows_by_cell_device takes, from which vectors was formed.
       points: device, K x 3 float64, in the caller's order, which is the order of every per-point output.
       THE POINT'S CELL is the cell order's key of its position: the wrapped fraction of pgsd.hoomd.domain_rows, the NaN
       test before the integer conversion; a point with a NaN fraction is nowhere: its count is 0 and every value +0.0,
       whatever normalise says.  It is OUTSIDE when it has a cell and its fraction before the wrap is < 0 or >= 1 on an
       axis that takes part: the single-shift minimum image holds inside the box only.
       CANDIDATES: the cells of the sums' order around the point's cell, inside a cell ascending list position; d is the
       minimum-image displacement from the point to x_j and j contributes when d2 < r2, strictly.  Entries of the list
       that are nowhere contribute to no point.
       ONE CONTRIBUTING PAIR, float64, no contraction: rr = sqrt(d2), q = rr * inv_h, w = w(q);
           count += 1, a_m += m_j * w, vw = V_j * w, a_v += vw, a_f[c] += vw * f_j[c]    (V_j = m_j / rho_j, once per entry)
       AFTER THE LAST: density = sigma * a_m, shepard = sigma * a_v, values[c] = sigma * a_f[c], or with normalise != 0
       values[c] = a_f[c] / a_v as IEEE gives it (a point without a contributing entry: 0/0, a NaN).
       Device outputs, each optional (NULL): out_count (K uint32), out_density, out_shepard (K float64), out_values (K x C
       float64).
       Host output, 11 words:
           out_summary[0 .. 4]    K; the points nowhere; the points outside; the points that have a cell and count 0; the
                                  points that have a cell and whose density, shepard or any value is NaN or infinite
           out_summary[5 .. 6]    the largest count over the points that have a cell and its point, the smaller index on
                                  a tie; 0 and 0xFFFFFFFF where no point has a cell
           out_summary[7 .. 10]   as float64 bit patterns the minimum and maximum of shepard, then of density, over the
                                  points that have a cell, by strict compares from +inf / -inf (a NaN never replaces a value)
       No float is summed over the points.  K == 0 returns the summary of no point and launches nothing; n == 0 with K > 0
       still runs: every point that has a cell is empty.  Staging and synchronisation are pgsd_sph_sums_device's.
       PGSD_ERROR_INVALID_ARGUMENT with a pgsd_last_error_string(), every output as it was: everything
       pgsd_sph_sums_device refuses; K >= 2^32; points NULL with K > 0; a column count above 4, or more than 8 together; a
       used slot after an unused one; a value chunk that is not float32 or float64, has another width than declared or
       another N than position; a value default that is NaN while its chunk is absent; a box whose lengths are not
       positive or that disagrees with vectors. */
    int pgsd_sph_samples_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                                const struct pgsd_index_entry* const values[4], const uint32_t value_columns[4],
                                const double value_defaults[4], const double defaults[2], const float box[6],
                                const double vectors[6], double h, uint32_t kernel, uint32_t dimensions,
                                const uint32_t cells[3], const uint32_t* rows, const int32_t* cell, uint64_t n,
                                const double* points, uint64_t K, uint32_t normalise, uint32_t* out_count,
                                double* out_density, double* out_shepard, double* out_values, uint64_t* out_summary);

    /* Indexed read: dst row k takes chunk row rows[k] for k < n (rows: device memory, any order), converted by the
       unpack's rules (dst_type, dst_stride / dst_col0, bitcast, fill_rest); dst->order must be NULL.  The chunk is
       staged whole; like pgsd_read_chunk_device the gather runs at pgsd_device_wait_read, which fails with
       PGSD_ERROR_INVALID_ARGUMENT if an entry is >= chunk->N (nothing is written for such an entry).  Chunks of 2^32
       rows or more are refused. */
    int pgsd_read_rows_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk, const uint32_t* rows,
                              uint64_t n, const struct pgsd_field_dst* dst);

    /* A row plan for sparse indexed reads of chunks of N rows: the rows are cut into blocks of R rows (the tuning
       variable PGSD_PLAN_BLOCK_ROWS, read once), the blocks that hold at least one of rows[0 .. n) are the touched blocks
       (ascending; a block's position in that list is its slot in the compact staging), neighbours merge into runs, and
       rows2[k] = slot(rows[k] / R) * R + rows[k] % R indexes the staging.  rows need not be ascending and may repeat; an
       entry >= N touches nothing and becomes 0xFFFFFFFF.  rows and rows2 (n entries each) are device memory of the
       caller's and must outlive the plan; the plan is computed on the handle's GPU and the call synchronises.  One plan
       serves every chunk of N rows, whatever its row size, in every frame.  Requires N + R < 2^32. */
    struct pgsd_row_plan;
    int pgsd_row_plan_create(struct pgsd_handle* handle, const uint32_t* rows, uint64_t n, uint64_t N, uint32_t* rows2,
                             struct pgsd_row_plan** out);
    void pgsd_row_plan_destroy(struct pgsd_row_plan* plan);
    /* counts: n, N, R, T (touched blocks), runs (of adjacent touched blocks), staged_rows (the height of the compact
       staging: T * R, less where the short last block is touched).  lists: rows, rows2 (device, n entries), blocks
       (host, T entries), run_first and run_blocks (host, runs entries: first block and number of blocks of each run);
       valid until the plan is destroyed. */
    int pgsd_row_plan_query(const struct pgsd_row_plan* plan, uint64_t counts[6], const uint32_t* lists[5]);

    /* pgsd_read_rows_device through a plan: only the plan's runs of the chunk are read from the file and staged (the HBM
       staging holds the touched blocks, not the chunk), and the gather at pgsd_device_wait_read indexes them with rows2.
       dst row k takes chunk row rows[k], k < n; an entry >= N fails the wait exactly as it does there.  A chunk whose N
       is not the plan's is refused with PGSD_ERROR_INVALID_ARGUMENT.  The plan must outlive the wait. */
    int pgsd_read_rows_planned_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk,
                                      const struct pgsd_row_plan* plan, const struct pgsd_field_dst* dst);

    /* File bytes the device read path of this handle has pread, and bytes it has copied host-to-device, since the
       pipeline was created or the counters were last reset (small reads through the pinned, device-mapped arena copy
       nothing).  Kept apart from pgsd_device_stats, whose layout is fixed. */
    int pgsd_device_read_counters(struct pgsd_handle* handle, uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset);

#ifdef __cplusplus
    }
#endif

#endif /* PGSD_PRIVATE_H */
