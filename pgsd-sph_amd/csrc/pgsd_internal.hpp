// pgsd_internal.hpp -- declarations shared by the translation units of libpgsd_amd.so.
#ifndef PGSD_INTERNAL_HPP
#define PGSD_INTERNAL_HPP

#include "pgsd.h"
#include "pgsd_private.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <sched.h>
#include <sys/uio.h>
#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace pgsd_amd
    {
void set_last_error(const std::string& s);
const char* last_error();
uint64_t last_error_serial(); // grows with every set_last_error of this thread: "did the callee leave a message?"
// Called from the catch-all of every C-ABI entry point (function-try-blocks): no C++ exception
// crosses the boundary.  Maps the exception in flight to a pgsd_error and records its text.
int abi_guard() noexcept;
pgsd_comm default_comm();
// The installed communicator is shared by reference: a handle keeps the one it was opened with alive, so
// pgsd_comm_finalize / pgsd_comm_init_* while files are open cannot pull the context (shm mapping, RCCL
// communicator, callbacks) from under them; its destroy hook runs when the last user lets go.
struct CommBox
    {
    pgsd_comm c;
    explicit CommBox(const pgsd_comm& comm) : c(comm) { }
    CommBox(const CommBox&) = delete;
    CommBox& operator=(const CommBox&) = delete;
    ~CommBox()
        {
        if (c.destroy)
            c.destroy(c.ctx);
        }
    };
std::shared_ptr<CommBox> default_comm_box();

// ---- phase timeline: roctx ranges around the phases of a frame (pack launch, frame exchange, each
// device->host piece, each pwrite, drain), the counterpart of the reference's PGSD_ACTIVATE_LOGGER
// output (pgsd.c:27, 1034, 1156, 2231).  Off unless PGSD_TRACE is set to a non-zero value; then
// librocprofiler-sdk-roctx is dlopen'ed (no link-time dependency) and `rocprofv3 --marker-trace` shows
// the ranges next to the kernels and copies they bracket.
bool trace_on();
void trace_push(const char* name);
void trace_pop();
struct TraceRange
    {
    bool on;
    explicit TraceRange(const char* name) : on(trace_on())
        {
        if (on)
            trace_push(name);
        }
    // name with one number (piece offset, byte count ...): formatted only when tracing
    TraceRange(const char* fmt, unsigned long long a, unsigned long long b = 0);
    TraceRange(const TraceRange&) = delete;
    TraceRange& operator=(const TraceRange&) = delete;
    ~TraceRange()
        {
        if (on)
            trace_pop();
        }
    };

inline int comm_barrier(const pgsd_comm& c)
    {
    if (c.size == 1)
        return PGSD_SUCCESS;
    if (c.barrier)
        return c.barrier(c.ctx) == 0 ? PGSD_SUCCESS : PGSD_ERROR_COMM;
    std::vector<char> all((size_t)c.size);
    char one = 0;
    return c.allgather(c.ctx, &one, all.data(), 1) == 0 ? PGSD_SUCCESS : PGSD_ERROR_COMM;
    }

// ---- file back ends (pgsd_io.cpp): POSIX, or the reference's own MPI-IO calls with PGSD_IO=mpiio.  The descriptor of
// io_open is what every other io_* call (and pwrite_full / pread_some below, which sit on them) takes.
int io_open(const char* path, int oflags, int mode);
int io_close(int fd);
int io_truncate(int fd, long long size);
long long io_file_size(int fd); // -1 + errno
ssize_t io_pwrite(int fd, const void* buf, size_t bytes, long long offset);
ssize_t io_pread(int fd, void* buf, size_t bytes, long long offset);
const char* io_backend_name(); // "posix" | "mpiio"

// ---- host IO: a pool of pwrite threads shared by the host and the device path ----
class WriterPool;
WriterPool* writer_pool_create(unsigned n_threads, const cpu_set_t* cpus = nullptr);
bool numa_cpus_of_pci_device(const char* pci_bus_id, cpu_set_t* out);
void writer_pool_destroy(WriterPool*);
void writer_pool_submit(WriterPool*, std::function<void()> fn);
// The warm-then-write pair (pgsd_io.cpp): a pool of ONE thread gets a helper, both on L3-sharing cores of `cpus` (null:
// of the process), and carries pieces above `sub_bytes` out as sub-pieces the two take in turn.  false -- and the pool
// stays as it was -- with several threads, the MPI-IO back end, or where sysfs names no two cores that share an L3
// (need_topology = false: the pair runs unplaced there; for tests of the lane itself).
bool writer_pool_enable_warm(WriterPool*, size_t sub_bytes, const cpu_set_t* cpus, bool need_topology = true);
// pwrite_locked of one piece through the pair, FROM A JOB OF THE POOL (its lane thread); plainly where there is no pair
// or the piece is no longer than a sub-piece.  0 or -errno; *pwrite_ms: the time inside pwrite calls
int writer_pool_pwrite_warm(WriterPool*, int fd, const void* buf, size_t bytes, long long offset, bool shared_file,
                            double* pwrite_ms);
// The side lane beside the pair (pgsd_io.cpp): up to three threads that insert whole pages of a piece through a
// MAP_SHARED mapping of `fd` (populate, then copy) while the pair pwrites the rest.  false -- nothing changes -- without
// the pair or where fstatfs does not say tmpfs; never used for a shared file.  fail_at: tests (-1: never).
bool writer_pool_enable_side(WriterPool*, int fd, unsigned n_threads, size_t block_bytes, const cpu_set_t* cpus, long fail_at = -1);
// bytes that went by the side lane and the time its threads spent on them, since the pool was made; is it still on?
void writer_pool_side_counters(WriterPool*, uint64_t* bytes, double* ms, bool* on);
// unmap the side lane's windows: from a job of the pool, or while it has none
void writer_pool_side_drop(WriterPool*);
// Write [buf, buf+bytes) at `offset` of fd, split over the pool; blocks until done.
// Returns 0 or -errno.
int writer_pool_pwrite_sync(WriterPool*, int fd, const void* buf, size_t bytes, long long offset,
                            bool shared_file = false);
// pwrite_full under an advisory flock when several processes write the same file
int pwrite_locked(int fd, const void* buf, size_t bytes, long long offset, bool shared_file);
int pwritev_locked(int fd, struct iovec* iov, int n, long long offset, bool shared_file); // one contiguous file range
// plain full-length pwrite / pread loops (0 / -errno; pread leaves a short tail untouched)
int pwrite_full(int fd, const void* buf, size_t bytes, long long offset);
void pread_some(int fd, void* buf, size_t bytes, long long offset);
void pread_parallel(int fd, void* buf, size_t bytes, long long offset); // >= 64 MiB: a few threads

// ---- device pipeline (pgsd_device.cpp, pgsd_device_write.cpp, pgsd_device_read.cpp); created lazily by the first device call ----
class DevicePipeline;
struct DeviceChunk
    {
    pgsd_pack_job job;      // dst filled in by the pipeline (device staging)
    uint64_t N;             // rows of this rank
    long long file_offset;  // where this rank's rows start in the file; <0: copy into host_dst
    void* host_dst;         // for small buffered chunks: synchronous copy target
    };
DevicePipeline* device_pipeline_create(const pgsd_device_config& cfg, int fd, bool shared_file, std::string* err);
void device_pipeline_destroy(DevicePipeline*);
int device_pipeline_device(DevicePipeline*); // the HIP device the pipeline runs on
// one fused pack launch for `chunks` (all share N), then async copy + write of each
int device_pipeline_submit(DevicePipeline*, std::vector<DeviceChunk>& chunks, uint64_t N, std::string* err);
// the same in two steps: pack now (one fused launch, returns a ticket), say later where chunk `index` of the
// ticket goes: a file offset, a host buffer (synchronous copy), or nowhere (file_offset < 0, host_dst null)
int device_pipeline_stage(DevicePipeline*, std::vector<DeviceChunk>& chunks, uint64_t N, int* ticket, std::string* err);
int device_pipeline_commit(DevicePipeline*, int ticket, size_t index, long long file_offset, void* host_dst,
                           std::string* err);
// staged, not yet committed chunks [first, first + count) of a ticket: packed rows == ref[i] (device memory; shorter
// than the chunk: repeating)?
// (one kernel + one stream wait) / copied into dst[i] (device memory, asynchronous on the pack stream)
int device_pipeline_compare(DevicePipeline*, int ticket, size_t first, size_t count, const void* const* ref,
                            const uint64_t* ref_bytes, uint8_t* equal, std::string* err);
int device_pipeline_copy_staged(DevicePipeline*, int ticket, size_t first, size_t count, void* const* dst,
                                std::string* err);
// asynchronous seal: chunks of the direct (small-frame) path are handed to the writer thread now
void device_pipeline_kick(DevicePipeline*);
// a few host bytes (metadata of an asynchronously sealed frame) through the writer thread, in FIFO order behind the
// pieces already queued; copied.  single_writer: that order is only defined with one writer thread
void device_pipeline_write_host(DevicePipeline*, const void* data, size_t bytes, long long file_offset);
bool device_pipeline_single_writer(DevicePipeline*);
int device_pipeline_wait_packed(DevicePipeline*, std::string* err);
void device_pipeline_set_source_stream(DevicePipeline*, void* stream);
// read side: rows at `file_offset` -> staging -> unpack into job.dst (job.src is filled in)
int device_pipeline_read(DevicePipeline*, long long file_offset, size_t bytes, const pgsd_unpack_job& job, uint64_t N,
                         std::string* err);
int device_pipeline_wait_read(DevicePipeline*, std::string* err);
// Domain selection over a staged position chunk (N x 3 float32 / float64 rows): the fractional coordinates of
// HOOMD's BoxDim::makeFraction, evaluated in float64 without contraction, wrapped into [0, 1) per axis.
struct DomainArgs
    {
    const void* pos;
    uint64_t N;
    uint32_t f64;   // 1: rows of doubles
    uint32_t dims;  // 2: z is ignored
    double L[3];    // box lengths
    double xy, xz, yz;
    double lo[3], hi[3];
    };
// Ghost layer selection (pgsd.hoomd.halo_rows is the definition): the domain's rows -- the OWNED rows -- plus the rows
// whose wrapped fraction is, on every axis, inside the domain or in one of the axis' four half-open ghost bands and on
// at least one axis in a band.  band[a] = {below lo, hi, below-wrapped lo, hi, above lo, hi, above-wrapped lo, hi}, an
// empty band {1, 0}; tested in that order after "inside", the wrapped ones meaning a shift of -1 / +1 box vectors.  The
// bounds are computed on the host (pgsd.hoomd.halo_bands): the kernel only compares.  divided[a] == 0: the axis has no
// bands and counts as inside.
struct HaloArgs
    {
    DomainArgs d;
    double band[3][8];
    uint32_t divided[3];
    uint32_t pad;
    };
// Group selection over up to four staged per-particle chunks (pgsd.hoomd.where_rows is the definition): row i is kept
// iff every term holds for element (i, column) of its chunk and -- with has_domain -- its position lies in the domain.
// A range term compares v = (double)x (exact for every element type allowed): kept iff v is no NaN, not v < lo and not
// v >= hi, so a NaN bound leaves that side open; a set term keeps x iff x < 64 as an unsigned word and bit x of `set`
// is set (a negative int32 is a large unsigned word).
enum
    {
    WHERE_MAX_TERMS = 4,
    WHERE_RANGE = 0,
    WHERE_SET = 1
    };
struct WhereTerm
    {
    const void* base; // the staged chunk: N x M elements of `type`
    uint32_t type;    // PGSD_TYPE_UINT32, _INT32, _FLOAT or _DOUBLE (ranges only)
    uint32_t M, column;
    uint32_t kind;    // WHERE_RANGE / WHERE_SET
    double lo, hi;
    uint64_t set;
    };
struct WhereArgs
    {
    uint64_t N;
    uint32_t n_terms;
    uint32_t has_domain; // d (and its staged position chunk) takes part
    WhereTerm t[WHERE_MAX_TERMS];
    DomainArgs d;
    };
// one whole chunk of a selection: its file range
struct ChunkRange
    {
    long long file_offset;
    size_t bytes;
    };
// stage the chunks of w's terms (ranges[0 .. n_terms); then the position chunk's, with has_domain) whole -- a chunk an
// earlier selection left staged is taken from there, one that several terms name is staged once --, fill in their
// addresses, select into out_rows (device, room for N), the count into *out_count; synchronous.  The staged chunks stay
// until the next wait_read, like select_domain's.
int device_pipeline_select_where(DevicePipeline*, const ChunkRange* ranges, const WhereArgs& w, uint32_t* out_rows,
                                 uint64_t* out_count, std::string* err);
// indexed read: the chunk's bytes at `file_offset` (src_N rows) are staged whole; wait_read gathers rows[0 .. n) of them
// into job.dst (job.dst.order is null).  The position rows a select_domain left staged are taken from there.
int device_pipeline_read_rows(DevicePipeline*, long long file_offset, size_t bytes, const pgsd_unpack_job& job,
                              uint64_t src_N, const uint32_t* rows, uint64_t n, std::string* err);
// stage the position chunk at `file_offset` (d.N rows; d.pos is filled in), select the rows inside the domain into
// out_rows (device), the count into *out_count; synchronous.  The staged rows stay until the next wait_read.
int device_pipeline_select_domain(DevicePipeline*, long long file_offset, size_t bytes, const DomainArgs& d,
                                  uint32_t* out_rows, uint64_t* out_count, std::string* err);
// the same staging, then the ghost layer selection: the owned rows at out_rows[0, out_counts[0]), the ghost rows behind
// them (out_counts[1]), each ascending; out_shift (device, room for 3 x d.N) receives the ghosts' shifts; synchronous
int device_pipeline_select_halo(DevicePipeline*, long long file_offset, size_t bytes, const HaloArgs& h, uint32_t* out_rows,
                                int32_t* out_shift, uint64_t out_counts[2], std::string* err);
// Domain census (pgsd.hoomd.axis_histograms / domain_counts are the definitions): the wrapped fractions of a staged
// position chunk -- DomainArgs without lo / hi -- binned instead of tested against one cell.
enum
    {
    CENSUS_MAX_BINS = 4096,     // bins per axis of a histogram: a power of two, so every edge k / bins is exact
    CENSUS_MAX_AXIS_CELLS = 64, // cells per axis of a count ...
    CENSUS_MAX_CELLS = 4096     // ... and in all
    };
// the cells of a rectilinear decomposition: n[a] cells on axis a, cut at the n[a] - 1 interior bounds bounds[a][...]
// (strictly ascending inside (0, 1)); a row's cell on an axis is the number of bounds <= its fraction
struct CellArgs
    {
    DomainArgs d;
    uint32_t n[3];
    uint32_t pad;
    double bounds[3][CENSUS_MAX_AXIS_CELLS - 1];
    };
// stage the position chunk at `file_offset` (d.N rows) -- or take it from what an earlier selection or census left
// staged --, count on the GPU, copy the result to the host; synchronous.  The staged rows stay until the next wait_read.
// out_hist: 3 x bins counts (x, y, z; the z row zero when d.dims == 2)
int device_pipeline_domain_histogram(DevicePipeline*, long long file_offset, size_t bytes, const DomainArgs& d, uint32_t bins,
                                     uint64_t* out_hist, std::string* err);
// out_counts: n[0] * n[1] * n[2] counts, cell (x, y, z) at x + n[0] * (y + n[1] * z); *out_nowhere: the rows with a NaN
// fraction on an axis that takes part
int device_pipeline_domain_counts(DevicePipeline*, long long file_offset, size_t bytes, const CellArgs& c,
                                  uint64_t* out_counts, uint64_t* out_nowhere, std::string* err);
// Cell order (pgsd.hoomd.cell_ids / cell_order are the definitions): a row list sorted by the cell its rows' wrapped
// fractions -- DomainArgs without lo / hi -- fall into in a uniform cells[0] x cells[1] x cells[2] grid, stably; entries
// [n_owned, n) are a second run (the ghosts) that is sorted on its own.
enum
    {
    ORDER_MAX_AXIS_CELLS = 1024 // cells per axis: 2 * (1024^3 + 1) keys still fit 32 bits
    };
struct OrderArgs
    {
    DomainArgs d;
    uint64_t n, n_owned; // entries of the list; the first n_owned are the owned run
    uint32_t cells[3];
    uint32_t n_cells;    // their product: the id of a row with a NaN fraction
    };
// stage the position chunk at `file_offset` (o.d.N rows) -- or take it from what an earlier selection left staged --,
// sort rows[0 .. o.n) (device, the caller's) by cell in place, permute shift (device, 3 x (o.n - o.n_owned) int32, or
// null) like the ghost run, write the sorted cell ids to out_cell (device, o.n int32, or null); synchronous.  An entry
// >= o.d.N refuses the call with nothing written.  The staged rows stay until the next wait_read.
int device_pipeline_order_rows(DevicePipeline*, long long file_offset, size_t bytes, const OrderArgs& o, uint32_t* rows,
                               int32_t* shift, int32_t* out_cell, std::string* err);
// Chunk statistics (pgsd.hoomd.column_stats is the definition): per column of a staged chunk of N x M float32, float64,
// int32 or uint32 elements -- of all its rows, or of the n entries of a row list in list order -- the count, the NaN and
// the infinite entries, minimum, maximum and the sum of the finite entries in the definition's order; with norm2 (float
// chunks of three columns) one more column, (x*x + y*y) + z*z in float64.
struct StatsArgs
    {
    const void* base;     // the staged chunk
    uint64_t N;           // its rows
    const uint32_t* rows; // device, or null: every row
    uint64_t n;           // entries of the list
    uint32_t type, M;     // enum pgsd_type, columns
    uint32_t norm2;
    uint32_t pad;
    };
// is (type, M, norm2) something the statistics kernels take?  `why` receives the refusal
inline bool chunk_stats_supported(uint32_t type, uint32_t M, uint32_t norm2, std::string* why)
    {
    const bool real = type == PGSD_TYPE_FLOAT || type == PGSD_TYPE_DOUBLE;
    const char* msg = nullptr;
    if (!real && type != PGSD_TYPE_INT32 && type != PGSD_TYPE_UINT32)
        msg = "the chunk holds float32, float64, int32 or uint32 elements";
    else if (M == 0 || M > 4)
        msg = "the chunk has 1 to 4 columns";
    else if (norm2 && (!real || M != 3))
        msg = "norm2 needs a float chunk of three columns";
    if (msg && why)
        *why = msg;
    return msg == nullptr;
    }
// the statistics of no entry, for C columns
inline void chunk_stats_of_nothing(uint32_t C, uint64_t* out_counts, double* out_values)
    {
    for (uint32_t c = 0; c < C; c++)
        {
        out_counts[3 * c + 0] = out_counts[3 * c + 1] = out_counts[3 * c + 2] = 0;
        out_values[3 * c + 0] = HUGE_VAL;
        out_values[3 * c + 1] = -HUGE_VAL;
        out_values[3 * c + 2] = 0.0;
        }
    }
// stage the chunk at `file_offset` (s.N rows; s.base is filled in) -- or take it from what an earlier selection, census
// or statistics call left staged --, reduce on the GPU, copy the results to the host: out_counts C x 3 (count, NaN,
// infinite), out_values C x 3 (min, max, sum), C = s.M + (s.norm2 ? 1 : 0), written on success only; synchronous.  An
// entry >= s.N refuses the call.  The staged rows stay until the next wait_read.
int device_pipeline_chunk_stats(DevicePipeline*, long long file_offset, size_t bytes, const StatsArgs& s, uint64_t* out_counts,
                                double* out_values, std::string* err);
// What the grouped reductions (conservation sums, frame displacements) share: up to five staged chunks of one N read row
// by row, one of them the typeid, and a group of up to four consecutive types.  Passed to the kernels by value inside
// the pass's own arguments.
enum
    {
    GROUPED_CHUNKS = 5,
    GROUPED_MAX_TYPES = 4 // types per launch
    };
struct GroupedArgs
    {
    const void* chunk[GROUPED_CHUNKS]; // the staged chunks in the pass's order; null: stored nowhere
    uint64_t N;                        // rows of every chunk that is present
    const uint32_t* rows;              // device, or null: every row
    uint64_t n;                        // entries of the list
    uint32_t type0, n_types;           // the types [type0, type0 + n_types); without a typeid chunk every entry is type0's
    uint32_t f64;                      // the float chunks hold float64 (else float32)
    uint32_t typeid_signed;            // the typeid chunk holds int32: a negative id belongs to no type
    uint32_t present;                  // bit i: chunk i is stored (its address is filled in by the staging)
    uint32_t pad;
    };
// the results of no entry, Q sums per type (and a largest value with its entry): zero counts, +0.0 sums, -inf at no entry
inline void grouped_of_nothing(uint32_t Q, bool largest, uint32_t n_types, uint64_t* out_counts, double* out_values)
    {
    const uint32_t cs = 2 + (largest ? 1 : 0), vs = Q + (largest ? 1 : 0);
    for (uint32_t t = 0; t < n_types; t++)
        {
        out_counts[cs * t + 0] = out_counts[cs * t + 1] = 0;
        for (uint32_t q = 0; q < Q; q++)
            out_values[vs * t + q] = 0.0;
        if (largest)
            {
            out_counts[cs * t + 2] = UINT64_MAX;
            out_values[vs * t + Q] = -HUGE_VAL;
            }
        }
    out_counts[cs * n_types] = 0;
    }
// Conservation sums (pgsd.hoomd.particle_moments is the definition): per particle type of a group of up to four
// consecutive types the entries, those with a value that is not finite, and nine sums in chunk statistics' order -- mass
// m, momentum m * v[a], kinetic energy (0.5 * m) * ((vx*vx + vy*vy) + vz*vz), internal energy m * e, first moment
// m * x[a] -- over several staged chunks of one N read row by row, every element converted to float64 first.
enum
    {
    MOMENTS_CHUNKS = GROUPED_CHUNKS, // typeid, mass, velocity, energy, position
    MOMENTS_QUANTITIES = 9,
    MOMENTS_MAX_TYPES = GROUPED_MAX_TYPES
    };
struct MomentsArgs : GroupedArgs // chunk: the order above; null: the default row stands for every row
    {
    double defaults[8]; // mass, v[3], energy, x[3]
    };
// stage the chunks that are present (ranges[i] belongs to chunk i; m.chunk[i] is filled in) -- or take them from what an
// earlier selection, census or statistics call left staged --, reduce on the GPU, copy the
// results to the host: out_counts n_types x 2 (entries, bad), then the entries of no type of the group; out_sums
// n_types x 9; written on success only; synchronous.  An entry >= m.N refuses the call.  The staged rows stay until the
// next wait_read.
int device_pipeline_frame_moments(DevicePipeline*, const ChunkRange* ranges, const MomentsArgs& m, uint64_t* out_counts,
                                  double* out_sums, std::string* err);
// Frame displacements (pgsd.hoomd.particle_displacements is the definition): row k of frame a and row k of frame b are
// one particle; per entry the difference d of the two positions, each unwrapped through its image flags and its box
// vectors (or folded into frame b's box: the minimum image), and s = |d|^2; per particle type of a group of up to four
// consecutive types the entries, those with a value that is not finite, the sums of d[a] and of s in chunk statistics'
// order, the largest s and the smallest entry that attains it.
enum
    {
    DISPLACEMENT_CHUNKS = GROUPED_CHUNKS, // position a, image a, position b, image b, typeid
    DISPLACEMENT_SUMS = 4,      // d[0], d[1], d[2], s
    DISPLACEMENT_VALUES = 5,    // the sums, then the largest s
    DISPLACEMENT_MAX_TYPES = GROUPED_MAX_TYPES,
    DISPLACEMENT_MINIMUM_IMAGE = 1u // bit of the entry point's flags
    };
struct DisplacementArgs : GroupedArgs // chunk: the order above; null: stored nowhere
    {
    double va[6], vb[6];                // Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz of frame a and of frame b
    double* out;                        // device, n x 3, or null: entry k's d
    uint32_t minimum_image, dimensions; // fold d into frame b's box (no image chunk then); 2: z is not folded
    };
// the results of no entry: zero counts, no largest entry, +0.0 sums, -inf
inline void displacements_of_nothing(uint32_t n_types, uint64_t* out_counts, double* out_values)
    {
    grouped_of_nothing(DISPLACEMENT_SUMS, true, n_types, out_counts, out_values);
    }
// stage the chunks that are present (ranges[i] belongs to chunk i; d.chunk[i] is filled in; two chunks of one file range
// are staged once and share the address) -- or take them from what an earlier call left staged --, reduce on the GPU,
// copy the results to the host: out_counts n_types x 3 (entries, bad, largest entry or UINT64_MAX), then the entries of
// no type of the group; out_values n_types x 5; written on success only; synchronous.  An entry >= d.N refuses the
// call.  The staged rows stay until the next wait_read.
int device_pipeline_frame_displacements(DevicePipeline*, const ChunkRange* ranges, const DisplacementArgs& d,
                                        uint64_t* out_counts, double* out_values, std::string* err);
// Cell fields (pgsd.hoomd.cell_moments is the definition): the nine values of the conservation sums per entry of a row
// list in cell order, summed per grid cell in an order of the cell's own (pieces of 1024 entries from the cell's first
// entry, 64 strided lanes, the wave tree, the pieces in sequence).  chunk: the conservation sums' order; the typeid slot
// stays empty.
enum
    {
    CELLS_MAX_CELLS = 1u << 20,
    CELLS_PIECE = 1024 // entries of a piece, and of a slab of the sorted list
    };
struct CellMomentsArgs : GroupedArgs
    {
    double defaults[8];  // mass, v[3], energy, x[3]
    const int32_t* cell; // device, n entries, non-decreasing, in [0, n_cells]; n_cells: nowhere
    uint32_t n_cells;
    uint32_t pad2;
    };
// the CSR offsets of a sorted cell list alone: out_offsets (device, n_cells + 2 words) is written on success only
int device_pipeline_cell_offsets(DevicePipeline*, const int32_t* cell, uint64_t n, uint32_t n_cells, uint32_t* out_offsets,
                                 std::string* err);
// stage the chunks that are present, check the lists, sum per cell on the GPU, copy the results to the host: out_counts
// n_cells x 2 (entries, bad), then the entries nowhere; out_sums n_cells x 9; written on success only; synchronous.  An
// entry >= c.N, an id outside [0, n_cells] and a descending id refuse the call.  The staged rows stay until the next
// wait_read.
int device_pipeline_cell_moments(DevicePipeline*, const ChunkRange* ranges, const CellMomentsArgs& c, uint64_t* out_counts,
                                 double* out_sums, std::string* err);
// Neighbour census (pgsd.hoomd.particle_neighbours is the definition): per entry of a row list in cell order the
// entries of the periodically adjacent cells whose single-shift minimum-image distance lies strictly inside r, the
// nearest of them, and over the list the count histogram, the closest pair and a pair histogram over given edges.
enum
    {
    NEIGHBOURS_MAX_BINS = 1024,  // bins of the pair histogram
    NEIGHBOURS_COUNT_BINS = 257, // 0 .. 255 neighbours, then 256 and more
    NEIGHBOURS_HEAD_WORDS = 8,   // n, nowhere, pairs, count_min, count_max, closest, the closest pair's two rows
    NEIGHBOURS_NONE = 0xFFFFFFFFu
    };
struct NeighboursArgs
    {
    const void* pos;      // the staged position chunk
    uint64_t N;           // its rows
    const uint32_t* rows; // device, n entries in cell order
    const int32_t* cell;  // device, n ids, non-decreasing, in [0, n_cells]; n_cells: nowhere
    uint64_t n;
    double vectors[6];    // Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz
    double r, r2;         // the range and r * r, formed once
    uint32_t cells[3];
    uint32_t n_cells;
    uint32_t dims, f64, bins, pad;
    };
// the summary of no entry: bins words of pair histogram behind the head and the count histogram
inline void neighbours_of_nothing(uint32_t bins, uint64_t* out_summary, double* out_closest2)
    {
    std::fill(out_summary, out_summary + NEIGHBOURS_HEAD_WORDS + NEIGHBOURS_COUNT_BINS + bins, (uint64_t)0);
    out_summary[5] = out_summary[6] = out_summary[7] = NEIGHBOURS_NONE;
    *out_closest2 = HUGE_VAL;
    }
// stage the position chunk at `file_offset` (a.N rows; a.pos is filled in) -- or take it from what the ordering left
// staged --, check the lists, search on the GPU; edges2 (host, a.bins + 1 doubles, or null without bins); out_count,
// out_nearest2, out_nearest (device, a.n entries each, or null); out_summary (host, 8 + 257 + a.bins words) and
// out_closest2 (host) are written on success only, and so are the device outputs; synchronous.  An entry >= a.N, an id
// outside [0, n_cells] and a descending id refuse the call.  The staged rows stay until the next wait_read.
int device_pipeline_neighbours(DevicePipeline*, long long file_offset, size_t bytes, const NeighboursArgs& a,
                               const double* edges2, uint32_t* out_count, double* out_nearest2, uint32_t* out_nearest,
                               uint64_t* out_summary, double* out_closest2, std::string* err);
// SPH kernel sums (pgsd.hoomd.sph_kernel_sums is the definition): per entry of a row list in cell order the sums
// sigma * sum w, sigma * sum m_j w and sigma * sum (m_j / rho_j) w over the entries inside the support 2h, in the defined
// order, and over the list their ranges, the largest deviation from the stored density and the entries below a threshold.
enum
    {
    SPH_WENDLAND_C2 = 0,
    SPH_CUBIC_SPLINE = 1,
    SPH_SUMMARY_WORDS = 13, // n, nowhere, not_finite, surface, deviation_at, deviation_row, 3 x (min, max), deviation
    SPH_NONE = 0xFFFFFFFFu
    };
struct SphArgs
    {
    const void* pos;      // the staged position chunk
    const void* mass;     // the staged mass and density chunks, or null: the default stands for every row
    const void* density;
    uint64_t N;           // their rows
    const uint32_t* rows; // device, n entries in cell order
    const int32_t* cell;  // device, n ids, non-decreasing, in [0, n_cells]; n_cells: nowhere
    uint64_t n;
    double vectors[6];    // Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz
    double r2, inv_h, sigma; // (2h)*(2h), 1/h and the normalisation, formed once on the host
    double mass_default, density_default;
    double surface_below;
    uint32_t cells[3];
    uint32_t n_cells;
    uint32_t dims, f64, mass_f64, density_f64; // f64: the position chunk's elements
    uint32_t kernel, volume, surface;          // volume: the third sum, the deviation and the surface count are formed
    uint32_t present;                          // bit 1: a mass chunk, bit 2: a density chunk is stored (ranges[1], ranges[2])
    };
// the summary of no entry
inline void sph_sums_of_nothing(uint64_t* out_summary)
    {
    const double lo = HUGE_VAL, hi = -HUGE_VAL, zero = 0.0;
    std::fill(out_summary, out_summary + SPH_SUMMARY_WORDS, (uint64_t)0);
    out_summary[4] = out_summary[5] = SPH_NONE;
    for (int s = 0; s < 3; s++)
        {
        memcpy(&out_summary[6 + 2 * s], &lo, sizeof(double));
        memcpy(&out_summary[7 + 2 * s], &hi, sizeof(double));
        }
    memcpy(&out_summary[12], &zero, sizeof(double));
    }
// stage the chunks that are present (ranges[0 .. 2]: position, mass, density; a.pos, a.mass and a.density are filled in)
// -- or take them from what an earlier call left staged --, check the lists, sum on the GPU; out_number, out_density,
// out_shepard (device, a.n entries each, or null; the last is written with a.volume only); out_summary (host, 13 words)
// is written on success only, and so are the device outputs; synchronous.  An entry >= a.N, an id outside [0, n_cells]
// and a descending id refuse the call.  The staged rows stay until the next wait_read.
int device_pipeline_sph_sums(DevicePipeline*, const ChunkRange* ranges, const SphArgs& a, double* out_number,
                             double* out_density, double* out_shepard, uint64_t* out_summary, std::string* err);
// SPH sums with a per-particle smoothing length (pgsd.hoomd.sph_adaptive_sums is the definition): per entry of a row list
// in cell order the candidates inside its own support, the sums' three values with its own h (gather) or the pair's mean
// (mean) and the grad-h factor omega, on the grid of the declared bound 2 h_max.  The grid, the list and the defaults are
// SphArgs' (r2 is (2 h_max)^2; inv_h is not looked at; sigma is the mean mode's constant sph_sigma(kernel, 1)).
enum
    {
    SPHA_GATHER = 0,
    SPHA_MEAN = 1,
    SPHA_SUMMARY_WORDS = 22 // n, nowhere, bad_h, not_finite, surface, deviation_at, deviation_row, count_min, count_max,
                            // count_min_at, 5 x (min, max): slength, number, density, shepard, omega; deviation, pairs
    };
struct SphAdaptiveArgs : SphArgs
    {
    const void* slength; // the staged smoothing-length chunk, or null: h_default stands for every row
    double h_default;
    double h_max;        // the declared bound: a listed valid h above it refuses the call
    uint32_t slength_f64, mode; // present bit 3: a slength chunk is stored (ranges[3])
    };
// the summary of no entry
inline void sph_adaptive_sums_of_nothing(uint64_t* out_summary)
    {
    const double lo = HUGE_VAL, hi = -HUGE_VAL;
    std::fill(out_summary, out_summary + SPHA_SUMMARY_WORDS, (uint64_t)0); // (+0.0 is the zero word)
    out_summary[5] = out_summary[6] = out_summary[9] = SPH_NONE;
    for (int s = 0; s < 5; s++)
        {
        memcpy(&out_summary[10 + 2 * s], &lo, sizeof(double));
        memcpy(&out_summary[11 + 2 * s], &hi, sizeof(double));
        }
    }
// the smoothing range of no entry: n = 0, bad = 0, h_min = +inf, h_max = -inf
inline void sph_range_of_nothing(uint64_t* out_words)
    {
    const double lo = HUGE_VAL, hi = -HUGE_VAL;
    out_words[0] = out_words[1] = 0;
    memcpy(&out_words[2], &lo, sizeof(double));
    memcpy(&out_words[3], &hi, sizeof(double));
    }
// stage the chunks that are present (ranges[0 .. 3]: position, mass, density, slength), check the lists and the bound, sum
// on the GPU; out_count (device, a.n uint32), out_number, out_density, out_shepard, out_omega (device, a.n doubles), each
// or null; out_summary (host, 22 words) is written on success only, and so are the device outputs; synchronous.  The
// refusals and the staging are device_pipeline_sph_sums'.
int device_pipeline_sph_adaptive(DevicePipeline*, const ChunkRange* ranges, const SphAdaptiveArgs& a, uint32_t* out_count,
                                 double* out_number, double* out_density, double* out_shepard, double* out_omega,
                                 uint64_t* out_summary, std::string* err);
// stage the smoothing-length chunk (or take it from what an earlier call left staged) and reduce it over a row list
// (device, n entries; null: every row): out_words (host, 4 words) is written on success only; synchronous
int device_pipeline_sph_smoothing_range(DevicePipeline*, long long file_offset, size_t bytes, uint32_t f64, const uint32_t* rows,
                                        uint64_t n, uint64_t N, uint64_t* out_words, std::string* err);
// SPH kernel gradients (pgsd.hoomd.sph_kernel_gradients is the definition): per entry of a row list in cell order the
// density rate, the velocity divergence and curl and the colour gradient over the entries inside the support 2h, in the
// sums' order, and over the list the ranges of the two scalars and the largest curl and normal.  The grid, the support,
// the list and the defaults are SphArgs' (surface and surface_below are not looked at).
enum
    {
    SPHG_SUMMARY_WORDS = 13 // n, nowhere, not_finite, curl_at, curl_row, normal_at, normal_row, 2 x (min, max), curl2, normal2
    };
struct SphGradientsArgs : SphArgs
    {
    const void* velocity;  // the staged velocity chunk, N x 3, or null: the zero vector stands for every row
    double G;              // -((sigma*inv_h)*inv_h), formed once on the host
    uint32_t velocity_f64; // present bit 3: a velocity chunk is stored (ranges[3])
    };
// the summary of no entry
inline void sph_gradients_of_nothing(uint64_t* out_summary)
    {
    const double lo = HUGE_VAL, hi = -HUGE_VAL, zero = 0.0;
    std::fill(out_summary, out_summary + SPHG_SUMMARY_WORDS, (uint64_t)0);
    out_summary[3] = out_summary[4] = out_summary[5] = out_summary[6] = SPH_NONE;
    for (int s = 0; s < 2; s++)
        {
        memcpy(&out_summary[7 + 2 * s], &lo, sizeof(double));
        memcpy(&out_summary[8 + 2 * s], &hi, sizeof(double));
        memcpy(&out_summary[11 + s], &zero, sizeof(double));
        }
    }
// stage the chunks that are present (ranges[0 .. 3]: position, mass, density, velocity; a.pos, a.mass, a.density and
// a.velocity are filled in) -- or take them from what an earlier call left staged --, check the lists, sum on the GPU;
// out_rate, out_divergence (device, a.n entries each, or null), out_curl, out_normal (device, a.n x 3, or null; the last
// three are written with a.volume only); out_summary (host, 13 words) is written on success only, and so are the device
// outputs; synchronous.  The refusals and the staging are device_pipeline_sph_sums'.
int device_pipeline_sph_gradients(DevicePipeline*, const ChunkRange* ranges, const SphGradientsArgs& a, double* out_rate,
                                  double* out_divergence, double* out_curl, double* out_normal, uint64_t* out_summary,
                                  std::string* err);
// SPH gradient tensors (pgsd.hoomd.sph_gradient_tensors is the definition): per entry of a row list in cell order the
// kernel-gradient correction matrix, its determinant, the corrected velocity-gradient tensor and the shear rate over the
// entries inside the support 2h, in the sums' order, and over the list the entries left uncorrected, the ranges of the
// determinant and of the trace and the largest shear rate.  The grid, the support, the list, the defaults and G are
// SphGradientsArgs' (volume is set: the density default is a number here; surface and surface_below are not looked at).
enum
    {
    SPHT_SUMMARY_WORDS = 14 // n, nowhere, not_finite, uncorrected, det_at, det_row, shear_at, shear_row, det (min, max),
                            // trace (min, max), the largest shear rate, 0
    };
struct SphTensorsArgs : SphGradientsArgs
    {
    double det_min; // an entry is corrected where det_min < det < +inf; a number, at least 0
    };
// the summary of no entry
inline void sph_tensors_of_nothing(uint64_t* out_summary)
    {
    const double lo = HUGE_VAL, hi = -HUGE_VAL;
    std::fill(out_summary, out_summary + SPHT_SUMMARY_WORDS, (uint64_t)0); // (+0.0 is the zero word)
    out_summary[4] = out_summary[5] = out_summary[6] = out_summary[7] = SPH_NONE;
    for (int s = 0; s < 2; s++)
        {
        memcpy(&out_summary[8 + 2 * s], &lo, sizeof(double));
        memcpy(&out_summary[9 + 2 * s], &hi, sizeof(double));
        }
    }
// stage the chunks that are present (ranges[0 .. 3] as device_pipeline_sph_gradients), check the lists, sum and invert
// on the GPU; out_correction (device, a.n x 6), out_determinant (a.n), out_gradient (a.n x 9), out_shear (a.n), each or
// null; out_summary (host, 14 words) is written on success only, and so are the device outputs; synchronous.  The
// refusals and the staging are device_pipeline_sph_sums'.
int device_pipeline_sph_tensors(DevicePipeline*, const ChunkRange* ranges, const SphTensorsArgs& a, double* out_correction,
                                double* out_determinant, double* out_gradient, double* out_shear, uint64_t* out_summary,
                                std::string* err);
// SPH accelerations (pgsd.hoomd.sph_accelerations is the definition): per entry of a row list in cell order the pressure
// acceleration -sum_j m_j (p_i/rho_i^2 + p_j/rho_j^2) grad_i W_ij, Morris' laminar viscous acceleration for one constant
// mu and their sum with gravity over the entries inside the support 2h, in the sums' order, and over the list the
// largest of each with its row.  The grid, the support, the list and the mass and density defaults are SphArgs'
// (volume, surface and surface_below are not looked at: the density default is a number here).
enum
    {
    SPHF_SUMMARY_WORDS = 12 // n, nowhere, not_finite, 3 x (at, row) of total, pressure, viscous, then total2, pressure2, viscous2
    };
struct SphForcesArgs : SphGradientsArgs
    {
    const void* pressure;    // the staged pressure chunk, N x 1, or null: the default stands for every row
    double pressure_default;
    double eta2, Gv;         // (0.01*h)*h and G*(2.0*mu), formed once on the host (Gv is not looked at without `viscous`)
    double gravity[3];
    uint32_t pressure_f64;   // present bit 4: a pressure chunk is stored (ranges[4])
    uint32_t viscous;        // a viscosity was given: the viscous term is formed
    };
// the summary of no entry
inline void sph_forces_of_nothing(uint64_t* out_summary)
    {
    std::fill(out_summary, out_summary + SPHF_SUMMARY_WORDS, (uint64_t)0); // (+0.0 is the zero word)
    std::fill(out_summary + 3, out_summary + 9, (uint64_t)SPH_NONE);
    }
// stage the chunks that are present (ranges[0 .. 4]: position, mass, density, velocity, pressure; the five pointers are
// filled in) -- or take them from what an earlier call left staged --, check the lists, sum on the GPU; out_pressure_acc,
// out_viscous_acc, out_total (device, a.n x 3, or null; the second is written with a.viscous only); out_summary (host, 12
// words) is written on success only, and so are the device outputs; synchronous.  The refusals and the staging are
// device_pipeline_sph_sums'.
int device_pipeline_sph_accelerations(DevicePipeline*, const ChunkRange* ranges, const SphForcesArgs& a,
                                      double* out_pressure_acc, double* out_viscous_acc, double* out_total,
                                      uint64_t* out_summary, std::string* err);
// SPH body forces (pgsd.hoomd.sph_body_force is the definition): a pair pass between two row lists in cell order on one
// grid -- the targets (the body: rows, cell and n of SphArgs) and the sources (the fluid) -- and over the targets the
// ordered sums of the force m_b * acc_b and of the torque r_b x it about a point.  The grid, the support, the columns,
// their defaults and the per-pair arithmetic are SphForcesArgs' (gravity is not looked at).
enum
    {
    SPHB_SUMMARY_WORDS = 22, // n_t, targets nowhere, n_s, sources nowhere, wetted, pairs, bad, largest (at, row, fp2), 12 sums
    SPHB_TILE = 4096         // entries of one tile of the ordered sum (pgsd.hoomd._ordered_sum)
    };
struct SphBodyArgs : SphForcesArgs
    {
    const uint32_t* fluid_rows; // device, n_fluid entries in cell order
    const int32_t* fluid_cell;  // device, n_fluid ids, non-decreasing, in [0, n_cells]
    uint64_t n_fluid;
    double about[3];            // the point the torque is taken about
    };
// the summary of no target: n_fluid sources, none of them looked at
inline void sph_body_force_of_nothing(uint64_t n_fluid, uint64_t* out_summary)
    {
    std::fill(out_summary, out_summary + SPHB_SUMMARY_WORDS, (uint64_t)0); // (+0.0 is the zero word)
    out_summary[2] = n_fluid;
    out_summary[7] = out_summary[8] = (uint64_t)SPH_NONE;
    }
// stage the chunks that are present (ranges[0 .. 4] as device_pipeline_sph_accelerations; both lists read the same staged
// chunks), check both lists, sum on the GPU; out_contacts (device, a.n words), out_pressure_acc, out_viscous_acc (device,
// a.n x 3, the second written with a.viscous only), each or null; out_summary (host, 22 words) is written on success
// only, and so are the device outputs; synchronous.  The refusals and the staging are device_pipeline_sph_sums'.
int device_pipeline_sph_body_force(DevicePipeline*, const ChunkRange* ranges, const SphBodyArgs& a, uint32_t* out_contacts,
                                   double* out_pressure_acc, double* out_viscous_acc, uint64_t* out_summary, std::string* err);
// SPH samples (pgsd.hoomd.sph_samples is the definition): per point of the caller's choosing the entries of a row list in
// cell order strictly inside the support 2h of it, the density sigma * sum m_j w, the Shepard sum sigma * sum V_j w and per
// value column sigma * sum V_j w f_j (or, normalised, sum V_j w f_j / sum V_j w), in the sums' order around the point's
// cell, and over the points how many are nowhere, outside the box, empty or not finite, the largest count and the ranges
// of the two sums.  The grid, the support, the list and the mass and density defaults are SphArgs' (volume, surface and
// surface_below are not looked at: the density default is a number here).
enum
    {
    SPHS_SUMMARY_WORDS = 11, // K, nowhere, outside, empty, not_finite, count_max, count_max_at, shepard min, max, density min, max
    SPHS_MAX_VALUES = 4,     // value chunks of one call
    SPHS_MAX_WIDTH = 4,      // columns of one value chunk
    SPHS_MAX_COLUMNS = 8,    // columns of all of them together
    SPHS_CHUNKS = 3 + SPHS_MAX_VALUES // position, mass, density, then the values
    };
struct SphSamplesArgs : SphArgs
    {
    const void* value[SPHS_MAX_VALUES];      // the staged value chunks, N x value_columns[s], or null: the default stands
    double value_default[SPHS_MAX_VALUES];   // ... for every element of the slot
    uint32_t value_columns[SPHS_MAX_VALUES]; // 0: the slot is unused (the used slots come first)
    uint32_t value_f64[SPHS_MAX_VALUES];     // present bit 3 + s: value chunk s is stored (ranges[3 + s])
    DomainArgs d;                            // the box as the cell order's key kernel takes it (L, xy, xz, yz, dims)
    const double* points;                    // device, K x 3
    uint64_t K;
    uint32_t C;                              // the columns together
    uint32_t normalise;
    };
// the summary of no point
inline void sph_samples_of_nothing(uint64_t* out_summary)
    {
    const double lo = HUGE_VAL, hi = -HUGE_VAL;
    std::fill(out_summary, out_summary + SPHS_SUMMARY_WORDS, (uint64_t)0);
    out_summary[6] = SPH_NONE;
    for (int s = 0; s < 2; s++)
        {
        memcpy(&out_summary[7 + 2 * s], &lo, sizeof(double));
        memcpy(&out_summary[8 + 2 * s], &hi, sizeof(double));
        }
    }
// stage the chunks that are present (ranges[0 .. 6]: position, mass, density, the values; the pointers are filled in) --
// or take them from what an earlier call left staged; a list of no entry stages nothing --, check the lists, sample on the
// GPU; out_count (device, a.K), out_density, out_shepard (device, a.K), out_values (device, a.K x a.C), each or null;
// out_summary (host, 11 words) is written on success only, and so are the device outputs; synchronous.  The refusals and
// the staging are device_pipeline_sph_sums'.
int device_pipeline_sph_samples(DevicePipeline*, const ChunkRange* ranges, const SphSamplesArgs& a, uint32_t* out_count,
                                double* out_density, double* out_shepard, double* out_values, uint64_t* out_summary,
                                std::string* err);
// Neighbour lists (pgsd.hoomd.neighbour_list is the definition): the neighbours the census counts, handed over as a CSR
// pair list -- per entry of a row list in cell order the list positions of its neighbours in the order the SPH kernel
// sums define, in two calls: the offsets (count, scan), then the segments (fill).  The grid, the range and the list are
// NeighboursArgs' (bins is not looked at).
enum
    {
    NLIST_HALF = 1u,         // bit of the entry points' flags: the segment of i keeps j > i by list position
    NLIST_SUMMARY_WORDS = 4  // n, nowhere, pairs, longest
    };
struct NeighbourListArgs : NeighboursArgs
    {
    uint32_t half, pad2;
    };
// stage the position chunk (or take it from what the ordering left staged), check the lists, count and scan on the GPU:
// out_offsets (device, a.n + 1 words) and out_summary (host, 4 words) are written on success only; synchronous.  n == 0:
// nothing is staged and no kernel runs, out_offsets[0] = 0 is one memset on the pipeline's stream.  The refusals and the
// staging are device_pipeline_neighbours'.
int device_pipeline_neighbour_offsets(DevicePipeline*, long long file_offset, size_t bytes, const NeighbourListArgs& a,
                                      uint64_t* out_offsets, uint64_t* out_summary, std::string* err);
// ... and fill the segments the offsets (device, a.n + 1 words, as the call above left them for the same arguments) cut
// out of out_neighbours (device, capacity words) and out_distance2 (device, capacity doubles, or null); synchronous.  No
// store lands at or beyond `capacity` or outside an entry's segment; offsets that are not this list's, or that hold more
// pairs than the capacity, refuse the call (PGSD_ERROR_INVALID_ARGUMENT): the outputs are then unspecified inside the
// capacity and untouched outside it.
int device_pipeline_neighbour_list(DevicePipeline*, long long file_offset, size_t bytes, const NeighbourListArgs& a,
                                   const uint64_t* offsets, uint64_t capacity, uint32_t* out_neighbours,
                                   double* out_distance2, std::string* err);
// Components (pgsd.hoomd.neighbour_components is the definition): the connected components of the graph whose edges are
// the pairs of the half neighbour list -- the friends-of-friends grouping of a list with the linking length r.  The grid,
// the range and the list are NeighboursArgs' (bins is not looked at).
enum
    {
    COMPONENTS_SUMMARY_WORDS = 6 // n, nowhere, components, singletons, largest, largest_label
    };
// stage the position chunk (or take it from what the ordering left staged), check the lists, link and number on the GPU:
// out_label (device, a.n words: the smallest list position of the entry's component), out_component (device, a.n words:
// the dense id, or null), out_sizes (device, room for a.n words of which the first `components` are written, or null);
// out_summary (host, 6 words) is written on success only; synchronous.  No store lands at an index >= a.n.  a.n > 0 (the
// entry point answers a list of no entry with six zeros and stages nothing).  The refusals and the staging are
// device_pipeline_neighbours'.
int device_pipeline_components(DevicePipeline*, long long file_offset, size_t bytes, const NeighboursArgs& a,
                               uint32_t* out_label, uint32_t* out_component, uint32_t* out_sizes, uint64_t* out_summary,
                               std::string* err);
// Component fields (pgsd.hoomd.component_moments is the definition): per component of a components result the nine sums
// of the cell fields with the position replaced by the single-shift minimum-image displacement from the component's root
// (its smallest member), in the cell fields' order over the component's entries in list order; the extent of those
// displacements, the root's position, and whether the extent reaches half a box length (the piece may percolate).
enum
    {
    CMOM_SUMMARY_WORDS = 6, // n, components, bad entries, wide components, heaviest, widest
    CMOM_EXTENT = 6         // lo[3], hi[3]
    };
struct ComponentMomentsArgs : GroupedArgs // chunk: the conservation sums' order; the typeid slot stays empty
    {
    double defaults[8];        // mass, v[3], energy, x[3] (the position is always a chunk: x is not looked at)
    double vectors[6];         // Lx, Ly, Lz, xy*Ly, xz*Lz, yz*Lz
    const uint32_t* label;     // device, n: the smallest list position of the entry's component
    const uint32_t* component; // device, n: the dense id
    uint32_t components;
    uint32_t dimensions;
    };
// stage the chunks that are present, check, sort and sum on the GPU; the results land in the caller's device arrays and
// out_summary (host, 6 words) is written on success only; synchronous.  c.n > 0.  The staged rows stay until the next
// wait_read.
int device_pipeline_component_moments(DevicePipeline*, const ChunkRange* ranges, const ComponentMomentsArgs& c,
                                      double* out_sums, double* out_extent, double* out_origin, uint32_t* out_flags,
                                      uint64_t* out_summary, std::string* err);
// A row plan (sparse indexed reads): the chunk's N rows cut into blocks of R rows; `blocks` are the blocks that hold at
// least one of rows[0 .. n) (ascending: block b's slot in the compact staging is its position in this list), merged
// into runs of neighbours (run_first[i], run_blocks[i]); rows2[k] = slot * R + rows[k] % R indexes that staging, whose
// height is staged_rows (T * R, less where the chunk's short last block is touched).  An entry >= N touches nothing
// and becomes 0xFFFFFFFF.  rows and rows2 are device memory of the caller's.
struct RowPlan
    {
    uint64_t n = 0, N = 0;
    uint32_t R = 0;
    uint64_t staged_rows = 0;
    const uint32_t* rows = nullptr;
    uint32_t* rows2 = nullptr;
    std::vector<uint32_t> blocks, run_first, run_blocks;
    };
// fill in a plan (n, N, rows, rows2 set by the caller; R == 0: the tuning variable PGSD_PLAN_BLOCK_ROWS) on the GPU;
// synchronous
int device_pipeline_plan_rows(DevicePipeline*, RowPlan& plan, std::string* err);
// sparse indexed read: only the plan's runs of the chunk at `chunk_offset` (plan.N rows of row_bytes each) are read and
// staged, block b at slot(b) * R rows; wait_read gathers through plan.rows2.  The plan outlives the wait.
int device_pipeline_read_planned(DevicePipeline*, long long chunk_offset, size_t row_bytes, const pgsd_unpack_job& job,
                                 const RowPlan& plan, std::string* err);
// file bytes the read side has pread and bytes it has copied host-to-device since creation / the last reset
void device_pipeline_read_counters(DevicePipeline*, uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset);
int device_pipeline_drain(DevicePipeline*, std::string* err);
void device_pipeline_stats(DevicePipeline*, pgsd_device_stats* out, int reset);

size_t sizeof_type(uint32_t type);
    } // namespace pgsd_amd

#endif
