// pgsd_read.cpp -- lookups and reads (pgsd_find_chunk pgsd.c:2295-2434, pgsd_read_chunk :2436-2537,
// pgsd_find_matching_chunk_name :2557-2641) and their device twin (file -> pinned slabs -> HBM -> unpack kernel).
// The index is replicated, so a lookup is valid on every rank; what a read flushes first is decided here
// (pgsd_set_local_reads).
#include "pgsd_file_impl.hpp"

namespace pgsd_amd
    {
int flush_for_lookup(Impl* s)
    {
    if (s->flags == PGSD_OPEN_READONLY)
        return PGSD_SUCCESS;
    // pgsd_set_local_reads covers the lookup that precedes the read: a frame that wrote buffered small
    // chunks only -- everything else elided -- leaves metadata pending behind pgsd_end_frame (pgsd.c:1941-1950), and
    // a rank that then looks one of frame 0's chunks up ALONE (it is the only one that compares that array) must not
    // start the collective flush.  It sees what the last flush committed; chunks of frames still pending are
    // not found until then.  (One rank: the flush is nobody else's business and runs as ever -- a one-rank file stays
    // the reference's byte for byte with local reads on, tests/test_product_golden.py.)  A lookup that MISSES while
    // metadata is pending says so in pgsd_last_error_string() (note_pending_miss below).
    if (metadata_pending(s) && (!s->local_reads || s->P == 1))
        return do_flush(s);
    return drain_own_copies(s);
    }

// What a READ needs before it touches the file: the reference's flush (collective) -- or, with
// pgsd_set_local_reads, only this rank's own asynchronous copies in place.
int flush_for_read(Impl* s)
    {
    if (s->flags == PGSD_OPEN_READONLY)
        return PGSD_SUCCESS;
    if (!s->local_reads)
        return do_flush(s);
    return drain_own_copies(s);
    }
    } // namespace pgsd_amd

using namespace pgsd_amd;

// ============================================================================ C ABI

// A LOCAL lookup (pgsd_set_local_reads, several ranks) that finds nothing while replicated metadata is still pending
// may have missed a chunk the next collective flush commits: the caller is told in pgsd_last_error_string()
// (callers of local_reads got the behaviour with no signal).
static void note_pending_miss(const Impl* s, const char* what, const char* name)
    {
    if (s->flags != PGSD_OPEN_READONLY && s->local_reads && s->P > 1 && metadata_pending(s))
        set_last_error(std::string(what) + " '" + name
                       + "': not found by a LOCAL lookup (pgsd_set_local_reads) while names / index entries of sealed "
                         "frames are pending: they are seen after the next collective pgsd_flush");
    }

static const pgsd_index_entry* find_chunk(Impl* s, uint64_t frame, const char* name)
    {
    auto it = s->name_map.find(name);
    if (it == s->name_map.end())
        return NULL;
    uint16_t match_id = it->second;

    if (!s->v1())
        {
        ssize_t L = 0, R = (ssize_t)s->file_index_size - 1;
        pgsd_index_entry T;
        memset(&T, 0, sizeof(T));
        T.frame = frame;
        T.id = match_id;
        while (L <= R)
            {
            size_t m = (size_t)((L + R) / 2);
            int c = cmp_entry(s->file_index[m], T);
            if (c == -1)
                L = (ssize_t)m + 1;
            else if (c == 1)
                R = (ssize_t)m - 1;
            else
                return &s->file_index[m];
            }
        return NULL;
        }
    // v1 files: the index is only ordered by frame (pgsd.c:2380-2430)
    if (s->file_index_size == 0)
        return NULL;
    size_t L = 0, R = s->file_index_size;
    do
        {
        size_t m = (L + R) / 2;
        if (frame < s->file_index[m].frame)
            R = m;
        else
            L = m;
        } while ((R - L) > 1);
    for (int64_t cur = (int64_t)L; cur >= 0 && s->file_index[(size_t)cur].frame == frame; cur--)
        if (s->file_index[(size_t)cur].id == match_id)
            return &s->file_index[(size_t)cur];
    return NULL;
    }

extern "C" const struct pgsd_index_entry* pgsd_find_chunk(struct pgsd_handle* handle, uint64_t frame,
                                                          const char* name)
    try
    {
    // pgsd.c:2295-2434; valid on every rank because the index is replicated
    Impl* s = impl_of(handle);
    if (!s || !name)
        return NULL;
    if (frame >= s->cur_frame)
        return NULL;
    if (s->flags != PGSD_OPEN_READONLY)
        {
        int rc = flush_for_lookup(s);
        publish(handle, s);
        if (rc != PGSD_SUCCESS)
            return NULL;
        }
    const pgsd_index_entry* e = find_chunk(s, frame, name);
    if (!e)
        note_pending_miss(s, "pgsd_find_chunk", name);
    return e;
    }
catch (...)
    {
        pgsd_amd::abi_guard();
        return nullptr;
    }

extern "C" int pgsd_read_chunk(struct pgsd_handle* handle, void* data, const struct pgsd_index_entry* chunk,
                               uint64_t N, uint32_t M, uint32_t offset, bool all)
    try
    {
    // pgsd.c:2436-2537
    Impl* s = impl_of(handle);
    if (!s || !data || !chunk)
        return PGSD_ERROR_INVALID_ARGUMENT;
    // copy first: a flush may move the index storage the entry points into
    pgsd_index_entry c = *chunk;
    if (s->flags != PGSD_OPEN_READONLY)
        {
        int rc = flush_for_read(s);
        publish(handle, s);
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    size_t sz = sizeof_type(c.type);
    uint64_t stride = 0;
    size_t size;
    uint64_t off_elems = (uint64_t)offset * M;
    if (!all)
        size = c.N * c.M * sz;
    else
        {
        size = N * M * sz;
        stride = off_elems * sz;
        }
    if (size == 0)
        return PGSD_ERROR_FILE_CORRUPT;
    if (c.location == 0)
        return PGSD_ERROR_FILE_CORRUPT;
    if ((uint64_t)(c.location + size + stride) > (uint64_t)s->file_size)
        return PGSD_ERROR_FILE_CORRUPT;
    pread_parallel(s->fd, data, size, c.location + (long long)stride);
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" const char* pgsd_find_matching_chunk_name(struct pgsd_handle* handle, const char* match,
                                                     const char* prev)
    try
    {
    // pgsd.c:2557-2641
    Impl* s = impl_of(handle);
    if (!s || !match)
        return NULL;
    if (s->file_n_names == 0)
        return NULL; // checked before the flush, like pgsd.c:2573-2584
    if (s->flags != PGSD_OPEN_READONLY)
        {
        // `prev` points into the name storage, which a flush may reallocate: carry it over
        size_t prev_off = 0;
        bool have_prev = prev != NULL;
        if (have_prev)
            {
            if (prev < s->file_names.d.data() || prev >= s->file_names.d.data() + s->file_names.reserved())
                return NULL;
            prev_off = (size_t)(prev - s->file_names.d.data());
            }
        int rc = flush_for_lookup(s);
        publish(handle, s);
        if (rc != PGSD_SUCCESS)
            return NULL;
        if (have_prev)
            prev = s->file_names.d.data() + prev_off;
        }
    if (s->file_n_names == 0)
        return NULL;
    const char* base = s->file_names.d.data();
    const char* end = base + s->file_names.reserved();
    if (end[-1] != 0)
        return NULL;
    const char* p;
    if (!prev)
        p = base;
    else
        {
        if (prev < base || prev >= end)
            return NULL;
        p = s->v1() ? prev + PGSD_NAME_SIZE : prev + strlen(prev) + 1;
        }
    size_t ml = strlen(match);
    while (p < end)
        {
        if (p[0] != 0 && 0 == strncmp(match, p, ml))
            return p;
        p += s->v1() ? (size_t)PGSD_NAME_SIZE : strlen(p) + 1;
        }
    return NULL;
    }
catch (...)
    {
        pgsd_amd::abi_guard();
        return nullptr;
    }

extern "C" int pgsd_set_local_reads(struct pgsd_handle* handle, int on)
    try
    {
    Impl* s = impl_of(handle);
    if (!s)
        return PGSD_ERROR_INVALID_ARGUMENT;
    s->local_reads = on != 0;
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_read_chunk_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk, uint64_t N,
                                      uint64_t row_offset, const struct pgsd_field_dst* dst)
    try
    {
    // device twin of pgsd_read_chunk's all==true slab read (pgsd.c:2498-2534)
    Impl* s = impl_of(handle);
    if (!s || !chunk || !dst || !dst->dst)
        return PGSD_ERROR_INVALID_ARGUMENT;
    pgsd_index_entry c = *chunk; // a flush may move the index storage
    if (s->flags != PGSD_OPEN_READONLY)
        {
        int rc = flush_for_read(s);
        publish(handle, s);
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    const size_t sz = sizeof_type(c.type);
    if (sz == 0 || c.M == 0)
        return PGSD_ERROR_FILE_CORRUPT;
    if (N == 0)
        return PGSD_SUCCESS;
    if (row_offset + N > c.N)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (c.location == 0)
        return PGSD_ERROR_FILE_CORRUPT;
    const uint64_t rowbytes = (uint64_t)c.M * sz;
    const long long foff = c.location + (long long)(row_offset * rowbytes);
    const size_t bytes = (size_t)(N * rowbytes);
    if ((uint64_t)(foff + (long long)bytes) > (uint64_t)s->file_size)
        return PGSD_ERROR_FILE_CORRUPT;
    int rc = ensure_device(s);
    if (rc != PGSD_SUCCESS)
        return rc;
    pgsd_unpack_job job;
    memset(&job, 0, sizeof(job));
    job.src_type = c.type;
    job.M = c.M;
    job.dst = *dst;
    std::string err;
    rc = device_pipeline_read(s->dev, foff, bytes, job, N, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_device_wait_read(struct pgsd_handle* handle)
    try
    {
    Impl* s = impl_of(handle);
    if (!s)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (!s->dev)
        return PGSD_SUCCESS;
    std::string err;
    int rc = device_pipeline_wait_read(s->dev, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

// An entry point's refusal: "<who>: <msg>" becomes the thread's last error.
struct Refusal
    {
    const char* who;
    int operator()(const std::string& msg) const
        {
        set_last_error(std::string(who) + ": " + msg);
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    };

// A float chunk of a pair pass, `subject` in the messages: float32 or float64 elements, `columns` columns, and -- the
// position chunk (no N_expected) -- fewer than 2^32 rows, or -- a column chunk -- the position chunk's *N_expected rows.
static int float_chunk(const Refusal& refuse, const pgsd_index_entry& c, const std::string& subject, uint32_t columns,
                       const uint64_t* N_expected, uint32_t* is_f64)
    {
    if (c.type != PGSD_TYPE_FLOAT && c.type != PGSD_TYPE_DOUBLE)
        return refuse(subject + " holds float32 or float64 elements");
    if (c.M != columns)
        return refuse(subject + " has " + std::to_string(columns) + (columns == 1 ? " column" : " columns"));
    if (!N_expected && c.N >= (1ull << 32))
        return refuse("chunks of 2^32 rows or more have no 32-bit row list");
    if (N_expected && c.N != *N_expected)
        return refuse(subject + " and the position chunk differ in their number of rows");
    *is_f64 = c.type == PGSD_TYPE_DOUBLE ? 1u : 0u;
    return PGSD_SUCCESS;
    }

// The grid of a pair pass against its box and its reach (`noun` in the messages: the range, the support 2h):
// pgsd.hoomd.ghost_fractions and cell_grid_for, from the tilt factors the vectors hold (xy * Ly is an exact product of
// float32 values, so the quotient is the stored factor).  *n_cells: the cells of the grid.
static int pair_grid(const Refusal& refuse, const double vectors[6], double reach, const char* noun, uint32_t dimensions,
                     const uint32_t cells[3], uint32_t* n_cells)
    {
    const double Lx = vectors[0], Ly = vectors[1], Lz = vectors[2];
    if (!(Lx > 0.0 && Ly > 0.0 && (dimensions == 2 || Lz > 0.0)))
        return refuse("box lengths must be positive (Lz unless dimensions == 2)");
    const double xy = vectors[3] / Ly, xz = Lz > 0.0 ? vectors[4] / Lz : 0.0, yz = Lz > 0.0 ? vectors[5] / Lz : 0.0;
    const double t = xy * yz - xz;
    const double u = 1.0 + xy * xy;
    const double plane[3] = {Lx / std::sqrt(u + t * t), Ly / std::sqrt(1.0 + yz * yz), Lz};
    uint64_t n = 1;
    for (int a = 0; a < 3; a++)
        {
        if (cells[a] < 1 || cells[a] > ORDER_MAX_AXIS_CELLS)
            return refuse("every axis takes 1 to 1024 cells");
        n *= cells[a];
        if (a == 2 && dimensions == 2)
            {
            if (cells[2] != 1)
                return refuse("dimensions == 2 takes one z cell (z is not looked at)");
            continue;
            }
        const double g = reach / plane[a];
        if (!(g <= 0.5))
            return refuse(std::string("the ") + noun
                          + " exceeds half the box's nearest plane distance on an axis: an image would count twice");
        const double most = std::min(std::max(std::floor(1.0 / g), 1.0), (double)ORDER_MAX_AXIS_CELLS);
        if ((double)cells[a] > most)
            return refuse(std::string("the cells are narrower than the ") + noun + " on an axis");
        }
    if (n > CELLS_MAX_CELLS)
        return refuse("a grid holds 1 to 2^20 cells");
    *n_cells = (uint32_t)n;
    return PGSD_SUCCESS;
    }

// The file range of a device read of a whole chunk, checked against the file; the flush a read needs comes first.
static int whole_chunk_range(Impl* s, struct pgsd_handle* handle, const pgsd_index_entry& c, long long* foff, size_t* bytes)
    {
    if (s->flags != PGSD_OPEN_READONLY)
        {
        int rc = flush_for_read(s);
        publish(handle, s);
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    const size_t sz = sizeof_type(c.type);
    if (sz == 0 || c.M == 0)
        return PGSD_ERROR_FILE_CORRUPT;
    if (c.N >= (1ull << 32))
        {
        set_last_error("chunks of 2^32 rows or more have no 32-bit row list");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    if (c.N == 0)
        {
        *foff = 0;
        *bytes = 0;
        return PGSD_SUCCESS;
        }
    if (c.location == 0)
        return PGSD_ERROR_FILE_CORRUPT;
    *bytes = (size_t)(c.N * c.M * sz);
    *foff = c.location;
    if ((uint64_t)(c.location + (long long)*bytes) > (uint64_t)s->file_size)
        return PGSD_ERROR_FILE_CORRUPT;
    return ensure_device(s);
    }

// The domain of a selection, checked (`who`: the entry point, for the message) and turned into the kernel's arguments
// (d->pos stays open).
static int domain_args(const char* who, const pgsd_index_entry& c, const float box[6], uint32_t dimensions,
                       const double lo[3], const double hi[3], DomainArgs* d)
    {
    if (dimensions != 2 && dimensions != 3)
        return PGSD_ERROR_INVALID_ARGUMENT;
    for (int a = 0; a < 3; a++)
        if (!(0.0 <= lo[a] && lo[a] < hi[a] && hi[a] <= 1.0))
            {
            set_last_error(std::string(who) + ": the domain must satisfy 0 <= lo < hi <= 1 on every axis");
            return PGSD_ERROR_INVALID_ARGUMENT;
            }
    if (!(box[0] > 0.0f && box[1] > 0.0f && (dimensions == 2 || box[2] > 0.0f)))
        {
        set_last_error(std::string(who) + ": box lengths must be positive (Lz unless dimensions == 2)");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    if ((c.type != PGSD_TYPE_FLOAT && c.type != PGSD_TYPE_DOUBLE) || c.M != 3)
        {
        set_last_error(std::string(who) + ": positions are N x 3 float32 or float64 rows");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    memset(d, 0, sizeof(*d));
    d->N = c.N;
    d->f64 = c.type == PGSD_TYPE_DOUBLE ? 1u : 0u;
    d->dims = dimensions;
    for (int a = 0; a < 3; a++)
        {
        d->L[a] = (double)box[a];
        d->lo[a] = lo[a];
        d->hi[a] = hi[a];
        }
    d->xy = (double)box[3];
    d->xz = (double)box[4];
    d->yz = (double)box[5];
    return PGSD_SUCCESS;
    }

extern "C" int pgsd_select_domain_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                         const float box[6], uint32_t dimensions, const double lo[3], const double hi[3],
                                         uint32_t* out_rows, uint64_t* out_count)
    try
    {
    Impl* s = impl_of(handle);
    if (!s || !position || !box || !lo || !hi || !out_count)
        return PGSD_ERROR_INVALID_ARGUMENT;
    pgsd_index_entry c = *position; // a flush may move the index storage
    DomainArgs d;
    int rc = domain_args("pgsd_select_domain_device", c, box, dimensions, lo, hi, &d);
    if (rc != PGSD_SUCCESS)
        return rc;
    long long foff = 0;
    size_t bytes = 0;
    rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    *out_count = 0;
    if (c.N == 0)
        return PGSD_SUCCESS;
    if (!out_rows)
        return PGSD_ERROR_INVALID_ARGUMENT;
    std::string err;
    rc = device_pipeline_select_domain(s->dev, foff, bytes, d, out_rows, out_count, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_select_halo_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position, const float box[6],
                                       uint32_t dimensions, const double lo[3], const double hi[3], const double bands[24],
                                       const uint32_t divided[3], uint32_t* out_rows, int32_t* out_shift,
                                       uint64_t out_counts[2])
    try
    {
    static const char* who = "pgsd_select_halo_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !box || !lo || !hi || !bands || !divided || !out_counts)
        return PGSD_ERROR_INVALID_ARGUMENT;
    pgsd_index_entry c = *position; // a flush may move the index storage
    HaloArgs h;
    memset(&h, 0, sizeof(h));
    int rc = domain_args(who, c, box, dimensions, lo, hi, &h.d);
    if (rc != PGSD_SUCCESS)
        return rc;
    for (int a = 0; a < 3; a++)
        {
        h.divided[a] = divided[a] ? 1u : 0u;
        for (int k = 0; k < 8; k++)
            {
            const double b = bands[a * 8 + k];
            if (!(0.0 <= b && b <= 1.0))
                {
                set_last_error(std::string(who) + ": the band bounds must lie in [0, 1]");
                return PGSD_ERROR_INVALID_ARGUMENT;
                }
            h.band[a][k] = b;
            }
        }
    long long foff = 0;
    size_t bytes = 0;
    rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    out_counts[0] = out_counts[1] = 0;
    if (c.N == 0)
        return PGSD_SUCCESS;
    if (!out_rows || !out_shift)
        return PGSD_ERROR_INVALID_ARGUMENT;
    std::string err;
    rc = device_pipeline_select_halo(s->dev, foff, bytes, h, out_rows, out_shift, out_counts, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

// The census entry points' first half: the checks and staging arguments of pgsd_select_domain_device over the whole box.
static int census_args(const char* who, Impl* s, struct pgsd_handle* handle, const pgsd_index_entry& c, const float box[6],
                       uint32_t dimensions, DomainArgs* d, long long* foff, size_t* bytes)
    {
    static const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.0, 1.0};
    int rc = domain_args(who, c, box, dimensions, lo, hi, d);
    if (rc != PGSD_SUCCESS)
        return rc;
    return whole_chunk_range(s, handle, c, foff, bytes);
    }

extern "C" int pgsd_domain_histogram_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                            const float box[6], uint32_t dimensions, uint32_t bins, uint64_t* out_hist)
    try
    {
    static const char* who = "pgsd_domain_histogram_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !box || !out_hist)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (bins < 2 || bins > CENSUS_MAX_BINS || (bins & (bins - 1)) != 0)
        {
        set_last_error(std::string(who) + ": bins must be a power of two in [2, 4096]");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    pgsd_index_entry c = *position; // a flush may move the index storage
    DomainArgs d;
    long long foff = 0;
    size_t bytes = 0;
    int rc = census_args(who, s, handle, c, box, dimensions, &d, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (c.N == 0)
        {
        memset(out_hist, 0, 3 * (size_t)bins * sizeof(uint64_t));
        return PGSD_SUCCESS;
        }
    std::string err;
    rc = device_pipeline_domain_histogram(s->dev, foff, bytes, d, bins, out_hist, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_domain_counts_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                         const float box[6], uint32_t dimensions, const uint32_t n[3],
                                         const double* interior_bounds, uint64_t* out_counts, uint64_t* out_nowhere)
    try
    {
    static const char* who = "pgsd_domain_counts_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !box || !n || !out_counts || !out_nowhere)
        return PGSD_ERROR_INVALID_ARGUMENT;
    CellArgs cells;
    memset(&cells, 0, sizeof(cells));
    uint64_t n_cells = 1;
    for (int a = 0; a < 3; a++)
        {
        if (n[a] < 1 || n[a] > CENSUS_MAX_AXIS_CELLS)
            {
            set_last_error(std::string(who) + ": every axis takes 1 to 64 cells");
            return PGSD_ERROR_INVALID_ARGUMENT;
            }
        n_cells *= n[a];
        }
    if (n_cells > CENSUS_MAX_CELLS)
        {
        set_last_error(std::string(who) + ": at most 4096 cells");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    if (dimensions == 2 && n[2] != 1)
        {
        set_last_error(std::string(who) + ": dimensions == 2 takes one z cell (z is not looked at)");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    if (!interior_bounds && n_cells > 1)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const double* b = interior_bounds;
    for (int a = 0; a < 3; a++)
        {
        cells.n[a] = n[a];
        double below = 0.0;
        for (uint32_t j = 0; j + 1 < n[a]; j++, b++)
            {
            if (!(below < *b && *b < 1.0))
                {
                set_last_error(std::string(who) + ": the interior bounds of an axis must ascend strictly inside (0, 1)");
                return PGSD_ERROR_INVALID_ARGUMENT;
                }
            cells.bounds[a][j] = below = *b;
            }
        }
    pgsd_index_entry c = *position; // a flush may move the index storage
    long long foff = 0;
    size_t bytes = 0;
    int rc = census_args(who, s, handle, c, box, dimensions, &cells.d, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    *out_nowhere = 0;
    if (c.N == 0)
        {
        memset(out_counts, 0, (size_t)n_cells * sizeof(uint64_t));
        return PGSD_SUCCESS;
        }
    std::string err;
    rc = device_pipeline_domain_counts(s->dev, foff, bytes, cells, out_counts, out_nowhere, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_order_rows_by_cell_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                              const float box[6], uint32_t dimensions, const uint32_t cells[3],
                                              uint32_t* rows, uint64_t n, uint64_t n_owned, int32_t* shift, int32_t* out_cell)
    try
    {
    static const char* who = "pgsd_order_rows_by_cell_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !box || !cells)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    OrderArgs o;
    memset(&o, 0, sizeof(o));
    o.n_cells = 1;
    for (int a = 0; a < 3; a++)
        {
        if (cells[a] < 1 || cells[a] > ORDER_MAX_AXIS_CELLS)
            return refuse("every axis takes 1 to 1024 cells");
        o.cells[a] = cells[a];
        o.n_cells *= cells[a];
        }
    if (dimensions == 2 && cells[2] != 1)
        return refuse("dimensions == 2 takes one z cell (z is not looked at)");
    if (n_owned > n)
        return refuse("n_owned exceeds the number of entries");
    if (n >= (1ull << 32))
        return refuse("a row list holds fewer than 2^32 entries");
    pgsd_index_entry c = *position; // a flush may move the index storage
    DomainArgs d;
    long long foff = 0;
    size_t bytes = 0;
    int rc = census_args(who, s, handle, c, box, dimensions, &d, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n == 0)
        return PGSD_SUCCESS;
    if (!rows)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (c.N == 0)
        return refuse("an entry of the row list lies outside the position chunk (nothing was reordered)");
    o.d = d;
    o.n = n;
    o.n_owned = n_owned;
    std::string err;
    rc = device_pipeline_order_rows(s->dev, foff, bytes, o, rows, shift, out_cell, &err);
    if (rc == PGSD_ERROR_INVALID_ARGUMENT)
        return refuse(err.empty() ? std::string("refused") : err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

namespace
    {
// The tail of a reduction's entry point: `call` runs the pipeline; a refusal loses the launcher's prefix and becomes
// the entry point's own, any other failure keeps its text.  The caller copies the results out on success only.
template<class Call> int reduction_call(const char* who, const std::string& prefix, Call call)
    {
    std::string err;
    const int rc = call(&err);
    if (rc == PGSD_ERROR_INVALID_ARGUMENT)
        {
        if (err.compare(0, prefix.size(), prefix) == 0)
            err.erase(0, prefix.size());
        set_last_error(std::string(who) + ": " + (err.empty() ? std::string("refused") : err));
        }
    else if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }

// One chunk slot of a grouped reduction (conservation sums, frame displacements): its name and columns, what it holds,
// and how the pass speaks of it where its elements are of another kind.
enum GroupedKind
    {
    GROUPED_TYPEID,
    GROUPED_FLOAT,
    GROUPED_IMAGE
    };
struct GroupedSlot
    {
    const char* name;
    uint32_t columns;
    GroupedKind kind;
    const char* subject;
    };
const GroupedSlot g_moments_slots[GROUPED_CHUNKS] = {{"typeid", 1, GROUPED_TYPEID, "the typeid chunk"},
                                                     {"mass", 1, GROUPED_FLOAT, "the mass chunk"},
                                                     {"velocity", 3, GROUPED_FLOAT, "the velocity chunk"},
                                                     {"energy", 1, GROUPED_FLOAT, "the energy chunk"},
                                                     {"position", 3, GROUPED_FLOAT, "the position chunk"}};
const GroupedSlot g_displacement_slots[GROUPED_CHUNKS] = {{"position", 3, GROUPED_FLOAT, "a position chunk"},
                                                          {"image", 3, GROUPED_IMAGE, "an image chunk"},
                                                          {"position", 3, GROUPED_FLOAT, "a position chunk"},
                                                          {"image", 3, GROUPED_IMAGE, "an image chunk"},
                                                          {"typeid", 1, GROUPED_TYPEID, "the typeid chunk"}};

// The chunks a grouped reduction was given: element kind, columns, N below 2^32 and equal, the whole chunk's file range.
// Fills ranges[i] and a's present, N, typeid_signed and f64.  A refusal sets *why; any other failure leaves it empty.
int grouped_chunks(Impl* s, struct pgsd_handle* handle, const GroupedSlot* slots, const char* floats,
                   const struct pgsd_index_entry* const* given, GroupedArgs* a, ChunkRange* ranges, std::string* why)
    {
    const auto refuse = [why](const std::string& msg)
    {
        *why = msg;
        return PGSD_ERROR_INVALID_ARGUMENT;
    };
    uint32_t float_type = 0;
    for (int i = 0; i < GROUPED_CHUNKS; i++)
        {
        if (!given[i])
            continue;
        const GroupedSlot& slot = slots[i];
        pgsd_index_entry c = *given[i]; // a flush may move the index storage
        if (slot.kind == GROUPED_TYPEID)
            {
            if (c.type != PGSD_TYPE_UINT32 && c.type != PGSD_TYPE_INT32)
                return refuse(std::string(slot.subject) + " holds uint32 or int32 elements");
            a->typeid_signed = c.type == PGSD_TYPE_INT32 ? 1u : 0u;
            }
        else if (slot.kind == GROUPED_IMAGE)
            {
            if (c.type != PGSD_TYPE_INT32)
                return refuse(std::string(slot.subject) + " holds int32 elements");
            }
        else
            {
            if (c.type != PGSD_TYPE_FLOAT && c.type != PGSD_TYPE_DOUBLE)
                return refuse(std::string(slot.subject) + " holds float32 or float64 elements");
            if (float_type && c.type != float_type)
                return refuse(std::string("the ") + floats + " chunks share one element type (float32 or float64, not mixed)");
            float_type = c.type;
            }
        if (c.M != slot.columns)
            return refuse(std::string("the ") + slot.name + " chunk has " + std::to_string(slot.columns)
                          + (slot.columns == 1 ? " column" : " columns"));
        if (c.N >= (1ull << 32))
            return refuse("chunks of 2^32 rows or more have no 32-bit row list");
        if (a->present && c.N != a->N)
            return refuse("the chunks differ in their number of rows");
        a->N = c.N;
        int rc = whole_chunk_range(s, handle, c, &ranges[i].file_offset, &ranges[i].bytes);
        if (rc != PGSD_SUCCESS)
            return rc;
        a->present |= 1u << i;
        }
    a->f64 = float_type == PGSD_TYPE_DOUBLE ? 1u : 0u;
    return PGSD_SUCCESS;
    }
    } // namespace

extern "C" int pgsd_chunk_stats_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk, const uint32_t* rows,
                                       uint64_t n, uint32_t with_norm2, uint64_t* out_counts, double* out_values)
    try
    {
    static const char* who = "pgsd_chunk_stats_device";
    Impl* s = impl_of(handle);
    if (!s || !chunk || !out_counts || !out_values)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    pgsd_index_entry c = *chunk; // a flush may move the index storage
    std::string why;
    if (!chunk_stats_supported(c.type, c.M, with_norm2, &why))
        return refuse(why);
    if (c.N >= (1ull << 32))
        return refuse("chunks of 2^32 rows or more have no 32-bit row list");
    if (rows && n >= (1ull << 32))
        return refuse("a row list holds fewer than 2^32 entries");
    long long foff = 0;
    size_t bytes = 0;
    int rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    StatsArgs a;
    memset(&a, 0, sizeof(a));
    a.N = c.N;
    a.rows = rows;
    a.n = rows ? n : c.N;
    a.type = c.type;
    a.M = c.M;
    a.norm2 = with_norm2 ? 1u : 0u;
    const uint32_t C = a.M + a.norm2;
    if (a.n == 0)
        {
        chunk_stats_of_nothing(C, out_counts, out_values);
        return PGSD_SUCCESS;
        }
    if (c.N == 0)
        return refuse("an entry of the row list lies outside the chunk (nothing was computed)");
    // (the outputs are written on success only: the launcher fills these and they are copied out then)
    uint64_t counts[15];
    double values[15];
    rc = reduction_call(who, "chunk statistics: ", [&](std::string* err)
                        { return device_pipeline_chunk_stats(s->dev, foff, bytes, a, counts, values, err); });
    if (rc != PGSD_SUCCESS)
        return rc;
    std::copy(counts, counts + 3 * C, out_counts);
    std::copy(values, values + 3 * C, out_values);
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_frame_moments_device(struct pgsd_handle* handle, const struct pgsd_index_entry* typeid_chunk,
                                         const struct pgsd_index_entry* mass, const struct pgsd_index_entry* velocity,
                                         const struct pgsd_index_entry* energy, const struct pgsd_index_entry* position,
                                         const double defaults[8], uint32_t type0, uint32_t n_types, const uint32_t* rows,
                                         uint64_t n, uint64_t* out_counts, double* out_sums)
    try
    {
    static const char* who = "pgsd_frame_moments_device";
    Impl* s = impl_of(handle);
    if (!s || !defaults || !out_counts || !out_sums)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    const struct pgsd_index_entry* given[MOMENTS_CHUNKS] = {typeid_chunk, mass, velocity, energy, position};
    if (n_types < 1 || n_types > MOMENTS_MAX_TYPES)
        return refuse("a call takes 1 to 4 types");
    if (!typeid_chunk && n_types != 1)
        return refuse("without a typeid chunk there is one group: n_types must be 1");
    MomentsArgs a;
    memset(&a, 0, sizeof(a));
    ChunkRange ranges[MOMENTS_CHUNKS];
    memset(ranges, 0, sizeof(ranges));
    std::string why;
    int rc = grouped_chunks(s, handle, g_moments_slots, "float", given, &a, ranges, &why);
    if (rc != PGSD_SUCCESS)
        return why.empty() ? rc : refuse(why);
    if (n >= (1ull << 32) && (rows || !a.present))
        return refuse("a row list holds fewer than 2^32 entries");
    // without a stored chunk nothing bounds the entries of a list (no row is loaded); without a list the call says how many
    if (!a.present)
        a.N = rows ? (1ull << 32) : n;
    std::copy(defaults, defaults + 8, a.defaults);
    a.rows = rows;
    a.n = rows ? n : a.N;
    a.type0 = type0;
    a.n_types = n_types;
    // (the outputs are written on success only: the launcher fills these and they are copied out then)
    uint64_t counts[2 * MOMENTS_MAX_TYPES + 1] = {};
    double sums[MOMENTS_QUANTITIES * MOMENTS_MAX_TYPES] = {};
    if (a.n > 0)
        {
        if (a.N == 0)
            return refuse("an entry of the row list lies outside the chunks (nothing was computed)");
        rc = reduction_call(who, "conservation sums: ", [&](std::string* err)
                            { return device_pipeline_frame_moments(s->dev, ranges, a, counts, sums, err); });
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    std::copy(counts, counts + 2 * n_types + 1, out_counts);
    std::copy(sums, sums + MOMENTS_QUANTITIES * n_types, out_sums);
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_cell_offsets_device(struct pgsd_handle* handle, const int32_t* cell, uint64_t n, uint32_t n_cells,
                                        uint32_t* out_offsets)
    try
    {
    static const char* who = "pgsd_cell_offsets_device";
    Impl* s = impl_of(handle);
    if (!s || !out_offsets || (n > 0 && !cell))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    if (n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    if (n_cells < 1 || n_cells > CELLS_MAX_CELLS)
        return refuse("a grid holds 1 to 2^20 cells");
    return reduction_call(who, "cell offsets: ", [&](std::string* err)
                          { return device_pipeline_cell_offsets(s->dev, cell, n, n_cells, out_offsets, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_cell_moments_device(struct pgsd_handle* handle, const struct pgsd_index_entry* mass,
                                        const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* energy,
                                        const struct pgsd_index_entry* position, const double defaults[8], const uint32_t* rows,
                                        const int32_t* cell, uint64_t n, uint32_t n_cells, uint64_t* out_counts,
                                        double* out_sums)
    try
    {
    static const char* who = "pgsd_cell_moments_device";
    Impl* s = impl_of(handle);
    if (!s || !defaults || !out_counts || !out_sums || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    const struct pgsd_index_entry* given[MOMENTS_CHUNKS] = {nullptr, mass, velocity, energy, position};
    CellMomentsArgs a;
    memset(&a, 0, sizeof(a));
    ChunkRange ranges[MOMENTS_CHUNKS];
    memset(ranges, 0, sizeof(ranges));
    std::string why;
    int rc = grouped_chunks(s, handle, g_moments_slots, "float", given, &a, ranges, &why);
    if (rc != PGSD_SUCCESS)
        return why.empty() ? rc : refuse(why);
    if (n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    if (n_cells < 1 || n_cells > CELLS_MAX_CELLS)
        return refuse("a grid holds 1 to 2^20 cells");
    // without a stored chunk nothing bounds the entries of the list (no row is loaded)
    if (!a.present)
        a.N = 1ull << 32;
    std::copy(defaults, defaults + 8, a.defaults);
    a.rows = rows;
    a.cell = cell;
    a.n = n;
    a.n_cells = n_cells;
    a.n_types = 1;
    if (n == 0)
        {
        std::fill(out_counts, out_counts + 2 * (size_t)n_cells + 1, (uint64_t)0);
        std::fill(out_sums, out_sums + (size_t)MOMENTS_QUANTITIES * n_cells, 0.0);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return refuse("an entry of the row list lies outside the chunks (nothing was computed)");
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "cell fields: ", [&](std::string* err)
                          { return device_pipeline_cell_moments(s->dev, ranges, a, out_counts, out_sums, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_neighbours_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                      const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                      const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t bins, const double* edges2,
                                      uint32_t* out_count, double* out_nearest2, uint32_t* out_nearest, uint64_t* out_summary,
                                      double* out_closest2)
    try
    {
    static const char* who = "pgsd_neighbours_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !vectors || !cells || !out_summary || !out_closest2 || (n > 0 && (!rows || !cell))
        || (bins > 0 && !edges2))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    pgsd_index_entry c = *position; // a flush may move the index storage
    NeighboursArgs a;
    memset(&a, 0, sizeof(a));
    int rc = float_chunk(refuse, c, "the position chunk", 3, nullptr, &a.f64);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    if (dimensions != 2 && dimensions != 3)
        return refuse("dimensions is 2 or 3");
    if (!(r > 0.0 && r < HUGE_VAL))
        return refuse("the range must be finite and positive");
    rc = pair_grid(refuse, vectors, r, "range", dimensions, cells, &a.n_cells);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (bins > NEIGHBOURS_MAX_BINS)
        return refuse("the pair histogram holds at most 1024 bins");
    for (uint32_t k = 0; k < bins; k++)
        if (!(edges2[k] <= edges2[k + 1]))
            return refuse("the edges of the pair histogram descend (or are not numbers)");
    long long foff = 0;
    size_t bytes = 0;
    rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    a.N = c.N;
    a.rows = rows;
    a.cell = cell;
    a.n = n;
    std::copy(vectors, vectors + 6, a.vectors);
    a.r = r;
    a.r2 = r * r;
    std::copy(cells, cells + 3, a.cells);
    a.dims = dimensions;
    a.bins = bins;
    if (n == 0)
        {
        neighbours_of_nothing(bins, out_summary, out_closest2);
        return PGSD_SUCCESS;
        }
    if (c.N == 0)
        return refuse("an entry of the row list lies outside the position chunk (nothing was computed)");
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "neighbour census: ", [&](std::string* err)
                          { return device_pipeline_neighbours(s->dev, foff, bytes, a, edges2, out_count, out_nearest2,
                                                              out_nearest, out_summary, out_closest2, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

// What pgsd_neighbour_offsets_device, pgsd_neighbour_list_device and pgsd_components_device share: every refusal of
// pgsd_neighbours_device, with its messages and in its order, the undefined bits of `flags` (`defined`: the bits the
// caller has, `undefined`: what it says of the others), the range of the position chunk and the arguments of the pass.
// PGSD_SUCCESS: `a`, `foff` and `bytes` are set (a.N == 0 is left to the caller: only n > 0 makes it a refusal).
static int neighbour_list_arguments(const char* who, Impl* s, struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                    const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                    const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t flags, NeighbourListArgs& a,
                                    long long* foff, size_t* bytes, uint32_t defined = NLIST_HALF,
                                    const char* undefined = "flags holds undefined bits (bit 0, the half list, is the only one)")
    {
    const Refusal refuse = {who};
    pgsd_index_entry c = *position; // a flush may move the index storage
    memset(&a, 0, sizeof(a));
    int rc = float_chunk(refuse, c, "the position chunk", 3, nullptr, &a.f64);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    if (dimensions != 2 && dimensions != 3)
        return refuse("dimensions is 2 or 3");
    if (!(r > 0.0 && r < HUGE_VAL))
        return refuse("the range must be finite and positive");
    rc = pair_grid(refuse, vectors, r, "range", dimensions, cells, &a.n_cells);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (flags & ~defined)
        return refuse(undefined);
    rc = whole_chunk_range(s, handle, c, foff, bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    a.N = c.N;
    a.rows = rows;
    a.cell = cell;
    a.n = n;
    std::copy(vectors, vectors + 6, a.vectors);
    a.r = r;
    a.r2 = r * r;
    std::copy(cells, cells + 3, a.cells);
    a.dims = dimensions;
    a.half = (flags & NLIST_HALF) ? 1u : 0u;
    return PGSD_SUCCESS;
    }

extern "C" int pgsd_neighbour_offsets_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                             const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                             const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t flags,
                                             uint64_t* out_offsets, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_neighbour_offsets_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !vectors || !cells || !out_offsets || !out_summary || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    NeighbourListArgs a;
    long long foff = 0;
    size_t bytes = 0;
    int rc = neighbour_list_arguments(who, s, handle, position, vectors, r, dimensions, cells, rows, cell, n, flags, a, &foff,
                                      &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n == 0)
        {
        // (out_offsets is device memory: its one word goes down the road too, as a memset on the pipeline's stream)
        rc = ensure_device(s);
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    else if (a.N == 0)
        return refuse("an entry of the row list lies outside the position chunk (nothing was computed)");
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "neighbour list: ", [&](std::string* err)
                          { return device_pipeline_neighbour_offsets(s->dev, foff, bytes, a, out_offsets, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_neighbour_list_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                          const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                          const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t flags,
                                          const uint64_t* offsets, uint64_t capacity, uint32_t* out_neighbours,
                                          double* out_distance2)
    try
    {
    static const char* who = "pgsd_neighbour_list_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !vectors || !cells || !offsets || (capacity > 0 && !out_neighbours)
        || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    NeighbourListArgs a;
    long long foff = 0;
    size_t bytes = 0;
    int rc = neighbour_list_arguments(who, s, handle, position, vectors, r, dimensions, cells, rows, cell, n, flags, a, &foff,
                                      &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n == 0)
        return PGSD_SUCCESS; // no segment to fill
    if (a.N == 0)
        return refuse("an entry of the row list lies outside the position chunk (nothing was computed)");
    return reduction_call(who, "neighbour list: ", [&](std::string* err)
                          { return device_pipeline_neighbour_list(s->dev, foff, bytes, a, offsets, capacity, out_neighbours,
                                                                  out_distance2, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_components_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                      const double vectors[6], double r, uint32_t dimensions, const uint32_t cells[3],
                                      const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t flags, uint32_t* out_label,
                                      uint32_t* out_component, uint32_t* out_sizes, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_components_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !vectors || !cells || !out_summary || (n > 0 && (!rows || !cell || !out_label)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    NeighbourListArgs a;
    long long foff = 0;
    size_t bytes = 0;
    int rc = neighbour_list_arguments(who, s, handle, position, vectors, r, dimensions, cells, rows, cell, n, flags, a, &foff,
                                      &bytes, 0u, "flags holds undefined bits (no bit is defined: flags is 0)");
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n == 0)
        {
        // no entry: nothing to stage, nothing to launch
        std::fill(out_summary, out_summary + COMPONENTS_SUMMARY_WORDS, (uint64_t)0);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return refuse("an entry of the row list lies outside the position chunk (nothing was computed)");
    // (the launcher writes the summary on success only, behind its last check)
    return reduction_call(who, "components: ", [&](std::string* err)
                          { return device_pipeline_components(s->dev, foff, bytes, a, out_label, out_component, out_sizes,
                                                              out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_component_moments_device(struct pgsd_handle* handle, const struct pgsd_index_entry* mass,
                                             const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* energy,
                                             const struct pgsd_index_entry* position, const double defaults[8],
                                             const double vectors[6], uint32_t dimensions, const uint32_t* rows,
                                             const uint32_t* label, const uint32_t* component, uint64_t n, uint64_t components,
                                             uint32_t flags, double* out_sums, double* out_extent, double* out_origin,
                                             uint32_t* out_flags, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_component_moments_device";
    Impl* s = impl_of(handle);
    if (!s || !defaults || !vectors || !out_summary
        || (n > 0 && (!rows || !label || !component || !out_sums || !out_extent || !out_origin || !out_flags)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    // what needs no chunk is refused first
    if (!position)
        return refuse("the position is stored nowhere: a component's origin and extent need the position chunk");
    if (dimensions != 2 && dimensions != 3)
        return refuse("dimensions is 2 or 3");
    for (int i = 0; i < 6; i++)
        if (!std::isfinite(vectors[i]))
            return refuse("the box vectors are finite");
    if (!(vectors[0] > 0.0) || !(vectors[1] > 0.0) || (dimensions == 3 && !(vectors[2] > 0.0)))
        return refuse("the box lengths are positive");
    if (flags != 0)
        return refuse("flags holds undefined bits (no bit is defined: flags is 0)");
    if (n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    if (components > n || (n > 0 && components == 0))
        return refuse("a list of n entries has 1 to n components (none for n == 0)");
    const struct pgsd_index_entry* given[MOMENTS_CHUNKS] = {nullptr, mass, velocity, energy, position};
    ComponentMomentsArgs a;
    memset(&a, 0, sizeof(a));
    ChunkRange ranges[MOMENTS_CHUNKS];
    memset(ranges, 0, sizeof(ranges));
    std::string why;
    int rc = grouped_chunks(s, handle, g_moments_slots, "float", given, &a, ranges, &why);
    if (rc != PGSD_SUCCESS)
        return why.empty() ? rc : refuse(why);
    if (n == 0)
        {
        // no entry: nothing to stage, nothing to launch
        std::fill(out_summary, out_summary + CMOM_SUMMARY_WORDS, (uint64_t)0);
        return PGSD_SUCCESS;
        }
    if (a.N == 0)
        return refuse("an entry of the row list lies outside the chunks (nothing was computed)");
    std::copy(defaults, defaults + 8, a.defaults);
    std::copy(vectors, vectors + 6, a.vectors);
    a.rows = rows;
    a.label = label;
    a.component = component;
    a.n = n;
    a.components = (uint32_t)components;
    a.dimensions = dimensions;
    a.n_types = 1;
    // (the launcher writes the summary on success only, behind its last check)
    return reduction_call(who, "component fields: ", [&](std::string* err)
                          { return device_pipeline_component_moments(s->dev, ranges, a, out_sums, out_extent, out_origin,
                                                                     out_flags, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

// What pgsd_sph_sums_device, pgsd_sph_gradients_device, pgsd_sph_accelerations_device and pgsd_sph_samples_device (which
// takes the sums' part of it and checks its value chunks, its points and its box itself) share: every refusal of the
// first (and, for the other two, of a velocity chunk; for the last, of a pressure chunk), the ranges of the chunks that
// are stored (position, mass, density, velocity, pressure) and the arguments of the pass -- the support, the grid, r2,
// inv_h, sigma and G, formed once in float64.  PGSD_SUCCESS: `ranges` and `a` are set (what the accelerations add to
// them -- the pressure default, the viscosity and the gravity -- is their entry point's).
static int sph_arguments(const char* who, Impl* s, struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                         const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                         const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* pressure,
                         const double defaults[2], const double vectors[6], double h, uint32_t kernel, uint32_t dimensions,
                         const uint32_t cells[3], const uint32_t* rows, const int32_t* cell, uint64_t n, double surface_below,
                         ChunkRange ranges[5], SphForcesArgs& a)
    {
    const Refusal refuse = {who};
    pgsd_index_entry c = *position; // a flush may move the index storage
    uint32_t f64 = 0, n_cells = 0;
    int rc = float_chunk(refuse, c, "the position chunk", 3, nullptr, &f64);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    if (dimensions != 2 && dimensions != 3)
        return refuse("dimensions is 2 or 3");
    if (!(h > 0.0 && h < HUGE_VAL))
        return refuse("the smoothing length must be finite and positive");
    if (kernel != SPH_WENDLAND_C2 && kernel != SPH_CUBIC_SPLINE)
        return refuse("the kernel is 0 (Wendland C2) or 1 (cubic spline)");
    memset(ranges, 0, 5 * sizeof(ChunkRange));
    a = SphForcesArgs();
    // the column chunks that are stored: ranges[1 + i] and bit 1 + i of `present`
    const struct
        {
        const struct pgsd_index_entry* entry;
        const char* subject;
        uint32_t columns;
        uint32_t* is_f64;
        } columns[4] = {{mass, "the mass chunk", 1, &a.mass_f64},
                        {density, "the density chunk", 1, &a.density_f64},
                        {velocity, "the velocity chunk", 3, &a.velocity_f64},
                        {pressure, "the pressure chunk", 1, &a.pressure_f64}};
    for (int i = 0; i < 4; i++)
        {
        if (!columns[i].entry)
            continue;
        const pgsd_index_entry m = *columns[i].entry;
        rc = float_chunk(refuse, m, columns[i].subject, columns[i].columns, &c.N, columns[i].is_f64);
        if (rc == PGSD_SUCCESS)
            rc = whole_chunk_range(s, handle, m, &ranges[1 + i].file_offset, &ranges[1 + i].bytes);
        if (rc != PGSD_SUCCESS)
            return rc;
        a.present |= 2u << i;
        }
    // the range of the search is the support 2h; the grid is checked as pgsd_neighbours_device checks its own
    const double r = 2.0 * h;
    if (!(r < HUGE_VAL))
        return refuse("the smoothing length must be finite and positive");
    rc = pair_grid(refuse, vectors, r, "support 2h", dimensions, cells, &n_cells);
    if (rc != PGSD_SUCCESS)
        return rc;
    rc = whole_chunk_range(s, handle, c, &ranges[0].file_offset, &ranges[0].bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    a.N = c.N;
    a.rows = rows;
    a.cell = cell;
    a.n = n;
    std::copy(vectors, vectors + 6, a.vectors);
    // host arithmetic in float64, formed once: the GPU receives these and never recomputes them
    const double pi = 3.141592653589793;
    a.r2 = r * r;
    a.inv_h = 1.0 / h;
    if (dimensions == 3)
        a.sigma = kernel == SPH_WENDLAND_C2 ? 21.0 / (16.0 * pi * (h * h * h)) : 1.0 / (pi * (h * h * h));
    else
        a.sigma = kernel == SPH_WENDLAND_C2 ? 7.0 / (4.0 * pi * (h * h)) : 10.0 / (7.0 * pi * (h * h));
    a.mass_default = defaults[0];
    a.density_default = defaults[1];
    a.volume = density || defaults[1] == defaults[1] ? 1u : 0u;
    a.surface = a.volume && surface_below == surface_below ? 1u : 0u;
    a.surface_below = surface_below;
    std::copy(cells, cells + 3, a.cells);
    a.n_cells = n_cells;
    a.dims = dimensions;
    a.f64 = f64;
    a.kernel = kernel;
    a.G = -((a.sigma * a.inv_h) * a.inv_h);
    // (a list of no entry has its result whatever the chunks hold: the entry points return it)
    if (n > 0 && c.N == 0)
        return refuse("an entry of the row list lies outside the chunks (nothing was computed)");
    return PGSD_SUCCESS;
    }

extern "C" int pgsd_sph_sums_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                    const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                                    const double defaults[2], const double vectors[6], double h, uint32_t kernel,
                                    uint32_t dimensions, const uint32_t cells[3], const uint32_t* rows, const int32_t* cell,
                                    uint64_t n, double surface_below, double* out_number, double* out_density,
                                    double* out_shepard, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_sums_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !defaults || !vectors || !cells || !out_summary || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    ChunkRange ranges[5];
    SphForcesArgs g;
    int rc = sph_arguments(who, s, handle, position, mass, density, nullptr, nullptr, defaults, vectors, h, kernel, dimensions,
                           cells, rows, cell, n, surface_below, ranges, g);
    if (rc != PGSD_SUCCESS)
        return rc;
    const SphArgs a = g;
    if (n == 0)
        {
        sph_sums_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "SPH kernel sums: ", [&](std::string* err)
                          { return device_pipeline_sph_sums(s->dev, ranges, a, out_number, out_density, out_shepard, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_smoothing_range_device(struct pgsd_handle* handle, const struct pgsd_index_entry* slength,
                                               double h_default, const uint32_t* rows, uint64_t n, uint64_t N,
                                               uint64_t* out_words)
    try
    {
    static const char* who = "pgsd_sph_smoothing_range_device";
    Impl* s = impl_of(handle);
    if (!s || !out_words)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    if (N >= (1ull << 32))
        return refuse("chunks of 2^32 rows or more have no 32-bit row list");
    if (rows && n >= (1ull << 32))
        return refuse("a list holds fewer than 2^32 entries");
    const uint64_t count = rows ? n : N;
    uint64_t words[4];
    if (!slength || count == 0)
        {
        // no chunk: the default in every row, whatever the list holds -- nothing to read on the device
        if (slength && slength->N != N)
            return refuse("the slength chunk holds N rows");
        sph_range_of_nothing(words);
        words[0] = count;
        if (count > 0)
            {
            if (h_default > 0.0 && h_default < HUGE_VAL)
                {
                memcpy(&words[2], &h_default, sizeof(double));
                memcpy(&words[3], &h_default, sizeof(double));
                }
            else
                words[1] = count;
            }
        std::copy(words, words + 4, out_words);
        return PGSD_SUCCESS;
        }
    pgsd_index_entry c = *slength; // a flush may move the index storage
    uint32_t f64 = 0;
    int rc = float_chunk(refuse, c, "the slength chunk", 1, nullptr, &f64);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (c.N != N)
        return refuse("the slength chunk holds N rows");
    long long foff = 0;
    size_t bytes = 0;
    rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    rc = reduction_call(who, "smoothing range: ", [&](std::string* err)
                        { return device_pipeline_sph_smoothing_range(s->dev, foff, bytes, f64, rows, count, N, words, err); });
    if (rc != PGSD_SUCCESS)
        return rc;
    std::copy(words, words + 4, out_words);
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_adaptive_sums_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                             const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                                             const struct pgsd_index_entry* slength, const double defaults[3],
                                             const double vectors[6], double h_max, uint32_t kernel, uint32_t mode,
                                             uint32_t dimensions, const uint32_t cells[3], const uint32_t* rows,
                                             const int32_t* cell, uint64_t n, double surface_below, uint32_t* out_count,
                                             double* out_number, double* out_density, double* out_shepard, double* out_omega,
                                             uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_adaptive_sums_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !defaults || !vectors || !cells || !out_summary || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    if (!(h_max > 0.0 && h_max < HUGE_VAL))
        return refuse("h_max, the largest listed smoothing length, must be finite and positive");
    if (mode != SPHA_GATHER && mode != SPHA_MEAN)
        return refuse("the mode is 0 (gather) or 1 (mean)");
    ChunkRange ranges[5];
    SphForcesArgs g;
    // (the grid, the box and the chunks: everything pgsd_sph_sums_device refuses for the range 2 h_max)
    int rc = sph_arguments(who, s, handle, position, mass, density, nullptr, nullptr, defaults, vectors, h_max, kernel,
                           dimensions, cells, rows, cell, n, surface_below, ranges, g);
    if (rc != PGSD_SUCCESS)
        return rc;
    SphAdaptiveArgs a = SphAdaptiveArgs();
    static_cast<SphArgs&>(a) = g;
    a.h_default = defaults[2];
    a.h_max = h_max;
    a.mode = mode;
    if (slength)
        {
        const pgsd_index_entry m = *slength;
        rc = float_chunk(refuse, m, "the slength chunk", 1, &a.N, &a.slength_f64);
        if (rc == PGSD_SUCCESS)
            rc = whole_chunk_range(s, handle, m, &ranges[3].file_offset, &ranges[3].bytes);
        if (rc != PGSD_SUCCESS)
            return rc;
        a.present |= 8u;
        }
    if (mode == SPHA_MEAN)
        {
        // the mean mode's constant: sph_sigma(kernel, 1.0, dimensions)
        const double pi = 3.141592653589793;
        if (dimensions == 3)
            a.sigma = kernel == SPH_WENDLAND_C2 ? 21.0 / (16.0 * pi * 1.0) : 1.0 / (pi * 1.0);
        else
            a.sigma = kernel == SPH_WENDLAND_C2 ? 7.0 / (4.0 * pi * 1.0) : 10.0 / (7.0 * pi * 1.0);
        }
    if (n == 0)
        {
        sph_adaptive_sums_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "adaptive SPH sums: ", [&](std::string* err)
                          { return device_pipeline_sph_adaptive(s->dev, ranges, a, out_count, out_number, out_density,
                                                                out_shepard, out_omega, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_gradients_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                         const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                         const struct pgsd_index_entry* density, const double defaults[2],
                                         const double vectors[6], double h, uint32_t kernel, uint32_t dimensions,
                                         const uint32_t cells[3], const uint32_t* rows, const int32_t* cell, uint64_t n,
                                         double* out_density_rate, double* out_divergence, double* out_curl,
                                         double* out_normal, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_gradients_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !defaults || !vectors || !cells || !out_summary || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    ChunkRange ranges[5];
    SphForcesArgs g;
    int rc = sph_arguments(who, s, handle, position, mass, density, velocity, nullptr, defaults, vectors, h, kernel, dimensions,
                           cells, rows, cell, n, NAN, ranges, g);
    if (rc != PGSD_SUCCESS)
        return rc;
    const SphGradientsArgs a = g;
    if (n == 0)
        {
        sph_gradients_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "SPH kernel gradients: ", [&](std::string* err)
                          { return device_pipeline_sph_gradients(s->dev, ranges, a, out_density_rate, out_divergence, out_curl,
                                                                 out_normal, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_tensors_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                       const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                       const struct pgsd_index_entry* density, const double defaults[2],
                                       const double vectors[6], double h, uint32_t kernel, uint32_t dimensions, double det_min,
                                       const uint32_t cells[3], const uint32_t* rows, const int32_t* cell, uint64_t n,
                                       double* out_correction, double* out_determinant, double* out_velocity_gradient,
                                       double* out_shear_rate, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_tensors_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !defaults || !vectors || !cells || !out_summary || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    ChunkRange ranges[5];
    SphForcesArgs g;
    int rc = sph_arguments(who, s, handle, position, mass, density, velocity, nullptr, defaults, vectors, h, kernel, dimensions,
                           cells, rows, cell, n, NAN, ranges, g);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (!(det_min >= 0.0))
        return refuse("det_min must be a number, at least 0");
    SphTensorsArgs a = SphTensorsArgs();
    static_cast<SphGradientsArgs&>(a) = g;
    a.volume = 1u; // (the density default is a number here: there is no "no volume")
    a.det_min = det_min;
    if (n == 0)
        {
        sph_tensors_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "SPH gradient tensors: ", [&](std::string* err)
                          { return device_pipeline_sph_tensors(s->dev, ranges, a, out_correction, out_determinant,
                                                               out_velocity_gradient, out_shear_rate, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_accelerations_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                             const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                             const struct pgsd_index_entry* density, const struct pgsd_index_entry* pressure,
                                             const double defaults[3], const double vectors[6], double h, uint32_t kernel,
                                             uint32_t dimensions, const uint32_t cells[3], double viscosity,
                                             const double gravity[3], const uint32_t* rows, const int32_t* cell, uint64_t n,
                                             double* out_pressure_acc, double* out_viscous_acc, double* out_total,
                                             uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_accelerations_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !defaults || !vectors || !cells || !gravity || !out_summary || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    ChunkRange ranges[5];
    SphForcesArgs a;
    int rc = sph_arguments(who, s, handle, position, mass, density, velocity, pressure, defaults, vectors, h, kernel,
                           dimensions, cells, rows, cell, n, NAN, ranges, a);
    if (rc != PGSD_SUCCESS)
        return rc;
    // (a negative viscosity says "none"; a NaN is neither)
    if (!(viscosity < HUGE_VAL && viscosity > -HUGE_VAL))
        return refuse("the viscosity must be finite (negative: no viscous term)");
    for (int k = 0; k < 3; k++)
        if (!(gravity[k] < HUGE_VAL && gravity[k] > -HUGE_VAL))
            return refuse("the gravity must hold three finite components");
    // host arithmetic in float64, formed once
    a.pressure_default = defaults[2];
    a.viscous = viscosity >= 0.0 ? 1u : 0u;
    a.eta2 = (0.01 * h) * h;
    a.Gv = a.viscous ? a.G * (2.0 * viscosity) : 0.0;
    std::copy(gravity, gravity + 3, a.gravity);
    if (n == 0)
        {
        sph_forces_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "SPH accelerations: ", [&](std::string* err)
                          { return device_pipeline_sph_accelerations(s->dev, ranges, a, out_pressure_acc, out_viscous_acc,
                                                                     out_total, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_samples_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                       const struct pgsd_index_entry* mass, const struct pgsd_index_entry* density,
                                       const struct pgsd_index_entry* const values[4], const uint32_t value_columns[4],
                                       const double value_defaults[4], const double defaults[2], const float box[6],
                                       const double vectors[6], double h, uint32_t kernel, uint32_t dimensions,
                                       const uint32_t cells[3], const uint32_t* rows, const int32_t* cell, uint64_t n,
                                       const double* points, uint64_t K, uint32_t normalise, uint32_t* out_count,
                                       double* out_density, double* out_shepard, double* out_values, uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_samples_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !value_columns || !value_defaults || !defaults || !box || !vectors || !cells || !out_summary
        || (n > 0 && (!rows || !cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    ChunkRange shared[5];
    SphForcesArgs g;
    int rc = sph_arguments(who, s, handle, position, mass, density, nullptr, nullptr, defaults, vectors, h, kernel, dimensions,
                           cells, rows, cell, n, NAN, shared, g);
    if (rc != PGSD_SUCCESS)
        return rc;
    SphSamplesArgs a = SphSamplesArgs();
    static_cast<SphArgs&>(a) = g;
    ChunkRange ranges[SPHS_CHUNKS];
    memset(ranges, 0, sizeof(ranges));
    std::copy(shared, shared + 3, ranges);
    if (K >= (1ull << 32))
        return refuse("a call takes fewer than 2^32 points");
    if (K > 0 && !points)
        return refuse("points is NULL with K > 0");
    // the value slots: the used ones first, 1 to 4 columns each, at most 8 together
    bool unused = false;
    for (int k = 0; k < SPHS_MAX_VALUES; k++)
        {
        const uint32_t width = value_columns[k];
        if (width == 0)
            {
            unused = true;
            continue;
            }
        if (unused)
            return refuse("a used value slot follows an unused one");
        if (width > SPHS_MAX_WIDTH)
            return refuse("a value chunk has 1 to 4 columns");
        a.C += width;
        a.value_columns[k] = width;
        a.value_default[k] = value_defaults[k];
        }
    if (a.C > SPHS_MAX_COLUMNS)
        return refuse("the value chunks have at most 8 columns together");
    const uint64_t N = position->N;
    for (int k = 0; k < SPHS_MAX_VALUES; k++)
        {
        if (a.value_columns[k] == 0)
            continue;
        const struct pgsd_index_entry* entry = values ? values[k] : nullptr;
        if (!entry)
            {
            if (value_defaults[k] != value_defaults[k])
                return refuse("value chunk " + std::to_string(k) + " is stored nowhere and its default is no number");
            continue;
            }
        const pgsd_index_entry m = *entry;
        rc = float_chunk(refuse, m, "value chunk " + std::to_string(k), a.value_columns[k], &N, &a.value_f64[k]);
        if (rc == PGSD_SUCCESS)
            rc = whole_chunk_range(s, handle, m, &ranges[3 + k].file_offset, &ranges[3 + k].bytes);
        if (rc != PGSD_SUCCESS)
            return rc;
        a.present |= 8u << k;
        }
    // the box of the points' cells is the cell order's, and the one the vectors were formed from
    if (!(box[0] > 0.0f && box[1] > 0.0f && (dimensions == 2 || box[2] > 0.0f)))
        return refuse("box lengths must be positive (Lz unless dimensions == 2)");
    const double expect[6] = {(double)box[0], (double)box[1], (double)box[2], (double)box[3] * (double)box[1],
                              (double)box[4] * (double)box[2], (double)box[5] * (double)box[2]};
    for (int k = 0; k < 6; k++)
        if (!(expect[k] == vectors[k]))
            return refuse("the box and the vectors disagree");
    memset(&a.d, 0, sizeof(a.d));
    a.d.dims = dimensions;
    for (int k = 0; k < 3; k++)
        {
        a.d.L[k] = (double)box[k];
        a.d.hi[k] = 1.0;
        }
    a.d.xy = (double)box[3];
    a.d.xz = (double)box[4];
    a.d.yz = (double)box[5];
    a.points = points;
    a.K = K;
    a.normalise = normalise ? 1u : 0u;
    if (K == 0)
        {
        sph_samples_of_nothing(out_summary);
        return PGSD_SUCCESS;
        }
    if (n == 0)
        {
        // (no chunk is staged for a list of no entry, but the points are sampled on the device all the same)
        rc = ensure_device(s);
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "SPH samples: ", [&](std::string* err)
                          { return device_pipeline_sph_samples(s->dev, ranges, a, out_count, out_density, out_shepard,
                                                               out_values, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_sph_body_force_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position,
                                          const struct pgsd_index_entry* velocity, const struct pgsd_index_entry* mass,
                                          const struct pgsd_index_entry* density, const struct pgsd_index_entry* pressure,
                                          const double defaults[3], const double vectors[6], double h, uint32_t kernel,
                                          uint32_t dimensions, const uint32_t cells[3], double viscosity, const double about[3],
                                          const uint32_t* body_rows, const int32_t* body_cell, uint64_t n_body,
                                          const uint32_t* fluid_rows, const int32_t* fluid_cell, uint64_t n_fluid,
                                          uint32_t* out_contacts, double* out_pressure_acc, double* out_viscous_acc,
                                          uint64_t* out_summary)
    try
    {
    static const char* who = "pgsd_sph_body_force_device";
    Impl* s = impl_of(handle);
    if (!s || !position || !defaults || !vectors || !cells || !about || !out_summary || (n_body > 0 && (!body_rows || !body_cell))
        || (n_fluid > 0 && (!fluid_rows || !fluid_cell)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    ChunkRange ranges[5];
    SphForcesArgs g;
    // (the chunks are checked against the longer list: a list of entries into chunks of no row is refused for either)
    const bool body_longer = n_body >= n_fluid;
    int rc = sph_arguments(who, s, handle, position, mass, density, velocity, pressure, defaults, vectors, h, kernel, dimensions,
                           cells, body_longer ? body_rows : fluid_rows, body_longer ? body_cell : fluid_cell,
                           body_longer ? n_body : n_fluid, NAN, ranges, g);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (!(viscosity < HUGE_VAL && viscosity > -HUGE_VAL))
        return refuse("the viscosity must be finite (negative: no viscous term)");
    for (int k = 0; k < 3; k++)
        if (!(about[k] < HUGE_VAL && about[k] > -HUGE_VAL))
            return refuse("about must hold three finite components");
    SphBodyArgs a = SphBodyArgs();
    static_cast<SphForcesArgs&>(a) = g;
    a.rows = body_rows;
    a.cell = body_cell;
    a.n = n_body;
    a.fluid_rows = fluid_rows;
    a.fluid_cell = fluid_cell;
    a.n_fluid = n_fluid;
    // host arithmetic in float64, formed once
    a.pressure_default = defaults[2];
    a.viscous = viscosity >= 0.0 ? 1u : 0u;
    a.eta2 = (0.01 * h) * h;
    a.Gv = a.viscous ? a.G * (2.0 * viscosity) : 0.0;
    std::fill(a.gravity, a.gravity + 3, 0.0);
    std::copy(about, about + 3, a.about);
    if (n_body == 0)
        {
        sph_body_force_of_nothing(n_fluid, out_summary);
        return PGSD_SUCCESS;
        }
    // (the launcher writes the outputs on success only, behind its last check)
    return reduction_call(who, "SPH body forces: ", [&](std::string* err)
                          { return device_pipeline_sph_body_force(s->dev, ranges, a, out_contacts, out_pressure_acc,
                                                                  out_viscous_acc, out_summary, err); });
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_frame_displacements_device(struct pgsd_handle* handle, const struct pgsd_index_entry* position_a,
                                               const struct pgsd_index_entry* image_a,
                                               const struct pgsd_index_entry* position_b,
                                               const struct pgsd_index_entry* image_b,
                                               const struct pgsd_index_entry* typeid_chunk, const double vectors_a[6],
                                               const double vectors_b[6], uint32_t flags, uint32_t dimensions, uint32_t type0,
                                               uint32_t n_types, const uint32_t* rows, uint64_t n, double* out_rows,
                                               uint64_t* out_counts, double* out_values)
    try
    {
    static const char* who = "pgsd_frame_displacements_device";
    Impl* s = impl_of(handle);
    if (!s || !position_a || !position_b || !vectors_a || !vectors_b || !out_counts || !out_values)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    const struct pgsd_index_entry* given[DISPLACEMENT_CHUNKS] = {position_a, image_a, position_b, image_b, typeid_chunk};
    if (n_types < 1 || n_types > DISPLACEMENT_MAX_TYPES)
        return refuse("a call takes 1 to 4 types");
    if (!typeid_chunk && n_types != 1)
        return refuse("without a typeid chunk there is one group: n_types must be 1");
    if (flags & ~(uint32_t)DISPLACEMENT_MINIMUM_IMAGE)
        return refuse("flags holds the minimum-image bit and nothing else");
    if ((flags & DISPLACEMENT_MINIMUM_IMAGE) && (image_a || image_b))
        return refuse("the minimum image is taken without image chunks");
    if (dimensions != 2 && dimensions != 3)
        return refuse("dimensions is 2 or 3");
    DisplacementArgs a;
    memset(&a, 0, sizeof(a));
    ChunkRange ranges[DISPLACEMENT_CHUNKS];
    memset(ranges, 0, sizeof(ranges));
    std::string why;
    int rc = grouped_chunks(s, handle, g_displacement_slots, "position", given, &a, ranges, &why);
    if (rc != PGSD_SUCCESS)
        return why.empty() ? rc : refuse(why);
    if (rows && n >= (1ull << 32))
        return refuse("a row list holds fewer than 2^32 entries");
    std::copy(vectors_a, vectors_a + 6, a.va);
    std::copy(vectors_b, vectors_b + 6, a.vb);
    a.rows = rows;
    a.n = rows ? n : a.N;
    a.out = out_rows;
    a.type0 = type0;
    a.n_types = n_types;
    a.minimum_image = (flags & DISPLACEMENT_MINIMUM_IMAGE) ? 1u : 0u;
    a.dimensions = dimensions;
    // (the outputs are written on success only: the launcher fills these and they are copied out then)
    uint64_t counts[3 * DISPLACEMENT_MAX_TYPES + 1];
    double values[DISPLACEMENT_VALUES * DISPLACEMENT_MAX_TYPES];
    displacements_of_nothing(n_types, counts, values);
    if (a.n > 0)
        {
        if (a.N == 0)
            return refuse("an entry of the row list lies outside the chunks (nothing was computed)");
        rc = reduction_call(who, "frame displacements: ", [&](std::string* err)
                            { return device_pipeline_frame_displacements(s->dev, ranges, a, counts, values, err); });
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    std::copy(counts, counts + 3 * n_types + 1, out_counts);
    std::copy(values, values + DISPLACEMENT_VALUES * n_types, out_values);
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_select_where_device(struct pgsd_handle* handle, uint32_t n_terms, const struct pgsd_index_entry* term_chunks,
                                        const uint32_t* columns, const uint32_t* kinds, const double* lo, const double* hi,
                                        const uint64_t* sets, const struct pgsd_index_entry* position, const float box[6],
                                        uint32_t dimensions, const double dlo[3], const double dhi[3], uint32_t* out_rows,
                                        uint64_t* out_count)
    try
    {
    static const char* who = "pgsd_select_where_device";
    Impl* s = impl_of(handle);
    if (!s || !out_count || (n_terms > 0 && (!term_chunks || !columns || !kinds || !lo || !hi || !sets))
        || (position && (!box || !dlo || !dhi)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    const Refusal refuse = {who};
    if (n_terms > WHERE_MAX_TERMS)
        return refuse("a predicate has at most 4 terms");
    if (n_terms == 0 && !position)
        return refuse("neither a term nor a domain");
    WhereArgs w;
    memset(&w, 0, sizeof(w));
    w.n_terms = n_terms;
    w.has_domain = position ? 1u : 0u;
    pgsd_index_entry chunks[WHERE_MAX_TERMS + 1]; // copies: a flush may move the index storage
    const uint32_t n_chunks = n_terms + w.has_domain;
    for (uint32_t j = 0; j < n_terms; j++)
        {
        const pgsd_index_entry& c = chunks[j] = term_chunks[j];
        const bool integer = c.type == PGSD_TYPE_UINT32 || c.type == PGSD_TYPE_INT32;
        if (!integer && c.type != PGSD_TYPE_FLOAT && c.type != PGSD_TYPE_DOUBLE)
            return refuse("a term's chunk holds uint32, int32, float32 or float64 elements");
        if (kinds[j] != WHERE_RANGE && kinds[j] != WHERE_SET)
            return refuse("a term is a range (kind 0) or a set (kind 1)");
        if (kinds[j] == WHERE_SET && !integer)
            return refuse("a set needs a chunk of integers");
        if (columns[j] >= c.M)
            return refuse("column " + std::to_string(columns[j]) + " of a chunk of " + std::to_string(c.M) + " column(s)");
        if (c.N != chunks[0].N)
            return refuse("the terms' chunks differ in N");
        w.t[j].type = c.type;
        w.t[j].M = c.M;
        w.t[j].column = columns[j];
        w.t[j].kind = kinds[j];
        w.t[j].lo = lo[j];
        w.t[j].hi = hi[j];
        w.t[j].set = sets[j];
        }
    if (position)
        {
        chunks[n_terms] = *position;
        int rc = domain_args(who, chunks[n_terms], box, dimensions, dlo, dhi, &w.d);
        if (rc != PGSD_SUCCESS)
            return rc;
        if (chunks[n_terms].N != chunks[0].N)
            return refuse("the position chunk and the terms' chunks differ in N");
        }
    w.N = chunks[0].N;
    ChunkRange ranges[WHERE_MAX_TERMS + 1];
    for (uint32_t j = 0; j < n_chunks; j++)
        {
        int rc = whole_chunk_range(s, handle, chunks[j], &ranges[j].file_offset, &ranges[j].bytes);
        if (rc != PGSD_SUCCESS)
            return rc;
        }
    *out_count = 0;
    if (w.N == 0)
        return PGSD_SUCCESS;
    if (!out_rows)
        return PGSD_ERROR_INVALID_ARGUMENT;
    std::string err;
    int rc = device_pipeline_select_where(s->dev, ranges, w, out_rows, out_count, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_read_rows_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk, const uint32_t* rows,
                                     uint64_t n, const struct pgsd_field_dst* dst)
    try
    {
    Impl* s = impl_of(handle);
    if (!s || !chunk || !dst || dst->order)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (n == 0)
        return PGSD_SUCCESS; // (an empty destination may have no address)
    if (!dst->dst)
        return PGSD_ERROR_INVALID_ARGUMENT;
    pgsd_index_entry c = *chunk; // a flush may move the index storage
    long long foff = 0;
    size_t bytes = 0;
    int rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (!rows || n > c.N)
        return PGSD_ERROR_INVALID_ARGUMENT;
    pgsd_unpack_job job;
    memset(&job, 0, sizeof(job));
    job.src_type = c.type;
    job.M = c.M;
    job.dst = *dst;
    std::string err;
    rc = device_pipeline_read_rows(s->dev, foff, bytes, job, c.N, rows, n, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

struct pgsd_row_plan
    {
    pgsd_amd::RowPlan p;
    };

extern "C" int pgsd_row_plan_create(struct pgsd_handle* handle, const uint32_t* rows, uint64_t n, uint64_t N, uint32_t* rows2,
                                    struct pgsd_row_plan** out)
    try
    {
    Impl* s = impl_of(handle);
    if (!s || !out || (n > 0 && (!rows || !rows2)))
        return PGSD_ERROR_INVALID_ARGUMENT;
    *out = nullptr;
    int rc = ensure_device(s);
    if (rc != PGSD_SUCCESS)
        return rc;
    std::unique_ptr<pgsd_row_plan> plan(new pgsd_row_plan);
    plan->p.n = n;
    plan->p.N = N;
    plan->p.rows = rows;
    plan->p.rows2 = rows2;
    std::string err;
    rc = device_pipeline_plan_rows(s->dev, plan->p, &err);
    if (rc != PGSD_SUCCESS)
        {
        set_last_error(err);
        return rc;
        }
    *out = plan.release();
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" void pgsd_row_plan_destroy(struct pgsd_row_plan* plan)
    {
    delete plan;
    }

extern "C" int pgsd_row_plan_query(const struct pgsd_row_plan* plan, uint64_t counts[6], const uint32_t* lists[5])
    {
    if (!plan || !counts || !lists)
        return PGSD_ERROR_INVALID_ARGUMENT;
    const pgsd_amd::RowPlan& p = plan->p;
    counts[0] = p.n;
    counts[1] = p.N;
    counts[2] = p.R;
    counts[3] = p.blocks.size();
    counts[4] = p.run_first.size();
    counts[5] = p.staged_rows;
    lists[0] = p.rows;
    lists[1] = p.rows2;
    lists[2] = p.blocks.data();
    lists[3] = p.run_first.data();
    lists[4] = p.run_blocks.data();
    return PGSD_SUCCESS;
    }

extern "C" int pgsd_read_rows_planned_device(struct pgsd_handle* handle, const struct pgsd_index_entry* chunk,
                                             const struct pgsd_row_plan* plan, const struct pgsd_field_dst* dst)
    try
    {
    Impl* s = impl_of(handle);
    if (!s || !chunk || !plan || !dst || dst->order)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (chunk->N != plan->p.N)
        {
        set_last_error("pgsd_read_rows_planned_device: the plan was made for chunks of another N");
        return PGSD_ERROR_INVALID_ARGUMENT;
        }
    if (plan->p.n == 0)
        return PGSD_SUCCESS; // (an empty destination may have no address)
    if (!dst->dst)
        return PGSD_ERROR_INVALID_ARGUMENT;
    pgsd_index_entry c = *chunk; // a flush may move the index storage
    long long foff = 0;
    size_t bytes = 0;
    int rc = whole_chunk_range(s, handle, c, &foff, &bytes);
    if (rc != PGSD_SUCCESS)
        return rc;
    if (c.N == 0)
        return PGSD_ERROR_INVALID_ARGUMENT; // (rows of an empty chunk: read_rows refuses n > N as well)
    pgsd_unpack_job job;
    memset(&job, 0, sizeof(job));
    job.src_type = c.type;
    job.M = c.M;
    job.dst = *dst;
    std::string err;
    rc = device_pipeline_read_planned(s->dev, foff, (size_t)c.M * sizeof_type(c.type), job, plan->p, &err);
    if (rc != PGSD_SUCCESS)
        set_last_error(err);
    return rc;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_device_read_counters(struct pgsd_handle* handle, uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset)
    {
    Impl* s = impl_of(handle);
    if (!s)
        return PGSD_ERROR_INVALID_ARGUMENT;
    if (pread_bytes)
        *pread_bytes = 0;
    if (h2d_bytes)
        *h2d_bytes = 0;
    if (s->dev)
        device_pipeline_read_counters(s->dev, pread_bytes, h2d_bytes, reset);
    return PGSD_SUCCESS;
    }
