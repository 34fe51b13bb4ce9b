// pgsd_device_read.cpp -- the read side of the device pipeline: file -> pinned slab (pread, shared reader threads) ->
// HBM staging (H2D on the copy stream) -> one deferred unpack launch per wait_read(); the direct road of small reads;
// sparse (planned) reads, indexed reads, domain and group selection on top of the same staging.
#include "pgsd_device_impl.hpp"

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>

namespace pgsd_amd
    {
// ---- the reader engine of a device ----
static std::mutex& registry_mutex()
    {
    static std::mutex mu;
    return mu;
    }

static std::vector<ReadEngine*>& registry()
    {
    static std::vector<ReadEngine*> r;
    return r;
    }

int ReadEngine::get_slab()
    {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [this] { return !free_slabs.empty(); });
    int si = (int)free_slabs.front();
    free_slabs.pop_front();
    return si;
    }

void ReadEngine::put_slab(int si)
    {
        {
        std::lock_guard<std::mutex> g(m);
        free_slabs.push_back((uint32_t)si);
        }
    cv.notify_one();
    }

ReadEngine* ReadEngine::acquire(int device, const cpu_set_t* cpus, hipError_t* err)
    {
    std::lock_guard<std::mutex> g(registry_mutex());
    for (ReadEngine* e : registry())
        if (e->device == device)
            {
            e->refs++;
            return e;
            }
    std::unique_ptr<ReadEngine> e(new ReadEngine);
    e->device = device;
    // Reads of the page cache take no exclusive lock and scale with threads; pieces smaller
    // than the write slabs keep all of them busy on one chunk and start the H2D copies
    // earlier (profiles/r01_read_sweep.log: 16 readers x 4 MiB pieces beat 8 x 16 MiB by 20-40 %).
    unsigned n = 16;
    if (const char* v = getenv("PGSD_READERS"))
        n = (unsigned)atoi(v) > 0 ? (unsigned)atoi(v) : n;
    if (const char* v = getenv("PGSD_READ_PIECE_MIB"))
        e->piece = (size_t)(atoi(v) > 0 ? atoi(v) : 4) << 20;
    e->slabs.resize((size_t)n * 2);
    *err = hipSuccess;
    run_on_gpu_node(device, cpus, // first touch on the GPU's node, like the write ring
                    [&]
                    {
                        for (auto& s : e->slabs)
                            {
                            hipError_t rc = s.alloc(e->piece);
                            if (rc != hipSuccess && *err == hipSuccess)
                                *err = rc;
                            }
                    });
    if (*err != hipSuccess)
        {
        for (auto& s : e->slabs)
            s.free();
        return nullptr;
        }
    for (uint32_t i = 0; i < e->slabs.size(); i++)
        e->free_slabs.push_back(i);
    e->pool = writer_pool_create(n, cpus);
    e->refs = 1;
    registry().push_back(e.get());
    return e.release();
    }

void ReadEngine::release(ReadEngine* e)
    {
        {
        std::lock_guard<std::mutex> g(registry_mutex());
        if (--e->refs > 0)
            return;
        auto& r = registry();
        for (size_t i = 0; i < r.size(); i++)
            if (r[i] == e)
                r.erase(r.begin() + (long)i);
        }
    if (e->pool)
        writer_pool_destroy(e->pool); // joins the readers (no pipeline has work queued any more)
    (void)hipSetDevice(e->device);
    for (auto& s : e->slabs)
        s.free();
    delete e;
    }

// ---- requests ----
std::shared_ptr<DevicePipeline::ReadReq> DevicePipeline::make_read_req(const pgsd_unpack_job& job, uint64_t N,
                                                                       const uint32_t* rows, uint64_t src_N, bool stage_only,
                                                                       size_t pieces)
    {
    auto req = std::make_shared<ReadReq>();
    req->job = job;
    req->N = N;
    req->pieces_left = pieces;
    req->rows = rows;
    req->src_N = src_N;
    req->stage_only = stage_only;
    return req;
    }

// A destination array fed by requests of MORE THAN ONE launch (their keys differ), one of which asks for a fill: every
// launch computes its fill from its own chunks, so the one with the fill would store the fill element over the columns
// another launch feeds (whole rows, in the row-per-lane kernel).  Those arrays get ONE fill pass here, ahead of all
// their launches, over the columns none of the pending requests covers and over the largest row count among them; their
// jobs lose fill_rest.  A wait whose arrays each belong to one launch -- every frame read of pgsd.hoomd -- launches
// nothing here and leaves its jobs alone.
void DevicePipeline::fill_across_launches(std::vector<std::shared_ptr<ReadReq>>& pending)
    {
    const auto same_launch = [](const ReadReq& a, const ReadReq& b)
    { return a.N == b.N && a.rows == b.rows && a.src_N == b.src_N; };
    std::vector<bool> seen(pending.size(), false);
    bool ordered = false;
    for (size_t i = 0; i < pending.size() && !failed(); i++)
        {
        if (seen[i])
            continue;
        const pgsd_field_dst& d0 = pending[i]->job.dst;
        const ReadReq* want = nullptr;
        bool several = false, plain = true;
        uint32_t covered = 0;
        uint64_t rows_max = 0;
        for (size_t k = i; k < pending.size(); k++)
            {
            const ReadReq& r = *pending[k];
            if (r.job.dst.dst != d0.dst)
                continue;
            seen[k] = true;
            several = several || !same_launch(r, *pending[i]);
            // (one array seen through different shapes, or scattered: left to the launches, as before)
            plain = plain && r.job.dst.order == nullptr && r.job.dst.dst_stride == d0.dst_stride
                    && r.job.dst.dst_type == d0.dst_type && d0.dst_stride <= 32;
            for (uint32_t c = 0; c < r.job.M && r.job.dst.dst_col0 + c < 32; c++)
                covered |= 1u << (r.job.dst.dst_col0 + c);
            rows_max = std::max(rows_max, r.N);
            if (r.job.dst.fill_rest && !want)
                want = &r;
            }
        if (!several || !plain || !want)
            continue;
        std::string err;
        if (!ordered && order_after_source() != PGSD_SUCCESS) // (the destinations are the caller's: see below)
            return;
        ordered = true;
        // the rows the fill's own list refuses stay as they are, like in its launch
        if (launch_fill_rest(want->job, covered, rows_max, m_res.pack_stream, &err, want->rows, want->src_N, want->N)
            != PGSD_SUCCESS)
            {
            fail(err);
            return;
            }
        for (size_t k = i; k < pending.size(); k++)
            if (pending[k]->job.dst.dst == d0.dst)
                pending[k]->job.dst.fill_rest = 0;
        }
    }

// The request's bytes are staged (or its copies enqueued, all_copied behind them).  The unpack itself is deferred to
// wait_read(): the chunks of a frame then go through ONE launch in which chunks restoring the same array are assembled
// into whole rows.  Reader threads come here in the order their preads finish; launch_pending_unpacks() puts the requests
// back into the order of their submission (ReadReq::seq).
void DevicePipeline::defer_unpack(const std::shared_ptr<ReadReq>& req)
    {
    if (req->stage_only)
        return;
    std::lock_guard<std::mutex> g(m_copy_mutex);
    m_unpack_pending.push_back(req);
    }

// n_spans file ranges into base + their stage_offset, each in one go (EINTR retried); stops at the first one the file
// does not fill -- it is shorter than its index claims.  Returns the bytes read, which are counted.
size_t DevicePipeline::pread_spans(const ReadSpan* spans, size_t n_spans, char* base)
    {
    size_t total = 0;
    for (size_t k = 0; k < n_spans; k++)
        {
        const ReadSpan& sp = spans[k];
        size_t got = 0;
        while (got < sp.bytes)
            {
            ssize_t r = io_pread(m_fd, base + sp.stage_offset + got, sp.bytes - got, sp.file_offset + (long long)got);
            if (r < 0 && errno == EINTR)
                continue;
            if (r <= 0)
                break;
            got += (size_t)r;
            }
        total += got;
        if (got != sp.bytes)
            break;
        }
    m_pread_bytes += total;
    return total;
    }

int DevicePipeline::read_submit(long long file_offset, size_t bytes, pgsd_unpack_job job, uint64_t N, const uint32_t* rows,
                                uint64_t src_N)
    {
    const ReadSpan whole = {file_offset, bytes, 0};
    return read_submit_spans(&whole, 1, bytes, job, N, rows, src_N, false, nullptr);
    }

// `bytes` of staging filled from n_spans file ranges that follow each other in it without gaps (a whole chunk: one
// span at 0; a sparse read: the touched runs)
int DevicePipeline::read_submit_spans(const ReadSpan* spans, size_t n_spans, size_t bytes, pgsd_unpack_job job, uint64_t N,
                                      const uint32_t* rows, uint64_t src_N, bool stage_only, std::shared_ptr<ReadReq>* out)
    {
    int rc = enter();
    if (rc != PGSD_SUCCESS)
        return rc;
    const size_t padded = pad256(bytes);
    if (bytes > 0 && bytes <= m_direct_max && direct_reserve(padded))
        {
        // Small read, the short road (twin of the direct write path): THIS thread preads the rows straight
        // into the pinned, device-mapped arena and the unpack kernel fetches them from there over PCIe --
        // no reader-thread hand-over, no host->device copy, no staging in HBM.  For a frame of a few
        // thousand particles those fixed costs were ten times the read itself.
        char* host = m_res.dhost + m_dused;
        job.src = m_res.ddev + m_dused;
        m_dused += padded;
        TraceRange tr("pgsd:pread_direct file_off=%llu bytes=%llu", (unsigned long long)spans[0].file_offset, bytes);
        if (pread_spans(spans, n_spans, host) != bytes)
            {
            fail("pread returned fewer bytes than the chunk holds", true);
            return PGSD_SUCCESS; // reported by pgsd_device_wait_read, like the threaded path
            }
        auto req = make_read_req(job, N, rows, src_N, stage_only, 0);
        req->seq = m_read_seq++;
        if (out)
            *out = req;
        defer_unpack(req);
        return PGSD_SUCCESS;
        }
    void* stage = nullptr;
    rc = arena_alloc(bytes, &stage);
    if (rc != PGSD_SUCCESS)
        return rc;
    job.src = stage;
    if (!m_reader)
        {
        hipError_t rerr = hipSuccess;
        m_reader = ReadEngine::acquire(m_cfg.device, m_numa ? &m_numa_cpus : nullptr, &rerr);
        if (!m_reader)
            HIP_TRY(rerr);
        }
    const size_t piece = m_reader->piece;
    // The pieces are cut along the STAGING: a piece of a sparse read holds many short runs, each pread into its place in
    // the slab, and goes to HBM in one copy (a piece per run cost 17 us each; 1 000 runs of 48 KB took as long as two
    // thirds of the whole chunk).
    auto req = make_read_req(job, N, rows, src_N, stage_only, (bytes + piece - 1) / piece);
    req->seq = m_read_seq++;
    if (out)
        *out = req;
    if (req->pieces_left == 0)
        {
        // (a sparse read none of whose rows lies in the chunk: nothing to stage, the gather still refuses them)
        defer_unpack(req);
        return PGSD_SUCCESS;
        }
    req->all_copied = get_event(false);
    if (!req->all_copied)
        return PGSD_ERROR_DEVICE;
    std::unique_lock<std::mutex> lk(m_mutex);
    m_reads_outstanding += req->pieces_left; // counted per piece: see read_piece()
    lk.unlock();
    size_t k = 0;
    for (size_t off = 0; off < bytes; off += piece)
        {
        const size_t n = std::min(piece, bytes - off);
        char* dst = (char*)stage + off;
        // the parts of the spans that fall into [off, off + n), placed relative to the piece
        auto parts = std::make_shared<std::vector<ReadSpan>>();
        while (k < n_spans && spans[k].stage_offset + spans[k].bytes <= off)
            k++;
        for (size_t j = k; j < n_spans && spans[j].stage_offset < off + n; j++)
            {
            const size_t a = std::max(spans[j].stage_offset, off);
            const size_t b = std::min(spans[j].stage_offset + spans[j].bytes, off + n);
            if (b > a)
                parts->push_back({spans[j].file_offset + (long long)(a - spans[j].stage_offset), b - a, a - off});
            }
        writer_pool_submit(m_reader->pool, [this, req, dst, n, parts] { read_piece(req, dst, n, parts); });
        }
    return PGSD_SUCCESS;
    }

// Sparse indexed read: the touched runs of the plan are read (same reader threads, pinned ring and piece size) and
// land at slot * R rows of a staging of plan.staged_rows rows; wait_read's deferred launch gathers through rows2.
int DevicePipeline::read_planned_submit(long long chunk_offset, size_t row_bytes, pgsd_unpack_job job, const RowPlan& plan)
    {
    std::vector<ReadSpan> spans(plan.run_first.size());
    uint64_t slot = 0;
    for (size_t i = 0; i < spans.size(); i++)
        {
        const uint64_t row0 = (uint64_t)plan.run_first[i] * plan.R;
        const uint64_t nrows = std::min<uint64_t>((uint64_t)plan.run_blocks[i] * plan.R, plan.N - row0);
        spans[i] = {chunk_offset + (long long)(row0 * row_bytes), (size_t)(nrows * row_bytes),
                    (size_t)(slot * plan.R * row_bytes)};
        slot += plan.run_blocks[i];
        }
    return read_submit_spans(spans.data(), spans.size(), (size_t)(plan.staged_rows * row_bytes), job, plan.n, plan.rows2,
                             plan.staged_rows, false, nullptr);
    }

// Row plan: mark / scan / remap on the pack stream, behind what the caller's stream still does with the row list.
int DevicePipeline::plan_rows(RowPlan& plan, std::string* err)
    {
    int rc = enter();
    if (rc == PGSD_SUCCESS)
        rc = order_after_source();
    if (rc != PGSD_SUCCESS)
        return rc;
    rc = launch_row_plan(plan, m_res.pack_stream, err);
    if (rc == PGSD_ERROR_DEVICE && err)
        fail(*err);
    return rc;
    }

// Indexed read: the whole chunk is staged as for a slab read -- or, when it is a chunk the last selection staged (same
// file range, no wait_read since), taken from that staging without reading the file again -- and wait_read's deferred
// launch gathers rows[0 .. n) of it.
int DevicePipeline::read_rows_submit(long long file_offset, size_t bytes, pgsd_unpack_job job, uint64_t src_N,
                                     const uint32_t* rows, uint64_t n)
    {
    const void* kept = kept_chunk(file_offset, bytes);
    if (!kept)
        return read_submit(file_offset, bytes, job, n, rows, src_N);
    int rc = enter();
    if (rc != PGSD_SUCCESS)
        return rc;
    job.src = kept;
    auto req = make_read_req(job, n, rows, src_N, false, 0); // (the selection synchronised the copies)
    req->seq = m_read_seq++;
    defer_unpack(req);
    return PGSD_SUCCESS;
    }

const void* DevicePipeline::kept_chunk(long long file_offset, size_t bytes) const
    {
    for (const Kept& k : m_kept)
        if (k.file_offset == file_offset && k.bytes == bytes)
            return k.src;
    return nullptr;
    }

// The n whole chunks of a selection (N rows each) into HBM (file -> pinned -> HBM, or the direct road): src[i] receives
// chunk i's staged rows, which the pack stream may read on return.  A chunk that is kept already -- by an earlier
// selection, or because an earlier entry of `ranges` names it -- is not read again; every chunk is kept until the next
// wait_read.
int DevicePipeline::stage_chunks(const ChunkRange* ranges, size_t n, uint64_t N, const void** src)
    {
    std::vector<std::shared_ptr<ReadReq>> reqs;
    const size_t kept_before = m_kept.size();
    int rc = PGSD_SUCCESS;
    for (size_t i = 0; i < n && rc == PGSD_SUCCESS; i++)
        {
        src[i] = kept_chunk(ranges[i].file_offset, ranges[i].bytes);
        if (src[i])
            continue;
        std::shared_ptr<ReadReq> req;
        pgsd_unpack_job job;
        memset(&job, 0, sizeof(job));
        const ReadSpan whole = {ranges[i].file_offset, ranges[i].bytes, 0};
        rc = read_submit_spans(&whole, 1, ranges[i].bytes, job, N, nullptr, 0, true, &req);
        if (rc == PGSD_SUCCESS && req)
            {
            src[i] = req->job.src;
            m_kept.push_back({src[i], ranges[i].file_offset, ranges[i].bytes});
            reqs.push_back(req);
            }
        }
    // (also after a refused submission: the pieces of the chunks before it are on their way)
    std::unique_lock<std::mutex> lk(m_mutex);
    m_cv_done.wait(lk, [this] { return m_reads_outstanding == 0; });
    lk.unlock();
    if (rc == PGSD_SUCCESS && failed())
        rc = failure_code();
    for (size_t i = 0; i < reqs.size() && rc == PGSD_SUCCESS; i++)
        if (reqs[i]->all_copied && hipStreamWaitEvent(m_res.pack_stream, reqs[i]->all_copied, 0) != hipSuccess)
            {
            fail("read pipeline event: hipStreamWaitEvent failed");
            rc = PGSD_ERROR_DEVICE;
            }
    for (size_t i = 0; i < n && rc == PGSD_SUCCESS; i++)
        if (!src[i])
            rc = failure_code();
    if (rc != PGSD_SUCCESS)
        m_kept.resize(kept_before);
    return rc;
    }

// The chunks of a pass that are present (bit i of `present`: ranges[i] is stored, N rows) into HBM through stage_chunks;
// *slots[i] receives chunk i's staged rows, null where the chunk is absent.  Two slots of one file range -- an elided chunk
// that both frames of a displacement read from frame 0, one chunk given as mass and as density -- are staged once and
// share the address: the staging is never handed one range twice.
int DevicePipeline::stage_present(const ChunkRange* ranges, const void** const* slots, size_t n, uint32_t present, uint64_t N)
    {
    if (n > STAGED_MAX_CHUNKS)
        return PGSD_ERROR_INVALID_ARGUMENT;
    ChunkRange stored[STAGED_MAX_CHUNKS] = {};
    const void* src[STAGED_MAX_CHUNKS] = {};
    int at[STAGED_MAX_CHUNKS]; // slot i's place in `stored`; -1: absent
    size_t n_stored = 0;
    for (size_t i = 0; i < n; i++)
        {
        at[i] = -1;
        if (!(present & (1u << i)))
            continue;
        for (size_t j = 0; j < i && at[i] < 0; j++)
            if (at[j] >= 0 && ranges[j].file_offset == ranges[i].file_offset && ranges[j].bytes == ranges[i].bytes)
                at[i] = at[j];
        if (at[i] < 0)
            {
            at[i] = (int)n_stored;
            stored[n_stored++] = ranges[i];
            }
        }
    const int rc = stage_chunks(stored, n_stored, N, src);
    for (size_t i = 0; i < n && rc == PGSD_SUCCESS; i++)
        *slots[i] = at[i] < 0 ? nullptr : src[at[i]];
    return rc;
    }

// One staged launch, the flow of every GPU pass over whole chunks and the body of its device_pipeline_<pass> below:
// enter(); `refused`, what the pass has against its arguments, returned once the pipeline is entered; the chunks that are
// present into HBM (stage_present) -- stage_chunks looks in the kept list first, so a chunk that an earlier selection,
// census, ordering or reduction of this frame staged is not read again, and every chunk stays kept until the next
// wait_read for an indexed read of the same chunk --; where the pass writes or reads memory of the caller's on the device
// (`callers_memory`: a row list, shifts), what the caller's stream still does with that memory comes first;
// `launch(stream, why)` launches on the pack stream, synchronises it and returns a pgsd_error; a PGSD_ERROR_DEVICE fails
// the pipeline with the launcher's message.  The message of a failure, for all nineteen passes: the launcher's own first,
// else the pipeline's, else the thread's last error.
template<class Launch>
int DevicePipeline::staged_launch(const ChunkRange* ranges, const void** const* slots, size_t n, uint32_t present, uint64_t N,
                                  bool callers_memory, std::string* err, Launch launch, int refused)
    {
    std::string why;
    int rc = enter();
    if (rc == PGSD_SUCCESS)
        rc = refused;
    if (rc == PGSD_SUCCESS)
        rc = stage_present(ranges, slots, n, present, N);
    if (rc == PGSD_SUCCESS && callers_memory)
        rc = order_after_source();
    if (rc == PGSD_SUCCESS)
        {
        rc = launch(m_res.pack_stream, &why);
        if (rc == PGSD_ERROR_DEVICE)
            fail(why);
        }
    if (rc != PGSD_SUCCESS && err)
        *err = !why.empty() ? why : !error().empty() ? error() : std::string(last_error());
    return rc;
    }

// a pass over one chunk (N rows, staged into *slot)
template<class Launch>
static int one_chunk_pass(DevicePipeline* p, long long file_offset, size_t bytes, const void** slot, uint64_t N,
                          bool callers_memory, std::string* err, Launch launch)
    {
    const ChunkRange range = {file_offset, bytes};
    return p->staged_launch(&range, &slot, 1, 1u, N, callers_memory, err, launch);
    }

// A grouped reduction over up to five chunks of one N: the stored chunks are staged, the absent ones stay null.
template<class Launch>
static int grouped_pass(DevicePipeline* p, const ChunkRange* ranges, GroupedArgs& g, std::string* err, Launch launch)
    {
    const void** slots[GROUPED_CHUNKS];
    for (int i = 0; i < GROUPED_CHUNKS; i++)
        slots[i] = &g.chunk[i];
    return p->staged_launch(ranges, slots, GROUPED_CHUNKS, g.present, g.N, true, err, launch);
    }

// Domain selection over the position chunk; the row list is the caller's.
int device_pipeline_select_domain(DevicePipeline* p, long long file_offset, size_t bytes, const DomainArgs& args,
                                  uint32_t* out_rows, uint64_t* out_count, std::string* err)
    {
    DomainArgs d = args;
    return one_chunk_pass(p, file_offset, bytes, &d.pos, d.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_select_domain(d, out_rows, out_count, stream, why); });
    }

// Ghost layer selection: the halo kernels in place of the domain's; the lists are the caller's.
int device_pipeline_select_halo(DevicePipeline* p, long long file_offset, size_t bytes, const HaloArgs& args, uint32_t* out_rows,
                                int32_t* out_shift, uint64_t out_counts[2], std::string* err)
    {
    HaloArgs h = args;
    return one_chunk_pass(p, file_offset, bytes, &h.d.pos, h.d.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_select_halo(h, out_rows, out_shift, out_counts, stream, why); });
    }

// Group selection: the chunks of the terms, then the position chunk of the domain, if there is one.
int device_pipeline_select_where(DevicePipeline* p, const ChunkRange* ranges, const WhereArgs& args, uint32_t* out_rows,
                                 uint64_t* out_count, std::string* err)
    {
    WhereArgs w = args;
    const int refused = w.n_terms > WHERE_MAX_TERMS ? PGSD_ERROR_INVALID_ARGUMENT : PGSD_SUCCESS;
    const void** slots[WHERE_MAX_TERMS + 1];
    const uint32_t n_terms = refused ? 0 : w.n_terms;
    for (uint32_t j = 0; j < n_terms; j++)
        slots[j] = &w.t[j].base;
    slots[n_terms] = &w.d.pos;
    const uint32_t n = n_terms + (w.has_domain ? 1 : 0);
    return p->staged_launch(
        ranges, slots, n, (1u << n) - 1, w.N, true, err,
        [&](hipStream_t stream, std::string* why) { return launch_select_where(w, out_rows, out_count, stream, why); }, refused);
    }

// Domain census: one counting pass, the result on the host.  Nothing of the caller's is touched on the device, so there
// is no source stream to order behind.
int device_pipeline_domain_histogram(DevicePipeline* p, long long file_offset, size_t bytes, const DomainArgs& args,
                                     uint32_t bins, uint64_t* out_hist, std::string* err)
    {
    DomainArgs d = args;
    return one_chunk_pass(p, file_offset, bytes, &d.pos, d.N, false, err, [&](hipStream_t stream, std::string* why)
                          { return launch_axis_histograms(d, bins, out_hist, stream, why); });
    }

int device_pipeline_domain_counts(DevicePipeline* p, long long file_offset, size_t bytes, const CellArgs& args,
                                  uint64_t* out_counts, uint64_t* out_nowhere, std::string* err)
    {
    CellArgs c = args;
    return one_chunk_pass(p, file_offset, bytes, &c.d.pos, c.d.N, false, err, [&](hipStream_t stream, std::string* why)
                          { return launch_cell_counts(c, out_counts, out_nowhere, stream, why); });
    }

// Cell order: keys, sort and apply; the lists are the caller's and are written in place.
int device_pipeline_order_rows(DevicePipeline* p, long long file_offset, size_t bytes, const OrderArgs& args, uint32_t* rows,
                               int32_t* shift, int32_t* out_cell, std::string* err)
    {
    OrderArgs o = args;
    return one_chunk_pass(p, file_offset, bytes, &o.d.pos, o.d.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_order_rows(o, rows, shift, out_cell, stream, why); });
    }

// Chunk statistics: the tile and the final kernel; the row list is the caller's.
int device_pipeline_chunk_stats(DevicePipeline* p, long long file_offset, size_t bytes, const StatsArgs& args,
                                uint64_t* out_counts, double* out_values, std::string* err)
    {
    StatsArgs s = args;
    return one_chunk_pass(p, file_offset, bytes, &s.base, s.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_chunk_stats(s, out_counts, out_values, stream, why); });
    }

// Conservation sums and frame displacements; the row list and the displacements' optional output are the caller's.
int device_pipeline_frame_moments(DevicePipeline* p, const ChunkRange* ranges, const MomentsArgs& args, uint64_t* out_counts,
                                  double* out_sums, std::string* err)
    {
    MomentsArgs m = args;
    return grouped_pass(p, ranges, m, err, [&](hipStream_t stream, std::string* why)
                        { return launch_frame_moments(m, out_counts, out_sums, stream, why); });
    }

int device_pipeline_frame_displacements(DevicePipeline* p, const ChunkRange* ranges, const DisplacementArgs& args,
                                        uint64_t* out_counts, double* out_values, std::string* err)
    {
    DisplacementArgs d = args;
    return grouped_pass(p, ranges, d, err, [&](hipStream_t stream, std::string* why)
                        { return launch_frame_displacements(d, out_counts, out_values, stream, why); });
    }

// Cell fields: the lists are the caller's.  The offsets call stages nothing; the sums stage the chunks that are present
// like the conservation sums (the typeid slot stays empty).
int device_pipeline_cell_offsets(DevicePipeline* p, const int32_t* cell, uint64_t n, uint32_t n_cells, uint32_t* out_offsets,
                                 std::string* err)
    {
    return p->staged_launch(nullptr, nullptr, 0, 0u, 0, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_cell_offsets(cell, n, n_cells, out_offsets, stream, why); });
    }

int device_pipeline_cell_moments(DevicePipeline* p, const ChunkRange* ranges, const CellMomentsArgs& args, uint64_t* out_counts,
                                 double* out_sums, std::string* err)
    {
    CellMomentsArgs c = args;
    return grouped_pass(p, ranges, c, err, [&](hipStream_t stream, std::string* why)
                        { return launch_cell_moments(c, out_counts, out_sums, stream, why); });
    }

// Neighbour census: the position chunk the ordering left staged (or staged here); the lists and the per-entry outputs are
// the caller's.
int device_pipeline_neighbours(DevicePipeline* p, long long file_offset, size_t bytes, const NeighboursArgs& args,
                               const double* edges2, uint32_t* out_count, double* out_nearest2, uint32_t* out_nearest,
                               uint64_t* out_summary, double* out_closest2, std::string* err)
    {
    NeighboursArgs a = args;
    return one_chunk_pass(p, file_offset, bytes, &a.pos, a.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_neighbours(a, edges2, out_count, out_nearest2, out_nearest, out_summary, out_closest2,
                                                     stream, why); });
    }

// SPH kernel sums: the position chunk the ordering left staged (or staged here) and the mass and density chunks that are
// present; the lists and the per-entry outputs are the caller's.
int device_pipeline_sph_sums(DevicePipeline* p, const ChunkRange* ranges, const SphArgs& args, double* out_number,
                             double* out_density, double* out_shepard, uint64_t* out_summary, std::string* err)
    {
    SphArgs a = args;
    const void** const slots[3] = {&a.pos, &a.mass, &a.density};
    return p->staged_launch(ranges, slots, 3, a.present | 1u, a.N, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_sph_sums(a, out_number, out_density, out_shepard, out_summary, stream, why); });
    }

// SPH sums with a per-particle smoothing length: the sums' three slots and the slength chunk where one is stored
int device_pipeline_sph_adaptive(DevicePipeline* p, const ChunkRange* ranges, const SphAdaptiveArgs& args, uint32_t* out_count,
                                 double* out_number, double* out_density, double* out_shepard, double* out_omega,
                                 uint64_t* out_summary, std::string* err)
    {
    SphAdaptiveArgs a = args;
    const void** const slots[4] = {&a.pos, &a.mass, &a.density, &a.slength};
    return p->staged_launch(ranges, slots, 4, a.present | 1u, a.N, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_sph_adaptive_sums(a, out_count, out_number, out_density, out_shepard, out_omega,
                                                              out_summary, stream, why); });
    }

// The smoothing range: the slength chunk alone; the row list is the caller's.
int device_pipeline_sph_smoothing_range(DevicePipeline* p, long long file_offset, size_t bytes, uint32_t f64,
                                        const uint32_t* rows, uint64_t n, uint64_t N, uint64_t* out_words, std::string* err)
    {
    const void* slength = nullptr;
    return one_chunk_pass(p, file_offset, bytes, &slength, N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_sph_smoothing_range(slength, f64, rows, n, N, out_words, stream, why); });
    }

// SPH kernel gradients: as the sums, with one more slot: the velocity chunk where one is stored
int device_pipeline_sph_gradients(DevicePipeline* p, const ChunkRange* ranges, const SphGradientsArgs& args, double* out_rate,
                                  double* out_divergence, double* out_curl, double* out_normal, uint64_t* out_summary,
                                  std::string* err)
    {
    SphGradientsArgs a = args;
    const void** const slots[4] = {&a.pos, &a.mass, &a.density, &a.velocity};
    return p->staged_launch(ranges, slots, 4, a.present | 1u, a.N, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_sph_gradients(a, out_rate, out_divergence, out_curl, out_normal, out_summary, stream,
                                                          why); });
    }

// SPH gradient tensors: the gradients' four slots
int device_pipeline_sph_tensors(DevicePipeline* p, const ChunkRange* ranges, const SphTensorsArgs& args, double* out_correction,
                                double* out_determinant, double* out_gradient, double* out_shear, uint64_t* out_summary,
                                std::string* err)
    {
    SphTensorsArgs a = args;
    const void** const slots[4] = {&a.pos, &a.mass, &a.density, &a.velocity};
    return p->staged_launch(ranges, slots, 4, a.present | 1u, a.N, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_sph_tensors(a, out_correction, out_determinant, out_gradient, out_shear, out_summary,
                                                        stream, why); });
    }

// SPH accelerations: as the gradients, with one more slot: the pressure chunk where one is stored
int device_pipeline_sph_accelerations(DevicePipeline* p, const ChunkRange* ranges, const SphForcesArgs& args,
                                      double* out_pressure_acc, double* out_viscous_acc, double* out_total,
                                      uint64_t* out_summary, std::string* err)
    {
    SphForcesArgs a = args;
    const void** const slots[5] = {&a.pos, &a.mass, &a.density, &a.velocity, &a.pressure};
    return p->staged_launch(ranges, slots, 5, a.present | 1u, a.N, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_sph_accelerations(a, out_pressure_acc, out_viscous_acc, out_total, out_summary,
                                                              stream, why); });
    }

// SPH body forces: the accelerations' five slots; both lists read the same staged chunks
int device_pipeline_sph_body_force(DevicePipeline* p, const ChunkRange* ranges, const SphBodyArgs& args, uint32_t* out_contacts,
                                   double* out_pressure_acc, double* out_viscous_acc, uint64_t* out_summary, std::string* err)
    {
    SphBodyArgs a = args;
    const void** const slots[5] = {&a.pos, &a.mass, &a.density, &a.velocity, &a.pressure};
    return p->staged_launch(ranges, slots, 5, a.present | 1u, a.N, true, err, [&](hipStream_t stream, std::string* why)
                            { return launch_sph_body_force(a, out_contacts, out_pressure_acc, out_viscous_acc, out_summary,
                                                           stream, why); });
    }

// SPH samples: the position, mass and density chunks as the sums take them and up to four value chunks where they are
// stored; the lists, the points and the per-point outputs are the caller's.  No entry: nothing to stage, as the cell offsets.
int device_pipeline_sph_samples(DevicePipeline* p, const ChunkRange* ranges, const SphSamplesArgs& args, uint32_t* out_count,
                                double* out_density, double* out_shepard, double* out_values, uint64_t* out_summary,
                                std::string* err)
    {
    SphSamplesArgs a = args;
    const auto launch = [&](hipStream_t stream, std::string* why)
    { return launch_sph_samples(a, out_count, out_density, out_shepard, out_values, out_summary, stream, why); };
    if (a.n == 0)
        return p->staged_launch(nullptr, nullptr, 0, 0u, 0, true, err, launch);
    const void** const slots[SPHS_CHUNKS] = {&a.pos, &a.mass, &a.density, &a.value[0], &a.value[1], &a.value[2], &a.value[3]};
    return p->staged_launch(ranges, slots, SPHS_CHUNKS, a.present | 1u, a.N, true, err, launch);
    }

// Neighbour lists: the census's staging for both calls (the fill finds the chunk the offsets call left staged); the lists,
// the offsets and the segments are the caller's.  No entry: nothing to stage, as the cell offsets.
int device_pipeline_neighbour_offsets(DevicePipeline* p, long long file_offset, size_t bytes, const NeighbourListArgs& args,
                                      uint64_t* out_offsets, uint64_t* out_summary, std::string* err)
    {
    NeighbourListArgs a = args;
    const auto launch = [&](hipStream_t stream, std::string* why)
    { return launch_neighbour_offsets(a, out_offsets, out_summary, stream, why); };
    if (a.n == 0)
        return p->staged_launch(nullptr, nullptr, 0, 0u, 0, true, err, launch);
    return one_chunk_pass(p, file_offset, bytes, &a.pos, a.N, true, err, launch);
    }

int device_pipeline_neighbour_list(DevicePipeline* p, long long file_offset, size_t bytes, const NeighbourListArgs& args,
                                   const uint64_t* offsets, uint64_t capacity, uint32_t* out_neighbours,
                                   double* out_distance2, std::string* err)
    {
    NeighbourListArgs a = args;
    return one_chunk_pass(p, file_offset, bytes, &a.pos, a.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_neighbour_list(a, offsets, capacity, out_neighbours, out_distance2, stream, why); });
    }

// Components: the census's staging; the lists and the per-entry outputs are the caller's (the entry point answers a list
// of no entry itself: nothing comes down here for it).
int device_pipeline_components(DevicePipeline* p, long long file_offset, size_t bytes, const NeighboursArgs& args,
                               uint32_t* out_label, uint32_t* out_component, uint32_t* out_sizes, uint64_t* out_summary,
                               std::string* err)
    {
    NeighboursArgs a = args;
    return one_chunk_pass(p, file_offset, bytes, &a.pos, a.N, true, err, [&](hipStream_t stream, std::string* why)
                          { return launch_components(a, out_label, out_component, out_sizes, out_summary, stream, why); });
    }

// Component fields: the cell fields' staging; the lists and every output array are the caller's.
int device_pipeline_component_moments(DevicePipeline* p, const ChunkRange* ranges, const ComponentMomentsArgs& args,
                                      double* out_sums, double* out_extent, double* out_origin, uint32_t* out_flags,
                                      uint64_t* out_summary, std::string* err)
    {
    ComponentMomentsArgs c = args;
    return grouped_pass(p, ranges, c, err, [&](hipStream_t stream, std::string* why)
                        { return launch_component_moments(c, out_sums, out_extent, out_origin, out_flags, out_summary, stream, why); });
    }

int DevicePipeline::wait_read()
    {
    if (!m_ok)
        return PGSD_SUCCESS;
    std::unique_lock<std::mutex> lk(m_mutex);
    m_cv_done.wait(lk, [this] { return m_reads_outstanding == 0; });
    lk.unlock();
    (void)hipSetDevice(m_cfg.device);
    launch_pending_unpacks();
    hipError_t e = m_copy_used.exchange(false) ? hipStreamSynchronize(m_res.copy_stream) : hipSuccess;
    if (e == hipSuccess)
        e = hipStreamSynchronize(m_res.pack_stream);
    if (e != hipSuccess)
        fail(std::string("stream synchronize: ") + hipGetErrorString(e));
    // an indexed read met a row outside its chunk: nothing was written for it (the pipeline itself is fine)
    const bool bad_rows = m_bad_host && __atomic_exchange_n(m_bad_host, 0u, __ATOMIC_ACQ_REL) != 0;
    m_kept.clear(); // the chunks a selection kept are given up with every wait, recycled or not
    bool writes_idle;
        {
        std::lock_guard<std::mutex> g(m_mutex);
        writes_idle = m_outstanding == 0;
        }
    if (writes_idle && !staged_open() && !direct_pending())
        reset_staging();
    if (failed())
        return failure_code();
    return bad_rows ? PGSD_ERROR_INVALID_ARGUMENT : PGSD_SUCCESS;
    }

// all chunks whose H2D copies are enqueued: one unpack launch per distinct row count, behind the copies
void DevicePipeline::launch_pending_unpacks()
    {
    std::vector<std::shared_ptr<ReadReq>> pending;
        {
        std::lock_guard<std::mutex> g(m_copy_mutex);
        pending.swap(m_unpack_pending);
        }
    // in the order the caller submitted them: "the later chunk wins" where two chunks write the same column, whichever
    // pread finished first; the grouping below is stable, so the order holds within every launch
    std::stable_sort(pending.begin(), pending.end(),
                     [](const std::shared_ptr<ReadReq>& a, const std::shared_ptr<ReadReq>& b) { return a->seq < b->seq; });
    fill_across_launches(pending);
    while (!pending.empty() && !failed())
        {
        const uint64_t N = pending.front()->N;
        const uint32_t* rows = pending.front()->rows;
        const uint64_t src_N = pending.front()->src_N;
        std::vector<pgsd_unpack_job> jobs;
        std::vector<std::shared_ptr<ReadReq>> rest;
        hipError_t e = hipSuccess;
        if (rows && !m_bad_host)
            {
            void* alias = nullptr;
            e = hipHostMalloc((void**)&m_bad_host, sizeof(uint32_t), hipHostMallocMapped);
            if (e == hipSuccess)
                e = hipHostGetDevicePointer(&alias, m_bad_host, 0);
            if (e == hipSuccess)
                {
                *m_bad_host = 0;
                m_bad_dev = (uint32_t*)alias;
                }
            }
        for (auto& r : pending)
            {
            if (r->N != N || r->rows != rows || r->src_N != src_N)
                {
                rest.push_back(r);
                continue;
                }
            jobs.push_back(r->job);
            if (e == hipSuccess && r->all_copied) // (direct reads have no copy to wait for)
                e = hipStreamWaitEvent(m_res.pack_stream, r->all_copied, 0);
            }
        std::string err;
        if (e != hipSuccess)
            fail(std::string("read pipeline event: ") + hipGetErrorString(e));
        // The destinations belong to the caller: whatever its stream still has in flight on them
        // (a caching allocator hands out blocks whose previous owner may not have finished) comes
        // first, exactly as the pack waits for the producers of its sources.
        // (a failure of which is recorded by order_after_source() itself)
        else if (order_after_source() == PGSD_SUCCESS
                 && launch_unpack((uint32_t)jobs.size(), jobs.data(), N, m_res.pack_stream, &err, rows, src_N,
                                  rows ? m_bad_dev : nullptr) != PGSD_SUCCESS)
            fail(err);
        pending.swap(rest);
        }
    }

// one piece of a request's staging: the file ranges `parts`, each at its stage_offset within the piece, make up its
// n bytes
void DevicePipeline::read_piece(std::shared_ptr<ReadReq> req, char* dst, size_t n,
                                std::shared_ptr<std::vector<ReadSpan>> parts)
    {
    (void)hipSetDevice(m_cfg.device);
    ReadEngine* const reader = m_reader; // the engine may outlive this pipeline, not the other way round
    const int si = failed() ? -1 : reader->get_slab();
    bool ok = si >= 0;
    if (ok)
        {
        const long long foff = parts->empty() ? 0 : parts->front().file_offset;
        TraceRange tr("pgsd:pread file_off=%llu bytes=%llu", (unsigned long long)foff, n);
        if (pread_spans(parts->data(), parts->size(), reader->slabs[(size_t)si].host) != n)
            {
            fail("pread returned fewer bytes than the chunk holds", true);
            ok = false;
            }
        }
    bool complete = false;
        {
        std::lock_guard<std::mutex> g(m_copy_mutex);
        if (ok)
            {
            PinnedSlab& s = reader->slabs[(size_t)si];
            m_copy_used.store(true);
            m_h2d_bytes += n;
            hipError_t e = hipMemcpyAsync(dst, s.host, n, hipMemcpyHostToDevice, m_res.copy_stream);
            if (e == hipSuccess)
                e = hipEventRecord(s.copied, m_res.copy_stream);
            if (e != hipSuccess)
                {
                fail(std::string("hipMemcpyAsync H2D: ") + hipGetErrorString(e));
                ok = false;
                }
            }
        if (--req->pieces_left == 0 && !failed())
            {
            // every piece of this chunk has been enqueued on the copy stream before this point
            hipError_t e = hipEventRecord(req->all_copied, m_res.copy_stream);
            if (e != hipSuccess)
                fail(std::string("read pipeline event: ") + hipGetErrorString(e));
            complete = e == hipSuccess;
            }
        }
    if (complete)
        defer_unpack(req);
    if (si >= 0)
        {
        if (ok)
            (void)hipEventSynchronize(reader->slabs[(size_t)si].copied);
        reader->put_slab(si);
        }
    // Last touch of the pipeline by this piece: the destructor (and wait_read) wait for the count
    // of PIECES to reach zero, so no straggler of a finished chunk is left behind.
    read_done();
    }

void DevicePipeline::read_done()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    if (m_reads_outstanding > 0)
        m_reads_outstanding--;
    m_cv_done.notify_all();
    }

void DevicePipeline::read_counters(uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset)
    {
    if (pread_bytes)
        *pread_bytes = reset ? m_pread_bytes.exchange(0) : m_pread_bytes.load();
    if (h2d_bytes)
        *h2d_bytes = reset ? m_h2d_bytes.exchange(0) : m_h2d_bytes.load();
    }
    } // namespace pgsd_amd
