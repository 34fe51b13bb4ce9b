// pgsd_device_write.cpp -- the write side of the device pipeline (described at the head of pgsd_device.cpp): pack into
// staging, dispatcher thread, pinned ring, writers, the direct road of small frames, drain, compare / copy-staged.
#include "pgsd_device_impl.hpp"

#include <chrono>
#include <cstring>

namespace pgsd_amd
    {
// Pack now, place later.  stage() packs the chunks into the staging arena with one fused launch and
// returns a ticket; commit() tells where chunk `index` of the ticket goes -- a file offset (asynchronous
// copy + pwrite), a host buffer (synchronous copy: small replicated chunks headed for the write
// buffer) or nowhere (both absent) -- and the ticket is closed by its last commit.  Between the two
// calls lies the frame's size exchange between the ranks: the pack kernel does not need file
// offsets, so it runs while the exchange is on its way.
int DevicePipeline::stage(std::vector<DeviceChunk>& chunks, uint64_t N, int* ticket)
    {
    int rc = enter();
    if (rc != PGSD_SUCCESS)
        return rc;
    TraceRange tr("pgsd:stage+pack_launch rows=%llu chunks=%llu", N, chunks.size());
    rc = recycle_staging();
    if (rc != PGSD_SUCCESS)
        return rc;

    std::vector<pgsd_pack_job> jobs;
    uint64_t bytes_in = 0, bytes_out = 0;
    // a small launch packs straight into pinned host memory (see the head of pgsd_device.cpp)
    size_t padded = 0;
    for (auto& c : chunks)
        padded += pad256(chunk_bytes(c));
    const bool direct = padded > 0 && padded <= m_direct_max && direct_reserve(padded);
    for (auto& c : chunks)
        {
        const size_t bytes = chunk_bytes(c);
        void* stage = nullptr;
        if (direct)
            {
            stage = m_res.ddev + m_dused;
            m_dused += pad256(bytes);
            }
        else
            {
            rc = arena_alloc(bytes, &stage);
            if (rc != PGSD_SUCCESS)
                return rc;
            }
        c.job.dst = stage;
        jobs.push_back(c.job);
        bytes_in += pack_algorithmic_bytes_in(c.job, c.N);
        bytes_out += bytes;
        }

    rc = order_after_source();
    if (rc != PGSD_SUCCESS)
        return rc;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (m_cfg.profile)
        {
        ev0 = get_event(true, false);
        ev1 = get_event(true, false);
        if (!ev0 || !ev1)
            return PGSD_ERROR_DEVICE;
        }
    std::string err;
    // profiled: the events are stamped by the kernel dispatch itself (begin / end)
    rc = launch_pack((uint32_t)jobs.size(), jobs.data(), N, m_res.pack_stream, &err, ev0, ev1);
    if (rc != PGSD_SUCCESS)
        {
        fail(err);
        return rc;
        }
    if (m_cfg.profile)
        {
        std::lock_guard<std::mutex> g(m_mutex);
        m_pack_events.insert(m_pack_events.end(), {ev0, ev1});
        }
    // the event behind the launch: what the copies of a staged chunk wait for.  A direct launch is waited for
    // with a stream synchronize by whoever writes it (drain, or the writer thread after an asynchronous
    // seal), so it needs none
    hipEvent_t packed = nullptr;
    if (!direct)
        {
        packed = get_event(false);
        if (!packed)
            return PGSD_ERROR_DEVICE;
        HIP_TRY(hipEventRecord(packed, m_res.pack_stream));
        }
    std::lock_guard<std::mutex> g(m_mutex);
    m_stats.pack_launches++;
    m_stats.pack_rows += N;
    m_stats.pack_bytes_in += bytes_in;
    m_stats.pack_bytes_out += bytes_out;
    Staged st;
    st.chunks = chunks;
    st.packed = packed;
    st.open = chunks.size();
    st.ramped = false;
    st.direct = direct;
    *ticket = m_next_ticket++;
    m_staged[*ticket] = st;
    return PGSD_SUCCESS;
    }

// the staged launch of a ticket that holds chunks [.., end), or m_staged.end(); the caller holds m_mutex
std::map<int, DevicePipeline::Staged>::iterator DevicePipeline::find_staged(int ticket, size_t end)
    {
    auto it = m_staged.find(ticket);
    return it != m_staged.end() && end <= it->second.chunks.size() ? it : m_staged.end();
    }

int DevicePipeline::commit(int ticket, size_t index, long long file_offset, void* host_dst)
    {
    DeviceChunk c;
    hipEvent_t packed;
    bool ramp, direct;
        {
        std::lock_guard<std::mutex> g(m_mutex);
        auto it = find_staged(ticket, index + 1);
        if (it == m_staged.end())
            return PGSD_ERROR_INVALID_ARGUMENT;
        c = it->second.chunks[index];
        packed = it->second.packed;
        direct = it->second.direct;
        ramp = !it->second.ramped && !host_dst && file_offset >= 0;
        if (ramp)
            it->second.ramped = true; // the first chunk of a launch starts with small pieces
        if (--it->second.open == 0)
            m_staged.erase(it);
        }
    const size_t bytes = chunk_bytes(c);
    if (bytes == 0 || (!host_dst && file_offset < 0))
        return PGSD_SUCCESS;
    if (failed())
        return PGSD_ERROR_DEVICE;
    if (direct)
        {
        // the kernel is packing (or has packed) these bytes into pinned host memory
        const char* host = m_res.dhost + ((const char*)c.job.dst - m_res.ddev);
        if (host_dst)
            {
            // small replicated chunk headed for the write buffer: wait for the launch, plain memcpy
            HIP_TRY(hipStreamSynchronize(m_res.pack_stream));
            memcpy(host_dst, host, bytes);
            return PGSD_SUCCESS;
            }
        std::lock_guard<std::mutex> g(m_mutex);
        m_direct.push_back({host, bytes, file_offset});
        return PGSD_SUCCESS;
        }
    if (host_dst)
        {
        // small replicated chunk headed for the write buffer: synchronous
        HIP_TRY(hipSetDevice(m_cfg.device));
        HIP_TRY(hipStreamSynchronize(m_res.pack_stream));
        HIP_TRY(hipMemcpy(host_dst, c.job.dst, bytes, hipMemcpyDeviceToHost));
        return PGSD_SUCCESS;
        }
    const CopyJob j = {(const char*)c.job.dst, bytes, file_offset, packed, ramp};
    size_t pieces = 0;
    for (size_t off = 0; off < bytes; off += piece_len(off, bytes, j.ramp))
        pieces++;
    std::unique_lock<std::mutex> lk(m_mutex);
    m_outstanding += pieces;
    m_jobs.push_back(j);
    lk.unlock();
    m_cv_jobs.notify_one();
    return PGSD_SUCCESS;
    }

// stage + commit at once: the caller already knows where the chunks go
int DevicePipeline::submit(std::vector<DeviceChunk>& chunks, uint64_t N)
    {
    int ticket = -1;
    int rc = stage(chunks, N, &ticket);
    for (size_t i = 0; i < chunks.size() && rc == PGSD_SUCCESS; i++)
        rc = commit(ticket, i, chunks[i].host_dst ? -1 : chunks[i].file_offset, chunks[i].host_dst);
    return rc;
    }

// the answer words of compare(): pinned and device-mapped, plus the early-exit words in HBM.  Made by the first
// comparison -- or by init() when the caller asked for everything up front (prealloc_mib)
int DevicePipeline::compare_buffers()
    {
    // (each step on its own: a call that failed half-way is picked up where it stopped by the next one)
    if (!m_cmp_host)
        {
        void* h = nullptr;
        HIP_TRY(hipHostMalloc(&h, CMP_MAX_JOBS * sizeof(uint32_t), hipHostMallocMapped));
        memset(h, 0, CMP_MAX_JOBS * sizeof(uint32_t));
        m_cmp_host = (uint32_t*)h;
        }
    if (!m_cmp_host_dev)
        {
        void* hd = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&hd, m_cmp_host, 0));
        m_cmp_host_dev = (uint32_t*)hd;
        }
    if (!m_cmp_dev)
        {
        void* d = nullptr;
        HIP_TRY(hipMalloc(&d, CMP_MAX_JOBS * sizeof(uint32_t)));
        // on the stream the kernels run on: a null-stream memset is not ordered with a non-blocking stream
        hipError_t me = hipMemsetAsync(d, 0, CMP_MAX_JOBS * sizeof(uint32_t), m_res.pack_stream);
        if (me != hipSuccess)
            {
            (void)hipFree(d);
            fail(std::string("hipMemsetAsync: ") + hipGetErrorString(me));
            return PGSD_ERROR_DEVICE;
            }
        m_cmp_dev = (uint32_t*)d;
        }
    return PGSD_SUCCESS;
    }

// Packed bytes of staged (not yet committed) chunks against reference bytes in device memory: one kernel behind
// the pack on the pack stream, one stream wait, the answers in pinned words the kernel wrote across PCIe.
int DevicePipeline::compare(int ticket, size_t first, size_t count, const void* const* ref, const uint64_t* ref_bytes,
                            uint8_t* equal)
    {
    int rc = enter();
    if (rc != PGSD_SUCCESS)
        return rc;
    std::vector<CompareJob> jobs;
    std::vector<size_t> who;
        {
        std::lock_guard<std::mutex> g(m_mutex);
        auto it = find_staged(ticket, first + count);
        if (it == m_staged.end())
            return PGSD_ERROR_INVALID_ARGUMENT;
        for (size_t i = 0; i < count; i++)
            {
            const DeviceChunk& c = it->second.chunks[first + i];
            const uint64_t bytes = chunk_bytes(c);
            equal[i] = ref[i] != nullptr && bytes == 0 ? 1 : 0; // no rows here: nothing that could differ
            if (ref[i] == nullptr || bytes == 0)
                continue;
            CompareJob j;
            memset(&j, 0, sizeof(j));
            j.a = c.job.dst;
            j.b = ref[i];
            j.bytes = bytes;
            j.mode = c.job.dst_type == PGSD_TYPE_FLOAT ? CMP_F32 : c.job.dst_type == PGSD_TYPE_DOUBLE ? CMP_F64 : CMP_BYTES;
            if (ref_bytes && ref_bytes[i] < bytes)
                {
                // a reference shorter than the chunk repeats: whole 16-byte vectors, whole ROWS (a period that
                // cuts a row would be compared out of phase from the second repetition on), and long enough for
                // the kernel's one-step wrap (256 vectors)
                const uint64_t p = ref_bytes[i];
                if (p < 4096 || p % 16 != 0 || p % ((uint64_t)c.job.M * sizeof_type(c.job.dst_type)) != 0
                    || ((uintptr_t)ref[i] & 15) != 0)
                    {
                    set_last_error("a repeating reference must be 16-byte aligned, at least 4096 bytes and a multiple "
                                   "of 16 bytes and of whole rows");
                    return PGSD_ERROR_INVALID_ARGUMENT;
                    }
                j.period = p;
                }
            jobs.push_back(j);
            who.push_back(i);
            }
        }
    if (jobs.empty())
        return PGSD_SUCCESS;
    TraceRange tr("pgsd:compare chunks=%llu", (unsigned long long)jobs.size(), 0ull);
    // the reference bytes may have been produced on the caller's stream a moment ago
    rc = order_after_source();
    if (rc == PGSD_SUCCESS)
        rc = compare_buffers();
    if (rc != PGSD_SUCCESS)
        return rc;
    for (size_t at = 0; at < jobs.size(); at += CMP_MAX_JOBS)
        {
        const uint32_t n = (uint32_t)std::min<size_t>(CMP_MAX_JOBS, jobs.size() - at);
        // one sequence for the process: a later pipeline may be handed the memory an earlier one marked
        static std::atomic<uint32_t> next_gen {0};
        do
            m_cmp_gen = ++next_gen;
        while (m_cmp_gen == 0);
        std::string err;
        rc = launch_compare(n, jobs.data() + at, m_cmp_gen, m_cmp_dev, m_cmp_host_dev, m_res.pack_stream, &err);
        if (rc != PGSD_SUCCESS)
            {
            fail(err);
            return rc;
            }
        hipError_t e = hipStreamSynchronize(m_res.pack_stream);
        if (e != hipSuccess)
            {
            fail(std::string("hipStreamSynchronize(compare): ") + hipGetErrorString(e));
            return PGSD_ERROR_DEVICE;
            }
        for (uint32_t k = 0; k < n; k++)
            equal[who[at + k]] = __atomic_load_n(&m_cmp_host[k], __ATOMIC_RELAXED) != m_cmp_gen ? 1 : 0;
        }
    return PGSD_SUCCESS;
    }

// Packed bytes of staged chunks into caller-owned device memory (frame 0's rows kept for later comparisons):
// copies on the pack stream behind the pack, asynchronous.
int DevicePipeline::copy_staged(int ticket, size_t first, size_t count, void* const* dst)
    {
    int rc = enter();
    if (rc != PGSD_SUCCESS)
        return rc;
    std::vector<std::pair<const void*, size_t>> src(count);
        {
        std::lock_guard<std::mutex> g(m_mutex);
        auto it = find_staged(ticket, first + count);
        if (it == m_staged.end())
            return PGSD_ERROR_INVALID_ARGUMENT;
        for (size_t i = 0; i < count; i++)
            src[i] = {it->second.chunks[first + i].job.dst, chunk_bytes(it->second.chunks[first + i])};
        }
    // the destinations are the caller's memory (torch's caching allocator hands out blocks that work queued on
    // the caller's stream may still be using): the copies are ordered behind that stream, as stage() orders the
    // pack behind it and compare() the comparison
    rc = order_after_source();
    if (rc != PGSD_SUCCESS)
        return rc;
    for (size_t i = 0; i < count; i++)
        if (dst[i] != nullptr && src[i].second > 0)
            HIP_TRY(hipMemcpyAsync(dst[i], src[i].first, src[i].second, hipMemcpyDefault, m_res.pack_stream));
    return PGSD_SUCCESS;
    }

// Asynchronous seal (pgsd_end_frame_async): nobody will call drain() for this frame, so the direct
// chunks committed so far are handed to the writer thread, which waits for their launch and writes them.
void DevicePipeline::kick_direct()
    {
    std::vector<DirectWrite> list;
        {
        std::lock_guard<std::mutex> g(m_mutex);
        if (m_direct.empty())
            return;
        list.swap(m_direct);
        m_outstanding += 1;
        }
    writer_pool_submit(m_pool,
                       [this, list]
                       {
                           (void)hipSetDevice(m_cfg.device);
                           // everything launched on the pack stream so far, these chunks' kernel included
                           hipError_t e = hipStreamSynchronize(m_res.pack_stream);
                           if (e != hipSuccess)
                               fail(std::string("hipStreamSynchronize(pack): ") + hipGetErrorString(e));
                           else
                               write_direct(list);
                           piece_done(0, 0);
                       });
    }

// host bytes (an asynchronously sealed frame's metadata) written by the writer thread, behind what is queued
void DevicePipeline::write_host(const void* data, size_t bytes, long long file_offset)
    {
    if (bytes == 0)
        return;
    auto copy = std::make_shared<std::vector<char>>((const char*)data, (const char*)data + bytes);
        {
        std::lock_guard<std::mutex> g(m_mutex);
        m_outstanding += 1;
        }
    writer_pool_submit(m_pool,
                       [this, copy, file_offset]
                       {
                           int w = pwrite_locked(m_fd, copy->data(), copy->size(), file_offset, m_shared);
                           if (w != 0)
                               fail(std::string("pwrite: ") + strerror(-w), true, -w);
                           piece_done(0, 0);
                       });
    }

int DevicePipeline::wait_packed()
    {
    if (!m_ok)
        return PGSD_SUCCESS;
    HIP_TRY(hipSetDevice(m_cfg.device));
    HIP_TRY(hipStreamSynchronize(m_res.pack_stream));
    return failed() ? PGSD_ERROR_DEVICE : PGSD_SUCCESS;
    }

// every submitted byte is in the file (or an error is reported); staging is recycled
int DevicePipeline::drain()
    {
    if (!m_ok)
        return PGSD_SUCCESS;
    TraceRange tr("pgsd:drain");
        {
        std::unique_lock<std::mutex> lk(m_mutex);
        m_cv_done.wait(lk, [this] { return m_outstanding == 0 || !m_error.empty(); });
        }
    (void)hipSetDevice(m_cfg.device);
    hipError_t e = hipStreamSynchronize(m_res.pack_stream);
    if (e == hipSuccess && m_copy_used.exchange(false))
        e = hipStreamSynchronize(m_res.copy_stream); // (a frame of direct chunks never touched it)
    if (e != hipSuccess)
        fail(std::string("stream synchronize: ") + hipGetErrorString(e));
    else
        {
        // direct chunks: their launch has finished (pack stream synchronised above), this thread writes them
        std::vector<DirectWrite> list;
            {
            std::lock_guard<std::mutex> g(m_mutex);
            list.swap(m_direct);
            }
        if (!list.empty())
            write_direct(list);
        }
    collect_timings();
    if (!staged_open())
        reset_staging();
    if (!failed())
        return PGSD_SUCCESS;
    // let the writers finish what they hold before the caller tears anything down
    std::unique_lock<std::mutex> lk(m_mutex);
    m_cv_done.wait_for(lk, std::chrono::seconds(30), [this] { return m_outstanding == 0; });
    lk.unlock();
    // the side lane's windows of the file go behind everything queued (a job of the lane: no piece is in flight in it)
    WriterPool* pool = m_pool;
    writer_pool_submit(pool, [pool] { writer_pool_side_drop(pool); });
    return failure_code();
    }

// Bytes of the piece that starts at `off`.  The writer cannot start before the first piece has
// crossed PCIe, so the first chunk of a frame begins with a 1 MiB and a 4 MiB piece (0.02 ms
// instead of 0.3 ms until the first pwrite: 5 % of a 1 M-particle frame) before full slabs follow.
size_t DevicePipeline::piece_len(size_t off, size_t bytes, bool ramp) const
    {
    size_t cap = (size_t)m_cfg.slab_bytes;
    if (ramp && off == 0)
        cap = std::min(cap, (size_t)1 << 20);
    else if (ramp && off < ((size_t)5 << 20))
        cap = std::min(cap, (size_t)4 << 20);
    return std::min(cap, bytes - off);
    }

// A free slab of the write ring, or -1 (the pipeline has failed or is stopping).  While the ring is not full-grown an
// empty free list pins one more slab instead of waiting: only the dispatcher thread -- the caller, pinned to the GPU's
// node -- grows the ring, and the slot exists already (the vector is full-sized), so a small file never pins 256 MiB.
int DevicePipeline::take_slab()
    {
        {
        std::unique_lock<std::mutex> lk(m_mutex);
        if (!(m_free_slabs.empty() && m_slabs_ready < m_cfg.n_slabs && m_error.empty()))
            {
            m_cv_slabs.wait(lk, [this] { return m_stop || !m_free_slabs.empty() || !m_error.empty(); });
            if (m_free_slabs.empty() || !m_error.empty())
                return -1;
            int si = (int)m_free_slabs.front();
            m_free_slabs.pop_front();
            return si;
            }
        }
    hipError_t e = m_res.slabs[m_slabs_ready].alloc(m_cfg.slab_bytes);
    if (e != hipSuccess)
        {
        fail(std::string("hipHostMalloc (pinned slab): ") + hipGetErrorString(e));
        return -1;
        }
    return (int)m_slabs_ready++;
    }

void DevicePipeline::release_slab(int si)
    {
        {
        std::lock_guard<std::mutex> g(m_mutex);
        m_free_slabs.push_back((uint32_t)si);
        }
    m_cv_slabs.notify_all();
    }

// feeds the copy stream: one hipMemcpyAsync per slab-sized piece
void DevicePipeline::dispatch_loop()
    {
    (void)hipSetDevice(m_cfg.device);
    for (;;)
        {
        CopyJob job;
            {
            std::unique_lock<std::mutex> lk(m_mutex);
            m_cv_jobs.wait(lk, [this] { return m_stop || !m_jobs.empty(); });
            if (m_jobs.empty())
                return;
            job = m_jobs.front();
            m_jobs.pop_front();
            }
        bool bad = failed();
        if (!bad && hipStreamWaitEvent(m_res.copy_stream, job.packed, 0) != hipSuccess)
            {
            fail("hipStreamWaitEvent failed");
            bad = true;
            }
        hipEvent_t c0 = nullptr, c1 = nullptr;
        if (!bad && m_cfg.profile)
            {
            c0 = get_event(true, false);
            c1 = get_event(true, false);
            if (c0 && c1)
                (void)hipEventRecord(c0, m_res.copy_stream);
            }
        for (size_t off = 0, n = 0; off < job.bytes; off += n)
            {
            n = piece_len(off, job.bytes, job.ramp);
            // (every piece is accounted for, also those of a job that cannot be copied any more)
            const int si = bad || failed() ? -1 : take_slab();
            if (si < 0)
                {
                bad = true;
                piece_done(0, 0);
                continue;
                }
            const long long foff = job.file_offset + (long long)off;
            TraceRange tr("pgsd:d2h_enqueue file_off=%llu bytes=%llu", (unsigned long long)foff, n);
            m_copy_used.store(true);
            hipError_t e = hipMemcpyAsync(m_res.slabs[(size_t)si].host, job.dsrc + off, n, hipMemcpyDeviceToHost, m_res.copy_stream);
            if (e == hipSuccess)
                e = hipEventRecord(m_res.slabs[(size_t)si].copied, m_res.copy_stream);
            if (e != hipSuccess)
                {
                fail(std::string("hipMemcpyAsync D2H: ") + hipGetErrorString(e));
                release_slab(si);
                bad = true;
                piece_done(0, 0);
                continue;
                }
            writer_pool_submit(m_pool, [this, si, n, foff] { write_piece(si, n, foff); });
            }
        if (c0 && c1)
            {
            (void)hipEventRecord(c1, m_res.copy_stream);
            std::lock_guard<std::mutex> g(m_mutex);
            m_copy_events.insert(m_copy_events.end(), {c0, c1});
            }
        }
    }

void DevicePipeline::write_piece(int si, size_t n, long long foff)
    {
    (void)hipSetDevice(m_cfg.device);
    PinnedSlab& s = m_res.slabs[(size_t)si];
    hipError_t e;
        {
        TraceRange tr("pgsd:wait_d2h file_off=%llu bytes=%llu", (unsigned long long)foff, n);
        e = hipEventSynchronize(s.copied);
        }
    double ms = 0;
    if (e != hipSuccess)
        fail(std::string("hipEventSynchronize(copy): ") + hipGetErrorString(e));
    else if (m_warm)
        {
        // the copy has landed: the slab goes down the lane in sub-pieces, warmed outside the turn, written inside it
        TraceRange tr("pgsd:lane file_off=%llu bytes=%llu", (unsigned long long)foff, n);
        int w = writer_pool_pwrite_warm(m_pool, m_fd, s.host, n, foff, m_shared, &ms);
        if (w != 0)
            fail(std::string("pwrite: ") + strerror(-w), true, -w);
        }
    else
        {
        TraceRange tr("pgsd:pwrite file_off=%llu bytes=%llu", (unsigned long long)foff, n);
        auto t0 = std::chrono::steady_clock::now();
        int w = pwrite_locked(m_fd, s.host, n, foff, m_shared);
        ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (w != 0)
            fail(std::string("pwrite: ") + strerror(-w), true, -w);
        }
    release_slab(si);
    piece_done(n, ms);
    }

// pwrite the packed bytes of direct chunks (their launch is known to have finished).  Chunks that follow each
// other in the file -- a rank's share of a one-rank file, or of any chunk list whose rows this rank owns
// alone -- go out in ONE pwritev: a small frame with the full schema is 14-20 chunks of a few KiB, and the
// system call was most of what each of them cost.
void DevicePipeline::write_direct(const std::vector<DirectWrite>& list)
    {
    std::vector<struct iovec> iov;
    for (size_t i = 0; i < list.size();)
        {
        size_t j = i;
        size_t bytes = 0;
        iov.clear();
        while (j < list.size() && list[j].file_offset == list[i].file_offset + (long long)bytes && (j == i || m_coalesce))
            {
            if (list[j].bytes > 0)
                iov.push_back({(void*)list[j].host, list[j].bytes});
            bytes += list[j].bytes;
            j++;
            }
        TraceRange tr("pgsd:pwrite_direct file_off=%llu bytes=%llu", (unsigned long long)list[i].file_offset, bytes);
        auto t0 = std::chrono::steady_clock::now();
        int w = iov.empty() ? 0
                : iov.size() == 1
                    ? pwrite_locked(m_fd, iov[0].iov_base, iov[0].iov_len, list[i].file_offset, m_shared)
                    : pwritev_locked(m_fd, iov.data(), (int)iov.size(), list[i].file_offset, m_shared);
        double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (w != 0)
            {
            fail(std::string("pwrite: ") + strerror(-w), true, -w);
            return;
            }
        std::lock_guard<std::mutex> g(m_mutex);
        m_stats.written_bytes += bytes;
        m_stats.write_ms += ms;
        i = j;
        }
    }

void DevicePipeline::piece_done(size_t n, double write_ms)
    {
    std::lock_guard<std::mutex> g(m_mutex);
    m_stats.d2h_bytes += n;
    m_stats.written_bytes += n;
    m_stats.write_ms += write_ms;
    if (--m_outstanding == 0)
        m_cv_done.notify_all();
    }
    } // namespace pgsd_amd
