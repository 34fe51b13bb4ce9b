// pgsd_device.cpp -- the HBM -> file pipeline behind pgsd_write_chunk_device().
//
//   pack stream   fused pack kernel(s) write dense chunk bytes into a device staging arena
//                 (one kernel per submit; the arena holds a whole frame: 288 GB of HBM make
//                 a 0.3-1.6 GB snapshot copy cheap, and the simulation only has to wait for
//                 the ~100 us pack, not for the file write)
//   copy stream   waits for the pack event, then streams the staged bytes piece by piece
//                 into a ring of pinned host slabs with hipMemcpyAsync, so the copy of piece
//                 k+1 overlaps the file write of piece k and the pack of the next chunk.
//                 With the HIP runtime PyTorch ships (bench.py, pgsd.hoomd under torch) these copies run as
//                 SHADER BLITS, not on an SDMA engine (a HIP-only process on ROCm 7.2's own runtime shows no
//                 copy kernels: examples/dump_writer.hip): they appear in the kernel trace as
//                 __amd_rocclr_copyBuffer (240 dispatches of ~256 us for 12 frames of 10 M
//                 particles, profiles/r03_kernel_stats_10M.csv) and share the CUs with whatever
//                 the simulation runs.  They are PCIe-bound (50-55 GB/s) and need few CUs:
//                 a queue of HBM-bound kernels runs 0.7 % slower while snapshots drain, an
//                 fp32 GEMM queue 0.25 % (tools/overlap_probe.py, profiles/r04_overlap_probe.jsonl;
//                 bench.py reports it as snapshot_overlap_slowdown_pct) -- which is why no SDMA
//                 route was built
//   writer pool   each piece is pwrite()n at the file offset the reference's
//                 MPI_File_write_at would use (pgsd.c:2225-2229) as soon as its copy event
//                 has fired; the slab then returns to the ring
//
// pgsd_end_frame()/pgsd_flush() call drain(): the frame is in the file when it returns.
//
// Small frames take a shorter road (the "direct" path): when the chunks of one fused launch hold at most
// PGSD_DIRECT_MAX_KIB (default 2048 KiB) the kernel packs them straight into a pinned, device-mapped host
// arena -- the stores cross PCIe themselves -- and the bytes are pwrite()n by the thread that calls drain()
// after ONE stream wait: no HBM staging, no device->host copy, no dispatcher / writer hand-over.  For a snapshot of a
// few thousand particles those fixed costs were several times the frame itself (round 2: 176 us against 67 us
// for the same frame from host arrays).  HIP events come from a pool instead of being created per launch.
//
// This unit: construction and destruction, what a pipeline owns (resource sets and their parking, HBM arenas, the direct
// arena, the event pool, preallocation, recycling of the staging), the error state, and the device_pipeline_* functions
// the rest of the library calls.  The write side is pgsd_device_write.cpp, the read side pgsd_device_read.cpp, the class
// itself pgsd_device_impl.hpp.
#include "pgsd_device_impl.hpp"

#include <cerrno>
#include <cstdlib>
#include <cstring>

namespace pgsd_amd
    {
hipError_t PinnedSlab::alloc(size_t bytes)
    {
    hipError_t e = hipHostMalloc((void**)&host, bytes, hipHostMallocDefault);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(&copied, hipEventDisableTiming);
    if (e != hipSuccess)
        free();
    return e;
    }

void PinnedSlab::free()
    {
    if (copied)
        (void)hipEventDestroy(copied);
    if (host)
        (void)hipHostFree(host);
    host = nullptr, copied = nullptr;
    }

void run_on_gpu_node(int device, const cpu_set_t* cpus, const std::function<void()>& fn)
    {
    std::thread t(
        [&]
        {
            if (cpus)
                (void)pthread_setaffinity_np(pthread_self(), sizeof(cpu_set_t), cpus);
            (void)hipSetDevice(device);
            fn();
        });
    t.join();
    }

void DeviceResources::release()
    {
    if (device >= 0)
        (void)hipSetDevice(device);
    for (auto& s : slabs)
        s.free();
    if (dhost)
        (void)hipHostFree(dhost);
    for (auto& a : arenas)
        (void)hipFree(a.base);
    for (hipEvent_t e : ev_plain)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_timing)
        (void)hipEventDestroy(e);
    if (pack_stream)
        (void)hipStreamDestroy(pack_stream);
    if (copy_stream)
        (void)hipStreamDestroy(copy_stream);
    *this = DeviceResources();
    }

// the parked sets and their lock (heap objects: see "never freed at exit" in pgsd_device_impl.hpp)
static std::mutex& parked_mutex()
    {
    static std::mutex* m = new std::mutex;
    return *m;
    }

static std::vector<DeviceResources>& parked()
    {
    static std::vector<DeviceResources>* v = new std::vector<DeviceResources>;
    return *v;
    }

// pgsd_device_release_parked
int release_parked_sets()
    {
    std::vector<DeviceResources> sets;
        {
        std::lock_guard<std::mutex> g(parked_mutex());
        sets.swap(parked());
        }
    int device = 0;
    const bool have = hipGetDevice(&device) == hipSuccess;
    for (auto& r : sets)
        r.release();
    if (have && !sets.empty())
        (void)hipSetDevice(device);
    return (int)sets.size();
    }

int DevicePipeline::init()
    {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        {
        (void)hipGetLastError();
        fail("no HIP device visible: the device path has no CPU fallback");
        return PGSD_ERROR_NO_DEVICE;
        }
    if (m_cfg.device < 0)
        HIP_TRY(hipGetDevice(&m_cfg.device));
    HIP_TRY(hipSetDevice(m_cfg.device));
    if (m_cfg.slab_bytes == 0)
        m_cfg.slab_bytes = (uint64_t)16 << 20;
    if (m_cfg.n_slabs == 0)
        m_cfg.n_slabs = 16;
    // Buffered writes into ONE file serialise on its inode lock: a second writer thread
    // halves the rate on tmpfs (profiles/r01_io_probe*.log), so one writer is the default.
    if (m_cfg.n_writers == 0)
        m_cfg.n_writers = 1;
    m_direct_max = (size_t)2048 << 10;
    if (const char* v = getenv("PGSD_DIRECT_MAX_KIB"))
        m_direct_max = (size_t)(atoll(v) > 0 ? atoll(v) : 0) << 10;
    if (const char* v = getenv("PGSD_DIRECT_COALESCE")) // 0: one pwrite per chunk (for A/B measurements)
        m_coalesce = atoi(v) != 0;
    if (const char* v = getenv("PGSD_STAGING_CAP_MIB")) // how much HBM asynchronously sealed frames may hold before a call waits
        m_soft_cap = (size_t)(atoll(v) > 0 ? atoll(v) : 6144) << 20;
    m_res.device = m_cfg.device;
    m_res.slab_bytes = m_cfg.slab_bytes;
        {
        // a parked set of this device and slab size is adopted whole
        std::lock_guard<std::mutex> g(parked_mutex());
        auto& v = parked();
        for (size_t i = 0; i < v.size(); i++)
            if (v[i].device == m_res.device && v[i].slab_bytes == m_res.slab_bytes)
                {
                m_res = std::move(v[i]);
                v.erase(v.begin() + (long)i);
                break;
                }
        }
    if (!m_res.pack_stream)
        {
        HIP_TRY(hipStreamCreateWithFlags(&m_res.pack_stream, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&m_res.copy_stream, hipStreamNonBlocking));
        }
    // The pinned slabs, the thread that copies them into the page cache and the pages it
    // allocates there all belong on the NUMA node the GPU hangs off (two-socket hosts: the
    // other node costs ~10 % of the write rate, profiles/r01_numa.log).
    char bdf[32] = {0};
    m_numa = hipDeviceGetPCIBusId(bdf, (int)sizeof(bdf), m_cfg.device) == hipSuccess
             && numa_cpus_of_pci_device(bdf, &m_numa_cpus);
    const cpu_set_t* pin = m_numa ? &m_numa_cpus : nullptr;
    // parked slabs first (already pinned on this device's NUMA node); what the ring cannot take is freed
    for (; m_res.slabs.size() > m_cfg.n_slabs; m_res.slabs.pop_back())
        m_res.slabs.back().free();
    m_slabs_ready = (uint32_t)m_res.slabs.size();
    m_res.slabs.resize(m_cfg.n_slabs);
    // Two slabs now; the dispatcher (pinned to the same node) adds the rest of the ring when a frame actually needs
    // them, so a small file never pins 256 MiB.  prealloc_mib: the whole ring and that much staging now, nothing in the
    // middle of the run
    const uint32_t first_slabs = m_cfg.prealloc_mib ? m_cfg.n_slabs : std::min<uint32_t>(m_cfg.n_slabs, 2);
    if (m_slabs_ready < first_slabs)
        {
        hipError_t alloc_err = hipSuccess;
        run_on_gpu_node(m_cfg.device, pin,
                        [&]
                        {
                            while (alloc_err == hipSuccess && m_slabs_ready < first_slabs)
                                if ((alloc_err = m_res.slabs[m_slabs_ready].alloc(m_cfg.slab_bytes)) == hipSuccess)
                                    m_slabs_ready++;
                        });
        HIP_TRY(alloc_err);
        }
    for (uint32_t i = 0; i < m_slabs_ready; i++)
        m_free_slabs.push_back(i);
    if (m_cfg.prealloc_mib)
        {
        warm_pack_kernels();
        warm_unpack_kernels();
        warm_select_kernels();
        warm_compaction_kernels();
        warm_census_kernels();
        warm_order_kernels();
        warm_cells_kernels();
        warm_neighbours_kernels();
        warm_neighbour_list_kernels();
        warm_components_kernels();
        warm_component_moments_kernels();
        warm_sph_kernels();
        warm_sph_adaptive_kernels();
        warm_sph_gradients_kernels();
        warm_sph_tensors_kernels();
        warm_sph_forces_kernels();
        warm_sph_samples_kernels();
        warm_sph_body_kernels();
        int brc = compare_buffers();
        if (brc != PGSD_SUCCESS)
            return brc;
        }
    size_t staged_cap = 0;
    for (auto& a : m_res.arenas)
        staged_cap += a.cap;
    for (; staged_cap < ((size_t)m_cfg.prealloc_mib << 20); staged_cap += ARENA_BYTES)
        {
        Arena a = {nullptr, ARENA_BYTES, 0};
        HIP_TRY(hipMalloc((void**)&a.base, a.cap));
        m_res.arenas.push_back(a);
        }
    m_pool = writer_pool_create(m_cfg.n_writers, pin);
    // The one ordered lane as a warm-then-write pair (pgsd_io.cpp): PGSD_WRITE_WARM=0 keeps the single thread,
    // PGSD_WRITE_SUBPIECE_KIB (a multiple of 4) sets the sub-piece.  Stays single with several writers, over MPI-IO and
    // where no two cores of `pin` are known to share an L3.
    // 512 KiB: on tmpfs 128-512 KiB are level and 1 MiB and more lose the gain; on the disk-backed page cache 256 KiB
    // loses to the single thread (a turn costs more per call there) and 512 KiB-2 MiB win (profiles/r23_warm_write_subpiece.jsonl)
    size_t sub_kib = 512;
    if (const char* v = getenv("PGSD_WRITE_SUBPIECE_KIB"))
        {
        if (atoll(v) > 0 && atoll(v) % 4 == 0)
            sub_kib = (size_t)atoll(v);
        else
            fprintf(stderr, "pgsd_amd: PGSD_WRITE_SUBPIECE_KIB=%s is no positive multiple of 4: %zu\n", v, sub_kib);
        }
    const char* warm = getenv("PGSD_WRITE_WARM");
    m_warm = (warm ? atoi(warm) != 0 : true) && m_cfg.n_writers == 1 && writer_pool_enable_warm(m_pool, sub_kib << 10, pin);
    // The side lane beside the pair (pgsd_io.cpp): PGSD_WRITE_SIDE threads (0: off; at most 3, which makes five I/O
    // threads per pipeline) insert whole pages of a piece through a shared mapping of the file, PGSD_WRITE_SIDE_BLOCK_KIB
    // at a time, while the pair pwrites the rest.  Only with the pair, on tmpfs, and for a file no other rank writes.
    // 3 threads of 512 KiB: profiles/r28_side_lane_lab.log.  With the side lane on, every thread of the lane gets a core
    // of its own in the pair's L3 group (writer_pool_enable_side).
    long side = 3, side_kib = 512, side_fail = -1;
    if (const char* v = getenv("PGSD_WRITE_SIDE"))
        side = std::min(std::max(atol(v), 0l), 3l);
    if (const char* v = getenv("PGSD_WRITE_SIDE_BLOCK_KIB"))
        {
        if (atol(v) > 0 && atol(v) % 4 == 0)
            side_kib = atol(v);
        else
            fprintf(stderr, "pgsd_amd: PGSD_WRITE_SIDE_BLOCK_KIB=%s is no positive multiple of 4: %ld\n", v, side_kib);
        }
    if (const char* v = getenv("PGSD_WRITE_SIDE_FAIL_AT")) // tests: the populate call of that number reports failure
        side_fail = atol(v);
    if (m_warm && !m_shared && side > 0)
        (void)writer_pool_enable_side(m_pool, m_fd, (unsigned)side, (size_t)side_kib << 10, pin, side_fail);
    m_dispatcher = std::thread([this] { dispatch_loop(); });
    if (pin)
        (void)pthread_setaffinity_np(m_dispatcher.native_handle(), sizeof(cpu_set_t), pin);
    m_ok = true;
    return PGSD_SUCCESS;
    }

DevicePipeline::~DevicePipeline()
    {
    if (m_dispatcher.joinable())
        {
            {
            std::lock_guard<std::mutex> g(m_mutex);
            m_stop = true;
            }
        m_cv_jobs.notify_all();
        m_cv_slabs.notify_all();
        m_dispatcher.join();
        }
    if (m_reader)
        {
            {
            // the readers are shared: wait for this handle's pieces instead of joining them
            std::unique_lock<std::mutex> lk(m_mutex);
            m_cv_done.wait(lk, [this] { return m_reads_outstanding == 0; });
            }
        ReadEngine::release(m_reader);
        }
    if (m_pool)
        writer_pool_destroy(m_pool); // joins the writers
    (void)hipSetDevice(m_cfg.device);
    release_events();
    if (m_cmp_host)
        (void)hipHostFree(m_cmp_host);
    if (m_bad_host)
        (void)hipHostFree(m_bad_host);
    if (m_cmp_dev)
        (void)hipFree(m_cmp_dev);
    if (!park())
        m_res.release();
    }

// Hand streams, pinned memory, HBM arenas and the idle events to the next pipeline on this device (see DeviceResources).
// Only a healthy pipeline of the default slab size, only while fewer than two sets are parked, and only what a default
// pipeline would hold: at most four slabs, four arenas of the default size.
bool DevicePipeline::park()
    {
    const uint64_t default_slab = (uint64_t)16 << 20;
    if (!m_ok || !m_error.empty() || m_cfg.slab_bytes != default_slab || !m_res.pack_stream || !m_res.copy_stream)
        return false;
    if (getenv("PGSD_NO_PARKING"))
        return false;
    if (hipStreamSynchronize(m_res.pack_stream) != hipSuccess || hipStreamSynchronize(m_res.copy_stream) != hipSuccess)
        {
        (void)hipGetLastError();
        return false;
        }
    // room is checked and the set pushed under ONE lock (two pipelines closing at once could both see
    // "one set parked" and leave three)
    std::lock_guard<std::mutex> g(parked_mutex());
    if (parked().size() >= 2)
        return false;
    DeviceResources excess;
    excess.device = m_res.device;
    m_res.slabs.resize(m_slabs_ready); // (the slots the ring never pinned)
    for (; m_res.slabs.size() > 4; m_res.slabs.pop_back())
        excess.slabs.push_back(m_res.slabs.back());
    // up to 1 GiB of staging stays with the set (a run of asynchronously sealed frames grows into it;
    // giving 256 MiB blocks back and asking for them again cost 3-5 ms apiece)
    std::vector<Arena> keep;
    for (auto& a : m_res.arenas)
        (keep.size() < 4 && a.cap == ARENA_BYTES ? keep : excess.arenas).push_back({a.base, a.cap, 0});
    m_res.arenas.swap(keep);
    excess.release();
    parked().push_back(std::move(m_res));
    return true;
    }

// ---- error state ----
void DevicePipeline::fail(const std::string& msg, bool io, int io_errno)
    {
    std::lock_guard<std::mutex> g(m_mutex);
    if (m_error.empty())
        {
        m_error = msg;
        m_io_error = io;
        m_io_errno = io_errno;
        }
    m_cv_done.notify_all();
    m_cv_slabs.notify_all();
    }

bool DevicePipeline::failed()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    return !m_error.empty();
    }

std::string DevicePipeline::error()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    return m_error;
    }

int DevicePipeline::enter()
    {
    if (!m_ok)
        return PGSD_ERROR_NO_DEVICE;
    if (failed())
        return PGSD_ERROR_DEVICE;
    HIP_TRY(hipSetDevice(m_cfg.device));
    return PGSD_SUCCESS;
    }

int DevicePipeline::failure_code()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    if (m_io_error && m_io_errno)
        errno = m_io_errno;
    return m_io_error ? PGSD_ERROR_IO : PGSD_ERROR_DEVICE;
    }

void DevicePipeline::stats(pgsd_device_stats* out, int reset)
    {
    std::lock_guard<std::mutex> g(m_mutex);
    *out = m_stats;
    // the side lane counts for itself, from the pool's first day
    uint64_t side_bytes = 0;
    double side_ms = 0;
    bool side_on = false;
    if (m_pool)
        writer_pool_side_counters(m_pool, &side_bytes, &side_ms, &side_on);
    out->side_bytes = side_bytes - m_side_bytes_base;
    out->side_ms = side_ms - m_side_ms_base;
    out->side_on = side_on ? 1 : 0;
    if (reset)
        {
        memset(&m_stats, 0, sizeof(m_stats));
        m_side_bytes_base = side_bytes;
        m_side_ms_base = side_ms;
        }
    }

bool DevicePipeline::staged_open()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    return !m_staged.empty();
    }

bool DevicePipeline::direct_pending()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    return !m_direct.empty();
    }

// order the pack stream after whatever the caller enqueued on its source stream -- an event there and a wait
// here, unless that stream has nothing in flight (one query instead of two calls: small frames)
int DevicePipeline::order_after_source()
    {
    if (hipStreamQuery(m_source_stream) != hipSuccess)
        {
        (void)hipGetLastError(); // hipErrorNotReady is the answer, not an error
        hipEvent_t ready = get_event(false);
        if (!ready)
            return PGSD_ERROR_DEVICE;
        HIP_TRY(hipEventRecord(ready, m_source_stream));
        HIP_TRY(hipStreamWaitEvent(m_res.pack_stream, ready, 0));
        }
    return PGSD_SUCCESS;
    }

// ---- events ----
// Events are taken from (and returned to) a pool: creating two to four per launch was a measurable part
// of a small frame.  tracked = handed back by release_events() with the other per-frame events.
hipEvent_t DevicePipeline::get_event(bool timing, bool tracked)
    {
    hipEvent_t ev = nullptr;
        {
        std::lock_guard<std::mutex> g(m_mutex);
        auto& pool = timing ? m_res.ev_timing : m_res.ev_plain;
        if (!pool.empty())
            {
            ev = pool.back();
            pool.pop_back();
            }
        }
    if (!ev)
        {
        hipError_t e = timing ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess)
            {
            fail(std::string("hipEventCreate: ") + hipGetErrorString(e));
            return nullptr;
            }
        }
    if (tracked)
        {
        std::lock_guard<std::mutex> g(m_mutex);
        (timing ? m_misc_timing_events : m_misc_events).push_back(ev);
        }
    return ev;
    }

void DevicePipeline::release_events()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    for (auto* list : {&m_pack_events, &m_copy_events, &m_misc_timing_events})
        {
        m_res.ev_timing.insert(m_res.ev_timing.end(), list->begin(), list->end());
        list->clear();
        }
    m_res.ev_plain.insert(m_res.ev_plain.end(), m_misc_events.begin(), m_misc_events.end());
    m_misc_events.clear();
    }

void DevicePipeline::collect_timings()
    {
    std::lock_guard<std::mutex> g(m_mutex);
    float ms = 0;
    for (size_t i = 0; i + 1 < m_pack_events.size(); i += 2)
        if (hipEventElapsedTime(&ms, m_pack_events[i], m_pack_events[i + 1]) == hipSuccess)
            m_stats.pack_ms += ms;
    for (size_t i = 0; i + 1 < m_copy_events.size(); i += 2)
        if (hipEventElapsedTime(&ms, m_copy_events[i], m_copy_events[i + 1]) == hipSuccess)
            m_stats.d2h_ms += ms;
    }

// ---- staging ----
int DevicePipeline::arena_alloc(size_t bytes, void** out)
    {
    const size_t need = std::max(pad256(bytes), (size_t)256);
    for (auto& a : m_res.arenas)
        if (a.cap - a.used >= need)
            {
            *out = a.base + a.used;
            a.used += need;
            return PGSD_SUCCESS;
            }
    Arena a = {nullptr, std::max(need, ARENA_BYTES), need};
    HIP_TRY(hipMalloc((void**)&a.base, a.cap));
    m_res.arenas.push_back(a);
    *out = a.base;
    return PGSD_SUCCESS;
    }

// Room for `bytes` in the pinned, device-mapped arena of the direct path?  The arena is pinned once
// (16 x the threshold, at least 8 MiB: asynchronously sealed frames may pile up in it); when it is full
// the launch simply takes the HBM staging road.
bool DevicePipeline::direct_reserve(size_t bytes)
    {
    if (!m_res.dhost)
        {
        if (m_direct_failed)
            return false;
        const size_t cap = std::max((size_t)8 << 20, m_direct_max * 16);
        void* dev = nullptr;
        if (hipHostMalloc((void**)&m_res.dhost, cap, hipHostMallocMapped) != hipSuccess
            || hipHostGetDevicePointer(&dev, m_res.dhost, 0) != hipSuccess)
            {
            (void)hipGetLastError();
            if (m_res.dhost)
                (void)hipHostFree(m_res.dhost);
            m_res.dhost = nullptr;
            m_direct_failed = true; // no pinned arena: everything goes through HBM staging
            return false;
            }
        m_res.ddev = (char*)dev;
        m_res.dcap = cap;
        }
    return m_res.dcap - m_dused >= bytes;
    }

// Everything staged is given back: the arenas and the direct arena are rewound, the per-frame events return to their
// pools, the chunks a selection kept (they lie in that staging) are forgotten.  The callers -- drain(),
// wait_read(), recycle_staging() -- each know when nothing staged is needed any more.
void DevicePipeline::reset_staging()
    {
    release_events();
    for (auto& a : m_res.arenas)
        a.used = 0;
    m_dused = 0;
    m_kept.clear();
    }

// Staging is recycled when nothing is in flight (cheap, also serves asynchronously sealed
// frames that have drained on their own); if frames are produced faster than the file takes
// them, block once staging exceeds the soft cap instead of growing without bound.
int DevicePipeline::recycle_staging()
    {
    size_t used = m_dused;
    for (auto& a : m_res.arenas)
        used += a.used;
    if (used == 0)
        return PGSD_SUCCESS;
    bool idle;
        {
        std::lock_guard<std::mutex> g(m_mutex);
        if (!m_staged.empty() || !m_direct.empty())
            return PGSD_SUCCESS; // packed chunks still wait for their place in the file
        idle = m_outstanding == 0 && m_reads_outstanding == 0 && m_jobs.empty();
        }
        {
        // ... and so may chunks that were READ: between pgsd_read_chunk_device(wait = false) and
        // pgsd_device_wait_read their bytes sit in the staging (arena or pinned direct arena) until the unpack
        // launch has taken them -- a direct read counts no outstanding piece
        std::lock_guard<std::mutex> g(m_copy_mutex);
        if (!m_unpack_pending.empty())
            return PGSD_SUCCESS;
        }
    if (!idle && used < m_soft_cap)
        return PGSD_SUCCESS;
    if (!idle)
        {
        std::unique_lock<std::mutex> lk(m_mutex);
        m_cv_done.wait(lk, [this] { return (m_outstanding == 0 && m_reads_outstanding == 0) || !m_error.empty(); });
        }
    hipError_t e = hipStreamSynchronize(m_res.copy_stream);
    if (e != hipSuccess)
        {
        fail(std::string("stream synchronize: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    collect_timings();
    reset_staging();
    return failed() ? PGSD_ERROR_DEVICE : PGSD_SUCCESS;
    }

// ---- the interface of pgsd_internal.hpp ----
DevicePipeline* device_pipeline_create(const pgsd_device_config& cfg, int fd, bool shared_file, std::string* err)
    {
    DevicePipeline* p = new DevicePipeline(cfg, fd, shared_file);
    if (p->init() != PGSD_SUCCESS)
        {
        if (err)
            *err = p->error();
        delete p;
        return nullptr;
        }
    return p;
    }

void device_pipeline_destroy(DevicePipeline* p)
    {
    delete p;
    }

int device_pipeline_device(DevicePipeline* p)
    {
    return p ? p->device() : -1;
    }

// the pipeline's message goes with a failure; `or_last`: the launchers leave theirs in the thread's last error
static int report(DevicePipeline* p, int rc, std::string* err, bool or_last = false)
    {
    if (rc != PGSD_SUCCESS && err)
        *err = or_last && p->error().empty() ? std::string(last_error()) : p->error();
    return rc;
    }

int device_pipeline_submit(DevicePipeline* p, std::vector<DeviceChunk>& chunks, uint64_t N, std::string* err)
    {
    return report(p, p->submit(chunks, N), err);
    }

int device_pipeline_stage(DevicePipeline* p, std::vector<DeviceChunk>& chunks, uint64_t N, int* ticket, std::string* err)
    {
    return report(p, p->stage(chunks, N, ticket), err);
    }

int device_pipeline_commit(DevicePipeline* p, int ticket, size_t index, long long file_offset, void* host_dst,
                           std::string* err)
    {
    return report(p, p->commit(ticket, index, file_offset, host_dst), err);
    }

int device_pipeline_compare(DevicePipeline* p, int ticket, size_t first, size_t count, const void* const* ref,
                            const uint64_t* ref_bytes, uint8_t* equal, std::string* err)
    {
    return report(p, p->compare(ticket, first, count, ref, ref_bytes, equal), err);
    }

int device_pipeline_copy_staged(DevicePipeline* p, int ticket, size_t first, size_t count, void* const* dst,
                                std::string* err)
    {
    return report(p, p->copy_staged(ticket, first, count, dst), err);
    }

void device_pipeline_kick(DevicePipeline* p)
    {
    p->kick_direct();
    }

void device_pipeline_write_host(DevicePipeline* p, const void* data, size_t bytes, long long file_offset)
    {
    p->write_host(data, bytes, file_offset);
    }

bool device_pipeline_single_writer(DevicePipeline* p)
    {
    return p->single_writer();
    }

int device_pipeline_wait_packed(DevicePipeline* p, std::string* err)
    {
    return report(p, p->wait_packed(), err);
    }

int device_pipeline_drain(DevicePipeline* p, std::string* err)
    {
    return report(p, p->drain(), err);
    }

int device_pipeline_read(DevicePipeline* p, long long file_offset, size_t bytes, const pgsd_unpack_job& job, uint64_t N,
                         std::string* err)
    {
    return report(p, p->read_submit(file_offset, bytes, job, N), err);
    }

int device_pipeline_wait_read(DevicePipeline* p, std::string* err)
    {
    int rc = p->wait_read();
    if (rc != PGSD_ERROR_INVALID_ARGUMENT)
        return report(p, rc, err);
    if (err)
        *err = "indexed read: a row index lies outside its chunk (nothing was written for it)";
    return rc;
    }

int device_pipeline_read_rows(DevicePipeline* p, long long file_offset, size_t bytes, const pgsd_unpack_job& job,
                              uint64_t src_N, const uint32_t* rows, uint64_t n, std::string* err)
    {
    return report(p, p->read_rows_submit(file_offset, bytes, job, src_N, rows, n), err);
    }

int device_pipeline_plan_rows(DevicePipeline* p, RowPlan& plan, std::string* err)
    {
    std::string local;
    int rc = report(p, p->plan_rows(plan, &local), err, true);
    if (rc != PGSD_SUCCESS && err && !local.empty())
        *err = local; // the launcher's own message comes first
    return rc;
    }

int device_pipeline_read_planned(DevicePipeline* p, long long chunk_offset, size_t row_bytes, const pgsd_unpack_job& job,
                                 const RowPlan& plan, std::string* err)
    {
    return report(p, p->read_planned_submit(chunk_offset, row_bytes, job, plan), err);
    }

void device_pipeline_read_counters(DevicePipeline* p, uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset)
    {
    p->read_counters(pread_bytes, h2d_bytes, reset);
    }

void device_pipeline_set_source_stream(DevicePipeline* p, void* stream)
    {
    p->set_source_stream(stream);
    }

void device_pipeline_stats(DevicePipeline* p, pgsd_device_stats* out, int reset)
    {
    p->stats(out, reset);
    }

    } // namespace pgsd_amd

extern "C" int pgsd_device_release_parked(void)
    try
    {
    return pgsd_amd::release_parked_sets();
    }
catch (...)
    {
        pgsd_amd::abi_guard();
        return 0;
    }
