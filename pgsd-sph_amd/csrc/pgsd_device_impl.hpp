// pgsd_device_impl.hpp -- the device pipeline as its three units see it (the pipeline itself is described at the head of
// pgsd_device.cpp):
//   pgsd_device.cpp        construction, what the pipeline owns (parked sets, arenas, direct arena, events), error state
//   pgsd_device_write.cpp  HBM -> file: stage / commit, dispatcher, writers, drain, compare / copy-staged
//   pgsd_device_read.cpp   file -> HBM: reader engine, spans, row plans, deferred unpack, the staged GPU passes
// Everything else in the library goes through the device_pipeline_* functions of pgsd_internal.hpp.
#ifndef PGSD_DEVICE_IMPL_HPP
#define PGSD_DEVICE_IMPL_HPP

#include "pgsd_internal.hpp"
#include "pgsd_pack.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace pgsd_amd
    {
// (inside a member of DevicePipeline)
#define HIP_TRY(expr)                                                                      \
    do                                                                                     \
        {                                                                                  \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            {                                                                              \
            fail(std::string(#expr) + ": " + hipGetErrorString(e_));                       \
            (void)hipGetLastError(); /* reported; not left for a later launch check to find */ \
            return PGSD_ERROR_DEVICE;                                                      \
            }                                                                              \
        } while (0)

// A pinned host slab and the event behind the copy that fills (read ring) or empties (write ring) it.
struct PinnedSlab
    {
    char* host = nullptr;
    hipEvent_t copied = nullptr;
    hipError_t alloc(size_t bytes); // on the current device; leaves nothing behind when it fails
    void free();
    };

// Runs fn on a thread of its own, bound to `cpus` (the GPU's NUMA node; null: unbound) with `device` set, and joins it:
// first touch decides the node of pinned memory, so it is allocated from a thread that runs there.
void run_on_gpu_node(int device, const cpu_set_t* cpus, const std::function<void()>& fn);

struct Arena // HBM staging
    {
    char* base;
    size_t cap, used;
    };

// What a pipeline needs from the HIP runtime is expensive to make and to give back: two streams (ms each),
// pinned slabs (2-3 ms per 16 MiB hipHostMalloc, more to free), the pinned arena of the direct path, HBM
// arenas, events.  A trajectory writer that opens one file per snapshot (or a benchmark that re-creates its
// file) paid 20-30 ms per open/close for them.  A closed pipeline of the default geometry therefore parks its
// set, at most two per process, and the next pipeline on the same device adopts one.
// Never freed at exit: no HIP calls from static destruction.
struct DeviceResources
    {
    int device = -1;
    uint64_t slab_bytes = 0;
    hipStream_t pack_stream = nullptr, copy_stream = nullptr;
    std::vector<PinnedSlab> slabs;
    char* dhost = nullptr; // direct path: pinned arena the kernels of small launches pack into, its device view, its size
    char* ddev = nullptr;
    size_t dcap = 0;
    std::vector<Arena> arenas;
    std::vector<hipEvent_t> ev_plain, ev_timing; // idle events (timing disabled / enabled)

    void release(); // everything goes back to the runtime; the set is empty afterwards
    };

static constexpr size_t ARENA_BYTES = (size_t)256 << 20; // default size of an HBM staging arena

inline size_t chunk_bytes(const DeviceChunk& c)
    {
    return (size_t)(c.N * c.job.M * sizeof_type(c.job.dst_type));
    }

inline size_t pad256(size_t bytes)
    {
    return (bytes + 255) & ~(size_t)255;
    }

// Reader threads and their pinned ring are shared by every handle that reads on a device: ten
// trajectories open for reading cost 16 threads and 128 MiB of pinned memory, not 160 and 1.3 GiB.
// Created by the first reading pipeline, destroyed with the last (refs and the registry: one lock of the registry's).
struct ReadEngine
    {
    int device = 0;
    int refs = 0;
    size_t piece = (size_t)4 << 20;
    WriterPool* pool = nullptr;
    std::vector<PinnedSlab> slabs;
    std::deque<uint32_t> free_slabs; // guarded by m
    std::mutex m;
    std::condition_variable cv;

    int get_slab(); // blocks until one is free
    void put_slab(int si);
    static ReadEngine* acquire(int device, const cpu_set_t* cpus, hipError_t* err);
    static void release(ReadEngine* e);
    };

class DevicePipeline
    {
    public:
    DevicePipeline(const pgsd_device_config& cfg, int fd, bool shared_file) : m_cfg(cfg), m_fd(fd), m_shared(shared_file) { }
    int init();
    ~DevicePipeline();

    // ---- write side (pgsd_device_write.cpp) ----
    int stage(std::vector<DeviceChunk>& chunks, uint64_t N, int* ticket);
    int commit(int ticket, size_t index, long long file_offset, void* host_dst);
    int submit(std::vector<DeviceChunk>& chunks, uint64_t N);
    int compare(int ticket, size_t first, size_t count, const void* const* ref, const uint64_t* ref_bytes, uint8_t* equal);
    int copy_staged(int ticket, size_t first, size_t count, void* const* dst);
    void kick_direct();
    void write_host(const void* data, size_t bytes, long long file_offset);
    int wait_packed();
    int drain();

    // ---- read side (pgsd_device_read.cpp): file -> pinned slab (pread) -> HBM staging (H2D) -> unpack kernel ----
    // a piece of the file and where it lands in the request's staging
    struct ReadSpan
        {
        long long file_offset;
        size_t bytes;
        size_t stage_offset;
        };
    int read_submit(long long file_offset, size_t bytes, pgsd_unpack_job job, uint64_t N, const uint32_t* rows = nullptr,
                    uint64_t src_N = 0);
    int read_planned_submit(long long chunk_offset, size_t row_bytes, pgsd_unpack_job job, const RowPlan& plan);
    int read_rows_submit(long long file_offset, size_t bytes, pgsd_unpack_job job, uint64_t src_N, const uint32_t* rows,
                         uint64_t n);
    int plan_rows(RowPlan& plan, std::string* err);
    // the one road of a GPU pass over whole staged chunks: the device_pipeline_<pass> functions are defined on it, in
    // pgsd_device_read.cpp
    template<class Launch>
    int staged_launch(const ChunkRange* ranges, const void** const* slots, size_t n, uint32_t present, uint64_t N,
                      bool callers_memory, std::string* err, Launch launch, int refused = PGSD_SUCCESS);
    int wait_read();

    // ---- accessors ----
    int device() const
        {
        return m_cfg.device;
        }
    bool single_writer() const
        {
        return m_cfg.n_writers == 1;
        }
    void set_source_stream(void* stream)
        {
        m_source_stream = (hipStream_t)stream;
        }
    void read_counters(uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset);
    void stats(pgsd_device_stats* out, int reset);
    std::string error();

    private:
    struct ReadReq
        {
        pgsd_unpack_job job;
        uint64_t N;
        size_t pieces_left;              // guarded by m_copy_mutex
        hipEvent_t all_copied = nullptr; // behind the last H2D piece; null: nothing to wait for, the bytes are there
        const uint32_t* rows;            // indexed read: N destination rows gathered from rows[] of the src_N staged ones
        uint64_t src_N;
        bool stage_only;                 // staged for a selection, which waits for the pieces itself: no unpack
        uint64_t seq = 0;                // submission number: the order of the unpacks, whichever pread finishes first
        };
    struct Staged
        {
        std::vector<DeviceChunk> chunks;
        hipEvent_t packed;
        size_t open;
        bool ramped;
        bool direct; // packed into the pinned host arena, written by drain() / kick_direct()
        };
    struct CopyJob
        {
        const char* dsrc;
        size_t bytes;
        long long file_offset;
        hipEvent_t packed;
        bool ramp;
        };
    struct DirectWrite
        {
        const char* host;
        size_t bytes;
        long long file_offset;
        };

    // ---- resources and error state (pgsd_device.cpp) ----
    bool park();
    int enter();        // the opening of every call that needs a healthy pipeline: is it up, has it failed, set the device
    int failure_code(); // the recorded failure as a return code (errno restored for a failed write or read)
    void fail(const std::string& msg, bool io = false, int io_errno = 0);
    bool failed();
    int order_after_source();
    hipEvent_t get_event(bool timing, bool tracked = true);
    void release_events();
    void collect_timings();
    int arena_alloc(size_t bytes, void** out);
    bool direct_reserve(size_t bytes);
    int compare_buffers();
    void reset_staging();
    int recycle_staging();
    bool staged_open();
    bool direct_pending();

    // ---- write side ----
    std::map<int, Staged>::iterator find_staged(int ticket, size_t end);
    size_t piece_len(size_t off, size_t bytes, bool ramp) const;
    void dispatch_loop();
    int take_slab();
    void release_slab(int si);
    void write_piece(int si, size_t n, long long foff);
    void write_direct(const std::vector<DirectWrite>& list);
    void piece_done(size_t n, double write_ms);

    // ---- read side ----
    int read_submit_spans(const ReadSpan* spans, size_t n_spans, size_t bytes, pgsd_unpack_job job, uint64_t N,
                          const uint32_t* rows, uint64_t src_N, bool stage_only, std::shared_ptr<ReadReq>* out);
    static std::shared_ptr<ReadReq> make_read_req(const pgsd_unpack_job& job, uint64_t N, const uint32_t* rows, uint64_t src_N,
                                                  bool stage_only, size_t pieces);
    void defer_unpack(const std::shared_ptr<ReadReq>& req);
    size_t pread_spans(const ReadSpan* spans, size_t n_spans, char* base);
    void read_piece(std::shared_ptr<ReadReq> req, char* dst, size_t n, std::shared_ptr<std::vector<ReadSpan>> parts);
    void read_done();
    void launch_pending_unpacks();
    void fill_across_launches(std::vector<std::shared_ptr<ReadReq>>& pending);
    const void* kept_chunk(long long file_offset, size_t bytes) const;
    int stage_chunks(const ChunkRange* ranges, size_t n, uint64_t N, const void** src);
    // the most chunks one pass stages: the largest of what a predicate, a grouped reduction and the SPH samples take
    enum
        {
        STAGED_GROUPED_CHUNKS = (WHERE_MAX_TERMS + 1 > GROUPED_CHUNKS ? WHERE_MAX_TERMS + 1 : GROUPED_CHUNKS),
        STAGED_MAX_CHUNKS = (STAGED_GROUPED_CHUNKS > SPHS_CHUNKS ? STAGED_GROUPED_CHUNKS : SPHS_CHUNKS)
        };
    int stage_present(const ChunkRange* ranges, const void** const* slots, size_t n, uint32_t present, uint64_t N);

    // Who guards what.  m_mutex: the slab ring's free list, the job queue, tickets, committed direct chunks, every event
    // list and pool, both outstanding counts, m_stop, the error state, the statistics.  m_copy_mutex: enqueues on the
    // copy stream from reader threads, ReadReq::pieces_left, m_unpack_pending.  Everything without a note belongs to the
    // thread that calls into the pipeline (one at a time per handle).
    std::mutex m_mutex;
    std::mutex m_copy_mutex;
    std::condition_variable m_cv_jobs, m_cv_slabs, m_cv_done;

    pgsd_device_config m_cfg;
    int m_fd;
    bool m_shared; // other processes write the same file
    bool m_ok = false;
    bool m_numa = false; // m_numa_cpus = CPUs of the GPU's NUMA node (two-socket hosts)
    cpu_set_t m_numa_cpus;
    hipStream_t m_source_stream = nullptr; // null stream unless the caller names another

    // streams, slab ring (full-sized from init() on: slots [0, m_slabs_ready) are pinned), direct arena, HBM arenas;
    // the two idle-event pools in it: m_mutex
    DeviceResources m_res;
    uint32_t m_slabs_ready = 0;        // grown by the dispatcher thread only
    std::deque<uint32_t> m_free_slabs; // m_mutex
    size_t m_dused = 0, m_direct_max = 0;
    bool m_direct_failed = false;
    bool m_coalesce = true;              // neighbours in the file leave in one pwritev (write_direct)
    bool m_warm = false;                 // slab pieces go down the lane as a warm-then-write pair (PGSD_WRITE_WARM)
    size_t m_soft_cap = (size_t)6 << 30; // staging held by frames on their way before stage() waits (PGSD_STAGING_CAP_MIB)

    // per-frame events, handed back to the pools by reset_staging() (m_mutex); the timed ones in (begin, end) pairs
    std::vector<hipEvent_t> m_pack_events, m_copy_events;
    std::vector<hipEvent_t> m_misc_events, m_misc_timing_events;

    // write side (all m_mutex)
    std::deque<CopyJob> m_jobs;
    std::map<int, Staged> m_staged;    // packed chunks whose file offsets are not known yet
    int m_next_ticket = 1;
    std::vector<DirectWrite> m_direct; // committed direct chunks waiting for their pwrite
    size_t m_outstanding = 0;
    bool m_stop = false;
    pgsd_device_stats m_stats = {};
    uint64_t m_side_bytes_base = 0;      // the side lane's counters at the last reset of the statistics
    double m_side_ms_base = 0;
    WriterPool* m_pool = nullptr;
    std::thread m_dispatcher;
    std::atomic<bool> m_copy_used {false}; // something was enqueued on the copy stream since drain() last synchronised it

    uint32_t* m_cmp_host = nullptr; // compare(): answers, pinned; its device alias; the early-exit words in HBM
    uint32_t* m_cmp_host_dev = nullptr;
    uint32_t* m_cmp_dev = nullptr;
    uint32_t m_cmp_gen = 0;

    // read side
    ReadEngine* m_reader = nullptr;          // shared reader threads + pinned ring of this device
    size_t m_reads_outstanding = 0;          // m_mutex; counted per piece
    uint64_t m_read_seq = 0;                 // ReadReq::seq of the next submission
    std::vector<std::shared_ptr<ReadReq>> m_unpack_pending; // m_copy_mutex
    std::atomic<uint64_t> m_pread_bytes {0}; // file bytes pread / bytes copied host-to-device (read_counters)
    std::atomic<uint64_t> m_h2d_bytes {0};
    uint32_t* m_bad_host = nullptr;          // indexed reads: set by a gather that met a row outside its chunk (pinned)
    uint32_t* m_bad_dev = nullptr;           // ... its device alias
    struct Kept                              // a whole chunk a selection staged, kept until the next wait_read
        {
        const void* src;
        long long file_offset;
        size_t bytes;
        };
    std::vector<Kept> m_kept;

    // error state (m_mutex)
    std::string m_error;
    bool m_io_error = false;
    int m_io_errno = 0; // errno of the failed write (worker thread), handed to the caller's thread
    };
    } // namespace pgsd_amd

#endif
