// pgsd_io.cpp -- positional file IO at the offsets of the reference's MPI-IO calls
// (MPI_File_write_at pgsd.c:2229/1154/2032, MPI_File_read_at pgsd.c:651/1559/2534).
// Each rank writes its own byte range at the offset the reference computes, through one of two back ends behind the
// io_* functions below: POSIX pwrite / pread (the default), or -- PGSD_IO=mpiio -- the reference's own
// MPI_File_write_at / MPI_File_read_at, reached through the optional plugin libpgsd_amd_mpiio.so
// (pgsd_mpiio_plugin.h; the library itself does not link MPI).  Same bytes at the same offsets either way.
// The small thread pool here carries the device pipeline's writer and reader threads.  For
// WRITES one thread per file is the measured optimum on the target boxes (buffered writes
// serialise on the file's inode lock: profiles/r01_io_probe*.log) -- one ordered lane, which may
// work as a warm-then-write pair (WarmPair below); page-cache READS take no exclusive lock and
// scale with threads.
#include "pgsd_internal.hpp"
#include "pgsd_mpiio_plugin.h"

#include <atomic>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>
#include <pthread.h>
#include <sched.h>
#include <string>
#include <cstdlib>
#include <sys/file.h>
#include <sys/uio.h>
#include <condition_variable>
#include <deque>
#include <dlfcn.h>
#include <fcntl.h>
#include <map>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/vfs.h>
#include <sys/syscall.h>
#include <linux/futex.h>
#include <functional>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <algorithm>
#include <vector>

#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif

namespace pgsd_amd
    {
// ------------------------------------------------------------------ file back ends
namespace
    {
struct MpiFiles
    {
    std::mutex lock; // serialises every call into the plugin: MPI_THREAD_SERIALIZED is all the caller must provide
    int mode = -1;   // -1: PGSD_IO not looked at yet, 0: POSIX, 1: MPI-IO
    bool loaded = false;
    pgsd_mpiio_api api {};
    std::map<int, void*> files; // descriptor -> the plugin's file handle
    };
MpiFiles g_mpi;
std::atomic<int> g_mpi_open {0}; // number of MPI-IO files: the POSIX back end never takes the lock

// the plugin lies next to this library unless PGSD_MPIIO_LIBRARY names another build (another MPI)
bool load_mpiio_plugin()
    {
    if (g_mpi.loaded)
        return true;
    std::string path;
    if (const char* e = getenv("PGSD_MPIIO_LIBRARY"))
        path = e;
    else
        {
        Dl_info info;
        if (dladdr((void*)&load_mpiio_plugin, &info) && info.dli_fname)
            {
            path = info.dli_fname;
            const size_t slash = path.rfind('/');
            path = (slash == std::string::npos ? std::string() : path.substr(0, slash + 1)) + "libpgsd_amd_mpiio.so";
            }
        else
            path = "libpgsd_amd_mpiio.so";
        }
    void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib)
        {
        set_last_error(std::string("PGSD_IO=mpiio: cannot load the MPI-IO back end (build it with `make -C pgsd-sph_amd/csrc mpiio`): ")
                       + dlerror());
        return false;
        }
    auto entry = (int (*)(pgsd_mpiio_api*))dlsym(lib, "pgsd_mpiio_plugin");
    if (!entry)
        {
        set_last_error("PGSD_IO=mpiio: " + path + " has no pgsd_mpiio_plugin");
        return false;
        }
    if (entry(&g_mpi.api) != 0)
        {
        set_last_error(std::string("PGSD_IO=mpiio: ") + (g_mpi.api.last_error ? g_mpi.api.last_error() : "the back end refused"));
        return false;
        }
    g_mpi.loaded = true;
    return true;
    }

// run f(plugin handle of fd) under the plugin lock when fd is an MPI-IO file; false: fd is a POSIX file
template<class F> bool with_mpi_file(int fd, F f)
    {
    if (g_mpi_open.load(std::memory_order_acquire) == 0)
        return false;
    std::lock_guard<std::mutex> guard(g_mpi.lock);
    auto it = g_mpi.files.find(fd);
    if (it == g_mpi.files.end())
        return false;
    f(it->second);
    return true;
    }
    } // namespace

const char* io_backend_name()
    {
    std::lock_guard<std::mutex> guard(g_mpi.lock);
    if (g_mpi.mode < 0)
        {
        const char* e = getenv("PGSD_IO");
        g_mpi.mode = (e && strcmp(e, "mpiio") == 0) ? 1 : 0;
        if (e && *e && strcmp(e, "mpiio") != 0 && strcmp(e, "posix") != 0)
            fprintf(stderr, "pgsd_amd: PGSD_IO=%s is neither posix nor mpiio: posix\n", e);
        }
    return g_mpi.mode == 1 ? "mpiio" : "posix";
    }

// open(2); with PGSD_IO=mpiio the file is ALSO opened through MPI-IO and every later io_* call on the descriptor
// goes there (the descriptor stays the file's identity and what the advisory write lock is taken on)
int io_open(const char* path, int oflags, int mode)
    {
    const int fd = open(path, oflags, mode);
    if (fd < 0 || strcmp(io_backend_name(), "mpiio") != 0)
        return fd;
    std::lock_guard<std::mutex> guard(g_mpi.lock);
    void* fh = nullptr;
    if (!load_mpiio_plugin() || g_mpi.api.open(path, (oflags & O_ACCMODE) == O_RDONLY, &fh) != 0)
        {
        if (g_mpi.loaded)
            set_last_error(std::string("PGSD_IO=mpiio: ") + g_mpi.api.last_error());
        close(fd);
        errno = EIO;
        return -1;
        }
    g_mpi.files[fd] = fh;
    g_mpi_open.fetch_add(1, std::memory_order_release);
    return fd;
    }

int io_close(int fd)
    {
    int rc = 0;
    bool mpi = false;
        {
        std::lock_guard<std::mutex> guard(g_mpi.lock);
        auto it = g_mpi.files.find(fd);
        if (it != g_mpi.files.end())
            {
            mpi = true;
            rc = g_mpi.api.close(it->second);
            g_mpi.files.erase(it);
            g_mpi_open.fetch_sub(1, std::memory_order_release);
            }
        }
    const int crc = close(fd);
    if (mpi && rc != 0)
        {
        errno = EIO;
        return -1;
        }
    return crc;
    }

int io_truncate(int fd, long long size)
    {
    int rc = 0;
    if (with_mpi_file(fd, [&](void* fh) { rc = g_mpi.api.set_size(fh, size); }))
        {
        if (rc != 0)
            errno = EIO;
        return rc;
        }
    return ftruncate(fd, (off_t)size);
    }

long long io_file_size(int fd)
    {
    long long size = -1;
    if (with_mpi_file(fd, [&](void* fh) { size = g_mpi.api.get_size(fh); }))
        {
        if (size < 0)
            errno = EIO;
        return size;
        }
    struct stat st;
    if (fstat(fd, &st) != 0)
        return -1;
    return (long long)st.st_size;
    }

// pwrite(2) / pread(2) semantics (bytes moved, -1 + errno) on either back end
ssize_t io_pwrite(int fd, const void* buf, size_t bytes, long long offset)
    {
    long long n = -1;
    if (with_mpi_file(fd, [&](void* fh) { n = g_mpi.api.write_at(fh, offset, buf, (long long)bytes); }))
        {
        if (n < 0)
            {
            set_last_error(std::string("PGSD_IO=mpiio: ") + g_mpi.api.last_error());
            errno = EIO;
            }
        return (ssize_t)n;
        }
    return pwrite(fd, buf, bytes, (off_t)offset);
    }

ssize_t io_pread(int fd, void* buf, size_t bytes, long long offset)
    {
    long long n = -1;
    if (with_mpi_file(fd, [&](void* fh) { n = g_mpi.api.read_at(fh, offset, buf, (long long)bytes); }))
        {
        if (n < 0)
            errno = EIO;
        return (ssize_t)n;
        }
    return pread(fd, buf, bytes, (off_t)offset);
    }

int pwrite_full(int fd, const void* buf, size_t bytes, long long offset)
    {
    const char* p = (const char*)buf;
    while (bytes > 0)
        {
        ssize_t w = io_pwrite(fd, p, bytes, offset);
        if (w < 0)
            {
            if (errno == EINTR)
                continue;
            return -errno;
            }
        p += w;
        offset += w;
        bytes -= (size_t)w;
        }
    return 0;
    }

// Buffered writes to one file serialise on its inode lock inside the kernel; when several
// PROCESSES (ranks) write the same file at once the lock convoy makes the aggregate rate drop
// well below a single writer's (profiles/r01_io_probe3.log, bench rehearsal: 7.0 -> 4.1 -> 3.6
// GB/s for 1/2/4 ranks on tmpfs).  Taking an advisory flock around each piece lets the ranks
// queue asleep instead, which keeps the file at the single-writer rate.
static int g_write_lock = -1;

static bool write_lock_wanted()
    {
    if (g_write_lock < 0)
        {
        const char* e = getenv("PGSD_WRITE_LOCK");
        g_write_lock = (e && atoi(e) == 0) ? 0 : 1;
        }
    return g_write_lock != 0;
    }

int pwrite_locked(int fd, const void* buf, size_t bytes, long long offset, bool shared_file)
    {
    if (!shared_file || !write_lock_wanted())
        return pwrite_full(fd, buf, bytes, offset);
    while (flock(fd, LOCK_EX) != 0)
        if (errno != EINTR)
            return pwrite_full(fd, buf, bytes, offset); // no lock support: write anyway
    int rc = pwrite_full(fd, buf, bytes, offset);
    flock(fd, LOCK_UN);
    return rc;
    }

// Several buffers, one contiguous file range, one system call (the chunks of a small frame follow each other in
// the file but not necessarily in memory).  `iov` is consumed.
int pwritev_locked(int fd, struct iovec* iov, int n, long long offset, bool shared_file)
    {
    if (g_write_lock < 0)
        {
        const char* e = getenv("PGSD_WRITE_LOCK");
        g_write_lock = (e && atoi(e) == 0) ? 0 : 1;
        }
    bool locked = false;
    if (shared_file && g_write_lock)
        {
        locked = true;
        while (flock(fd, LOCK_EX) != 0)
            if (errno != EINTR)
                {
                locked = false; // no lock support: write anyway
                break;
                }
        }
    int rc = 0;
    if (g_mpi_open.load(std::memory_order_acquire) != 0 && with_mpi_file(fd, [](void*) { }))
        {
        // MPI-IO has no gather write: one MPI_File_write_at per buffer, in file order
        for (; n > 0 && rc == 0; iov++, n--)
            {
            rc = pwrite_full(fd, iov->iov_base, iov->iov_len, offset);
            offset += (long long)iov->iov_len;
            }
        n = 0;
        }
    while (n > 0)
        {
        ssize_t w = pwritev(fd, iov, n > 1024 ? 1024 : n, (off_t)offset);
        if (w < 0)
            {
            if (errno == EINTR)
                continue;
            rc = -errno;
            break;
            }
        offset += w;
        size_t left = (size_t)w;
        while (n > 0 && left >= iov->iov_len)
            {
            left -= iov->iov_len;
            iov++;
            n--;
            }
        if (n > 0 && left > 0)
            {
            iov->iov_base = (char*)iov->iov_base + left;
            iov->iov_len -= left;
            }
        else if (n > 0 && w == 0 && iov->iov_len > 0)
            {
            rc = -EIO; // no progress on a non-empty buffer
            break;
            }
        }
    if (locked)
        flock(fd, LOCK_UN);
    return rc;
    }

void pread_some(int fd, void* buf, size_t bytes, long long offset)
    {
    char* p = (char*)buf;
    while (bytes > 0)
        {
        ssize_t r = io_pread(fd, p, bytes, offset);
        if (r <= 0)
            {
            if (r < 0 && errno == EINTR)
                continue;
            return; // short read: the tail keeps its previous contents
            }
        p += r;
        offset += r;
        bytes -= (size_t)r;
        }
    }

// Large host reads (restart files read on the CPU side) are split over a few short-lived
// threads: page-cache reads take no exclusive lock and scale (profiles/r01_read_sweep.log).
void pread_parallel(int fd, void* buf, size_t bytes, long long offset)
    {
    const size_t min_piece = (size_t)32 << 20;
    unsigned hw = std::thread::hardware_concurrency();
    size_t n = bytes / min_piece;
    size_t cap = 8;
    if (const char* e = getenv("PGSD_HOST_READ_THREADS"))
        cap = (size_t)(atoi(e) > 0 ? atoi(e) : 1);
    if (n > cap)
        n = cap;
    if (hw && n > hw)
        n = hw;
    if (n < 2)
        {
        pread_some(fd, buf, bytes, offset);
        return;
        }
    const size_t piece = ((bytes + n - 1) / n + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (size_t off = piece; off < bytes; off += piece)
        {
        const size_t len = bytes - off < piece ? bytes - off : piece;
        th.emplace_back([=] { pread_some(fd, (char*)buf + off, len, offset + (long long)off); });
        }
    pread_some(fd, buf, piece < bytes ? piece : bytes, offset);
    for (auto& t : th)
        t.join();
    }

// ------------------------------------------------------------------ the warm-then-write pair
// One 16 MiB pwrite into a growing tmpfs file holds the file's inode lock for 2.4-2.8 ms, and a sixth of that is the
// kernel's copy missing the cache on every source line: the GPU's PCIe writes leave a slab in DRAM.  Reading a piece into
// cache needs no lock, so the ORDERED LANE of a pool (its one writer thread) may run large pieces as a pair: the piece is cut
// into sub-pieces which the lane thread and one helper thread take in turn -- touch one byte per 64-byte line of the
// sub-piece, wait for the turn on a ticket, pwrite, pass the ticket on.  Never are the two inside pwrite at once (the
// ticket, not the kernel's lock, orders them) and the lane thread returns when the piece's last sub-piece is in the file,
// so what the pool promises about submission order is untouched: the pair is how one job is carried out.
// tools/labs/warm_write_lab.hip measured it (profiles/r23_warm_write_lab.log).
namespace
    {
inline void futex_sleep(std::atomic<uint32_t>* word, uint32_t seen)
    {
    syscall(SYS_futex, (uint32_t*)word, FUTEX_WAIT_PRIVATE, seen, nullptr, nullptr, 0);
    }

// a word that threads wait on: a bounded spin (the other thread is a sub-piece away), then asleep in the kernel
struct WaitWord
    {
    std::atomic<uint32_t> value {0};
    std::atomic<uint32_t> sleepers {0};

    template<class Done> uint32_t wait(Done done)
        {
        for (int spin = 0; spin < 4000; spin++)
            {
            const uint32_t v = value.load(std::memory_order_acquire);
            if (done(v))
                return v;
#if defined(__x86_64__) || defined(__i386__)
            __builtin_ia32_pause();
#endif
            }
        sleepers.fetch_add(1);
        uint32_t v;
        while (!done(v = value.load()))
            futex_sleep(&value, v);
        sleepers.fetch_sub(1);
        return v;
        }

    void post(uint32_t v)
        {
        value.store(v);
        if (sleepers.load() != 0)
            syscall(SYS_futex, (uint32_t*)&value, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
        }

    void add(uint32_t n)
        {
        value.fetch_add(n);
        if (sleepers.load() != 0)
            syscall(SYS_futex, (uint32_t*)&value, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
        }
    };
    } // namespace

// cores (with their hardware threads) that lanes of this process have for themselves: two pipelines never share one
static std::mutex g_lane_mutex;
static cpu_set_t g_lane_cores;

class WarmPair
    {
    public:
    WarmPair(size_t sub_bytes, const cpu_set_t* cpus) : m_sub((sub_bytes + PAGE - 1) / PAGE * PAGE), m_placed(cpus != nullptr)
        {
        if (cpus)
            m_cpus = *cpus;
        m_helper = std::thread([this] { helper(); });
        if (cpus)
            (void)pthread_setaffinity_np(m_helper.native_handle(), sizeof(cpu_set_t), cpus);
        }

    // the CPUs the pair was put on (those that share one L3); null: unplaced
    const cpu_set_t* cpus() const
        {
        return m_placed ? &m_cpus : nullptr;
        }

    std::thread& helper_thread()
        {
        return m_helper;
        }

    ~WarmPair()
        {
        m_stop.store(true);
        m_gen.post(m_gen.value.load() + 1);
        m_helper.join();
        for (auto& t : m_side)
            t.join();
        drop_windows();
        if (m_has_cores)
            {
            std::lock_guard<std::mutex> g(g_lane_mutex);
            for (int c = 0; c < CPU_SETSIZE; c++)
                if (CPU_ISSET(c, &m_cores))
                    CPU_CLR(c, &g_lane_cores);
            }
        }

    // cores of g_lane_cores that are this lane's until it goes
    void keep_cores(const cpu_set_t& cores)
        {
        m_cores = cores;
        m_has_cores = true;
        }

    size_t sub_bytes() const
        {
        return m_sub;
        }

    // `n` side threads (at most three) for pieces that go to `fd`, blocks of `block` bytes (rounded up to whole pages);
    // fail_at >= 0: the populate call of that number (counted over the handle) reports failure, for tests
    // side thread i goes to CPU cores[i] where there is one, else on `cpus`
    void enable_side(int fd, unsigned n, size_t block, const cpu_set_t* cpus, const std::vector<int>& cores, long fail_at)
        {
        if (!m_side.empty() || n == 0)
            return;
        m_side_fd = fd;
        m_block_pages = (uint32_t)std::min<size_t>(std::max<size_t>((block + PAGE - 1) / PAGE, 1), MAX_PAGES);
        m_fail_at = fail_at;
        for (unsigned i = 0; i < std::min(n, 3u); i++)
            {
            m_side.emplace_back([this] { side(); });
            cpu_set_t one;
            CPU_ZERO(&one);
            if (i < cores.size())
                CPU_SET(cores[i], &one);
            if (i < cores.size() || cpus)
                (void)pthread_setaffinity_np(m_side.back().native_handle(), sizeof(cpu_set_t), i < cores.size() ? &one : cpus);
            }
        }

    bool side_on() const
        {
        return !m_side.empty() && !m_side_off.load();
        }

    void side_counters(uint64_t* bytes, double* ms) const
        {
        *bytes = m_side_bytes.load();
        *ms = (double)m_side_ns.load() * 1e-6;
        }

    // every window goes; only while no piece is in flight (a job of the lane, or the lane's threads joined)
    void drop_windows()
        {
        std::vector<char*> all;
            {
            std::lock_guard<std::mutex> g(m_win_mutex);
            all.swap(m_retired);
            }
        for (Window& w : m_windows)
            all.push_back(w.base);
        m_windows.clear();
        for (char* m : all)
            munmap(m, WINDOW);
        }

    // The lane thread's half of one piece (longer than a sub-piece); 0 or -errno of the first pwrite that failed, after
    // which the rest of the piece is skipped -- its tickets still pass.  With `side`, side threads and whole pages of
    // the file inside the piece, the piece is split and the side lane takes part (below); every other piece goes the
    // pair's own road, run().
    int write(int fd, const char* buf, size_t bytes, long long offset, double* pwrite_ms, bool side)
        {
        const long long end = offset + (long long)bytes;
        long long a0 = offset, a1 = end;
        m_err.store(0);
        m_pwrite_ns.store(0);
        bool split = false;
        if (side && side_on() && fd == m_side_fd)
            {
            // cut on page boundaries of the FILE: the head fragment up to the first, the tail fragment from the last
            const long long h = (offset + (long long)PAGE - 1) & ~((long long)PAGE - 1), t = (end - 1) & ~((long long)PAGE - 1);
            if (t > h && (size_t)(t - h) / PAGE <= MAX_PAGES && map_windows(fd, h, t))
                {
                split = true;
                a0 = h;
                a1 = t;
                // the tail first: real bytes that put end-of-file behind the piece before a side thread touches the mapping
                pwrite_timed(fd, buf + (size_t)(a1 - offset), (size_t)(end - a1), a1);
                if (a0 != offset)
                    pwrite_timed(fd, buf, (size_t)(a0 - offset), offset);
                }
            }
        const uint32_t gen = m_gen.value.load() + 1;
        if (!split)
            {
            // the pair alone, as ever: sub-pieces of the whole piece, taken in turn by the two threads
            m_fd = fd;
            m_buf = buf;
            m_bytes = bytes;
            m_offset = offset;
            m_base = m_ticket.value.load();
            m_road.store((uint64_t)gen << 1);
            m_gen.post(gen); // publishes the piece to the helper
            const uint32_t n = run(0);
            const uint32_t last = m_base + n;
            m_ticket.wait([last](uint32_t v) { return v == last; });
            if (pwrite_ms)
                *pwrite_ms = (double)m_pwrite_ns.load() * 1e-6;
            return m_err.load();
            }
        const uint32_t pages = (uint32_t)(((size_t)(a1 - a0) + PAGE - 1) / PAGE);
        const uint32_t base = m_ticket.value.load();
        m_vfd.store(fd, std::memory_order_relaxed);
        m_vbuf.store(buf + (size_t)(a0 - offset), std::memory_order_relaxed);
        m_va0.store(a0, std::memory_order_relaxed);
        m_vlen.store((size_t)(a1 - a0), std::memory_order_relaxed);
        m_vbase.store(base, std::memory_order_relaxed);
        m_side_done.value.store(0);
        m_cursors.store(pack(gen, 0, pages));
        m_road.store((uint64_t)gen << 1 | 1);
        m_gen.post(gen); // publishes the piece to the helper and the side threads
        pair(gen);
        // the cursors have met: what lies below them was the pair's, in claims of m_sub, what lies above the side lane's
        const uint32_t front = front_of(m_cursors.load()), per = (uint32_t)(m_sub / PAGE);
        const uint32_t turn_end = base + (front + per - 1) / per, side_pages = pages - front;
        m_ticket.wait([turn_end](uint32_t v) { return v == turn_end; });
        m_side_done.wait([side_pages](uint32_t v) { return v == side_pages; });
        // blocks a side thread gave back (its populate failed): through pwrite, so that ENOSPC reaches the caller as ever
        std::vector<std::pair<uint32_t, uint32_t>> back;
            {
            std::lock_guard<std::mutex> g(m_win_mutex);
            back.swap(m_returned);
            }
        for (auto& b : back)
            {
            const size_t at = (size_t)b.first * PAGE, len = std::min((size_t)b.second * PAGE, (size_t)(a1 - a0) - at);
            pwrite_timed(fd, buf + (size_t)(a0 - offset) + at, len, a0 + (long long)at);
            }
        if (pwrite_ms)
            *pwrite_ms = (double)m_pwrite_ns.load() * 1e-6;
        return m_err.load();
        }

    private:
    static const size_t PAGE = 4096;
    static const size_t WINDOW = (size_t)256 << 20; // of the file, per mapping (profiles/r28_side_lane_lab.log)
    static const uint32_t MAX_PAGES = (1u << 22) - 1;

    // the cursors of the piece in flight in one word, with the piece's number: a thread that still holds an earlier
    // piece's view cannot claim (its compare-and-swap fails)
    static uint64_t pack(uint32_t gen, uint32_t front, uint32_t back)
        {
        return (uint64_t)(gen & 0xfffffu) << 44 | (uint64_t)front << 22 | back;
        }
    static uint32_t front_of(uint64_t c)
        {
        return (uint32_t)(c >> 22) & MAX_PAGES;
        }
    static uint32_t back_of(uint64_t c)
        {
        return (uint32_t)c & MAX_PAGES;
        }

    struct View // a thread's copy of the piece in flight
        {
        int fd;
        const char* buf;
        long long a0;
        size_t len;
        uint32_t base;
        };
    View view() const
        {
        return {m_vfd.load(std::memory_order_relaxed), m_vbuf.load(std::memory_order_relaxed), m_va0.load(std::memory_order_relaxed),
                m_vlen.load(std::memory_order_relaxed), m_vbase.load(std::memory_order_relaxed)};
        }

    void pwrite_timed(int fd, const char* p, size_t n, long long off)
        {
        if (n == 0 || m_err.load() != 0)
            return;
        TraceRange tr("pgsd:pwrite file_off=%llu bytes=%llu", (unsigned long long)off, n);
        auto t0 = std::chrono::steady_clock::now();
        int w = pwrite_full(fd, p, n, off);
        m_pwrite_ns.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
        int none = 0;
        if (w != 0)
            m_err.compare_exchange_strong(none, w);
        }

    void helper()
        {
        uint32_t seen = 0;
        for (;;)
            {
            seen = m_gen.wait([seen](uint32_t v) { return v != seen; });
            if (m_stop.load())
                return;
            // Which road piece `seen` takes was stored before m_gen moved.  Where the word already speaks of a later
            // piece, `seen` was a split one that the other threads finished (a piece of the pair alone cannot end
            // without its helper): look again.
            const uint64_t road = m_road.load();
            if ((uint32_t)(road >> 1) != seen)
                continue;
            if (road & 1)
                pair(seen);
            else
                run(1);
            }
        }

    // The pair alone: sub-pieces who, who + 2, ... of the piece in flight; returns how many sub-pieces the piece has
    uint32_t run(uint32_t who)
        {
        const int fd = m_fd;
        const char* const buf = m_buf;
        const size_t bytes = m_bytes, sub = m_sub;
        const long long offset = m_offset;
        const uint32_t base = m_base, n = (uint32_t)((bytes + sub - 1) / sub);
        for (uint32_t g = who; g < n; g += 2)
            {
            const size_t at = (size_t)g * sub, len = std::min(sub, bytes - at);
            const unsigned long long foff = (unsigned long long)(offset + (long long)at);
                {
                TraceRange tr("pgsd:warm file_off=%llu bytes=%llu", foff, len);
                unsigned acc = 0;
                for (const char* q = buf + at; q < buf + at + len; q = (const char*)(((uintptr_t)q | 63) + 1))
                    acc += (unsigned char)*(const volatile char*)q;
                m_sink.store(acc, std::memory_order_relaxed);
                }
            const uint32_t turn = base + g;
            m_ticket.wait([turn](uint32_t v) { return v == turn; });
            if (m_err.load() == 0)
                {
                TraceRange tr("pgsd:pwrite file_off=%llu bytes=%llu", foff, len);
                auto t0 = std::chrono::steady_clock::now();
                int w = pwrite_full(fd, buf + at, len, offset + (long long)at);
                m_pwrite_ns.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
                int none = 0;
                if (w != 0)
                    m_err.compare_exchange_strong(none, w);
                }
            m_ticket.post(turn + 1);
            }
        return n;
        }

    // With the side lane, the pair's half of piece `gen`: claim a sub-piece upwards from the front, read it into cache, wait for the turn
    // (claim order), pwrite, pass the turn on -- until the cursors meet.
    void pair(uint32_t gen)
        {
        const View v = view();
        const uint32_t per = (uint32_t)(m_sub / PAGE);
        for (;;)
            {
            uint64_t c = m_cursors.load();
            uint32_t front, n;
            for (;;)
                {
                front = front_of(c);
                const uint32_t back = back_of(c);
                if (c >> 44 != (gen & 0xfffffu) || front >= back)
                    return;
                n = std::min(per, back - front);
                if (m_cursors.compare_exchange_weak(c, pack(gen, front + n, back)))
                    break;
                }
            const size_t at = (size_t)front * PAGE, len = std::min((size_t)n * PAGE, v.len - at);
            const unsigned long long foff = (unsigned long long)(v.a0 + (long long)at);
                {
                TraceRange tr("pgsd:warm file_off=%llu bytes=%llu", foff, len);
                unsigned acc = 0;
                for (const char* q = v.buf + at; q < v.buf + at + len; q = (const char*)(((uintptr_t)q | 63) + 1))
                    acc += (unsigned char)*(const volatile char*)q;
                m_sink.store(acc, std::memory_order_relaxed);
                }
            const uint32_t turn = v.base + front / per; // every claim but a piece's last takes `per` pages
            m_ticket.wait([turn](uint32_t t) { return t == turn; });
            pwrite_timed(v.fd, v.buf + at, len, v.a0 + (long long)at);
            m_ticket.post(turn + 1);
            }
        }

    // ---- the side lane: a second stream of page insertions beside the pair's, through a MAP_SHARED mapping of the file.
    // A store through a mapping inserts a fresh tmpfs page WITHOUT the file's inode lock, which is what the pair's
    // pwrite spends its time under.  Side threads claim blocks downwards from the back of the piece's whole pages,
    // populate a block's pages with madvise(MADV_POPULATE_WRITE) -- one call, an error code where a store would have
    // raised a signal -- and copy the block from the slab into pages that are then present.  A populate error gives
    // the block back to the lane thread (pwrite: ENOSPC as ever) and switches the side lane off for good.
    // tools/labs/side_lane_lab.cpp measured it (profiles/r28_side_lane_lab.log).
    struct Window
        {
        size_t index; // the window covers [index * WINDOW, (index + 1) * WINDOW) of the file
        char* base;
        };

    // windows for [a0, a1) of the file, by the lane thread before the piece is published; windows out of use go to a
    // side thread, which unmaps them.  false: the piece takes the pair's road (and on a failed mmap every later one)
    bool map_windows(int fd, long long a0, long long a1)
        {
        const size_t first = (size_t)a0 / WINDOW, last = (size_t)(a1 - 1) / WINDOW;
        if (last - first > 1)
            return false;
        char* base[2] = {nullptr, nullptr};
        for (size_t w = first; w <= last; w++)
            {
            for (Window& have : m_windows)
                if (have.index == w)
                    base[w - first] = have.base;
            if (base[w - first])
                continue;
            void* m = mmap(nullptr, WINDOW, PROT_READ | PROT_WRITE, MAP_SHARED, fd, (off_t)(w * WINDOW));
            if (m == MAP_FAILED)
                {
                m_side_off.store(true);
                return false;
                }
            m_windows.push_back({w, (char*)m});
            base[w - first] = (char*)m;
            }
        if (m_windows.size() > 3)
            {
            std::lock_guard<std::mutex> g(m_win_mutex);
            for (size_t i = 0; i < m_windows.size();)
                if (m_windows[i].index < first || m_windows[i].index > last)
                    {
                    m_retired.push_back(m_windows[i].base);
                    m_windows.erase(m_windows.begin() + (long)i);
                    }
                else
                    i++;
            }
        m_win_first.store(first, std::memory_order_relaxed);
        m_win_base[0].store(base[0], std::memory_order_relaxed);
        m_win_base[1].store(base[1], std::memory_order_relaxed);
        return true;
        }

    void side()
        {
        uint32_t seen = 0;
        for (;;)
            {
            seen = m_gen.wait([seen](uint32_t v) { return v != seen; });
            if (m_stop.load())
                return;
            std::vector<char*> retired;
                {
                std::lock_guard<std::mutex> g(m_win_mutex);
                retired.swap(m_retired);
                }
            for (char* m : retired)
                munmap(m, WINDOW);
            const uint64_t road = m_road.load();
            if ((uint32_t)(road >> 1) != seen || !(road & 1)) // a later piece already, or one of the pair alone
                continue;
            const View v = view();
            const size_t win_first = m_win_first.load(std::memory_order_relaxed);
            char* const win_base[2] = {m_win_base[0].load(std::memory_order_relaxed), m_win_base[1].load(std::memory_order_relaxed)};
            while (!m_side_off.load() && m_err.load() == 0)
                {
                uint64_t c = m_cursors.load();
                uint32_t back = 0, n = 0;
                for (;;)
                    {
                    const uint32_t front = front_of(c);
                    back = back_of(c);
                    n = 0;
                    if (c >> 44 != (seen & 0xfffffu) || front >= back)
                        break;
                    n = std::min(m_block_pages, back - front);
                    if (m_cursors.compare_exchange_weak(c, pack(seen, front, back - n)))
                        break;
                    }
                if (n == 0)
                    break;
                // (a successful claim says that piece `seen` is still in flight: the view above is that piece's)
                const uint32_t first = back - n;
                size_t len = std::min((size_t)n * PAGE, v.len - (size_t)first * PAGE);
                long long foff = v.a0 + (long long)first * (long long)PAGE;
                TraceRange tr("pgsd:side file_off=%llu bytes=%llu", (unsigned long long)foff, len);
                auto t0 = std::chrono::steady_clock::now();
                const size_t block_bytes = len;
                bool ok = true;
                while (ok && len != 0)
                    {
                    const size_t w = (size_t)foff / WINDOW, in = (size_t)foff % WINDOW, now = std::min(len, WINDOW - in);
                    char* dst = win_base[w - win_first] + in;
                    const long k = m_populates.fetch_add(1);
                    errno = 0;
                    if (k == m_fail_at || madvise(dst, now, MADV_POPULATE_WRITE) != 0)
                        {
                        ok = false; // EFAULT (a full tmpfs), ENOMEM, EINVAL (a kernel without the call): no store
                        if (!m_side_off.exchange(true))
                            fprintf(stderr, "pgsd_amd: the side lane of the writer is off from here on: populating pages failed (%s)\n",
                                    errno ? strerror(errno) : "PGSD_WRITE_SIDE_FAIL_AT");
                        }
                    else
                        memcpy(dst, v.buf + (size_t)(foff - v.a0), now);
                    foff += (long long)now;
                    len -= now;
                    }
                if (ok)
                    {
                    m_side_bytes.fetch_add(block_bytes);
                    m_side_ns.fetch_add((uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
                    }
                else
                    {
                    m_side_off.store(true);
                    std::lock_guard<std::mutex> g(m_win_mutex);
                    m_returned.push_back({first, n});
                    }
                m_side_done.add(n);
                }
            }
        }

    const size_t m_sub;
    const bool m_placed;
    cpu_set_t m_cpus;
    bool m_has_cores = false;
    cpu_set_t m_cores;
    std::thread m_helper;
    // the piece in flight on the pair's own road: written by the lane thread before m_gen moves, read by the helper behind it
    int m_fd = -1;
    const char* m_buf = nullptr;
    size_t m_bytes = 0;
    long long m_offset = 0;
    uint32_t m_base = 0;
    std::atomic<uint64_t> m_road {0};         // piece number << 1 | the piece is split (the side lane takes part)
    // the piece in flight with the side lane (atomics: a thread that slept through a whole piece may read while the
    // next is set up; it then cannot claim)
    std::atomic<int> m_vfd {-1};
    std::atomic<const char*> m_vbuf {nullptr}; // the byte that goes to m_va0
    std::atomic<long long> m_va0 {0};          // the claimed range of the file starts here ...
    std::atomic<size_t> m_vlen {0};            // ... and is this long: the cursors count its 4 KiB pages
    std::atomic<uint32_t> m_vbase {0};
    std::atomic<uint64_t> m_cursors {0};
    WaitWord m_gen, m_ticket; // pieces handed to the other threads; sub-pieces written, of all pieces so far
    std::atomic<int> m_err {0};
    std::atomic<uint64_t> m_pwrite_ns {0};
    std::atomic<unsigned> m_sink {0};
    std::atomic<bool> m_stop {false};
    // the side lane
    std::vector<std::thread> m_side;
    int m_side_fd = -1;
    uint32_t m_block_pages = 0;
    long m_fail_at = -1;
    std::atomic<long> m_populates {0};
    std::atomic<bool> m_side_off {false};
    WaitWord m_side_done;                     // pages of the piece in flight that side threads are done with
    std::vector<Window> m_windows;            // the lane thread's
    std::atomic<size_t> m_win_first {0};
    std::atomic<char*> m_win_base[2] = {{nullptr}, {nullptr}};
    std::mutex m_win_mutex;                   // m_retired, m_returned
    std::vector<char*> m_retired;
    std::vector<std::pair<uint32_t, uint32_t>> m_returned; // first page, pages
    std::atomic<uint64_t> m_side_bytes {0}, m_side_ns {0};
    };

class WriterPool
    {
    public:
    explicit WriterPool(unsigned n, const cpu_set_t* cpus = nullptr) : m_stop(false)
        {
        if (n == 0)
            n = 1;
        for (unsigned i = 0; i < n; i++)
            {
            m_threads.emplace_back([this] { run(); });
            if (cpus) // keep the copy loops next to the memory they touch
                (void)pthread_setaffinity_np(m_threads.back().native_handle(), sizeof(cpu_set_t), cpus);
            }
        }

    ~WriterPool()
        {
            {
            std::lock_guard<std::mutex> g(m_mutex);
            m_stop = true;
            }
        m_cv.notify_all();
        for (auto& t : m_threads)
            t.join();
        delete m_warm;
        }

    // the lane becomes a pair (one helper thread more); both threads on `cpus`
    void enable_warm(size_t sub_bytes, const cpu_set_t* cpus)
        {
        if (m_warm || m_threads.size() != 1)
            return;
        m_warm = new WarmPair(sub_bytes, cpus);
        if (cpus)
            (void)pthread_setaffinity_np(m_threads[0].native_handle(), sizeof(cpu_set_t), cpus);
        }

    WarmPair* warm() const
        {
        return m_warm;
        }

    std::thread& lane_thread()
        {
        return m_threads[0];
        }

    void submit(std::function<void()> fn)
        {
            {
            std::lock_guard<std::mutex> g(m_mutex);
            m_jobs.push_back(std::move(fn));
            }
        m_cv.notify_one();
        }

    unsigned size() const
        {
        return (unsigned)m_threads.size();
        }

    private:
    void run()
        {
        for (;;)
            {
            std::function<void()> fn;
                {
                std::unique_lock<std::mutex> lk(m_mutex);
                m_cv.wait(lk, [this] { return m_stop || !m_jobs.empty(); });
                if (m_jobs.empty())
                    return;
                fn = std::move(m_jobs.front());
                m_jobs.pop_front();
                }
            fn();
            }
        }

    std::vector<std::thread> m_threads;
    std::deque<std::function<void()>> m_jobs;
    std::mutex m_mutex;
    std::condition_variable m_cv;
    bool m_stop;
    WarmPair* m_warm = nullptr;
    };

WriterPool* writer_pool_create(unsigned n_threads, const cpu_set_t* cpus)
    {
    return new WriterPool(n_threads, cpus);
    }

// "0-7,64-71" -> the CPUs of the list that are also in `allowed`; returns how many
static int parse_cpulist(const char* buf, const cpu_set_t* allowed, cpu_set_t* out)
    {
    CPU_ZERO(out);
    int count = 0;
    for (const char* p = buf; *p;)
        {
        char* end;
        long a = strtol(p, &end, 10);
        if (end == p)
            break;
        long b = a;
        if (*end == '-')
            b = strtol(end + 1, &end, 10);
        for (long c = a; c <= b && c < CPU_SETSIZE; c++)
            if (CPU_ISSET((int)c, allowed))
                {
                CPU_SET((int)c, out);
                count++;
                }
        if (*end != ',')
            break;
        p = end + 1;
        }
    return count;
    }

// CPUs of the NUMA node a PCI device hangs off, intersected with what this process may run on.
// false when the node is unknown (-1), the machine has one node, or PGSD_NUMA=0.
bool numa_cpus_of_pci_device(const char* pci_bus_id, cpu_set_t* out)
    {
    if (const char* e = getenv("PGSD_NUMA"))
        if (atoi(e) == 0)
            return false;
    char path[256], buf[4096];
    std::string bdf(pci_bus_id);
    for (char& c : bdf)
        c = (char)tolower((unsigned char)c);
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf.c_str());
    FILE* f = fopen(path, "r");
    if (!f)
        return false;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1)
        node = -1;
    fclose(f);
    if (node < 0)
        return false;
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f)
        return false;
    size_t n = fread(buf, 1, sizeof(buf) - 1, f);
    fclose(f);
    buf[n] = 0;
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0)
        return false;
    const int count = parse_cpulist(buf, &allowed, out);
    int total = CPU_COUNT(&allowed);
    return count > 0 && count < total; // a single node (or all CPUs) needs no pinning
    }

void writer_pool_destroy(WriterPool* p)
    {
    delete p;
    }

void writer_pool_submit(WriterPool* p, std::function<void()> fn)
    {
    p->submit(std::move(fn));
    }

// The CPUs of `within` (null: of this process) that share an L3 with the one this thread runs on -- or, where that one
// is not among them, with the first that has a neighbour: at least two cores.  Read from sysfs; false where it does not say.
static bool l3_sharing_cpus(const cpu_set_t* within, cpu_set_t* out)
    {
    cpu_set_t allowed;
    if (!within)
        {
        CPU_ZERO(&allowed);
        if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0)
            return false;
        within = &allowed;
        }
    if (CPU_COUNT(within) < 2)
        return false;
    cpu_set_t tried;
    CPU_ZERO(&tried);
    const int here = sched_getcpu();
    for (int i = -1; i < CPU_SETSIZE; i++)
        {
        const int c = i < 0 ? here : i;
        if (c < 0 || c >= CPU_SETSIZE || !CPU_ISSET(c, within) || CPU_ISSET(c, &tried))
            continue;
        char path[128], buf[4096];
        cpu_set_t siblings;
        size_t n = 0;
        snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", c);
        FILE* f = fopen(path, "r");
        if (!f)
            return false;
        n = fread(buf, 1, sizeof(buf) - 1, f);
        fclose(f);
        buf[n] = 0;
        const int in_group = parse_cpulist(buf, within, out);
        CPU_OR(&tried, &tried, out);
        CPU_SET(c, &tried);
        snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
        f = fopen(path, "r");
        if (!f)
            return false;
        n = fread(buf, 1, sizeof(buf) - 1, f);
        fclose(f);
        buf[n] = 0;
        if (in_group > parse_cpulist(buf, within, &siblings)) // more than the hardware threads of one core
            return true;
        }
    return false;
    }

bool writer_pool_enable_warm(WriterPool* p, size_t sub_bytes, const cpu_set_t* cpus, bool need_topology)
    {
    if (!p || p->size() != 1 || sub_bytes == 0 || strcmp(io_backend_name(), "posix") != 0)
        return false;
    cpu_set_t pair;
    const bool placed = l3_sharing_cpus(cpus, &pair);
    if (!placed && need_topology)
        return false;
    p->enable_warm(sub_bytes, placed ? &pair : nullptr);
    return p->warm() != nullptr;
    }

// Up to `want` CPUs, no two of them hardware threads of one core and none on a core that another lane of this process
// has: those of `first`, then those of `then` (may be null).  Fewer than `least`: none.  What is picked is entered in
// g_lane_cores, hardware threads included, and returned in *kept for the lane to give back.
static std::vector<int> cores_of_their_own(const cpu_set_t* first, const cpu_set_t* then, unsigned want, unsigned least, cpu_set_t* kept)
    {
    std::lock_guard<std::mutex> g(g_lane_mutex);
    std::vector<int> picked;
    cpu_set_t taken, all;
    taken = g_lane_cores;
    memset(&all, 0xff, sizeof(all));
    for (const cpu_set_t* from : {first, then})
        for (int c = 0; from && c < CPU_SETSIZE && picked.size() < want; c++)
            {
            if (!CPU_ISSET(c, from) || CPU_ISSET(c, &taken))
                continue;
            picked.push_back(c);
            CPU_SET(c, &taken);
            char path[128], buf[4096];
            snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", c);
            if (FILE* f = fopen(path, "r"))
                {
                const size_t n = fread(buf, 1, sizeof(buf) - 1, f);
                fclose(f);
                buf[n] = 0;
                cpu_set_t siblings;
                parse_cpulist(buf, &all, &siblings);
                CPU_OR(&taken, &taken, &siblings);
                }
            }
    CPU_ZERO(kept);
    if (picked.size() < least)
        return {};
    for (int c = 0; c < CPU_SETSIZE; c++)
        if (CPU_ISSET(c, &taken) && !CPU_ISSET(c, &g_lane_cores))
            CPU_SET(c, kept);
    g_lane_cores = taken;
    return picked;
    }

bool writer_pool_enable_side(WriterPool* p, int fd, unsigned n_threads, size_t block_bytes, const cpu_set_t* cpus, long fail_at)
    {
    WarmPair* pair = p ? p->warm() : nullptr;
    struct statfs fs;
    if (!pair || n_threads == 0 || block_bytes == 0 || fstatfs(fd, &fs) != 0 || (unsigned long)fs.f_type != 0x01021994ul) // TMPFS_MAGIC
        return false;
    // Placement as the lab had it (tools/labs/side_lane_lab.cpp): every thread of the lane on a core of its own -- the
    // lane thread and the helper, which so far moved within their L3 group, on its first two cores, the side threads on
    // the next ones, and on cores of `cpus` outside the group where it has too few.  Two of these threads on one core
    // (or on the two hardware threads of one) halve the lane's rate: side threads merely somewhere on `cpus` gave
    // 5.9-6.6 GB/s in three of five runs, less than the pair alone.  So cores that another pipeline of this process has
    // are passed over, there are only as many side threads as cores were found for, and where not even one is left
    // (a small cpuset) the side lane stays off and the pair stays as it was.  A pair that runs unplaced (tests of the
    // lane itself: nothing is known about the cores) has unplaced side threads.
    n_threads = std::min(n_threads, 3u);
    std::vector<int> cores;
    if (pair->cpus())
        {
        cpu_set_t kept;
        cores = cores_of_their_own(pair->cpus(), cpus, 2 + n_threads, 3, &kept);
        if (cores.empty())
            return false;
        pair->keep_cores(kept);
        n_threads = (unsigned)cores.size() - 2;
        }
    if (cores.size() >= 2)
        {
        cpu_set_t one;
        CPU_ZERO(&one);
        CPU_SET(cores[0], &one);
        (void)pthread_setaffinity_np(p->lane_thread().native_handle(), sizeof(one), &one);
        CPU_ZERO(&one);
        CPU_SET(cores[1], &one);
        (void)pthread_setaffinity_np(pair->helper_thread().native_handle(), sizeof(one), &one);
        cores.erase(cores.begin(), cores.begin() + 2);
        }
    else
        cores.clear();
    pair->enable_side(fd, n_threads, block_bytes, cpus, cores, fail_at);
    return pair->side_on();
    }

void writer_pool_side_counters(WriterPool* p, uint64_t* bytes, double* ms, bool* on)
    {
    *bytes = 0;
    *ms = 0;
    *on = false;
    if (WarmPair* pair = p ? p->warm() : nullptr)
        {
        pair->side_counters(bytes, ms);
        *on = pair->side_on();
        }
    }

void writer_pool_side_drop(WriterPool* p)
    {
    if (WarmPair* pair = p ? p->warm() : nullptr)
        pair->drop_windows();
    }

int writer_pool_pwrite_warm(WriterPool* p, int fd, const void* buf, size_t bytes, long long offset, bool shared_file,
                            double* pwrite_ms)
    {
    WarmPair* pair = p ? p->warm() : nullptr;
    if (!pair || bytes <= pair->sub_bytes())
        {
        auto t0 = std::chrono::steady_clock::now();
        int rc = pwrite_locked(fd, buf, bytes, offset, shared_file);
        if (pwrite_ms)
            *pwrite_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return rc;
        }
    // the advisory lock of a shared file is taken once per piece: both threads write through the one descriptor
    bool locked = shared_file && write_lock_wanted();
    while (locked && flock(fd, LOCK_EX) != 0)
        if (errno != EINTR)
            locked = false; // no lock support: write anyway
    int rc = pair->write(fd, (const char*)buf, bytes, offset, pwrite_ms, !shared_file);
    if (locked)
        flock(fd, LOCK_UN);
    return rc;
    }

int writer_pool_pwrite_sync(WriterPool* pool, int fd, const void* buf, size_t bytes, long long offset,
                            bool shared_file)
    {
    const size_t piece = (size_t)8 << 20;
    if (!pool || bytes <= piece || shared_file)
        {
        // pieces keep the lock hold time bounded so that ranks interleave
        int rc = 0;
        for (size_t off = 0; off < bytes && rc == 0; off += piece)
            rc = pwrite_locked(fd, (const char*)buf + off, bytes - off < piece ? bytes - off : piece,
                               offset + (long long)off, shared_file);
        return rc;
        }
    struct Latch
        {
        std::mutex m;
        std::condition_variable cv;
        size_t pending;
        int err;
        } latch;
    size_t n_pieces = (bytes + piece - 1) / piece;
    latch.pending = n_pieces;
    latch.err = 0;
    for (size_t i = 0; i < n_pieces; i++)
        {
        size_t off = i * piece;
        size_t n = bytes - off < piece ? bytes - off : piece;
        const char* p = (const char*)buf + off;
        pool->submit(
            [&latch, fd, p, n, offset, off]
            {
                int e = pwrite_full(fd, p, n, offset + (long long)off);
                std::lock_guard<std::mutex> g(latch.m);
                if (e != 0 && latch.err == 0)
                    latch.err = e;
                if (--latch.pending == 0)
                    latch.cv.notify_all();
            });
        }
    std::unique_lock<std::mutex> lk(latch.m);
    latch.cv.wait(lk, [&latch] { return latch.pending == 0; });
    return latch.err;
    }
    } // namespace pgsd_amd
