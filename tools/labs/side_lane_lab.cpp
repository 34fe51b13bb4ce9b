// tools/labs/side_lane_lab.cpp -- does a second stream of page insertions, through a MAP_SHARED mapping of the same file,
// pay beside the warm-then-write pair?  ("End-to-end bound".)  Host only: no GPU is touched.
//
// The device writer's frame is the time its lane spends inside pwrite: under the file's inode lock the kernel allocates,
// inserts and fills fresh 4 KiB pages.  A store through a shared mapping inserts pages WITHOUT that lock.  This lab lands
// `frames` frames of 280 MB in one fresh file, out of a ring of 16 source buffers of 16 MiB, frame k at 5416 + k x 280 MB
// (1320 mod 4096 for the first), with the lane built one of these ways per process:
//
//   lane=1                       one thread, one pwrite per 16 MiB piece
//   lane=2 side=0                the pair of WarmPair (pgsd_io.cpp): 512 KiB sub-pieces, each read into cache by the
//                                thread that then waits for its turn on a ticket and pwrites it
//   lane=2 side=1|2|3 block=B    the piece is cut on page boundaries of the FILE: the head fragment (up to the first
//                                4096-aligned offset) and the tail fragment (from the last one) are pwritten by the lane
//                                thread, the tail first, so that end-of-file lies behind the piece before a mapping is
//                                touched; the whole pages in between are claimed through one atomic pair of cursors --
//                                the pair takes 512 KiB upwards from the front (ticket in claim order: never two threads
//                                inside pwrite), the side threads take B KiB downwards from the back,
//                                madvise(MADV_POPULATE_WRITE) the block and memcpy into it -- until the cursors meet
//   window=0                     the side threads' mapping covers one piece: mapped by the lane thread, unmapped by the
//                                last side thread that leaves the piece
//   window=W MiB                 long-lived windows of W MiB of the file, mapped by the lane thread when a piece first
//                                reaches one and unmapped by a side thread once every piece below its end is in the file
//
// One JSON line per process; tools/labs/side_lane_lab.sh interleaves the variants over five repetitions.  The first and
// the last frame are read back and checked.  pwrite_us_per_16MiB is the time inside pwrite per 16 MiB that went through
// pwrite: set against the pair's own figure it is what the side stream costs the lane.
//
//   g++ -O2 -std=c++17 tools/labs/side_lane_lab.cpp -o tools/labs/build/side_lane_lab -lpthread
//   side_lane_lab <dir> <lane 1|2> <side 0-3> <block KiB> <window MiB> [frames=6]
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <linux/futex.h>
#include <pthread.h>
#include <sched.h>
#include <string>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <thread>
#include <unistd.h>
#include <vector>

#ifndef MADV_POPULATE_WRITE
#define MADV_POPULATE_WRITE 23
#endif

static const size_t FRAME_BYTES = 280000000; // 10 M particles x 28 B
static const long long FIRST_OFFSET = 5416;  // 1320 mod 4096
static const size_t SLAB_BYTES = (size_t)16 << 20;
static const unsigned N_SLABS = 16;
static const size_t GRANULE = (size_t)256 << 10; // what the cursors count
static const size_t SUB_BYTES = (size_t)512 << 10; // the pair's sub-piece
static const long long PAGE = 4096;

static inline uint32_t pattern(uint64_t word)
    {
    return (uint32_t)(word * 2654435761ull) ^ (uint32_t)(word >> 13);
    }

static inline uint64_t now_ns()
    {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }

// a word that threads wait on: a bounded spin, then asleep in the kernel (as in pgsd_io.cpp)
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
            __builtin_ia32_pause();
            }
        sleepers.fetch_add(1);
        uint32_t v;
        while (!done(v = value.load()))
            syscall(SYS_futex, (uint32_t*)&value, FUTEX_WAIT_PRIVATE, v, nullptr, nullptr, 0);
        sleepers.fetch_sub(1);
        return v;
        }

    void wake()
        {
        if (sleepers.load() != 0)
            syscall(SYS_futex, (uint32_t*)&value, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
        }

    void post(uint32_t v)
        {
        value.store(v);
        wake();
        }

    void add(uint32_t n)
        {
        value.fetch_add(n);
        wake();
        }
    };

struct Piece
    {
    const char* src = nullptr;
    size_t bytes = 0;
    long long off = 0;
    long long a0 = 0, a1 = 0; // the claimed range of the file: whole pages with side threads, the whole piece without
    uint32_t ngran = 0;
    bool split = false; // head and tail cut off: the side threads may claim
    char* map = nullptr;                 // window=0: the mapping of [a0, a1)
    std::atomic<uint64_t> cursors {0};   // front | back << 32, in granules from a0
    WaitWord ticket;                     // claims of the pair that are in the file
    WaitWord done;                       // granules that are in the file
    std::atomic<uint32_t> sides_in {0};  // side threads that have not left the piece
    };

struct Lab
    {
    std::vector<Piece> pieces;
    int fd = -1;
    unsigned lane = 1, side = 0;
    size_t block = 0, window = 0;
    std::vector<std::atomic<char*>> win;
    std::atomic<uint32_t> retire_upto {0}, sides_running {0};
    WaitWord published; // pieces handed to the helper and the side threads
    std::atomic<int> error {0};
    std::atomic<uint64_t> pwrite_ns {0}, pwrite_bytes {0}, warm_ns {0}, wait_ns {0};
    std::atomic<uint64_t> side_bytes {0}, populate_ns {0}, copy_ns {0}, unmap_ns {0}, map_ns {0};
    std::atomic<uint64_t> sink {0};
    };

static void fail(Lab& L, int e)
    {
    int none = 0;
    L.error.compare_exchange_strong(none, e ? e : EIO);
    }

static void pwrite_timed(Lab& L, const char* p, size_t n, long long off)
    {
    if (n == 0 || L.error.load() != 0)
        return;
    const uint64_t t0 = now_ns();
    size_t done = 0;
    while (done < n)
        {
        ssize_t w = pwrite(L.fd, p + done, n - done, (off_t)(off + (long long)done));
        if (w < 0 && errno == EINTR)
            continue;
        if (w <= 0)
            {
            fail(L, errno);
            break;
            }
        done += (size_t)w;
        }
    L.pwrite_ns.fetch_add(now_ns() - t0);
    L.pwrite_bytes.fetch_add(n);
    }

static inline size_t gran_bytes(const Piece& p, uint32_t first, uint32_t n)
    {
    const size_t at = (size_t)first * GRANULE;
    return std::min((size_t)n * GRANULE, (size_t)(p.a1 - p.a0) - at);
    }

// the pair's half: claim SUB_BYTES from the front, read it into cache, wait for the turn, pwrite, pass the turn on
static void pair_run(Lab& L, Piece& p)
    {
    const uint32_t per = (uint32_t)(SUB_BYTES / GRANULE);
    for (;;)
        {
        uint64_t c = p.cursors.load();
        uint32_t front, n;
        for (;;)
            {
            front = (uint32_t)c;
            const uint32_t back = (uint32_t)(c >> 32);
            if (front >= back)
                return;
            n = std::min(per, back - front);
            if (p.cursors.compare_exchange_weak(c, (uint64_t)(front + n) | (uint64_t)back << 32))
                break;
            }
        const size_t at = (size_t)front * GRANULE, len = gran_bytes(p, front, n);
        const char* src = p.src + (size_t)(p.a0 - p.off) + at;
        const uint64_t t0 = now_ns();
        uint64_t acc = 0;
        for (const char* q = src; q < src + len; q = (const char*)(((uintptr_t)q | 63) + 1))
            acc += (unsigned char)*(const volatile char*)q;
        L.sink.fetch_add(acc, std::memory_order_relaxed);
        const uint64_t t1 = now_ns();
        const uint32_t turn = front / per; // every claim but a piece's last takes `per` granules
        p.ticket.wait([turn](uint32_t v) { return v == turn; });
        L.warm_ns.fetch_add(t1 - t0);
        L.wait_ns.fetch_add(now_ns() - t1);
        pwrite_timed(L, src, len, p.a0 + (long long)at);
        p.ticket.post(turn + 1);
        p.done.add(n);
        }
    }

static char* mapped_at(Lab& L, Piece& p, long long foff, size_t* room)
    {
    if (L.window == 0)
        {
        *room = (size_t)(p.a1 - foff);
        return p.map + (foff - p.a0);
        }
    const size_t w = (size_t)foff / L.window, in = (size_t)foff % L.window;
    *room = L.window - in;
    return L.win[w].load() + in;
    }

static void retire_windows(Lab& L, uint32_t upto)
    {
    for (uint32_t w = 0; w < upto; w++)
        if (L.win[w].load() != nullptr)
            if (char* m = L.win[w].exchange(nullptr))
                {
                const uint64_t t0 = now_ns();
                munmap(m, L.window);
                L.unmap_ns.fetch_add(now_ns() - t0);
                }
    }

static void side_thread(Lab& L)
    {
    const uint32_t per = (uint32_t)(L.block / GRANULE);
    for (uint32_t i = 0; i < L.pieces.size(); i++)
        {
        L.published.wait([i](uint32_t v) { return v > i; });
        if (L.window != 0)
            retire_windows(L, L.retire_upto.load());
        Piece& p = L.pieces[i];
        if (p.ngran == 0 || !p.split)
            continue;
        for (;;)
            {
            uint64_t c = p.cursors.load();
            uint32_t back, n;
            bool got = false;
            for (;;)
                {
                const uint32_t front = (uint32_t)c;
                back = (uint32_t)(c >> 32);
                if (front >= back)
                    break;
                n = std::min(per, back - front);
                if (p.cursors.compare_exchange_weak(c, (uint64_t)front | (uint64_t)(back - n) << 32))
                    {
                    got = true;
                    break;
                    }
                }
            if (!got)
                break;
            const uint32_t first = back - n;
            size_t len = gran_bytes(p, first, n);
            long long foff = p.a0 + (long long)first * (long long)GRANULE;
            L.side_bytes.fetch_add(len);
            while (len != 0 && L.error.load() == 0)
                {
                size_t room;
                char* dst = mapped_at(L, p, foff, &room);
                const size_t now = std::min(len, room);
                const uint64_t t0 = now_ns();
                if (madvise(dst, now, MADV_POPULATE_WRITE) != 0)
                    {
                    fail(L, errno);
                    break;
                    }
                const uint64_t t1 = now_ns();
                memcpy(dst, p.src + (size_t)(foff - p.off), now);
                L.populate_ns.fetch_add(t1 - t0);
                L.copy_ns.fetch_add(now_ns() - t1);
                foff += (long long)now;
                len -= now;
                }
            p.done.add(n);
            }
        if (L.window == 0 && p.sides_in.fetch_sub(1) == 1)
            {
            const uint64_t t0 = now_ns();
            munmap(p.map, (size_t)(p.a1 - p.a0));
            L.unmap_ns.fetch_add(now_ns() - t0);
            }
        }
    if (L.window != 0 && L.sides_running.fetch_sub(1) == 1) // the others may still copy into the last window
        retire_windows(L, (uint32_t)L.win.size());
    }

static void helper_thread(Lab& L)
    {
    for (uint32_t i = 0; i < L.pieces.size(); i++)
        {
        L.published.wait([i](uint32_t v) { return v > i; });
        if (L.pieces[i].ngran != 0)
            pair_run(L, L.pieces[i]);
        }
    }

static void lane_thread(Lab& L)
    {
    for (uint32_t i = 0; i < L.pieces.size(); i++)
        {
        Piece& p = L.pieces[i];
        const long long end = p.off + (long long)p.bytes;
        if (L.lane == 1)
            {
            pwrite_timed(L, p.src, p.bytes, p.off);
            continue;
            }
        if (L.side == 0)
            {
            p.a0 = p.off;
            p.a1 = end;
            }
        else
            {
            p.a0 = (p.off + PAGE - 1) & ~(PAGE - 1);
            p.a1 = (end - 1) & ~(PAGE - 1);
            if (p.a1 <= p.a0) // no whole page: the pair takes the piece as it is
                {
                p.a0 = p.off;
                p.a1 = end;
                }
            else
                {
                p.split = true;
                pwrite_timed(L, p.src + (size_t)(p.a1 - p.off), (size_t)(end - p.a1), p.a1); // end-of-file first
                pwrite_timed(L, p.src, (size_t)(p.a0 - p.off), p.off);
                const uint64_t t0 = now_ns();
                if (L.window == 0)
                    {
                    void* m = mmap(nullptr, (size_t)(p.a1 - p.a0), PROT_READ | PROT_WRITE, MAP_SHARED, L.fd, (off_t)p.a0);
                    if (m == MAP_FAILED)
                        fail(L, errno);
                    p.map = (char*)m;
                    p.sides_in.store(L.side);
                    }
                else
                    for (size_t w = (size_t)p.a0 / L.window; w <= (size_t)(p.a1 - 1) / L.window; w++)
                        if (L.win[w].load() == nullptr)
                            {
                            void* m = mmap(nullptr, L.window, PROT_READ | PROT_WRITE, MAP_SHARED, L.fd, (off_t)(w * L.window));
                            if (m == MAP_FAILED)
                                fail(L, errno);
                            L.win[w].store((char*)m);
                            }
                L.map_ns.fetch_add(now_ns() - t0);
                }
            }
        p.ngran = L.error.load() != 0 ? 0 : (uint32_t)(((size_t)(p.a1 - p.a0) + GRANULE - 1) / GRANULE);
        p.cursors.store((uint64_t)p.ngran << 32);
        L.published.post(i + 1);
        if (p.ngran != 0)
            pair_run(L, p);
        const uint32_t all = p.ngran;
        p.done.wait([all](uint32_t v) { return v == all; });
        if (L.window != 0)
            L.retire_upto.store((uint32_t)((size_t)end / L.window));
        }
    }

// ------------------------------------------------------------------ where the threads go
static bool read_text(const std::string& path, std::string* out)
    {
    FILE* f = fopen(path.c_str(), "r");
    if (!f)
        return false;
    char buf[4096];
    size_t n = fread(buf, 1, sizeof(buf) - 1, f);
    fclose(f);
    buf[n] = 0;
    *out = buf;
    return true;
    }

static std::vector<int> parse_cpulist(const char* buf, const cpu_set_t* allowed)
    {
    std::vector<int> out;
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
                out.push_back((int)c);
        if (*end != ',')
            break;
        p = end + 1;
        }
    return out;
    }

// `want` CPUs this process may use, no two of them hardware threads of one core: first those that share an L3 with the
// CPU this thread runs on (the pair takes the first two), then the rest of that CPU's NUMA node, then any
static std::vector<int> pick_cores(unsigned want)
    {
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    sched_getaffinity(0, sizeof(allowed), &allowed);
    const int here = sched_getcpu();
    const std::string cpu = "/sys/devices/system/cpu/cpu" + std::to_string(here);
    std::vector<int> order;
    std::string text;
    if (!read_text(cpu + "/cache/index3/shared_cpu_list", &text))
        return {};
    for (int c : parse_cpulist(text.c_str(), &allowed))
        order.push_back(c);
    for (int node = 0; node < 64; node++)
        if (read_text("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist", &text))
            {
            std::vector<int> on = parse_cpulist(text.c_str(), &allowed);
            if (std::find(on.begin(), on.end(), here) != on.end())
                order.insert(order.end(), on.begin(), on.end());
            }
    for (int c = 0; c < CPU_SETSIZE; c++)
        if (CPU_ISSET(c, &allowed))
            order.push_back(c);
    std::vector<int> picked;
    cpu_set_t taken;
    CPU_ZERO(&taken);
    for (int c : order)
        {
        if (picked.size() == want)
            break;
        if (CPU_ISSET(c, &taken))
            continue;
        picked.push_back(c);
        CPU_SET(c, &taken);
        cpu_set_t all;
        memset(&all, 0xff, sizeof(all));
        if (read_text("/sys/devices/system/cpu/cpu" + std::to_string(c) + "/topology/thread_siblings_list", &text))
            for (int s : parse_cpulist(text.c_str(), &all))
                CPU_SET(s, &taken);
        }
    if (picked.size() != want)
        return {};
    return picked;
    }

int main(int argc, char** argv)
    {
    if (argc < 6)
        {
        fprintf(stderr, "usage: %s <dir> <lane 1|2> <side 0-3> <block KiB> <window MiB> [frames=6]\n", argv[0]);
        return 2;
        }
    const std::string dir = argv[1];
    Lab L;
    L.lane = (unsigned)atoi(argv[2]);
    L.side = (unsigned)atoi(argv[3]);
    L.block = (size_t)atol(argv[4]) << 10;
    L.window = (size_t)atol(argv[5]) << 20;
    const unsigned frames = argc > 6 ? (unsigned)atoi(argv[6]) : 6;
    if (L.lane < 1 || L.lane > 2 || L.side > 3 || (L.side != 0 && (L.lane != 2 || L.block == 0 || L.block % GRANULE != 0)) || frames < 1)
        {
        fprintf(stderr, "lane 1-2, side 0-3 (with lane 2), block a multiple of 256 KiB\n");
        return 2;
        }

    // the source ring; every word says where in the ring it lies
    std::vector<char*> slab(N_SLABS);
    for (unsigned s = 0; s < N_SLABS; s++)
        {
        if (posix_memalign((void**)&slab[s], 4096, SLAB_BYTES) != 0)
            return 2;
        uint32_t* w = (uint32_t*)slab[s];
        for (size_t j = 0; j < SLAB_BYTES / 4; j++)
            w[j] = pattern((uint64_t)s * (SLAB_BYTES / 4) + j);
        }
    const size_t per_frame = (FRAME_BYTES + SLAB_BYTES - 1) / SLAB_BYTES;
    L.pieces = std::vector<Piece>(per_frame * frames);
    for (unsigned f = 0; f < frames; f++)
        for (size_t k = 0; k < per_frame; k++)
            {
            Piece& p = L.pieces[f * per_frame + k];
            p.src = slab[(f * per_frame + k) % N_SLABS];
            p.bytes = std::min(SLAB_BYTES, FRAME_BYTES - k * SLAB_BYTES);
            p.off = FIRST_OFFSET + (long long)f * (long long)FRAME_BYTES + (long long)(k * SLAB_BYTES);
            }
    const size_t file_end = (size_t)FIRST_OFFSET + (size_t)frames * FRAME_BYTES;
    if (L.window != 0)
        {
        L.win = std::vector<std::atomic<char*>>(file_end / L.window + 1);
        for (auto& w : L.win)
            w.store(nullptr);
        }

    const std::string path = dir + "/side_lane_lab." + std::to_string((long)getpid());
    L.fd = open(path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    if (L.fd < 0)
        {
        fprintf(stderr, "open %s: %s\n", path.c_str(), strerror(errno));
        return 2;
        }

    const unsigned n_threads = L.lane + L.side;
    std::vector<int> cores = n_threads > 1 ? pick_cores(n_threads) : std::vector<int>();
    auto pin = [&cores](std::thread& t, unsigned k)
        {
        if (cores.empty())
            return;
        cpu_set_t one;
        CPU_ZERO(&one);
        CPU_SET(cores[k], &one);
        (void)pthread_setaffinity_np(t.native_handle(), sizeof(one), &one);
        };

    L.sides_running.store(L.side);
    const uint64_t t0 = now_ns();
    std::vector<std::thread> th;
    th.emplace_back([&L] { lane_thread(L); });
    pin(th.back(), 0);
    if (L.lane == 2)
        {
        th.emplace_back([&L] { helper_thread(L); });
        pin(th.back(), 1);
        }
    for (unsigned s = 0; s < L.side; s++)
        {
        th.emplace_back([&L] { side_thread(L); });
        pin(th.back(), 2 + s);
        }
    th[0].join(); // the frames are in the file when the lane thread returns; unmapping the last window is not the lane's
    const double seconds = (double)(now_ns() - t0) * 1e-9;
    for (size_t t = 1; t < th.size(); t++)
        th[t].join();

    // the first and the last frame, read back
    bool same = L.error.load() == 0;
    std::vector<uint32_t> back(SLAB_BYTES / 4);
    for (unsigned f : {0u, frames - 1})
        for (size_t k = 0; same && k < per_frame; k++)
            {
            const Piece& p = L.pieces[f * per_frame + k];
            size_t got = 0;
            while (same && got < p.bytes)
                {
                ssize_t r = pread(L.fd, (char*)back.data() + got, p.bytes - got, (off_t)(p.off + (long long)got));
                if (r <= 0)
                    same = false;
                else
                    got += (size_t)r;
                }
            same = same && memcmp(back.data(), p.src, p.bytes) == 0;
            }
    close(L.fd);
    unlink(path.c_str());

    std::string core_list;
    for (int c : cores)
        core_list += (core_list.empty() ? "" : ",") + std::to_string(c);
    const double total = (double)frames * FRAME_BYTES;
    const double pw_bytes = (double)L.pwrite_bytes.load(), sd_bytes = (double)L.side_bytes.load();
    const double slab_us = (double)SLAB_BYTES * 1e-3;
    printf("{\"lab\": \"side_lane\", \"lane\": %u, \"side\": %u, \"block_KiB\": %zu, \"window_MiB\": %zu, \"frames\": %u, "
           "\"GBps\": %.3f, \"seconds\": %.4f, \"pwrite_us_per_16MiB\": %.0f, \"warm_us_per_16MiB\": %.0f, "
           "\"ticket_wait_us_per_16MiB\": %.0f, \"side_share\": %.3f, \"populate_us_per_16MiB\": %.0f, "
           "\"copy_us_per_16MiB\": %.0f, \"map_ms\": %.2f, \"unmap_ms\": %.2f, \"cores\": \"%s\", \"verified\": %s, \"errno\": %d}\n",
           L.lane, L.side, L.block >> 10, L.window >> 20, frames, total / seconds / 1e9, seconds,
           pw_bytes > 0 ? (double)L.pwrite_ns.load() / pw_bytes * slab_us : 0.0,
           pw_bytes > 0 ? (double)L.warm_ns.load() / pw_bytes * slab_us : 0.0,
           pw_bytes > 0 ? (double)L.wait_ns.load() / pw_bytes * slab_us : 0.0, sd_bytes / total,
           sd_bytes > 0 ? (double)L.populate_ns.load() / sd_bytes * slab_us : 0.0,
           sd_bytes > 0 ? (double)L.copy_ns.load() / sd_bytes * slab_us : 0.0, (double)L.map_ns.load() * 1e-6,
           (double)L.unmap_ns.load() * 1e-6, core_list.c_str(), same ? "true" : "false", L.error.load());
    return same ? 0 : 1;
    }
