// tools/labs/warm_write_lab.hip -- does it pay to pull a slab piece into cache before its pwrite?  (DESIGN section 5,
// "End-to-end bound".)
//
// The device writer's frame is one thread inside pwrite: per 4 KiB page the kernel allocates and inserts a page (needs
// the file's inode lock) and copies into it from a pinned slab whose lines the GPU's PCIe writes left in DRAM (needs no
// lock, but is done under it).  This lab lands `frames` frames of 280 MB in one fresh file the way the pipeline does --
// a dispatcher refills a ring of 16 pinned 16 MiB slabs from device memory with hipMemcpyAsync, an ordered lane writes
// each piece when its copy event has fired -- with the lane built one of these ways per process:
//
//   threads=1 warm=0               the pipeline's writer today: one thread, one pwrite per 16 MiB piece
//   threads=2|3 warm=1 sub=S       each piece cut into sub-pieces of S KiB that the threads take in turn: a thread
//                                  touches its sub-piece with one load per 64-byte line, waits for its turn on a ticket
//                                  (bounded spin, then futex), pwrites it and passes the ticket on.  Never are two
//                                  threads inside pwrite; the threads sit on distinct cores that share an L3
//   congruent=1                    the piece lies in its slab at (file offset mod 4096), so that every page copy of the
//                                  kernel reads a page-aligned source (the device side of the copy keeps its alignment)
//
// One JSON line per process; tools/labs/warm_write_lab.sh interleaves the variants over three repetitions, each process
// under its own time limit, and prints mean and range.  The first and the last frame are read back and checked.
//
//   hipcc -O2 --offload-arch=gfx950 tools/labs/warm_write_lab.hip -o tools/labs/build/warm_write_lab -lpthread
//   warm_write_lab <dir> <threads> <sub KiB> <warm 0|1> <congruent 0|1> [frames=6]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <climits>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fcntl.h>
#include <linux/futex.h>
#include <mutex>
#include <pthread.h>
#include <sched.h>
#include <string>
#include <sys/syscall.h>
#include <thread>
#include <unistd.h>
#include <vector>

#define CK(x)                                                                                 \
    do                                                                                        \
        {                                                                                     \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess)                                                                 \
            {                                                                                 \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            exit(2);                                                                          \
            }                                                                                 \
        } while (0)

static const size_t FRAME_BYTES = 280000000;      // 10 M particles x 28 B
static const long long FIRST_OFFSET = 5416;       // frame k starts at 5416 + k x 280 MB: 1 400 005 416 for k = 5
static const size_t SLAB_BYTES = (size_t)16 << 20;
static const unsigned N_SLABS = 16;

static inline uint32_t pattern(uint64_t word)
    {
    return (uint32_t)(word * 2654435761ull) ^ (uint32_t)(word >> 13);
    }

__global__ void fill_kernel(uint32_t* dst, uint64_t words)
    {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x)
        dst[i] = (uint32_t)(i * 2654435761ull) ^ (uint32_t)(i >> 13);
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

// "0-7,64-71" -> the CPUs of the list that are also in `allowed`
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
            if (CPU_ISSET((int)c, allowed) && !CPU_ISSET((int)c, out))
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

// CPUs this process may use that lie on the GPU's NUMA node (all it may use where the node is unknown or has none of them)
static bool node_cpus(int device, cpu_set_t* out)
    {
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    sched_getaffinity(0, sizeof(allowed), &allowed);
    *out = allowed;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), device) != hipSuccess)
        return false;
    for (char* c = bdf; *c; c++)
        *c = (char)tolower((unsigned char)*c);
    std::string text;
    if (!read_text(std::string("/sys/bus/pci/devices/") + bdf + "/numa_node", &text) || atoi(text.c_str()) < 0)
        return false;
    const int node = atoi(text.c_str());
    if (!read_text("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist", &text))
        return false;
    cpu_set_t on_node;
    if (parse_cpulist(text.c_str(), &allowed, &on_node) == 0)
        return false;
    *out = on_node;
    return true;
    }

// `want` CPUs of `from` that share one L3 and are no hardware threads of one core; empty where sysfs does not say
static std::vector<int> l3_sharing_cores(const cpu_set_t* from, unsigned want, std::string* l3_list)
    {
    cpu_set_t tried;
    CPU_ZERO(&tried);
    for (int c = 0; c < CPU_SETSIZE; c++)
        {
        if (!CPU_ISSET(c, from) || CPU_ISSET(c, &tried))
            continue;
        std::string text;
        const std::string cpu = "/sys/devices/system/cpu/cpu" + std::to_string(c);
        if (!read_text(cpu + "/cache/index3/shared_cpu_list", &text))
            return {};
        cpu_set_t group;
        parse_cpulist(text.c_str(), from, &group);
        CPU_OR(&tried, &tried, &group);
        std::vector<int> picked;
        cpu_set_t siblings_taken;
        CPU_ZERO(&siblings_taken);
        for (int k = 0; k < CPU_SETSIZE && picked.size() < want; k++)
            {
            if (!CPU_ISSET(k, &group) || CPU_ISSET(k, &siblings_taken))
                continue;
            picked.push_back(k);
            std::string sib;
            cpu_set_t all, s;
            memset(&all, 0xff, sizeof(all));
            if (read_text("/sys/devices/system/cpu/cpu" + std::to_string(k) + "/topology/thread_siblings_list", &sib))
                {
                parse_cpulist(sib.c_str(), &all, &s);
                CPU_OR(&siblings_taken, &siblings_taken, &s);
                }
            }
        if (picked.size() == want)
            {
            while (!text.empty() && (text.back() == '\n' || text.back() == ' '))
                text.pop_back();
            *l3_list = text;
            return picked;
            }
        }
    return {};
    }

// ------------------------------------------------------------------ the lane
struct Sub
    {
    uint32_t piece;    // which piece of the run
    size_t slab_off;   // where in the slab
    size_t len;
    long long foff;
    bool last;         // the piece's last sub-piece: the slab goes back behind it
    };

struct Piece
    {
    size_t dev_off, shift, n;
    int slab;
    };

struct Lane
    {
    std::vector<Piece> pieces;
    std::vector<Sub> subs;
    char* slab[N_SLABS];
    hipEvent_t copied[N_SLABS];
    std::mutex m;
    std::condition_variable cv_free, cv_dispatched;
    std::deque<int> free_slabs;
    uint32_t dispatched = 0;
    std::atomic<uint32_t> ticket {0};
    std::atomic<uint32_t> sleepers {0};
    std::atomic<int> error {0};
    int fd = -1;
    bool warm = false;
    unsigned threads = 1;
    double warm_us[8] = {0}, wait_us[8] = {0}, pwrite_us[8] = {0};
    uint64_t slept[8] = {0};
    };

static inline double now_us()
    {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }

static uint64_t touch_lines(const char* p, size_t n)
    {
    const char* q = (const char*)((uintptr_t)p & ~(uintptr_t)63);
    uint64_t acc = 0;
    for (; q < p + n; q += 64)
        acc += *(const volatile uint64_t*)q;
    return acc;
    }

static void wait_turn(Lane& L, uint32_t mine, unsigned t)
    {
    for (int spin = 0; spin < 4000; spin++)
        {
        if (L.ticket.load(std::memory_order_acquire) == mine)
            return;
        __builtin_ia32_pause();
        }
    L.sleepers.fetch_add(1);
    for (uint32_t v; (v = L.ticket.load()) != mine;)
        {
        L.slept[t]++;
        syscall(SYS_futex, (uint32_t*)&L.ticket, FUTEX_WAIT_PRIVATE, v, nullptr, nullptr, 0);
        }
    L.sleepers.fetch_sub(1);
    }

static void pass_turn(Lane& L, uint32_t mine)
    {
    L.ticket.store(mine + 1);
    if (L.sleepers.load() != 0)
        syscall(SYS_futex, (uint32_t*)&L.ticket, FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
    }

static void lane_thread(Lane& L, unsigned t, int device)
    {
    CK(hipSetDevice(device));
    uint32_t synced = UINT32_MAX;
    uint64_t sink = 0;
    for (uint32_t g = t; g < L.subs.size(); g += L.threads)
        {
        const Sub& s = L.subs[g];
        int si;
            {
            std::unique_lock<std::mutex> lk(L.m);
            L.cv_dispatched.wait(lk, [&] { return L.dispatched > s.piece; });
            si = L.pieces[s.piece].slab;
            }
        if (synced != s.piece)
            {
            CK(hipEventSynchronize(L.copied[si]));
            synced = s.piece;
            }
        const char* src = L.slab[si] + s.slab_off;
        double t0 = now_us();
        if (L.warm)
            sink += touch_lines(src, s.len);
        double t1 = now_us();
        wait_turn(L, g, t);
        double t2 = now_us();
        if (L.error.load() == 0)
            {
            size_t done = 0;
            while (done < s.len)
                {
                ssize_t w = pwrite(L.fd, src + done, s.len - done, (off_t)(s.foff + (long long)done));
                if (w < 0 && errno == EINTR)
                    continue;
                if (w <= 0)
                    {
                    L.error.store(errno ? errno : EIO);
                    break;
                    }
                done += (size_t)w;
                }
            }
        double t3 = now_us();
        pass_turn(L, g);
        if (s.last)
            {
                {
                std::lock_guard<std::mutex> lk(L.m);
                L.free_slabs.push_back(si);
                }
            L.cv_free.notify_all();
            }
        L.warm_us[t] += t1 - t0;
        L.wait_us[t] += t2 - t1;
        L.pwrite_us[t] += t3 - t2;
        }
    if (sink == 0x5a5a5a5a5a5a5a5aull)
        fprintf(stderr, "\n");
    }

int main(int argc, char** argv)
    {
    if (argc < 6)
        {
        fprintf(stderr, "usage: %s <dir> <threads 1-3> <sub KiB> <warm 0|1> <congruent 0|1> [frames=6]\n", argv[0]);
        return 2;
        }
    const std::string dir = argv[1];
    Lane L;
    L.threads = (unsigned)atoi(argv[2]);
    const size_t sub_bytes = (size_t)atol(argv[3]) << 10;
    L.warm = atoi(argv[4]) != 0;
    const bool congruent = atoi(argv[5]) != 0;
    const unsigned frames = argc > 6 ? (unsigned)atoi(argv[6]) : 6;
    if (L.threads < 1 || L.threads > 3 || sub_bytes < 4096 || sub_bytes % 4096 != 0 || frames < 1)
        {
        fprintf(stderr, "threads 1-3, sub-piece a multiple of 4 KiB\n");
        return 2;
        }
    const int device = 0;
    CK(hipSetDevice(device));

    // placement: everything on the GPU's node; the lane's threads on L3-sharing cores when there are several
    cpu_set_t node;
    const bool on_node = node_cpus(device, &node);
    std::string l3_list;
    std::vector<int> cores;
    if (L.threads > 1)
        {
        cores = l3_sharing_cores(&node, L.threads, &l3_list);
        if (cores.empty())
            {
            fprintf(stderr, "no %u cores that share an L3 among the CPUs this process may use\n", L.threads);
            return 3;
            }
        }
    (void)pthread_setaffinity_np(pthread_self(), sizeof(node), &node);

    uint32_t* dev = nullptr;
    const uint64_t words = FRAME_BYTES / 4;
    CK(hipMalloc(&dev, FRAME_BYTES));
    fill_kernel<<<1024, 256>>>(dev, words);
    CK(hipDeviceSynchronize());
    hipStream_t copy_stream;
    CK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    for (unsigned i = 0; i < N_SLABS; i++)
        {
        CK(hipHostMalloc((void**)&L.slab[i], SLAB_BYTES, hipHostMallocDefault));
        CK(hipEventCreateWithFlags(&L.copied[i], hipEventDisableTiming));
        L.free_slabs.push_back((int)i);
        }

    // the run's pieces and sub-pieces
    for (unsigned f = 0; f < frames; f++)
        for (size_t off = 0; off < FRAME_BYTES;)
            {
            const long long foff = FIRST_OFFSET + (long long)f * (long long)FRAME_BYTES + (long long)off;
            Piece p;
            p.dev_off = off;
            p.shift = congruent ? (size_t)(foff % 4096) : 0;
            p.n = std::min(SLAB_BYTES - p.shift, FRAME_BYTES - off);
            p.slab = -1;
            const size_t cut = L.threads == 1 && !L.warm ? SLAB_BYTES : sub_bytes;
            for (size_t at = p.shift; at < p.shift + p.n;)
                {
                const size_t end = std::min(p.shift + p.n, (at / cut + 1) * cut);
                L.subs.push_back({(uint32_t)L.pieces.size(), at, end - at, foff + (long long)(at - p.shift), end == p.shift + p.n});
                at = end;
                }
            L.pieces.push_back(p);
            off += p.n;
            }

    const std::string path = dir + "/warm_write_lab." + std::to_string((long)getpid());
    L.fd = open(path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    if (L.fd < 0)
        {
        fprintf(stderr, "open %s: %s\n", path.c_str(), strerror(errno));
        return 2;
        }

    const double t0 = now_us();
    std::vector<std::thread> th;
    for (unsigned t = 0; t < L.threads; t++)
        {
        th.emplace_back([&L, t] { lane_thread(L, t, device); });
        cpu_set_t one;
        CPU_ZERO(&one);
        if (!cores.empty())
            CPU_SET(cores[t], &one);
        (void)pthread_setaffinity_np(th.back().native_handle(), sizeof(cpu_set_t), cores.empty() ? &node : &one);
        }
    // the dispatcher: one hipMemcpyAsync per piece into a free slab, as DevicePipeline::dispatch_loop does
    for (uint32_t i = 0; i < L.pieces.size(); i++)
        {
        Piece& p = L.pieces[i];
        int si;
            {
            std::unique_lock<std::mutex> lk(L.m);
            L.cv_free.wait(lk, [&] { return !L.free_slabs.empty(); });
            si = L.free_slabs.front();
            L.free_slabs.pop_front();
            }
        CK(hipMemcpyAsync(L.slab[si] + p.shift, (const char*)dev + p.dev_off, p.n, hipMemcpyDeviceToHost, copy_stream));
        CK(hipEventRecord(L.copied[si], copy_stream));
            {
            std::lock_guard<std::mutex> lk(L.m);
            p.slab = si;
            L.dispatched = i + 1;
            }
        L.cv_dispatched.notify_all();
        }
    for (auto& t : th)
        t.join();
    const double seconds = (now_us() - t0) * 1e-6;

    // the first and the last frame, read back
    bool same = L.error.load() == 0;
    std::vector<uint32_t> back(FRAME_BYTES / 4);
    for (unsigned f : {0u, frames - 1})
        {
        size_t got = 0;
        while (same && got < FRAME_BYTES)
            {
            ssize_t r = pread(L.fd, (char*)back.data() + got, FRAME_BYTES - got, (off_t)(FIRST_OFFSET + (long long)f * (long long)FRAME_BYTES + (long long)got));
            if (r <= 0)
                same = false;
            else
                got += (size_t)r;
            }
        for (uint64_t i = 0; same && i < words; i++)
            same = back[i] == pattern(i);
        }
    close(L.fd);
    unlink(path.c_str());

    double warm = 0, wait = 0, pw = 0;
    uint64_t slept = 0;
    for (unsigned t = 0; t < L.threads; t++)
        {
        warm += L.warm_us[t];
        wait += L.wait_us[t];
        pw += L.pwrite_us[t];
        slept += L.slept[t];
        }
    std::string core_list;
    for (int c : cores)
        core_list += (core_list.empty() ? "" : ",") + std::to_string(c);
    const double total = (double)frames * FRAME_BYTES;
    printf("{\"lab\": \"warm_write\", \"threads\": %u, \"sub_KiB\": %zu, \"warm\": %d, \"congruent\": %d, \"frames\": %u, "
           "\"GBps\": %.3f, \"seconds\": %.4f, \"pwrite_us_per_16MiB\": %.0f, \"warm_us_per_16MiB\": %.0f, "
           "\"ticket_wait_us_per_16MiB\": %.0f, \"futex_sleeps\": %llu, \"sub_pieces\": %zu, \"on_gpu_node\": %s, "
           "\"cores\": \"%s\", \"l3\": \"%s\", \"verified\": %s, \"errno\": %d}\n",
           L.threads, L.threads == 1 && !L.warm ? SLAB_BYTES >> 10 : sub_bytes >> 10, (int)L.warm, (int)congruent, frames,
           total / seconds / 1e9, seconds, pw / total * SLAB_BYTES, warm / total * SLAB_BYTES, wait / total * SLAB_BYTES,
           (unsigned long long)slept, L.subs.size(), on_node ? "true" : "false", core_list.c_str(), l3_list.c_str(),
           same ? "true" : "false", L.error.load());
    return same ? 0 : 1;
    }
