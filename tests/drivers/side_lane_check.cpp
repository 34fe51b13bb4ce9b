// tests/drivers/side_lane_check.cpp -- the side lane of pgsd_io.cpp (page insertions through a shared mapping beside the
// warm-then-write pair) driven with host buffers, as a plain program of its own (tests/test_side_lane.py builds it plainly,
// under ThreadSanitizer and under AddressSanitizer + UBSan).  No GPU.
//
//   side_lane_check <directory on tmpfs> [k]
//
// Pieces of one byte, 4095 bytes, two pages minus one byte (no whole block), two pages plus one byte, one block plus 16
// bytes, 64 pages minus 100 bytes and 8 MiB plus 16 bytes (long enough for the side threads to wake up and take
// part) go through writer_pool_submit / writer_pool_pwrite_warm with two side
// threads, 4 KiB sub-pieces and 8 KiB blocks -- each size at a page-aligned file offset, at 1320 mod 4096 and placed so
// that it ends exactly on a page boundary; one more piece lies across the boundary of two mapping windows (256 MiB).
// The file must equal one written with plain pwrite of the same bytes, end-of-file must never move backwards while the
// lane works (a thread watches it), bytes must have gone by the side lane and it must still be on.  With k, the k-th
// populate call reports failure: the same file, and the side lane is off afterwards.
//
// Exit 0 and "ok" on the last line, or a message and exit 1.
#include "pgsd_internal.hpp"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

using namespace pgsd_amd;

static const long long PAGE = 4096;
static const size_t SUB = 4096, BLOCK = 8192;
static const long long WINDOW = 256ll << 20;

static unsigned char value_of(size_t job, size_t i)
    {
    return (unsigned char)((i * 131 + (i >> 8) * 7 + job * 53 + 1) & 0xff);
    }

struct Job
    {
    long long offset;
    size_t bytes;
    };

static bool same_files(int a, int b, long long* at)
    {
    struct stat sa, sb;
    if (fstat(a, &sa) != 0 || fstat(b, &sb) != 0 || sa.st_size != sb.st_size)
        {
        *at = -1;
        return false;
        }
    std::vector<char> x(1 << 20), y(1 << 20);
    for (long long off = 0; off < sa.st_size; off += (long long)x.size())
        {
        const ssize_t n = pread(a, x.data(), x.size(), off), m = pread(b, y.data(), y.size(), off);
        if (n <= 0 || n != m || memcmp(x.data(), y.data(), (size_t)n) != 0)
            {
            *at = off;
            return false;
            }
        }
    return true;
    }

int main(int argc, char** argv)
    {
    if (argc < 2)
        {
        fprintf(stderr, "usage: %s <directory on tmpfs> [failing populate call]\n", argv[0]);
        return 2;
        }
    const long fail_at = argc > 2 ? atol(argv[2]) : -1;
    const std::string lane_path = std::string(argv[1]) + "/side_lane.bin", plain_path = std::string(argv[1]) + "/plain.bin";
    const int fd = open(lane_path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    const int plain = open(plain_path.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
    if (fd < 0 || plain < 0)
        {
        perror("open");
        return 2;
        }
    WriterPool* pool = writer_pool_create(1);
    if (!writer_pool_enable_warm(pool, SUB, nullptr, false))
        {
        printf("the pool refused the pair\n");
        return 1;
        }
    if (!writer_pool_enable_side(pool, fd, 2, BLOCK, nullptr, fail_at))
        {
        printf("the pool refused the side lane (is %s on tmpfs?)\n", argv[1]);
        return 1;
        }

    const size_t sizes[] = {1, 4095, 2 * 4096 - 1, 2 * 4096 + 1, BLOCK + 16, 64 * 4096 - 100, 2048 * 4096 + 16};
    std::vector<Job> jobs;
    long long cursor = 0;
    for (int mode = 0; mode < 3; mode++)
        for (size_t bytes : sizes)
            {
            const long long up = (cursor + PAGE - 1) / PAGE * PAGE;
            const long long offset = mode == 0 ? up : mode == 1 ? up + 1320 : (cursor + (long long)bytes + PAGE - 1) / PAGE * PAGE - (long long)bytes;
            jobs.push_back({offset, bytes});
            cursor = offset + (long long)bytes;
            }
    jobs.push_back({WINDOW - 5 * PAGE + 1320, 64 * 4096}); // the file is sparse below it

    std::vector<std::vector<unsigned char>> buffers(jobs.size());
    std::vector<std::atomic<int>> rc(jobs.size());
    for (size_t j = 0; j < jobs.size(); j++)
        {
        buffers[j].resize(jobs[j].bytes);
        for (size_t i = 0; i < jobs[j].bytes; i++)
            buffers[j][i] = value_of(j, i);
        rc[j].store(1);
        }

    std::atomic<bool> stop {false};
    std::atomic<int> went_back {0};
    std::thread watcher(
        [&]
        {
            long long seen = 0;
            while (!stop.load())
                {
                struct stat st;
                if (fstat(fd, &st) == 0)
                    {
                    if ((long long)st.st_size < seen)
                        went_back.fetch_add(1);
                    seen = std::max(seen, (long long)st.st_size);
                    }
                }
        });
    for (size_t j = 0; j < jobs.size(); j++)
        writer_pool_submit(pool,
                           [&, j]
                           {
                               double ms = -1;
                               rc[j].store(writer_pool_pwrite_warm(pool, fd, buffers[j].data(), jobs[j].bytes, jobs[j].offset, false, &ms));
                               if (ms < 0)
                                   rc[j].store(-EDOM); // the time inside pwrite was not reported
                           });
    uint64_t side_bytes = 0;
    double side_ms = 0;
    bool side_on = false;
    // (behind everything queued: a job of the lane)
    writer_pool_submit(pool,
                       [&]
                       {
                           writer_pool_side_counters(pool, &side_bytes, &side_ms, &side_on);
                           writer_pool_side_drop(pool);
                       });
    writer_pool_destroy(pool); // runs what is queued, joins the lane's threads
    stop.store(true);
    watcher.join();

    int bad = 0;
    size_t total = 0;
    for (size_t j = 0; j < jobs.size(); j++)
        {
        total += jobs[j].bytes;
        if (rc[j].load() != 0)
            bad += printf("job %zu: returned %d\n", j, rc[j].load());
        if (pwrite_full(plain, buffers[j].data(), jobs[j].bytes, jobs[j].offset) != 0)
            bad += printf("job %zu: the plain pwrite failed\n", j);
        }
    long long at = 0;
    if (!same_files(fd, plain, &at))
        bad += printf("the file differs from the plainly written one (%lld)\n", at);
    if (went_back.load() != 0)
        bad += printf("end-of-file moved backwards %d times\n", went_back.load());
    printf("side lane: %llu of %zu bytes, still on: %d\n", (unsigned long long)side_bytes, total, (int)side_on);
    if (fail_at < 0 && (side_bytes == 0 || !side_on))
        bad += printf("no bytes went by the side lane, or it switched itself off\n");
    if (fail_at >= 0 && side_on)
        bad += printf("the side lane is still on after a failed populate\n");
    if (side_bytes >= total)
        bad += printf("the side lane claims more than whole pages\n");
    close(fd);
    close(plain);
    unlink(lane_path.c_str());
    unlink(plain_path.c_str());
    if (bad)
        return 1;
    printf("ok\n");
    return 0;
    }
