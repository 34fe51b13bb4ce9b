// tests/drivers/writer_lane_check.cpp -- the warm-then-write pair of pgsd_io.cpp driven with host buffers, as a plain
// program of its own (tests/test_writer_lane.py builds it under ThreadSanitizer and under AddressSanitizer + UBSan).
//
//   writer_lane_check file <path>   64 sub-pieces of 4 KiB per piece: three pieces that overlap in the file, with a plain
//                                   write between them, all through writer_pool_submit.  The file's content shows the
//                                   submission order; every buffer is released once
//   writer_lane_check full          the same pieces into /dev/full: every pwrite fails with ENOSPC.  Each piece must
//                                   return -ENOSPC, release its buffer once, and the pool must shut down
//
// Exit 0 and "ok" on the last line, or a message and exit 1.
#include "pgsd_internal.hpp"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <fcntl.h>
#include <unistd.h>
#include <vector>

using namespace pgsd_amd;

static const size_t SUB = 4096;
static const size_t PIECE = 64 * SUB - 100; // 64 sub-pieces, the last one short

static unsigned char value_of(int job, size_t i)
    {
    return (unsigned char)((i * 131 + (i >> 8) * 7 + (size_t)job * 53) & 0xff);
    }

int main(int argc, char** argv)
    {
    const bool full = argc > 1 && strcmp(argv[1], "full") == 0;
    if (argc < 2 || (!full && argc < 3))
        {
        fprintf(stderr, "usage: %s file <path> | full\n", argv[0]);
        return 2;
        }
    const int fd = full ? open("/dev/full", O_WRONLY) : open(argv[2], O_CREAT | O_TRUNC | O_RDWR, 0644);
    if (fd < 0)
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
    // job 0, 2, 3: pieces through the pair; job 1: a plain write inside job 0's range, which job 2 half covers again
    struct Job
        {
        int id;
        long long offset;
        size_t bytes;
        bool pair;
        };
    const std::vector<Job> jobs = {{0, 808, PIECE, true}, {1, 808 + 5000, 9000, false}, {2, 808 + 10000, PIECE, true},
                                   {3, 808 + 10000 + (long long)PIECE - 3 * SUB, PIECE, true}};
    std::vector<std::vector<unsigned char>> buffers(jobs.size());
    std::vector<std::atomic<int>> released(jobs.size()), rc(jobs.size());
    for (size_t j = 0; j < jobs.size(); j++)
        {
        buffers[j].resize(jobs[j].bytes);
        for (size_t i = 0; i < jobs[j].bytes; i++)
            buffers[j][i] = value_of(jobs[j].id, i);
        released[j].store(0);
        rc[j].store(1);
        }
    for (size_t j = 0; j < jobs.size(); j++)
        writer_pool_submit(pool,
                           [&, j]
                           {
                               double ms = -1;
                               const Job& job = jobs[j];
                               rc[j].store(job.pair ? writer_pool_pwrite_warm(pool, fd, buffers[j].data(), job.bytes, job.offset, false, &ms)
                                                    : pwrite_locked(fd, buffers[j].data(), job.bytes, job.offset, false));
                               if (job.pair && ms < 0)
                                   rc[j].store(-EDOM); // the time inside pwrite was not reported
                               released[j].fetch_add(1);
                           });
    writer_pool_destroy(pool); // runs what is queued, joins the lane thread and the helper

    int bad = 0;
    for (size_t j = 0; j < jobs.size(); j++)
        {
        if (released[j].load() != 1)
            bad += printf("job %zu: buffer released %d times\n", j, released[j].load());
        if (rc[j].load() != (full ? -ENOSPC : 0))
            bad += printf("job %zu: returned %d\n", j, rc[j].load());
        }
    if (!full)
        {
        // the model: the jobs applied in submission order
        long long end = 0;
        for (const Job& job : jobs)
            end = std::max(end, job.offset + (long long)job.bytes);
        std::vector<unsigned char> want((size_t)end, 0), got((size_t)end + 1, 0);
        for (const Job& job : jobs)
            for (size_t i = 0; i < job.bytes; i++)
                want[(size_t)job.offset + i] = value_of(job.id, i);
        const ssize_t n = pread(fd, got.data(), got.size(), 0);
        if (n != (ssize_t)end)
            bad += printf("the file holds %zd bytes, not %lld\n", n, end);
        else if (memcmp(got.data(), want.data(), (size_t)end) != 0)
            {
            size_t at = 0;
            while (got[at] == want[at])
                at++;
            bad += printf("the file differs from the model at byte %zu\n", at);
            }
        }
    close(fd);
    if (bad)
        return 1;
    printf("ok\n");
    return 0;
    }
