// pgsd_scratch.cpp -- DeviceScope, Scratch and LaunchScope (pgsd_scratch.hpp).  HIP runtime API only: the host compiler
// builds it.
#include "pgsd_scratch.hpp"

namespace pgsd_amd
    {
std::mutex g_select_lock;

DeviceScope::DeviceScope(int device)
    {
    if (hipGetDevice(&m_back) != hipSuccess)
        m_back = -1;
    m_device = m_back;
    if (device >= 0 && device != m_back)
        {
        if (hipSetDevice(device) == hipSuccess)
            m_device = device;
        else
            m_ok = false;
        }
    if (m_device < 0)
        m_ok = false; // no current device and none asked for
    }

DeviceScope::~DeviceScope()
    {
    if (m_back >= 0 && m_device != m_back)
        (void)hipSetDevice(m_back);
    }

int Scratch::fail(const char* what)
    {
    (void)hipGetLastError();
    set_last_error(std::string(m_family) + ": cannot allocate " + what);
    return PGSD_ERROR_MEMORY_ALLOCATION_FAILED;
    }

int Scratch::reserve(int device, size_t bytes, Block** out, size_t zero_head)
    {
    Block& b = m_blocks[device];
    if (bytes > b.cap)
        {
        if (b.dev)
            (void)hipFree(b.dev);
        b.dev = nullptr;
        b.cap = 0;
        const size_t cap = std::max((size_t)((double)bytes * m_factor), m_floor); // (exact: sizes stay far below 2^53)
        if (hipMalloc((void**)&b.dev, cap) != hipSuccess || (zero_head && hipMemset(b.dev, 0, zero_head) != hipSuccess))
            {
            if (b.dev)
                (void)hipFree(b.dev);
            b.dev = nullptr;
            return fail(m_room);
            }
        b.cap = cap;
        }
    if (m_host_bytes && !b.host && hipHostMalloc(&b.host, m_host_bytes, hipHostMallocDefault) != hipSuccess)
        {
        b.host = nullptr;
        return fail("pinned memory");
        }
    if (m_mapped_bytes && !b.mapped)
        {
        if (hipHostMalloc(&b.mapped, m_mapped_bytes, hipHostMallocMapped) != hipSuccess
            || hipHostGetDevicePointer(&b.mapped_dev, b.mapped, 0) != hipSuccess)
            {
            if (b.mapped)
                (void)hipHostFree(b.mapped);
            b.mapped = b.mapped_dev = nullptr;
            return fail("pinned memory");
            }
        }
    *out = &b;
    return PGSD_SUCCESS;
    }

int hip_check(hipError_t e, const char* what, std::string* err)
    {
    if (e == hipSuccess)
        return PGSD_SUCCESS;
    return launch_fail(err, PGSD_ERROR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    }

LaunchScope::LaunchScope(std::mutex& lock, Scratch& scratch, size_t bytes, hipStream_t stream, std::string* err,
                         size_t zero_head, int device)
    : m_guard(lock), m_device(device), m_stream(stream), m_err(err)
    {
    if (!m_device.ok())
        {
        m_rc = PGSD_ERROR_DEVICE;
        return;
        }
    m_rc = scratch.reserve(m_device.device(), bytes, &m_mem, zero_head);
    if (m_rc != PGSD_SUCCESS)
        launch_fail(err, m_rc, last_error());
    else
        drop_stale_error();
    }

int LaunchScope::finish(const char* what, hipError_t e)
    {
    if (e == hipSuccess)
        e = hipStreamSynchronize(m_stream);
    return hip_check(e, what, m_err);
    }

void warm_kernel(const void* kernel)
    {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, kernel);
    (void)hipGetLastError();
    }
    } // namespace pgsd_amd
