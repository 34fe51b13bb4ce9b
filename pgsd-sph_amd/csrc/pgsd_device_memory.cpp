// pgsd_device_memory.cpp -- device memory owned by the library (pgsd.fl.DeviceBuffer): pgsd_device_alloc, pgsd_device_free,
// pgsd_device_copy.  They launch nothing: HIP runtime API only, built by the host compiler.
#include "pgsd_scratch.hpp"

using namespace pgsd_amd;

extern "C" void* pgsd_device_alloc(int device, size_t bytes, const void* pattern, size_t pattern_bytes)
    try
    {
    if (!pgsd_device_available())
        {
        set_last_error("pgsd_device_alloc: no HIP device visible (the HIP path has no CPU fallback)");
        return nullptr;
        }
    DeviceScope scope(device);
    if (!scope.ok())
        {
        set_last_error("pgsd_device_alloc: no device " + std::to_string(device));
        return nullptr;
        }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (e == hipSuccess && pattern && pattern_bytes > 0 && bytes > 0)
        {
        // the pattern repeated over a host image of at most 1 MiB (a multiple of the pattern), copied piecewise
        const size_t reps = std::max<size_t>(1, std::min<size_t>((1u << 20) / pattern_bytes, (bytes + pattern_bytes - 1) / pattern_bytes));
        std::vector<char> img(reps * pattern_bytes);
        for (size_t r = 0; r < reps; r++)
            memcpy(img.data() + r * pattern_bytes, pattern, pattern_bytes);
        for (size_t at = 0; at < bytes && e == hipSuccess; at += img.size())
            e = hipMemcpy((char*)p + at, img.data(), std::min(img.size(), bytes - at), hipMemcpyHostToDevice);
        }
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_device_alloc: ") + hipGetErrorString(e));
        if (p)
            (void)hipFree(p);
        p = nullptr;
        }
    return p;
    }
catch (...)
    {
        pgsd_amd::abi_guard();
        return nullptr;
    }

// pgsd_device_free and pgsd_device_copy go on where the switch to `device` is refused: neither hipFree nor a
// hipMemcpyDefault needs the memory's device to be current, so the runtime's answer to the operation itself is the result.
extern "C" int pgsd_device_free(int device, void* ptr)
    try
    {
    if (!ptr)
        return PGSD_SUCCESS;
    DeviceScope scope(device);
    const hipError_t e = hipFree(ptr);
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_device_free: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" int pgsd_device_copy(int device, void* dst, const void* src, size_t bytes)
    try
    {
    if (bytes == 0)
        return PGSD_SUCCESS;
    if (!dst || !src)
        return PGSD_ERROR_INVALID_ARGUMENT;
    DeviceScope scope(device);
    const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDefault); // either side may be host memory
    if (e != hipSuccess)
        {
        set_last_error(std::string("pgsd_device_copy: ") + hipGetErrorString(e));
        return PGSD_ERROR_DEVICE;
        }
    return PGSD_SUCCESS;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }
