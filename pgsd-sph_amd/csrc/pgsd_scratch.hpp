// pgsd_scratch.hpp -- the host-side scaffolding every GPU pass over staged chunks stands on (definitions: pgsd_scratch.cpp;
// HIP runtime API only, no kernel):
//   DeviceScope   switch to a device that is not current, restore the caller's on every way out
//   Scratch       a family's per-device, grow-only scratch space: one device allocation, optionally a pinned host block
//                 and a pinned, device-mapped block with its device alias
//   LaunchScope   what a synchronising launcher does around its kernels: the family's lock, the current device, the
//                 scratch space, a clean last-error slot on the way in; the runtime's and the stream's verdict on the way out
// The families keep one Scratch each and share two locks: g_select_lock covers the compaction (selections, row plan,
// pgsd_select_rows), the census and the cell order; the reductions of pgsd_stats.hip have their own, and so have the
// cell fields of pgsd_cells.hip, the neighbour census of pgsd_neighbours.hip, the neighbour lists of
// pgsd_neighbour_list.hip, the components of pgsd_components.hip, the component fields of
// pgsd_component_moments.hip, the SPH kernel sums of pgsd_sph.hip, the SPH kernel gradients of pgsd_sph_gradients.hip, the
// SPH gradient tensors of pgsd_sph_tensors.hip, the SPH sums with a per-particle smoothing length of pgsd_sph_adaptive.hip, the
// SPH accelerations of pgsd_sph_forces.hip and the SPH samples of pgsd_sph_samples.hip (each with a Scratch of its own).  Neither the
// locks nor the allocations are merged: that would change what may run concurrently and how much memory is held.
#ifndef PGSD_SCRATCH_HPP
#define PGSD_SCRATCH_HPP

#include "pgsd_kernels.hpp"

#include <hip/hip_runtime_api.h>

namespace pgsd_amd
    {
// `device` current for the scope's lifetime (a negative one, or the current one: nothing to do)
class DeviceScope
    {
    public:
    explicit DeviceScope(int device);
    ~DeviceScope();
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    bool ok() const // false: the switch was refused, the caller's device is still current
        {
        return m_ok;
        }
    int device() const // the device that is current inside the scope
        {
        return m_device;
        }

    private:
    int m_back = -1, m_device = -1;
    bool m_ok = true;
    };

class Scratch
    {
    public:
    struct Block
        {
        char* dev = nullptr;         // device memory, `cap` bytes
        size_t cap = 0;
        void* host = nullptr;        // pinned: the landing place of a device-to-host copy
        void* mapped = nullptr;      // pinned, device-mapped: words a kernel stores straight into host memory ...
        void* mapped_dev = nullptr;  // ... through this alias
        };

    // family: the name the allocation errors carry; room: what they call the device allocation.  A need beyond the
    // capacity is answered with max(need * factor, floor) bytes.  host_bytes / mapped_bytes: the pinned blocks (0: none).
    Scratch(const char* family, double factor, size_t floor, size_t host_bytes, size_t mapped_bytes,
            const char* room = "the scratch space")
        : m_family(family), m_room(room), m_factor(factor), m_floor(floor), m_host_bytes(host_bytes), m_mapped_bytes(mapped_bytes)
        {
        }

    // Room for `bytes` on `device` (current; the family's lock held).  A call that finds everything large enough
    // allocates nothing.  zero_head: that many bytes at the start of a FRESH device allocation are cleared.  On failure
    // what was half built is freed, the runtime's last-error slot is cleared, the library's last error names the family,
    // and PGSD_ERROR_MEMORY_ALLOCATION_FAILED is returned.
    int reserve(int device, size_t bytes, Block** out, size_t zero_head = 0);

    private:
    int fail(const char* what);
    const char *m_family, *m_room;
    double m_factor;
    size_t m_floor, m_host_bytes, m_mapped_bytes;
    std::map<int, Block> m_blocks;
    };

extern std::mutex g_select_lock;

// the size of one part of a scratch space: the part behind it starts on a 16-byte boundary
inline size_t round16(size_t bytes)
    {
    return (bytes + 15) & ~(size_t)15;
    }

// Whatever an earlier call of this thread left in the runtime's last-error slot (a failed hipMalloc, the caller's own
// calls, an unrelated launch) is not this launch's: the slot is read again right behind the launches.
inline void drop_stale_error()
    {
    (void)hipGetLastError();
    }

// PGSD_SUCCESS, or PGSD_ERROR_DEVICE with "<what>: <the runtime's text>" through launch_fail
int hip_check(hipError_t e, const char* what, std::string* err);

class LaunchScope
    {
    public:
    // device < 0: the current one; otherwise the scope switches to it and back (DeviceScope)
    LaunchScope(std::mutex& lock, Scratch& scratch, size_t bytes, hipStream_t stream, std::string* err, size_t zero_head = 0,
                int device = -1);
    int rc() const // not PGSD_SUCCESS: nothing may be launched; *err holds the message, if there is one
        {
        return m_rc;
        }
    const Scratch::Block& mem() const
        {
        return *m_mem;
        }
    int device() const // the device the scratch space is on: current inside the scope
        {
        return m_device.device();
        }
    hipStream_t stream() const
        {
        return m_stream;
        }
    // Behind the launches: the runtime's verdict on them, then the stream's.  When this returns PGSD_SUCCESS the kernels
    // are through and the pinned words are written.
    int finish(const char* what)
        {
        return finish(what, hipGetLastError());
        }
    // ... where the caller has read the runtime's verdict itself (memsets and copies around the launches): `e` is it
    int finish(const char* what, hipError_t e);

    private:
    std::lock_guard<std::mutex> m_guard;
    DeviceScope m_device;
    hipStream_t m_stream;
    std::string* m_err;
    Scratch::Block* m_mem = nullptr;
    int m_rc = PGSD_SUCCESS;
    };

// the first kernel of a code object, named once: the runtime loads the object now instead of at its first launch
void warm_kernel(const void* kernel);
    } // namespace pgsd_amd

#endif
