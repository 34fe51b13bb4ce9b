// pgsd_kernels.cpp -- the host side the kernel files share (declarations: pgsd_kernels.hpp, pgsd_pack.hpp): the tuning
// variables of all three of them, the device's CU count, the conversion class of a type pair, the tile geometry of the
// LDS-tiled launches and the exports that launch nothing.  No kernel here: the host compiler builds it.
#include "pgsd_kernels.hpp"

#include <climits>

namespace pgsd_amd
    {
uint32_t conv_kind(uint32_t src_type, uint32_t dst_type, uint32_t bitcast)
    {
    const bool s_int = src_type <= PGSD_TYPE_INT64, d_int = dst_type <= PGSD_TYPE_INT64;
    const size_t ssz = sizeof_type(src_type), dsz = sizeof_type(dst_type);
    if (bitcast || src_type == dst_type)
        return PACK_BITS;
    if (s_int && d_int)
        {
        const bool s_signed = src_type >= PGSD_TYPE_INT8;
        return (dsz > ssz && s_signed) ? PACK_SEXT : PACK_BITS;
        }
    if (!s_int && !d_int)
        return PACK_F2F;
    // integer -> float (checked by the caller: source <= 32 bit)
    return src_type >= PGSD_TYPE_INT8 ? PACK_S2F : PACK_U2F;
    }

uint64_t pack_algorithmic_bytes_in(const pgsd_pack_job& j, uint64_t N)
    {
    return N * (uint64_t)j.M * sizeof_type(j.src.src_type) + (j.src.order ? N * 4 : 0);
    }

uint64_t pack_bytes_out(const pgsd_pack_job& j, uint64_t N)
    {
    return N * (uint64_t)j.M * sizeof_type(j.dst_type);
    }

int num_cus()
    {
    static int g_num_cus = 0;
    if (g_num_cus == 0)
        {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            g_num_cus = prop.multiProcessorCount;
        if (g_num_cus <= 0)
            g_num_cus = 256;
        }
    return g_num_cus;
    }

uint32_t div_magic(uint32_t M)
    {
    return M == 1 ? 0u : (uint32_t)(((1ull << 32) + M - 1) / M);
    }

TileGeometry tile_geometry(uint64_t N, uint32_t rowbytes, uint32_t tile_cap, size_t lds_budget)
    {
    uint32_t tile = 16;
    while (tile * 2 <= tile_cap && (uint64_t)tile * 2 * rowbytes <= lds_budget)
        tile <<= 1;
    return TileGeometry {tile, (N + tile - 1) / tile};
    }

uint64_t blocks_for(uint64_t n_tiles, size_t lds_bytes, uint64_t per_cu)
    {
    const uint64_t resident = lds_bytes ? std::max<uint64_t>(1, (160u * 1024u) / lds_bytes) : 8;
    return std::min(n_tiles, (uint64_t)num_cus() * std::min(per_cu, resident));
    }

// ---- tuning knobs (struct PackTuning: pgsd_kernels.hpp)
static std::mutex g_tuning_lock;
static bool g_tuning_loaded = false;
static PackTuning g_tuning;

// the integer in variable `name`, parsed once; false (and *out untouched) where it is unset or outside [min, max]
static bool env_int(const char* name, long long min, long long max, long long* out)
    {
    const char* e = getenv(name);
    const long long v = e ? strtoll(e, nullptr, 10) : 0;
    if (!e || v < min || v > max)
        return false;
    *out = v;
    return true;
    }

// "<threads>x<rows per lane>"; only the instantiated pairs: the grid is sized from T x U, so a pair the dispatcher does
// not know would cover too few rows per block and leave a part of every array unwritten
static void env_rows_cfg(const char* name, bool (*known)(int, int), const char* shapes, int* t_out, int* u_out)
    {
    const char* e = getenv(name);
    if (!e)
        return;
    int t = 0, u = 0;
    if (sscanf(e, "%dx%d", &t, &u) == 2 && known(t, u))
        *t_out = t, *u_out = u;
    else
        fprintf(stderr, "pgsd_amd: %s=%s is not one of%s: ignored\n", name, e, shapes);
    }

static PackTuning read_tuning()
    {
    PackTuning t;
    long long v = 0;
    env_rows_cfg("PGSD_PACK_ROWS_CFG", pack_rows_shape_known, PGSD_PACK_ROWS_SHAPES(PGSD_SHAPE_TEXT), &t.rows_t, &t.rows_u);
    if (const char* e = getenv("PGSD_PACK_KERNEL"))
        t.pack_tiles = strcmp(e, "tiles") == 0;
    if (env_int("PGSD_PACK_BLOCKS_PER_CU", 1, INT_MAX, &v))
        t.per_cu = (uint64_t)v;
    if (env_int("PGSD_PACK_TILE", 16, INT_MAX, &v))
        t.tile_cap = (uint32_t)v;
    if (env_int("PGSD_PACK_LDS_KB", 1, INT_MAX, &v))
        t.lds_budget = (size_t)v << 10;
    if (env_int("PGSD_PACK_PREFETCH", INT_MIN, INT_MAX, &v))
        t.prefetch = (int)v;
    env_rows_cfg("PGSD_UNPACK_ROWS_CFG", unpack_rows_shape_known, PGSD_UNPACK_ROWS_SHAPES(PGSD_SHAPE_TEXT), &t.unrows_t, &t.unrows_u);
    if (env_int("PGSD_UNPACK_TILE", 16, INT_MAX, &v))
        t.unpack_tile_cap = (uint32_t)v;
    if (env_int("PGSD_UNPACK_BLOCKS_PER_CU", 1, INT_MAX, &v))
        t.unpack_per_cu = (uint64_t)v;
    if (const char* e = getenv("PGSD_UNPACK_KERNEL"))
        t.unpack_tiles = strcmp(e, "tiles") == 0;
    if (env_int("PGSD_PLAN_BLOCK_ROWS", 1, 1 << 24, &v))
        t.plan_block_rows = (uint32_t)v;
    return t;
    }

PackTuning tuning()
    {
    std::lock_guard<std::mutex> guard(g_tuning_lock);
    if (!g_tuning_loaded)
        {
        g_tuning = read_tuning();
        g_tuning_loaded = true;
        }
    return g_tuning;
    }

void reload_pack_tuning()
    {
    std::lock_guard<std::mutex> guard(g_tuning_lock);
    g_tuning_loaded = false;
    }
    } // namespace pgsd_amd

extern "C" int pgsd_device_available(void)
    try
    {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        {
        (void)hipGetLastError();
        return 0;
        }
    return n > 0 ? 1 : 0;
    }
catch (...)
    {
        return pgsd_amd::abi_guard();
    }

extern "C" void pgsd_reload_tuning(void)
    try
    {
    pgsd_amd::reload_pack_tuning();
    }
catch (...)
    {
        pgsd_amd::abi_guard();
    }

extern "C" uint32_t pgsd_abi_version(void)
    {
    return PGSD_ABI_VERSION;
    }
