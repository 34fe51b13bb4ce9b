// pgsd_device_stub.cpp -- NOT part of libpgsd_amd.so.  Link-time stand-ins for the device
// pipeline so that the HOST file layer (pgsd_container.cpp, pgsd_placement.cpp, pgsd_read.cpp, pgsd_comm.cpp, pgsd_io.cpp) can be built
// with gcc -fsanitize=address,undefined and exercised by the scenario driver on a CPU box
// (`make asan`; GPU AddressSanitizer is not available on the pool).  Every device entry point
// fails with PGSD_ERROR_NO_DEVICE, exactly as the real library does without a GPU.
#include "pgsd_internal.hpp"

namespace pgsd_amd
    {
DevicePipeline* device_pipeline_create(const pgsd_device_config&, int, bool, std::string* err)
    {
    if (err)
        *err = "sanitizer build: no device pipeline";
    return nullptr;
    }
void device_pipeline_destroy(DevicePipeline*) { }
int device_pipeline_device(DevicePipeline*) { return -1; }
int device_pipeline_submit(DevicePipeline*, std::vector<DeviceChunk>&, uint64_t, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_stage(DevicePipeline*, std::vector<DeviceChunk>&, uint64_t, int*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_commit(DevicePipeline*, int, size_t, long long, void*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_compare(DevicePipeline*, int, size_t, size_t, const void* const*, const uint64_t*, uint8_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_copy_staged(DevicePipeline*, int, size_t, size_t, void* const*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
void device_pipeline_kick(DevicePipeline*) { }
void device_pipeline_write_host(DevicePipeline*, const void*, size_t, long long) { }
bool device_pipeline_single_writer(DevicePipeline*) { return false; }
int device_pipeline_wait_packed(DevicePipeline*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
void device_pipeline_set_source_stream(DevicePipeline*, void*) { }
int device_pipeline_read(DevicePipeline*, long long, size_t, const pgsd_unpack_job&, uint64_t, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_wait_read(DevicePipeline*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_read_rows(DevicePipeline*, long long, size_t, const pgsd_unpack_job&, uint64_t, const uint32_t*, uint64_t, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_select_domain(DevicePipeline*, long long, size_t, const DomainArgs&, uint32_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_select_where(DevicePipeline*, const ChunkRange*, const WhereArgs&, uint32_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_select_halo(DevicePipeline*, long long, size_t, const HaloArgs&, uint32_t*, int32_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_domain_histogram(DevicePipeline*, long long, size_t, const DomainArgs&, uint32_t, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_domain_counts(DevicePipeline*, long long, size_t, const CellArgs&, uint64_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_order_rows(DevicePipeline*, long long, size_t, const OrderArgs&, uint32_t*, int32_t*, int32_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_chunk_stats(DevicePipeline*, long long, size_t, const StatsArgs&, uint64_t*, double*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_frame_moments(DevicePipeline*, const ChunkRange*, const MomentsArgs&, uint64_t*, double*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_frame_displacements(DevicePipeline*, const ChunkRange*, const DisplacementArgs&, uint64_t*, double*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_cell_offsets(DevicePipeline*, const int32_t*, uint64_t, uint32_t, uint32_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_cell_moments(DevicePipeline*, const ChunkRange*, const CellMomentsArgs&, uint64_t*, double*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_neighbours(DevicePipeline*, long long, size_t, const NeighboursArgs&, const double*, uint32_t*, double*, uint32_t*, uint64_t*, double*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_sums(DevicePipeline*, const ChunkRange*, const SphArgs&, double*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_adaptive(DevicePipeline*, const ChunkRange*, const SphAdaptiveArgs&, uint32_t*, double*, double*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_smoothing_range(DevicePipeline*, long long, size_t, uint32_t, const uint32_t*, uint64_t, uint64_t, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_gradients(DevicePipeline*, const ChunkRange*, const SphGradientsArgs&, double*, double*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_tensors(DevicePipeline*, const ChunkRange*, const SphTensorsArgs&, double*, double*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_accelerations(DevicePipeline*, const ChunkRange*, const SphForcesArgs&, double*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_body_force(DevicePipeline*, const ChunkRange*, const SphBodyArgs&, uint32_t*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_sph_samples(DevicePipeline*, const ChunkRange*, const SphSamplesArgs&, uint32_t*, double*, double*, double*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_neighbour_offsets(DevicePipeline*, long long, size_t, const NeighbourListArgs&, uint64_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_neighbour_list(DevicePipeline*, long long, size_t, const NeighbourListArgs&, const uint64_t*, uint64_t, uint32_t*, double*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_components(DevicePipeline*, long long, size_t, const NeighboursArgs&, uint32_t*, uint32_t*, uint32_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_component_moments(DevicePipeline*, const ChunkRange*, const ComponentMomentsArgs&, double*, double*, double*, uint32_t*, uint64_t*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_plan_rows(DevicePipeline*, RowPlan&, std::string*) { return PGSD_ERROR_NO_DEVICE; }
int device_pipeline_read_planned(DevicePipeline*, long long, size_t, const pgsd_unpack_job&, const RowPlan&, std::string*) { return PGSD_ERROR_NO_DEVICE; }
void device_pipeline_read_counters(DevicePipeline*, uint64_t* a, uint64_t* b, int) { if (a) *a = 0; if (b) *b = 0; }
int device_pipeline_drain(DevicePipeline*, std::string*) { return PGSD_ERROR_NO_DEVICE; }
void device_pipeline_stats(DevicePipeline*, pgsd_device_stats*, int) { }
    } // namespace pgsd_amd

extern "C" int pgsd_device_available(void) { return 0; }
extern "C" int pgsd_comm_rccl_unique_id(void*) { return PGSD_ERROR_NO_DEVICE; }
extern "C" int pgsd_comm_create_rccl(const void*, int, int, int, struct pgsd_comm*) { return PGSD_ERROR_NO_DEVICE; }
extern "C" int pgsd_comm_rccl_available(int) { return PGSD_ERROR_NO_DEVICE; }
extern "C" int pgsd_device_release_parked(void) { return 0; }
