# libpgsd_amd.pxd -- Cython view of include/pgsd.h (the C ABI of libpgsd_amd.so).
#
# Counterpart of the reference's pgsd/pgsd/libpgsd.pxd (lines 51-144): the same sixteen entry points and
# on-disk structs, minus `mpi4py.MPI` (the reference cimports it for the MPI_File member of its handle,
# libpgsd.pxd:6; this library's handle starts with a POSIX fd), plus the device path.  The declarations are
# checked by the C compiler against the real header when pgsd/_fl.pyx is built: a prototype that drifts
# from include/pgsd.h does not compile.
from libc.stdint cimport uint8_t, uint16_t, int32_t, uint32_t, uint64_t, int64_t


cdef extern from "pgsd.h" nogil:
    cdef enum pgsd_type:
        PGSD_TYPE_UINT8
        PGSD_TYPE_UINT16
        PGSD_TYPE_UINT32
        PGSD_TYPE_UINT64
        PGSD_TYPE_INT8
        PGSD_TYPE_INT16
        PGSD_TYPE_INT32
        PGSD_TYPE_INT64
        PGSD_TYPE_FLOAT
        PGSD_TYPE_DOUBLE

    cdef enum pgsd_open_flag:
        PGSD_OPEN_READWRITE
        PGSD_OPEN_READONLY
        PGSD_OPEN_APPEND

    cdef enum pgsd_error:
        PGSD_SUCCESS
        PGSD_ERROR_IO
        PGSD_ERROR_INVALID_ARGUMENT
        PGSD_ERROR_NOT_A_PGSD_FILE
        PGSD_ERROR_INVALID_PGSD_FILE_VERSION
        PGSD_ERROR_FILE_CORRUPT
        PGSD_ERROR_MEMORY_ALLOCATION_FAILED
        PGSD_ERROR_NAMELIST_FULL
        PGSD_ERROR_FILE_MUST_BE_WRITABLE
        PGSD_ERROR_FILE_MUST_BE_READABLE
        PGSD_ERROR_DEVICE
        PGSD_ERROR_COMM
        PGSD_ERROR_NO_DEVICE

    cdef uint64_t PGSD_PARTITION_AUTO

    cdef struct pgsd_header:
        uint64_t magic
        uint64_t index_location
        uint64_t index_allocated_entries
        uint64_t namelist_location
        uint64_t namelist_allocated_entries
        uint32_t schema_version
        uint32_t pgsd_version
        char application[64]
        char schema[64]
        char reserved[80]

    cdef struct pgsd_index_entry:
        uint64_t frame
        uint64_t N
        int64_t location
        uint32_t M
        uint16_t id
        uint8_t type
        uint8_t flags

    cdef struct pgsd_handle:
        int fd
        pgsd_header header
        uint64_t cur_frame
        long long file_size
        pgsd_open_flag open_flags
        uint64_t pending_index_entries
        uint64_t maximum_write_buffer_size
        uint64_t index_entries_to_buffer
        int rank
        int nprocs
        void* impl

    cdef struct pgsd_comm:
        void* ctx
        int rank
        int size

    # ---- part 1: the reference's entry points (pgsd.h:362-735 there)
    uint32_t pgsd_make_version(unsigned int major, unsigned int minor)
    int pgsd_create_and_open(pgsd_handle* handle, const char* fname, const char* application, const char* schema,
                             uint32_t schema_version, pgsd_open_flag flags, int exclusive_create)
    int pgsd_open(pgsd_handle* handle, const char* fname, pgsd_open_flag flags)
    int pgsd_close(pgsd_handle* handle)
    int pgsd_end_frame(pgsd_handle* handle)
    int pgsd_flush(pgsd_handle* handle)
    int pgsd_write_chunk(pgsd_handle* handle, const char* name, pgsd_type type, uint64_t N, uint32_t M,
                         uint64_t N_global, uint32_t M_global, uint64_t offset, uint64_t global_size, bint all,
                         uint8_t flags, const void* data)
    const pgsd_index_entry* pgsd_find_chunk(pgsd_handle* handle, uint64_t frame, const char* name)
    int pgsd_read_chunk(pgsd_handle* handle, void* data, const pgsd_index_entry* chunk, uint64_t N, uint32_t M,
                        uint32_t offset, bint all)
    uint64_t pgsd_get_nframes(pgsd_handle* handle)
    uint64_t pgsd_get_nnames(pgsd_handle* handle)
    size_t pgsd_sizeof_type(pgsd_type type)
    const char* pgsd_find_matching_chunk_name(pgsd_handle* handle, const char* match, const char* prev)
    uint64_t pgsd_get_maximum_write_buffer_size(pgsd_handle* handle)
    int pgsd_set_maximum_write_buffer_size(pgsd_handle* handle, uint64_t size)
    uint64_t pgsd_get_index_entries_to_buffer(pgsd_handle* handle)
    int pgsd_set_index_entries_to_buffer(pgsd_handle* handle, uint64_t number)
    const char* pgsd_last_error_string()

    # ---- frame exchange, communicators
    int pgsd_set_frame_exchange(pgsd_handle* handle, int batched)
    int pgsd_set_local_reads(pgsd_handle* handle, int on)
    int pgsd_set_partition(pgsd_handle* handle, const uint64_t* rows, uint32_t n_ranks)
    cdef struct pgsd_exchange_stats:
        uint64_t collectives
        uint64_t count
        double total_us
        double max_us
        double min_us
    int pgsd_get_exchange_stats(pgsd_handle* handle, pgsd_exchange_stats* out, int reset)
    int pgsd_comm_size()
    int pgsd_create_and_open_on(const pgsd_comm* comm, pgsd_handle* handle, const char* fname, const char* application,
                                const char* schema, uint32_t schema_version, pgsd_open_flag flags, int exclusive_create)
    int pgsd_open_on(const pgsd_comm* comm, pgsd_handle* handle, const char* fname, pgsd_open_flag flags)
    int pgsd_handle_allgather(pgsd_handle* handle, const void* send, void* recv, size_t bytes)

    # ---- part 3: device path
    cdef struct pgsd_field_desc:
        const void* src
        const uint32_t* order
        uint32_t src_type
        uint32_t src_stride
        uint32_t src_col0
        uint32_t bitcast

    cdef struct pgsd_chunk_req:
        const char* name
        uint32_t type
        uint32_t M
        pgsd_field_desc src

    cdef struct pgsd_field_dst:
        void* dst
        const uint32_t* order
        uint32_t dst_type
        uint32_t dst_stride
        uint32_t dst_col0
        uint32_t bitcast
        uint32_t fill_rest
        uint32_t reserved
        uint64_t fill_bits

    cdef struct pgsd_device_config:
        int device
        uint64_t slab_bytes
        uint32_t n_slabs
        uint32_t n_writers
        uint32_t profile
        uint32_t prealloc_mib

    cdef struct pgsd_device_stats:
        uint64_t pack_launches
        double pack_ms
        uint64_t pack_rows
        uint64_t pack_bytes_out
        uint64_t pack_bytes_in
        uint64_t d2h_bytes
        uint64_t written_bytes
        double d2h_ms
        double write_ms
        uint64_t side_bytes
        double side_ms
        uint64_t side_on

    int pgsd_write_chunk_device(pgsd_handle* handle, const char* name, pgsd_type type, uint64_t N, uint32_t M,
                                uint64_t N_global, uint32_t M_global, uint64_t offset, uint64_t global_size, bint all,
                                uint8_t flags, const pgsd_field_desc* src)
    int pgsd_write_chunks_device(pgsd_handle* handle, uint32_t n_chunks, const pgsd_chunk_req* chunks, uint64_t N,
                                 uint64_t N_global, uint64_t offset_rows)
    int pgsd_stage_chunks_device(pgsd_handle* handle, uint32_t n_chunks, const pgsd_chunk_req* chunks, uint64_t N,
                                 uint64_t* ticket)
    int pgsd_write_staged_chunks(pgsd_handle* handle, uint64_t ticket, uint32_t first, uint32_t count,
                                 uint64_t N_global, uint64_t offset_rows)
    int pgsd_compare_staged_chunks(pgsd_handle* handle, uint64_t ticket, uint32_t first, uint32_t count,
                                   const void* const* ref, const uint64_t* ref_bytes, uint8_t* equal)
    int pgsd_copy_staged_chunks(pgsd_handle* handle, uint64_t ticket, uint32_t first, uint32_t count,
                                void* const* dst)
    int pgsd_end_frame_async(pgsd_handle* handle)
    int pgsd_frame_sync(pgsd_handle* handle)
    int pgsd_device_wait_packed(pgsd_handle* handle)
    int pgsd_device_configure(pgsd_handle* handle, const pgsd_device_config* cfg)
    int pgsd_device_set_source_stream(pgsd_handle* handle, void* stream)
    int pgsd_device_get_stats(pgsd_handle* handle, pgsd_device_stats* out, int reset)
    int pgsd_select_rows(const uint8_t* flags, uint64_t N, uint32_t* out_index, uint64_t* out_count, void* stream)
    void* pgsd_device_alloc(int device, size_t bytes, const void* pattern, size_t pattern_bytes)
    int pgsd_device_free(int device, void* ptr)
    uint32_t PGSD_ABI_VERSION
    uint32_t pgsd_abi_version()
    int pgsd_read_chunk_device(pgsd_handle* handle, const pgsd_index_entry* chunk, uint64_t N, uint64_t row_offset,
                               const pgsd_field_dst* dst)
    int pgsd_device_wait_read(pgsd_handle* handle)


# entry points that are not part of the public C ABI (csrc/pgsd_private.h): queue plumbing and binding helpers
cdef extern from "pgsd_private.h" nogil:
    int pgsd_set_deferred_rows(pgsd_handle* handle, int on)
    int pgsd_frame_exchange(pgsd_handle* handle)
    int pgsd_device_of(pgsd_handle* handle)
    int pgsd_device_copy(int device, void* dst, const void* src, size_t bytes)
    int pgsd_select_domain_device(pgsd_handle* handle, const pgsd_index_entry* position, const float* box,
                                  uint32_t dimensions, const double* lo, const double* hi, uint32_t* out_rows,
                                  uint64_t* out_count)
    int pgsd_select_halo_device(pgsd_handle* handle, const pgsd_index_entry* position, const float* box,
                                uint32_t dimensions, const double* lo, const double* hi, const double* bands,
                                const uint32_t* divided, uint32_t* out_rows, int32_t* out_shift, uint64_t* out_counts)
    int pgsd_select_where_device(pgsd_handle* handle, uint32_t n_terms, const pgsd_index_entry* chunks,
                                 const uint32_t* columns, const uint32_t* kinds, const double* lo, const double* hi,
                                 const uint64_t* sets, const pgsd_index_entry* position, const float* box,
                                 uint32_t dimensions, const double* dlo, const double* dhi, uint32_t* out_rows,
                                 uint64_t* out_count)
    int pgsd_domain_histogram_device(pgsd_handle* handle, const pgsd_index_entry* position, const float* box,
                                     uint32_t dimensions, uint32_t bins, uint64_t* out_hist)
    int pgsd_domain_counts_device(pgsd_handle* handle, const pgsd_index_entry* position, const float* box,
                                  uint32_t dimensions, const uint32_t* n, const double* interior_bounds,
                                  uint64_t* out_counts, uint64_t* out_nowhere)
    int pgsd_order_rows_by_cell_device(pgsd_handle* handle, const pgsd_index_entry* position, const float* box,
                                       uint32_t dimensions, const uint32_t* cells, uint32_t* rows, uint64_t n,
                                       uint64_t n_owned, int32_t* shift, int32_t* out_cell)
    int pgsd_frame_moments_device(pgsd_handle* handle, const pgsd_index_entry* typeid_chunk, const pgsd_index_entry* mass,
                                  const pgsd_index_entry* velocity, const pgsd_index_entry* energy,
                                  const pgsd_index_entry* position, const double* defaults, uint32_t type0,
                                  uint32_t n_types, const uint32_t* rows, uint64_t n, uint64_t* out_counts,
                                  double* out_sums)
    int pgsd_frame_displacements_device(pgsd_handle* handle, const pgsd_index_entry* position_a,
                                        const pgsd_index_entry* image_a, const pgsd_index_entry* position_b,
                                        const pgsd_index_entry* image_b, const pgsd_index_entry* typeid_chunk,
                                        const double* vectors_a, const double* vectors_b, uint32_t flags,
                                        uint32_t dimensions, uint32_t type0, uint32_t n_types, const uint32_t* rows,
                                        uint64_t n, double* out_rows, uint64_t* out_counts, double* out_values)
    int pgsd_cell_offsets_device(pgsd_handle* handle, const int32_t* cell, uint64_t n, uint32_t n_cells,
                                 uint32_t* out_offsets)
    int pgsd_cell_moments_device(pgsd_handle* handle, const pgsd_index_entry* mass, const pgsd_index_entry* velocity,
                                 const pgsd_index_entry* energy, const pgsd_index_entry* position, const double* defaults,
                                 const uint32_t* rows, const int32_t* cell, uint64_t n, uint32_t n_cells,
                                 uint64_t* out_counts, double* out_sums)
    int pgsd_neighbours_device(pgsd_handle* handle, const pgsd_index_entry* position, const double* vectors, double r,
                               uint32_t dimensions, const uint32_t* cells, const uint32_t* rows, const int32_t* cell,
                               uint64_t n, uint32_t bins, const double* edges2, uint32_t* out_count, double* out_nearest2,
                               uint32_t* out_nearest, uint64_t* out_summary, double* out_closest2)
    int pgsd_neighbour_offsets_device(pgsd_handle* handle, const pgsd_index_entry* position, const double* vectors, double r,
                                      uint32_t dimensions, const uint32_t* cells, const uint32_t* rows, const int32_t* cell,
                                      uint64_t n, uint32_t flags, uint64_t* out_offsets, uint64_t* out_summary)
    int pgsd_neighbour_list_device(pgsd_handle* handle, const pgsd_index_entry* position, const double* vectors, double r,
                                   uint32_t dimensions, const uint32_t* cells, const uint32_t* rows, const int32_t* cell,
                                   uint64_t n, uint32_t flags, const uint64_t* offsets, uint64_t capacity,
                                   uint32_t* out_neighbours, double* out_distance2)
    int pgsd_components_device(pgsd_handle* handle, const pgsd_index_entry* position, const double* vectors, double r,
                               uint32_t dimensions, const uint32_t* cells, const uint32_t* rows, const int32_t* cell,
                               uint64_t n, uint32_t flags, uint32_t* out_label, uint32_t* out_component,
                               uint32_t* out_sizes, uint64_t* out_summary)
    int pgsd_component_moments_device(pgsd_handle* handle, const pgsd_index_entry* mass, const pgsd_index_entry* velocity,
                                      const pgsd_index_entry* energy, const pgsd_index_entry* position, const double* defaults,
                                      const double* vectors, uint32_t dimensions, const uint32_t* rows, const uint32_t* label,
                                      const uint32_t* component, uint64_t n, uint64_t components, uint32_t flags,
                                      double* out_sums, double* out_extent, double* out_origin, uint32_t* out_flags,
                                      uint64_t* out_summary)
    int pgsd_sph_sums_device(pgsd_handle* handle, const pgsd_index_entry* position, const pgsd_index_entry* mass,
                             const pgsd_index_entry* density, const double* defaults, const double* vectors, double h,
                             uint32_t kernel, uint32_t dimensions, const uint32_t* cells, const uint32_t* rows,
                             const int32_t* cell, uint64_t n, double surface_below, double* out_number,
                             double* out_density, double* out_shepard, uint64_t* out_summary)
    int pgsd_sph_gradients_device(pgsd_handle* handle, const pgsd_index_entry* position, const pgsd_index_entry* velocity,
                                  const pgsd_index_entry* mass, const pgsd_index_entry* density, const double* defaults,
                                  const double* vectors, double h, uint32_t kernel, uint32_t dimensions,
                                  const uint32_t* cells, const uint32_t* rows, const int32_t* cell, uint64_t n,
                                  double* out_density_rate, double* out_divergence, double* out_curl, double* out_normal,
                                  uint64_t* out_summary)
    int pgsd_sph_smoothing_range_device(pgsd_handle* handle, const pgsd_index_entry* slength, double h_default,
                                        const uint32_t* rows, uint64_t n, uint64_t N, uint64_t* out_words)
    int pgsd_sph_adaptive_sums_device(pgsd_handle* handle, const pgsd_index_entry* position, const pgsd_index_entry* mass,
                                      const pgsd_index_entry* density, const pgsd_index_entry* slength,
                                      const double* defaults, const double* vectors, double h_max, uint32_t kernel,
                                      uint32_t mode, uint32_t dimensions, const uint32_t* cells, const uint32_t* rows,
                                      const int32_t* cell, uint64_t n, double surface_below, uint32_t* out_count,
                                      double* out_number, double* out_density, double* out_shepard, double* out_omega,
                                      uint64_t* out_summary)
    int pgsd_sph_tensors_device(pgsd_handle* handle, const pgsd_index_entry* position, const pgsd_index_entry* velocity,
                                const pgsd_index_entry* mass, const pgsd_index_entry* density, const double* defaults,
                                const double* vectors, double h, uint32_t kernel, uint32_t dimensions, double det_min,
                                const uint32_t* cells, const uint32_t* rows, const int32_t* cell, uint64_t n,
                                double* out_correction, double* out_determinant, double* out_velocity_gradient,
                                double* out_shear_rate, uint64_t* out_summary)
    int pgsd_sph_accelerations_device(pgsd_handle* handle, const pgsd_index_entry* position,
                                      const pgsd_index_entry* velocity, const pgsd_index_entry* mass,
                                      const pgsd_index_entry* density, const pgsd_index_entry* pressure,
                                      const double* defaults, const double* vectors, double h, uint32_t kernel,
                                      uint32_t dimensions, const uint32_t* cells, double viscosity, const double* gravity,
                                      const uint32_t* rows, const int32_t* cell, uint64_t n, double* out_pressure_acc,
                                      double* out_viscous_acc, double* out_total, uint64_t* out_summary)
    int pgsd_sph_body_force_device(pgsd_handle* handle, const pgsd_index_entry* position, const pgsd_index_entry* velocity,
                                   const pgsd_index_entry* mass, const pgsd_index_entry* density,
                                   const pgsd_index_entry* pressure, const double* defaults, const double* vectors, double h,
                                   uint32_t kernel, uint32_t dimensions, const uint32_t* cells, double viscosity,
                                   const double* about, const uint32_t* body_rows, const int32_t* body_cell, uint64_t n_body,
                                   const uint32_t* fluid_rows, const int32_t* fluid_cell, uint64_t n_fluid,
                                   uint32_t* out_contacts, double* out_pressure_acc, double* out_viscous_acc,
                                   uint64_t* out_summary)
    int pgsd_sph_samples_device(pgsd_handle* handle, const pgsd_index_entry* position, const pgsd_index_entry* mass,
                                const pgsd_index_entry* density, const pgsd_index_entry* const* values,
                                const uint32_t* value_columns, const double* value_defaults, const double* defaults,
                                const float* box, const double* vectors, double h, uint32_t kernel, uint32_t dimensions,
                                const uint32_t* cells, const uint32_t* rows, const int32_t* cell, uint64_t n,
                                const double* points, uint64_t K, uint32_t normalise, uint32_t* out_count,
                                double* out_density, double* out_shepard, double* out_values, uint64_t* out_summary)
    int pgsd_chunk_stats_device(pgsd_handle* handle, const pgsd_index_entry* chunk, const uint32_t* rows, uint64_t n,
                                uint32_t with_norm2, uint64_t* out_counts, double* out_values)
    int pgsd_read_rows_device(pgsd_handle* handle, const pgsd_index_entry* chunk, const uint32_t* rows, uint64_t n,
                              const pgsd_field_dst* dst)
    cdef struct pgsd_row_plan:
        pass
    int pgsd_row_plan_create(pgsd_handle* handle, const uint32_t* rows, uint64_t n, uint64_t N, uint32_t* rows2,
                             pgsd_row_plan** out)
    void pgsd_row_plan_destroy(pgsd_row_plan* plan)
    int pgsd_row_plan_query(const pgsd_row_plan* plan, uint64_t* counts, const uint32_t** lists)
    int pgsd_read_rows_planned_device(pgsd_handle* handle, const pgsd_index_entry* chunk, const pgsd_row_plan* plan,
                                      const pgsd_field_dst* dst)
    int pgsd_device_read_counters(pgsd_handle* handle, uint64_t* pread_bytes, uint64_t* h2d_bytes, int reset)
