// api_mip_levels.cpp -- caller-supplied mip levels behind the C ABI of libbasisu_hip.so: one table of records, one stream-ordered copy of it, one launch.
#include "api_internal.h"
#include "mip_levels.h"

extern "C" {

int bu_hip_k_prepare_mip_levels(bu_hip_context* ctx, const void* d_payload, size_t payload_bytes, const bu_hip_mip_level_record* records, uint32_t n, void* d_out,
                                size_t out_bytes, uint32_t* d_flags) {
    if (!ctx) return 0;
    static const char* const fn = "prepare_mip_levels";
    bu::slice_table table;
    if (!checked(ctx, [&](bu::err_text e) { return bu::build_mip_level_records(table, fn, d_payload, payload_bytes, records, n, d_out, out_bytes, d_flags, e); })) return 0;
    if (!n) return 1;
    device_guard g(ctx->device);
    uploaded_slices d;
    if (!upload_slice_table(ctx, table, d)) return 0;
    prof_scope ps(ctx, fn);
    BU_TRY(ctx, bu::launch_prepare_mip_levels(ctx->stream, d_payload, static_cast<const bu_hip_mip_level_record*>(d.records), d.prefix, n, table.total, d_out, d_flags));
    return 1;
}

} // extern "C"
