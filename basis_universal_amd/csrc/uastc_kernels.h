// uastc_kernels.h -- host-side launch interface of uastc_kernels.hip (internal to libbasisu_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uastc_rdo_params.h"

namespace bu {

// Bytes of device workspace bu::launch_encode_uastc needs for n_blocks at the given pack flags (level in the low bits).
size_t uastc_workspace_bytes(uint32_t n_blocks, uint32_t flags);
// encode_uastc (encoder/basisu_uastc_enc.cpp:3126) over n_blocks resident 4x4 RGBA tiles -> 16 B UASTC blocks.
// Stream-ordered; d_workspace must hold uastc_workspace_bytes(); kernel_ms (optional, 4 entries) is not touched here.
hipError_t launch_encode_uastc(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, uint32_t flags, void* d_workspace, void* d_out_blocks);
// The four phases separately (profiling brackets in the C ABI layer).
hipError_t launch_uastc_phase(hipStream_t st, int phase, const void* d_pixel_blocks, uint32_t n_blocks, uint32_t flags, void* d_workspace, void* d_out_blocks);

// uastc_rdo (encoder/basisu_uastc_enc.h:139, uastc_enc.cpp:4095) in place over resident UASTC blocks (uastc_rdo_kernels.hip): one slice, or several that lie back to
// back, every slice cut into its own strips exactly as the reference cuts it (total_jobs). uastc_rdo_strips.h's rdo_slices_layout states the strips and the
// workspace of a call; d_workspace holds L.total_bytes. Three launches, stream-ordered: prepare (clears [0, L.zero_bytes), then what depends on a block alone, in
// parallel), the walk (serial per strip; fat = the build with the refit in it, for the strips the prepare pass flagged, beside the lean build for the others: both
// cover all strips) and the finish (refit + hints of the modified blocks) for the longest per-strip list: the strip counts at d_workspace + L.strip_counts say it,
// L.longest bounds it. Four counters {modified, failed, refined, skipped} per slice lie at d_workspace + L.counters.
// table = false, the arithmetic form, for a layout of ONE slice: a strip's range follows from its index and the slice's per_job. table = true: every strip is read
// from its record, workgroups take the longest strips first; the caller has copied L.recs to d_workspace + L.strips and L.order to d_workspace + L.order_at.
struct rdo_slices_layout;
hipError_t launch_uastc_rdo_prepare(hipStream_t st, void* d_blocks, const void* d_pixel_blocks, const rdo_slices_layout& L, const bu_uastc::rdo_params& p, void* d_workspace,
                                    bool table);
hipError_t launch_uastc_rdo_walk(hipStream_t st, bool fat, void* d_blocks, const void* d_pixel_blocks, const rdo_slices_layout& L, const bu_uastc::rdo_params& p,
                                 void* d_workspace, bool table);
hipError_t launch_uastc_rdo_finish(hipStream_t st, void* d_blocks, const void* d_pixel_blocks, const rdo_slices_layout& L, const bu_uastc::rdo_params& p, uint32_t flags,
                                   void* d_workspace, bool table, uint32_t longest_list);

} // namespace bu
