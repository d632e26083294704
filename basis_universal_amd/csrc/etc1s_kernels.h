// etc1s_kernels.h -- host-side launch interface of the ETC1S frontend's kernels (internal to libbasisu_hip.so). One unit per stage:
//   etc1s_block_fit_kernels.hip    a6   the per-block etc1_optimizer                          } etc1s_fit_common.h: what the two fits share
//   etc1s_cluster_fit_kernels.hip  a9   the cluster fit, free and with forced selectors       }   (+ etc1s_codebook_wide.inc: large clusters)
//   etc1s_refine_kernels.hip       a10  refine_endpoint_clusterization: plain lists, pre-sorted lists per wave, pre-sorted lists with one block per lane
//   etc1s_selector_kernels.hip     a11-a14  determine_selectors, selector training vectors, k_cosc_*, k_fosc_*
//   etc1s_misc_kernels.hip         a7, sub-block errors, the backend's block errors, k_extract_blocks
//
// All kernels are integer-ALU bound (hundreds of integer ops per byte of pixel data), so the design rules are:
//   * wave64 mappings that keep all 64 lanes on the SAME kind of work -- and where a wave's blocks need different NUMBERS of steps (the per-block fit's trials), the
//     cheap part (finding the next step worth taking) loops per block while the expensive part (evaluating it) runs for all blocks at once;
//   * the 64-byte pixel tile is read once per kernel with 16-byte loads and kept in registers in the metric's separable
//     basis (etc1s_device.h: cvec), so a colour distance is 3 subtractions + 3 24-bit multiplies + shifts;
//   * wavefront reductions (DPP/ds_swizzle via __shfl_xor) pick the best intensity table / candidate, with the
//     reference's tie rules encoded in the reduction key (lowest index wins on equal error);
//   * candidate codebooks are read through the scalar/vector caches (they are KB-sized and shared by all lanes).
// Result parity with the reference CPU encoder is bit-exact; each kernel cites the code it restates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/basisu_hip.h"   // bu_hip_slice_source

namespace bu {

enum { BU_Q_FAST = 0, BU_Q_MEDIUM = 1, BU_Q_SLOW = 2, BU_Q_UBER = 3 }; // basis_etc_quality, basisu_etc.h:794-801

// the two etc1_optimizer tables of the per-block and of the cluster fit unit, onto the current device (every new context calls both)
hipError_t upload_block_fit_tables();
hipError_t upload_cluster_fit_tables();

hipError_t launch_encode_etc1s_blocks(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, int quality, bool perceptual, void* d_out);
hipError_t launch_endpoint_training_vectors(hipStream_t st, const void* d_etc_blocks, uint32_t n_blocks, float* d_out6);
hipError_t launch_selector_training_vectors(hipStream_t st, const void* d_enc_blocks, uint32_t n_blocks, bool perceptual, float* d_out16, uint64_t* d_w);
hipError_t launch_generate_endpoint_codebook(hipStream_t st, const void* d_pixel_blocks, uint32_t n_clusters, const uint32_t* d_order,
                                             const uint32_t* d_offsets, const uint32_t* d_indices, int quality, bool perceptual, uint32_t step,
                                             uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid);
// LARGE clusters (etc1s_codebook_wide.inc): many workgroups per cluster, a launch per pass over the texels of all large clusters of the call. h_cluster / h_first /
// h_subblocks: per large cluster its index, the position of its first member in d_indices and its member (sub-block) count. prepare() lays out the workspace
// [states | chunk table | scratch] and fills `image` with the bytes of its first two parts (the caller uploads them to d_work before launch_codebook_wide).
struct cb_wide_layout { size_t states_at, chunks_at, sum_at, total, image_bytes; uint32_t n_big, n_chunks; };
cb_wide_layout codebook_wide_prepare(const uint32_t* h_cluster, const uint32_t* h_first, const uint32_t* h_subblocks, uint32_t n_big, std::vector<unsigned char>& image);
hipError_t launch_codebook_wide_means(hipStream_t st, const void* d_pixel_blocks, const uint32_t* d_indices, void* d_work, const cb_wide_layout& L, float* d_out /* 3 per large cluster */);
hipError_t launch_codebook_wide(hipStream_t st, const void* d_pixel_blocks, const uint32_t* d_indices, void* d_work, const cb_wide_layout& L, int quality, bool perceptual, bool forced,
                                uint32_t step, const void* d_enc_blocks, uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid, uint64_t* d_cur_err);
hipError_t launch_refit_endpoints_given_selectors(hipStream_t st, const void* d_pixel_blocks, const void* d_enc_blocks, uint32_t n_clusters, const uint32_t* d_order,
                                                  const uint32_t* d_offsets, const uint32_t* d_indices, int quality, bool perceptual, uint8_t* d_params, uint64_t* d_err,
                                                  uint8_t* d_valid, uint64_t* d_cur_err);
hipError_t launch_subblock_errors(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
                                  bool perceptual, uint64_t* d_out);
hipError_t launch_backend_block_errors(hipStream_t st, const void* d_pixel_blocks, const void* d_etc_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
                                       uint32_t first_block, uint32_t nbx, uint32_t nby, uint32_t n_clusters, bool perceptual, bool with_neighbours, uint32_t* d_own,
                                       uint32_t* d_neighbour);
hipError_t launch_refine_endpoint_clusterization(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, const uint32_t* d_block_cluster,
                                                 const uint8_t* d_cluster_params, uint32_t n_clusters, uint32_t n_parents, const uint32_t* d_cand_offsets,
                                                 const uint32_t* d_cand_indices, const uint8_t* d_block_parent, bool perceptual, uint32_t* d_out_best,
                                                 int path /* refine_path() */, void* d_work /* refine_workspace_bytes(); path 1 takes none */);
// which kernels a call takes, from bu_hip_tuning::refine_unsorted and what the lists and the metric allow: 0 = sorted lists, one block per lane (k_refine_block_lanes),
// 1 = the lists as they come (k_refine_endpoint_clusterization), 2 = sorted lists, one block per wave (k_refine_sorted)
int refine_path(uint32_t refine_unsorted, uint32_t n_clusters, uint32_t n_parents, bool perceptual);
size_t refine_workspace_bytes(uint32_t n_clusters, uint32_t n_parents, uint32_t n_blocks);   // sorted lists + the blocks bucketed by (parent, table); 0: lists too long for the sorted form
hipError_t launch_determine_selectors(hipStream_t st, const void* d_pixel_blocks, uint32_t n_blocks, const uint8_t* d_color5_inten,
                                      const uint32_t* d_block_cluster, bool perceptual, void* d_out);
// d_workspace: create_optimized_selector_codebook_workspace_bytes()
size_t create_optimized_selector_codebook_workspace_bytes(uint32_t n_clusters);
hipError_t launch_create_optimized_selector_codebook(hipStream_t st, const void* d_pixel_blocks, const void* d_enc_blocks, uint32_t n_clusters,
                                                     const uint32_t* d_offsets, const uint32_t* d_block_indices, bool perceptual,
                                                     void* d_workspace, void* d_selector_blocks);
hipError_t launch_find_optimal_selector_clusters(hipStream_t st, const void* d_pixel_blocks, void* d_enc_blocks, uint32_t n_blocks,
                                                 const void* d_selector_blocks, uint32_t n_selectors, uint32_t n_parents, const uint32_t* d_cand_offsets,
                                                 const uint32_t* d_cand_indices, const uint8_t* d_block_parent, bool perceptual, uint32_t chunk,
                                                 uint32_t* d_scratch_idx, uint32_t* d_out_idx, uint32_t* d_cand_words /* scratch for the candidates' selector words, or NULL */, size_t cand_words_capacity /* entries */);

hipError_t launch_extract_blocks(hipStream_t st, const void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* d_out_blocks);
// every slice of a call in one launch: d_slices = n_slices records, d_prefix = n_slices + 1 ascending tile counts (the last = total_tiles <= 2^30); both resident
hipError_t launch_extract_slices(hipStream_t st, const bu_hip_slice_source* d_slices, const uint32_t* d_prefix, uint32_t n_slices, uint32_t total_tiles, void* d_out_blocks);

} // namespace bu
