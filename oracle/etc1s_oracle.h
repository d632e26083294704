/* oracle/etc1s_oracle.h -- TEST INFRASTRUCTURE ONLY (see etc1s_oracle.c). */
#ifndef ORACLE_ETC1S_ORACLE_H
#define ORACLE_ETC1S_ORACLE_H
#include <stdint.h>
/* marks the exported functions: tests/native_libs.py reads their ctypes signatures from these prototypes */
#define ORC_API
#ifdef __cplusplus
extern "C" {
#endif

/* basis_etc_quality (encoder/basisu_etc.h:794-801) */
enum { ORC_QUALITY_FAST = 0, ORC_QUALITY_MEDIUM = 1, ORC_QUALITY_SLOW = 2, ORC_QUALITY_UBER = 3 };

ORC_API uint32_t orc_color_distance(int perceptual, const uint8_t* a_rgb, const uint8_t* b_rgb);
ORC_API uint32_t orc_hash_hsieh3(uint8_t r, uint8_t g, uint8_t b);

/* etc1_optimizer::init + compute with m_cluster_fit (etc.cpp:776-1278), ETC1S colour555 mode.
   rgba: n pixels, 4 bytes each. out_selectors (n bytes) may be NULL. Returns 1 on success. */
ORC_API int orc_etc1_optimize(const uint8_t* rgba, uint32_t n, int quality, int perceptual,
                              uint8_t out_color5[3], uint32_t* out_inten, uint64_t* out_err, uint8_t* out_selectors);

/* The same optimizer with m_pForce_selectors (etc.cpp:780-784, 1137-1160): pixel i is scored against colour force_selectors[i] of every
   trial instead of the nearest one. quality must be ORC_QUALITY_SLOW or _UBER (the reference refuses anything lower); returns 0 otherwise. */
ORC_API int orc_etc1_optimize_forced(const uint8_t* rgba, uint32_t n, int quality, int perceptual, const uint8_t* force_selectors,
                                     uint8_t out_color5[3], uint32_t* out_inten, uint64_t* out_err);

/* basisu_frontend::init_etc1_images CPU branch (frontend.cpp:765-818): pixel blocks (64 B) -> etc_block (8 B). */
ORC_API void orc_encode_etc1s_blocks(const uint8_t* pixel_blocks, uint32_t n_blocks, int comp_level, int perceptual, uint8_t* out_blocks);

/* etc_block::determine_selectors (etc.h:374-436) for ETC1S blocks: colour5+inten per block (4 B: r,g,b,inten). */
ORC_API void orc_determine_selectors(const uint8_t* pixel_blocks, uint32_t n_blocks, const uint8_t* color5_inten, int perceptual, uint8_t* out_blocks);

/* basisu_frontend::generate_endpoint_codebook CPU branch (frontend.cpp:1482-1613).
   Clusters are CSR lists of training-vector indices (block*2+subblock). prev_params/valid may be NULL when step==0.
   params: per cluster {r,g,b,inten}; err: per cluster u64; valid: per cluster u8 (in/out for step>0). */
ORC_API void orc_generate_endpoint_codebook(const uint8_t* pixel_blocks, uint32_t n_clusters, const uint32_t* offsets, const uint32_t* indices,
                                            int comp_level, int perceptual, uint32_t step, uint8_t* params, uint64_t* err, uint8_t* valid);

/* basisu_frontend::refine_block_endpoints_given_selectors (frontend.cpp:2718-2976) up to the caller's "only if better" test: per cluster
   (CSR lists of training-vector indices block*2+subblock, duplicates allowed) the forced-selector optimizer over the listed sub-blocks'
   texels (flipped layout), every texel's selector taken from its OWN block's encoding in encoded_blocks (8 B each); never keeps previous
   endpoints. cur_err: the listed sub-blocks' error under their own blocks' colours and selectors. quality: ORC_QUALITY_SLOW or _UBER.
   The four entries of an empty list are left untouched. */
ORC_API void orc_refit_endpoints_given_selectors(const uint8_t* pixel_blocks, const uint8_t* encoded_blocks, uint32_t n_clusters, const uint32_t* offsets,
                                                 const uint32_t* indices, int quality, int perceptual, uint8_t* params, uint64_t* err, uint8_t* valid, uint64_t* cur_err);

/* compute_endpoint_subblock_error_vec (frontend.cpp:1006-1091): out_err[block*2+subblock] = nearest-colour error of the sub-block under
   cluster_params[block_cluster[block]] = {r5,g5,b5,inten}, the colours built from the UNSCALED 5-bit values as the reference does there. */
ORC_API void orc_subblock_errors(const uint8_t* pixel_blocks, uint32_t n_blocks, const uint32_t* block_cluster, const uint8_t* cluster_params,
                                 int perceptual, uint64_t* out_err);

/* The stateless part of basisu_backend::create_encoder_blocks (backend.cpp:406-617) for one slice of num_blocks_x x num_blocks_y blocks
   starting at first_block (see bu_hip_k_backend_block_errors): own_err[b] = error of block b as encoded; with_neighbours:
   neighbour_err[3b + p] = its error under the endpoints of its left / upper / upper-left neighbour with its own selectors, ~0u for all
   three when own_err is 0 or ANY existing neighbour shares block b's cluster, ~0u for a neighbour outside the slice or whose cluster
   index is >= n_clusters. b is the ABSOLUTE block index first_block + y * num_blocks_x + x; other entries are not touched. */
ORC_API void orc_backend_block_errors(const uint8_t* pixel_blocks, const uint8_t* etc_blocks, const uint32_t* block_cluster, const uint8_t* cluster_params,
                                      uint32_t first_block, uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t n_clusters, int perceptual, int with_neighbours,
                                      uint32_t* own_err, uint32_t* neighbour_err);

/* basisu_frontend::refine_endpoint_clusterization CPU branch (frontend.cpp:1772-1917): per-block argmin.
   cand_offsets/cand_indices: CSR of candidate cluster lists per parent (n_parents+1 offsets), block_parent per block;
   pass n_parents==0 for the non-hierarchical case (all clusters in index order). */
ORC_API void orc_refine_endpoint_clusterization(const uint8_t* pixel_blocks, uint32_t n_blocks, const uint32_t* block_cluster,
                                                const uint8_t* cluster_params, uint32_t n_clusters,
                                                uint32_t n_parents, const uint32_t* cand_offsets, const uint32_t* cand_indices, const uint8_t* block_parent,
                                                int perceptual, uint32_t* out_best_cluster);

/* basisu_frontend::create_optimized_selector_codebook (frontend.cpp:2259-2354). blocks: m_encoded_blocks (8 B each). */
ORC_API void orc_create_optimized_selector_codebook(const uint8_t* pixel_blocks, const uint8_t* encoded_blocks, uint32_t n_clusters,
                                                    const uint32_t* offsets, const uint32_t* block_indices, int perceptual,
                                                    uint8_t* inout_selector_blocks /* 8 B per cluster; empty clusters untouched */);

/* basisu_frontend::find_optimal_selector_clusters_for_each_block CPU branch (frontend.cpp:2534-2706), levels >= 1.
   selector_blocks: m_optimized_cluster_selectors (8 B each). Candidate CSR as for refine. chunk = job size (2048 in the reference;
   it bounds the "same pixels as previous block" shortcut). Rewrites encoded_blocks' selector bits in place. */
ORC_API void orc_find_optimal_selector_clusters(const uint8_t* pixel_blocks, uint8_t* encoded_blocks, uint32_t n_blocks,
                                                const uint8_t* selector_blocks, uint32_t n_selectors,
                                                uint32_t n_parents, const uint32_t* cand_offsets, const uint32_t* cand_indices, const uint8_t* block_parent,
                                                int perceptual, uint32_t chunk, uint32_t* out_block_selector_cluster);

/* init_endpoint_training_vectors (frontend.cpp:825-866): per block 6 floats (low rgb, high rgb)/255. */
ORC_API void orc_endpoint_training_vectors(const uint8_t* etc1s_blocks, uint32_t n_blocks, float* out6);
/* generate_selector_clusters training part (frontend.cpp:2155-2183): per block 16 floats + u64 weight. */
ORC_API void orc_selector_training_vectors(const uint8_t* encoded_blocks, uint32_t n_blocks, int perceptual, float* out16, uint64_t* out_weight);

#ifdef __cplusplus
}
#endif
#endif
