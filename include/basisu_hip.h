/* include/basisu_hip.h -- C ABI of libbasisu_hip.so, the MI355X (gfx950) replacement for the reference's accelerator seam.
 *
 * The reference's seam is encoder/basisu_opencl.h (namespace basisu, ten entry points, opaque per-thread context).
 * Section 1 below exports the same ten operations with the same POD layouts, ownership and error conventions, so that a
 * reference maintainer can bind them from basisu_opencl.cpp's call sites one-for-one (see INTEGRATION.md for the shim).
 * Section 2 is the device-resident layer the ETC1S frontend actually runs on (stream-ordered, device pointers, no
 * implicit copies); it also covers the stages the reference never offloaded (frontend.cpp CPU-only branches).
 *
 * Conventions (same as basisu_opencl.h):
 *   - every int-returning function returns 1 on success and 0 on failure; nothing throws, nothing aborts;
 *     on failure the outputs are untouched or unspecified and the caller falls back / reports (frontend.cpp:757-762);
 *   - host pointers are caller-owned and only used during the call; the library owns all device memory it allocates;
 *   - one context per calling thread; calls on one context are serialised on its HIP stream;
 *   - bu_hip_init() is process-global and not re-entrant (opencl.cpp:730-736).
 */
#ifndef BASISU_HIP_H
#define BASISU_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define BU_HIP_API __attribute__((visibility("default")))
#else
#define BU_HIP_API
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * Section 1 -- drop-in for encoder/basisu_opencl.h
 * ------------------------------------------------------------------------------------------------------------------ */

typedef struct bu_hip_context bu_hip_context; /* = basisu::opencl_context (basisu_opencl.h:28-31) */

#pragma pack(push, 1)
typedef struct { uint8_t m_pixels[16][4]; } bu_pixel_block;          /* = cl_pixel_block, basisu_opencl.h:37-40: [y*4+x] RGBA */
typedef struct { uint8_t m_bytes[8]; } bu_etc_block;                 /* = basisu::etc_block, basisu_etc.h:91-103 (big-endian u64) */
typedef struct { uint8_t r, g, b, a; } bu_color_rgba;                /* = basisu::color_rgba, basisu_enc.h:893-907 */
typedef struct { uint64_t m_total_pixels, m_first_pixel_index; } bu_pixel_cluster;      /* = cl_pixel_cluster, basisu_opencl.h:53-57 */
typedef struct { uint16_t m_first_cluster_ofs, m_num_clusters, m_cur_cluster_index; uint8_t m_cur_cluster_etc_inten; } bu_block_info;   /* = cl_block_info_struct :73-79 */
typedef struct { bu_color_rgba m_unscaled_color; uint8_t m_etc_inten; uint16_t m_cluster_index; } bu_endpoint_cluster;               /* = cl_endpoint_cluster_struct :81-86 */
typedef struct { uint32_t m_packed_selectors; } bu_fosc_selector;    /* = fosc_selector_struct :101-104 */
typedef struct { bu_color_rgba m_etc_color5_inten; uint32_t m_first_selector, m_num_selectors; } bu_fosc_block;                       /* = fosc_block_struct :106-111 */
#pragma pack(pop)

#define BU_HIP_ENCODE_ETC1S_MAX_PERMS 165u /* = OPENCL_ENCODE_ETC1S_MAX_PERMS, basisu_opencl.h:44 */

BU_HIP_API int  bu_hip_init(int force_serialization);     /* opencl_init            basisu_opencl.h:24 */
BU_HIP_API void bu_hip_deinit(void);                      /* opencl_deinit          :25 */
BU_HIP_API int  bu_hip_is_available(void);                /* opencl_is_available    :26 */
BU_HIP_API bu_hip_context* bu_hip_create_context(void);   /* opencl_create_context  :33 (current HIP device) */
BU_HIP_API void bu_hip_destroy_context(bu_hip_context*);  /* opencl_destroy_context :34 */

/* opencl_set_pixel_blocks :46 -- uploads once; the blocks stay resident in the context */
BU_HIP_API int bu_hip_set_pixel_blocks(bu_hip_context*, size_t total_blocks, const bu_pixel_block* pixel_blocks);
/* opencl_encode_etc1s_blocks :48 -- total_perms in {4,16,64,165} selects the etc1_optimizer quality (fast/medium/slow/uber); a value off the table takes the next
 * one up (<= 4 fast, <= 16 medium, <= 64 slow, above that uber) */
BU_HIP_API int bu_hip_encode_etc1s_blocks(bu_hip_context*, bu_etc_block* output_blocks, int perceptual, uint32_t total_perms);
/* opencl_encode_etc1s_pixel_clusters :60-68 -- weighted, de-duplicated pixel lists: cluster c is pixels[first .. first + total) with multiplicities pixel_weights[..]
 * (zero weights are allowed inside a cluster whose weights do not all vanish). Needs no resident pixel blocks.
 *   - total_perms as above, except that the cluster fit has no FAST quality (frontend.cpp:1530-1533): 4 is treated as 16.
 *   - output_blocks[c] is the ETC1S block of the fitted colour5 + intensity table and nothing else: colour5 in the top five bits of bytes 0-2 with zero deltas,
 *     BOTH table fields of byte 3 = the table, diff and flip bits set, the four selector bytes zero.
 *   - The device layer fits unweighted lists of 8-texel training vectors, so a cluster is written out weight by weight, and where its total n is no multiple
 *     of 8 the whole list is written 8 / gcd(n, 8) times over. Errors scale by that factor and the argmin does not move; the float colour mean the optimizer
 *     starts from is unchanged as long as 255 * n * 8 / gcd(n, 8) < 2^24 (every float sum exact) -- the exact-parity regime: there the block is the one
 *     etc1_optimizer gives for the list itself. Beyond it the repeated list's mean is a sum of rounded adds, and equality with the unrepeated list is a
 *     property of the input, not a guarantee (tests/test_gpu_seam_section1.py holds two such lists of 20,001 and 66,001 pixels to it).
 *   - Refused (0, nothing written): a cluster that reaches past total_pixels, a cluster whose weights are all zero, a cluster of more than 2^31 - 1 texels
 *     after expansion, more than 2^31 - 1 texels after expansion over the WHOLE call (what 32-bit texel arithmetic addresses; checked before anything is
 *     expanded), null pointers with non-zero counts. */
BU_HIP_API int bu_hip_encode_etc1s_pixel_clusters(bu_hip_context*, bu_etc_block* output_blocks, uint32_t total_clusters,
    const bu_pixel_cluster* clusters, uint64_t total_pixels, const bu_color_rgba* pixels, const uint32_t* pixel_weights,
    int perceptual, uint32_t total_perms);
/* opencl_refine_endpoint_clusterization :89-96 -- per block the best cluster of its candidate window [m_first_cluster_ofs, + m_num_clusters) of cluster_info,
 * returned as that entry's m_cluster_index (frontend.cpp:1684-1750, ocl_kernels.cl:1063-1136).
 *   - Windows are told apart by (first, count): they may overlap, nest or share a first offset, the layout may hold empty parents, and a cluster may be filed in
 *     several windows (frontend.cpp:1706). At most 255 DISTINCT windows per call.
 *   - A block's window is never empty and lies inside cluster_info, and the block's m_cur_cluster_index is the m_cluster_index of one of its entries (the reference
 *     always files it there, frontend.cpp:971-996): the intensity filter and the tie rule go by that entry. m_cur_cluster_etc_inten is not read.
 *   - Ties go to the block's current cluster, otherwise to the lower position. sorted_block_indices only orders the reference's work items: not read, may be NULL.
 *   - Refused on the host (0, a text in bu_hip_last_error, nothing written, nothing launched): a window past the end, an empty window, a current cluster that is
 *     not in its window, a 256th window, null pointers with non-zero counts. */
BU_HIP_API int bu_hip_refine_endpoint_clusterization(bu_hip_context*, const bu_block_info* pixel_block_info, uint32_t total_clusters,
    const bu_endpoint_cluster* cluster_info, const uint32_t* sorted_block_indices, uint32_t* output_cluster_indices, int perceptual);
/* opencl_find_optimal_selector_clusters_for_each_block :120-127 -- per block the selector of its window [m_first_selector, + m_num_selectors) of input_selectors
 * (texel y * 4 + x at bits [2p, 2p + 2), frontend.cpp:2462-2464) with the least error under the block's colour5 + table, returned as
 * selector_cluster_indices[position in input_selectors] (any mapping, not only the identity); the first minimum in window order wins; no "same tile as the previous
 * block" shortcut (ocl_kernels.cl:1159-1216). Windows as for refine: overlapping, nested, sharing a first offset, a selector in several of them; at most 255 distinct
 * ones; a block's own window non-empty and inside input_selectors -- anything else is refused on the host in the same way. */
BU_HIP_API int bu_hip_find_optimal_selector_clusters_for_each_block(bu_hip_context*, const bu_fosc_block* input_block_info,
    uint32_t total_input_selectors, const bu_fosc_selector* input_selectors, const uint32_t* selector_cluster_indices,
    uint32_t* output_selector_cluster_indices, int perceptual);
/* opencl_determine_selectors :137-141 */
BU_HIP_API int bu_hip_determine_selectors(bu_hip_context*, const bu_color_rgba* input_etc_color5_and_inten, bu_etc_block* output_blocks, int perceptual);

/* NEW seam (the reference has none): basisu::encode_uastc (encoder/basisu_uastc_enc.h:69, uastc_enc.cpp:3126) for every
 * resident pixel block, replacing the per-block job loop of basis_compressor::encode_slices_to_uastc_4x4_ldr (comp.cpp:2020-2033).
 * `flags` are the reference's pack flags verbatim: cPackUASTCLevel* in the low bits, cPackUASTCFavor*, cPackUASTCETC1* (uastc_enc.h:24-66).
 * Output blocks are bit-identical to the reference's for every level and flag. */
typedef struct { uint8_t m_bytes[16]; } bu_uastc_block;             /* = basist::uastc_block, transcoder/basisu_transcoder_uastc.h:198-205 */
BU_HIP_API int bu_hip_encode_uastc_blocks(bu_hip_context*, bu_uastc_block* output_blocks, uint32_t flags);

/* ------------------------------------------------------------------------------------------------------------------
 * Section 2 -- device-resident layer. All `d_` pointers are DEVICE pointers valid on the context's device; every call is
 * enqueued on the context's stream and returns without synchronising unless stated. `h_` pointers are host pointers.
 * ------------------------------------------------------------------------------------------------------------------ */

/* bu_hip_destroy_context PARKS a healthy context instead of tearing it down: its streams, workspaces and block pool (whatever it grew to -- up to 16 GiB of
 * cached device blocks) stay allocated and the next bu_hip_create_context* on that device gets it back warm (the reference's basis_parallel_compress creates and
 * destroys a context per image; a context's worth of hipMalloc / hipFree calls are device-wide synchronisations that stall every other image's stream). At most
 * BU_HIP_PARKED_CONTEXTS (default 16; 0 = destroy means destroy) are kept; bu_hip_deinit releases them all. A context whose streams report an error is never parked.
 * A process that shares the GPU with other allocators and wants the memory back at once sets BU_HIP_PARKED_CONTEXTS=0 or calls bu_hip_deinit. */
BU_HIP_API bu_hip_context* bu_hip_create_context_on(int device);
/* Objects that keep device memory of a context (a resident frontend, say) may ask to be told when it is being destroyed: fn(user) runs at the
 * start of bu_hip_destroy_context, while the context still works, so that they can let go of their buffers instead of freeing them through a
 * dead context later. bu_hip_cancel_on_destroy removes a registration (same fn and user). */
typedef void (*bu_hip_destroy_fn)(void* user);
BU_HIP_API int  bu_hip_on_destroy(bu_hip_context*, bu_hip_destroy_fn fn, void* user);
BU_HIP_API void bu_hip_cancel_on_destroy(bu_hip_context*, bu_hip_destroy_fn fn, void* user);
BU_HIP_API int   bu_hip_context_device(const bu_hip_context*);
/* Use an externally owned hipStream_t (e.g. torch's current stream) instead of the context's own; NULL restores it. */
BU_HIP_API int   bu_hip_set_stream(bu_hip_context*, void* hip_stream);
BU_HIP_API void* bu_hip_get_stream(bu_hip_context*);
BU_HIP_API int   bu_hip_sync(bu_hip_context*);
/* Tuning of the device paths that have more than one (all bit-identical: tests run every one of them). Each field has a measured default; the
 * environment variable named beside it overrides that default ONCE per process (read when the first context is created); bu_hip_set_tuning overrides both for one
 * context (trees created on it afterwards take the values; NULL restores the process defaults; parking a context restores them too). Versioned by size:
 * struct_bytes = sizeof(bu_hip_tuning) of the caller's header, fields a caller does not have keep their defaults. */
typedef struct bu_hip_tuning {
    uint32_t struct_bytes;
    uint32_t tsvq_wide_min;       /* BU_TSVQ_WIDE_MIN      8192   selector (packed) nodes of this many members and more take the many-workgroup passes; 0 (BU_TSVQ_WIDE=0) = never */
    uint32_t tsvq_wide6_min;      /* BU_TSVQ_WIDE6_MIN     8192   the same for endpoint (6-float) nodes; 0 (BU_TSVQ_WIDE6=0 or BU_TSVQ_WIDE=0) = never */
    uint32_t tsvq_wide_cov_min;   /* BU_TSVQ_WIDE_COV_MIN  98304  batches whose largest node is smaller run the covariance pass chained instead of through the maps */
    uint32_t tsvq_windows;        /* BU_TSVQ_WINDOWS       0      pre-composed 64-block windows in the walks: 0 = batches averaging >= 2048 blocks per node, 1 = always, 2 (env "0") = never */
    uint32_t tsvq_dense_min;      /* BU_TSVQ_DENSE_MIN     257    rounds of this many nodes take the 128-register (two workgroups per CU) build of the exact split kernel; 0 = never */
    uint32_t tsvq_zero_copy;      /* BU_TSVQ_ZEROCOPY      1      node / result records of a round in coherent pinned memory + a flag the host looks at; 0 = staged copies + synchronise */
    uint32_t tsvq_chained_only;   /* BU_TSVQ_CHAINED       0      1 = every float sum member by member in one workgroup per node (the slowest path; what the others are tested against) */
    uint32_t tsvq_poll;           /* BU_TSVQ_POLL          0      waiting for a round: 0 = spin when this is the process's only context, else yield / nap; 1 (spin) / 2 (yield) force it */
    uint32_t refine_unsorted;     /*                       0      refine_endpoint_clusterization: 0 = sorted candidate lists, one block per lane (blocks bucketed by parent and table; the perceptual metric -- the linear metric takes 2's path); 1 = the unsorted kernel (the one lists beyond 65,535 entries take anyway); 2 = sorted lists, one block per wave. bu_hip_refine_path tells which one a call takes */
    uint32_t debug;               /* BU_TSVQ_ROUNDS = 1 | BU_TSVQ_SERIAL = 2 | BU_TSVQ_STATS = 4: developer aids (round time line on stderr, one node per round, walk statistics) */
    uint32_t tsvq_deep_levels;    /* BU_TSVQ_DEEP          0      deep rounds: generations of descendants of a round's one-workgroup nodes split in the same round trip (bu_hip_tsvq_split_deep); 0 = none, <= 2. Measured SLOWER at 4096^2 (17.4-18.0 against 16.8-17.6 ms per step: the rounds it saves cost ~50 us each, the splits nobody pops cost device time in rounds that fill the chip), hence off */
    uint32_t uastc_walk_cus;      /* BU_UASTC_WALK_CUS     0      UASTC pipeline lanes: this many CUs (every (CUs / n)-th one) carry the strip walks of uastc_rdo and nothing else -- the lanes' other kernels are masked off them; 0 = no reservation */
    uint32_t codebook_wide_min;   /* BU_CODEBOOK_WIDE_MIN  32768  endpoint clusters of this many texels and more are fitted by many workgroups (a launch per pass over the texels of all of them) instead of one workgroup each; 0 = never */
} bu_hip_tuning;
BU_HIP_API void bu_hip_get_tuning(const bu_hip_context* /* NULL: the process defaults */, bu_hip_tuning* out, uint32_t struct_bytes);
BU_HIP_API int  bu_hip_set_tuning(bu_hip_context*, const bu_hip_tuning* /* NULL: back to the process defaults */);

/* Cooperative waiting. By default a call that needs a device result blocks its host thread (hipStreamSynchronize, or a look-loop on a zero-copy flag). A host that
 * drives SEVERAL contexts from ONE thread -- bu_frontend_pipeline_* (basisu_hip_frontend.h): every image in flight is a task with a stack of its own on the pipeline's
 * one driver thread -- installs a hook instead: wherever a call on this context would block, the stream is only queried, and fn(user) is called between the looks;
 * fn switches to another task and returns when it is this one's turn again. fn NULL removes the hook (parking a context removes it too). The reference has no
 * counterpart: its opencl_context calls all end in clFinish (opencl.cpp:972-976), one blocked host thread per image in flight (comp.cpp:5466-5559). */
typedef void (*bu_hip_wait_fn)(void* user);
BU_HIP_API int   bu_hip_set_wait_hook(bu_hip_context*, bu_hip_wait_fn fn, void* user);
BU_HIP_API const char* bu_hip_last_error(const bu_hip_context*); /* NULL context -> last global (init) error */
/* For the libraries layered on this one (libbasisu_frontend.so refuses a resampling plan on the host, before any call here): the text a failed call of theirs leaves
 * for bu_hip_last_error, cut at 511 characters. NULL context -> the global text. */
BU_HIP_API void bu_hip_set_last_error(bu_hip_context*, const char* text);

/* Per-kernel timing with HIP events recorded on the launch stream around every section-2 kernel. enable(1) resets the totals and times every region; enable(2) only
 * the regions that are ONE kernel launch each (per-block and per-cluster kernels) -- the regions of many launches (codebook builders' rounds, de-duplication, list
 * bookkeeping: names tsvq_*, unique_*, map_*, kmeans_*) go untimed, and the step runs as it does without instrumentation (an event between two kernels of a chain
 * costs the chain ~3 us, and a round's two kinds of nodes only share the device when nobody times them apart: 0.5-0.7 ms of a 17 ms step, tools/headline_ab.py).
 * read() synchronises the pending events and returns the number of distinct kernels (names are static strings). */
BU_HIP_API int      bu_hip_profile_enable(bu_hip_context*, int on);
BU_HIP_API uint32_t bu_hip_profile_read(bu_hip_context*, const char** names, double* total_ms, uint32_t* launches, uint32_t cap);

BU_HIP_API void* bu_hip_malloc(bu_hip_context*, size_t bytes);
BU_HIP_API void  bu_hip_free(bu_hip_context*, void* d_ptr);
BU_HIP_API int   bu_hip_memcpy_h2d(bu_hip_context*, void* d_dst, const void* h_src, size_t bytes); /* synchronises */
/* ... stream-ordered instead of blocking: the source has been copied out when the call returns (it may be released), the copy itself is ordered on the context's stream */
BU_HIP_API int bu_hip_memcpy_h2d_async(bu_hip_context*, void* d_dst, const void* h_src, size_t bytes);
BU_HIP_API int   bu_hip_memcpy_d2h(bu_hip_context*, void* h_dst, const void* d_src, size_t bytes); /* synchronises */
/* A download that nobody waits for yet: the bytes d_src holds once everything enqueued on the context's stream so far has run are brought to h_dst (pageable or pinned)
 * by the copy engine on a stream of their own, driven by a helper thread, while the caller goes on enqueueing work. bu_hip_download_wait blocks until they are there
 * (1 = arrived) and releases the handle; it must be called exactly once per handle, before h_dst is released and before anything overwrites d_src. NULL: not available
 * on this context now (a wait hook is installed, or a resource could not be had) -- use bu_hip_memcpy_d2h. */
/* Page-locked host memory (for callers that want their tiles taken by the copy engine as they are: bu_hip_k_upload_and_encode_etc1s_blocks, bu_frontend_init with host tiles). */
BU_HIP_API void* bu_hip_host_alloc(size_t bytes);
BU_HIP_API void  bu_hip_host_free(void* p);
typedef struct bu_hip_download bu_hip_download;
BU_HIP_API bu_hip_download* bu_hip_download_begin(bu_hip_context*, void* h_dst, const void* d_src, size_t bytes);
BU_HIP_API int   bu_hip_download_wait(bu_hip_download*);
BU_HIP_API int   bu_hip_memset(bu_hip_context*, void* d_dst, int value, size_t bytes);
BU_HIP_API int   bu_hip_memcpy_d2d(bu_hip_context*, void* d_dst, const void* d_src, size_t bytes); /* stream-ordered */

/* Adopt pixel blocks that are already resident (no copy, not owned). Counterpart of bu_hip_set_pixel_blocks. */
BU_HIP_API int   bu_hip_set_pixel_blocks_device(bu_hip_context*, size_t total_blocks, const void* d_pixel_blocks);
BU_HIP_API const void* bu_hip_get_pixel_blocks_device(const bu_hip_context*, size_t* total_blocks);

/* Input side: basis_compressor::extract_source_blocks (comp.cpp:3207-3268) on the device. d_rgba is a resident RGBA8 raster
 * (row pitch in bytes >= 4*width); writes ceil(w/4)*ceil(h/4) tiles in block-raster order with the right/bottom edges clamped like
 * image::extract_block_clamped. The result can be adopted with bu_hip_set_pixel_blocks_device. */
BU_HIP_API int bu_hip_k_extract_blocks(bu_hip_context*, const void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* d_out_pixel_blocks);

/* The same for EVERY slice of a call in one launch: what a multi-image call (array layers, cubemap faces, video frames, each with its levels, for ETC1S with alpha a
 * colour and an alpha slice per level) would otherwise pay a launch per slice for. `slices` is a HOST array of n records; slice i's ceil(w/4)*ceil(h/4) tiles are
 * written in block-raster order from tile first_block on (64 bytes per tile, counted from d_out_pixel_blocks), edges clamped exactly as bu_hip_k_extract_blocks
 * clamps them. mode: BU_HIP_SLICE_AS_IS the pixels as they are; BU_HIP_SLICE_RGB (r, g, b, 255); BU_HIP_SLICE_ALPHA (a, a, a, 255) -- the two ETC1S slices of a
 * level with alpha (comp.cpp:2883-2903) straight from the RGBA raster, so no split plane is needed. The records and the table of the slices' tile counts go up in
 * one stream-ordered copy; `slices` may be released on return. One launch on the context's stream, no synchronisation.
 * Fails -- nothing copied, nothing launched, nothing written, the reason by name in bu_hip_last_error -- on n == 0, a null pointer, an output that is not 16-byte
 * aligned, a slice of zero size, a pitch below 4 * width, an unknown mode, a first_block that is not at or beyond the end of the slice before it (the ranges must
 * ascend and may not overlap; gaps are left untouched), or more than 2^30 tiles in all. */
enum { BU_HIP_SLICE_AS_IS = 0, BU_HIP_SLICE_RGB = 1, BU_HIP_SLICE_ALPHA = 2 };
typedef struct bu_hip_slice_source {
    const void* d_raster;        /* resident RGBA8 raster */
    uint32_t width, height;      /* pixels */
    uint32_t pitch_bytes;        /* >= 4 * width */
    uint32_t mode;               /* BU_HIP_SLICE_* */
    uint64_t first_block;        /* index of the slice's first tile in d_out_pixel_blocks */
} bu_hip_slice_source;
BU_HIP_API int bu_hip_k_extract_slices(bu_hip_context*, const bu_hip_slice_source* slices, uint32_t n, void* d_out_pixel_blocks);

/* The compressor's source-image options (basis_compressor::read_source_images, comp.cpp:2569-2640) over resident RGBA8 rasters: 4-byte aligned, row pitches in
 * bytes (>= 4 * width, multiples of 4), 1..16384 pixels each way. Per pixel, in the reference's order (csrc/source_prep.h): image::renormalize_normal_map when
 * `renormalize`; the swizzle, one source-channel index 0..3 per byte (s0 | s1 << 8 | s2 << 16 | s3 << 24; 0x03020100 = none, 0x01000000 = the tool's
 * -separate_rg_to_color_alpha); the alpha policy -- force_alpha or s3 != 3: alpha is kept and the image has alpha; else without check_for_alpha: alpha becomes 255;
 * else the image has alpha where a prepared alpha value is below 255 --; and with y_flip destination row y is made from source row height - 1 - y.
 * *out_has_alpha (may be NULL) gets the policy's answer, *out_alpha_below_255 (may be NULL) whether any prepared alpha value is below 255 (what image::has_alpha
 * says of the prepared raster). d_dst may equal d_src unless y_flip is set. One launch on the context's stream; the call synchronises once to read the flag.
 * bu_hip_k_renormalize_normal_map: image::renormalize_normal_map in place (the mip levels of m_mip_renormalize); one launch, no synchronisation.
 * bu_hip_k_split_alpha: the two ETC1S slices of a level with alpha (comp.cpp:2883-2903): (r, g, b, 255) to d_out_rgb, which may equal d_rgba, and (a, a, a, 255) to
 * d_out_alpha, which may not; one read, two writes, one launch, no synchronisation. Only width x height pixels are written: a padded pitch stays untouched.
 * Each fails -- nothing launched, nothing written, the reason by name in bu_hip_last_error -- on a null pointer, a zero dimension, a pitch below 4 * width, a
 * misaligned raster or pitch, more than 16384 pixels a side, a swizzle entry above 3, or source equal to destination with y_flip. */
BU_HIP_API int bu_hip_k_prepare_source(bu_hip_context*, const void* d_src, uint32_t width, uint32_t height, uint32_t src_pitch_bytes, void* d_dst, uint32_t dst_pitch_bytes,
        int renormalize, uint32_t swizzle, int check_for_alpha, int force_alpha, int y_flip, uint32_t* out_has_alpha, uint32_t* out_alpha_below_255);
BU_HIP_API int bu_hip_k_renormalize_normal_map(bu_hip_context*, void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes);
BU_HIP_API int bu_hip_k_split_alpha(bu_hip_context*, const void* d_rgba, uint32_t width, uint32_t height, uint32_t pitch_bytes, void* d_out_rgb, uint32_t rgb_pitch_bytes,
        void* d_out_alpha, uint32_t alpha_pitch_bytes);

/* Mip levels the caller made (basis_compressor_params::m_source_mipmap_images, comp.cpp:2737-2818; the levels of a .dds source, comp.cpp:2310-2439) into tight
 * RGBA8 rasters: every level of every image of a call from ONE resident payload -- the levels' bytes back to back, or a .dds file's payload as it was uploaded -- in
 * ONE launch. `records` is a HOST array of n records. Level i's width x height pixels are read as tight 32-bit pixels from d_payload + src_offset, each pixel's
 * bytes permuted by `selector` -- byte k of the word names the source byte 0..3 of output channel k: 0x03020100 copies, 0x03000102 reads B8G8R8A8, and the host
 * composes the byte order with the compressor's swizzle, which is all the reference applies to a supplied level -- and written as a tight raster to
 * d_out + dst_offset. d_flags[i] (n device words, cleared by the call) becomes 1 where a written alpha value of level i is not 255: image::has_alpha of the level
 * as written. The rasters must not overlap each other or the payload. The records and the table of their pixel counts go up in one stream-ordered copy; `records`
 * may be released on return. One launch on the context's stream, no synchronisation: the flags are read after bu_hip_sync or by a blocking copy.
 * n == 0 succeeds and does nothing. Fails -- nothing copied, nothing launched, nothing written, the reason by name in bu_hip_last_error -- on a null pointer, a
 * payload, output or flags pointer or an offset that is not 4-byte aligned, a level that ends past payload_bytes or past out_bytes, a size outside 1..16384, a
 * selector entry above 3, more than 0xFFFFFF records (BASISU_MAX_SLICES), or more than 2^30 pixels in all. */
typedef struct bu_hip_mip_level_record {
    uint64_t src_offset;         /* bytes from d_payload, a multiple of 4 */
    uint64_t dst_offset;         /* bytes from d_out, a multiple of 4 */
    uint32_t width, height;      /* pixels, 1..16384 */
    uint32_t selector;           /* s0 | s1 << 8 | s2 << 16 | s3 << 24, each 0..3 */
    uint32_t reserved;           /* 0 */
} bu_hip_mip_level_record;
BU_HIP_API int bu_hip_k_prepare_mip_levels(bu_hip_context*, const void* d_payload, size_t payload_bytes, const bu_hip_mip_level_record* records, uint32_t n,
        void* d_out, size_t out_bytes, uint32_t* d_flags);

/* etc1_optimizer quality (basis_etc_quality, basisu_etc.h:794-801) */
enum { BU_ETC_QUALITY_FAST = 0, BU_ETC_QUALITY_MEDIUM = 1, BU_ETC_QUALITY_SLOW = 2, BU_ETC_QUALITY_UBER = 3 };

/* a6  basisu_frontend::init_etc1_images (frontend.cpp:733-823): per block etc1_optimizer, n = 16. out: n_blocks x 8 B. */
BU_HIP_API int bu_hip_k_encode_etc1s_blocks(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_blocks, int quality, int perceptual, void* d_out_etc_blocks);
/*     The same over tiles that are still in HOST memory, as one pipeline: the tiles go to d_pixel_blocks in 4 MiB pieces on the context's side stream (page-locked source
 *     memory as it is, pageable memory through a pinned ring filled by BU_UPLOAD_THREADS (default 4) helper threads) and piece i's kernel starts behind piece i's copy, so
 *     the transfer hides behind the kernel (SURVEY 8d figure (i): the hot path with the H2D inside). On return h_pixel_blocks may be released; the device side is ordered
 *     on the context's stream. Replaces opencl_set_pixel_blocks + opencl_encode_etc1s_blocks (encoder/basisu_opencl.h:112-116) for a caller that wants both. */
BU_HIP_API int bu_hip_k_upload_and_encode_etc1s_blocks(bu_hip_context*, void* d_pixel_blocks, const void* h_pixel_blocks, uint32_t n_blocks, int quality, int perceptual,
    void* d_out_etc_blocks);
/* a7  init_endpoint_training_vectors (frontend.cpp:825-866): per block 6 floats (low rgb, high rgb)/255. */
BU_HIP_API int bu_hip_k_endpoint_training_vectors(bu_hip_context*, const void* d_etc_blocks, uint32_t n_blocks, float* d_out_vec6);
/* a9  generate_endpoint_codebook (frontend.cpp:1214-1617), CPU semantics incl. step > 0. Clusters are CSR lists of
 *     training-vector indices (block*2+subblock); h_offsets is a HOST array of n_clusters+1 entries (used to schedule
 *     large clusters first), d_offsets its device copy. d_params: n_clusters x {r5,g5,b5,inten}; d_err: u64; d_valid: u8. */
BU_HIP_API int bu_hip_k_generate_endpoint_codebook(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_clusters,
    const uint32_t* h_offsets, const uint32_t* d_offsets, const uint32_t* d_indices, int quality, int perceptual, uint32_t step,
    uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid);
/*     Clusters of bu_hip_tuning::codebook_wide_min texels and more (a sky, a flat wall, a constant alpha plane: 10^5-10^7 texels in ONE cluster) are fitted by many
 *     workgroups each -- a launch per pass over the texels of all of them -- with the same results, the order-dependent float colour mean included (H4).
 *     Test hook: that mean (etc.cpp:1034-1041: running float sum in texel order / count), evaluated the many-workgroup way for EVERY cluster given; h_out: 3 floats each. */
BU_HIP_API int bu_hip_k_cluster_colour_means(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_clusters, const uint32_t* h_offsets, const uint32_t* d_indices, float* h_out);
/* a15 refine_block_endpoints_given_selectors (frontend.cpp:2718-2976, ETC1S levels 4-6): per endpoint cluster, the uber-quality
 *     etc1_optimizer with the selectors of d_encoded_blocks held fixed (m_pForce_selectors). Lists are CSR over training-vector indices
 *     like a9 and MAY contain duplicates (the reference's m_subblocks lists grow from iteration to iteration). Outputs per cluster:
 *     the refitted {r5,g5,b5,inten}, its error, a validity flag, and the CURRENT error of the listed sub-blocks under their blocks'
 *     present colours -- the caller applies the refit only where new error < current error (:2822). An EMPTY list is allowed (a cluster
 *     no block uses any more): no texel is read for it and its four output entries are unspecified -- callers skip them. */
BU_HIP_API int bu_hip_k_refit_endpoints_given_selectors(bu_hip_context*, const void* d_pixel_blocks, const void* d_encoded_blocks, uint32_t n_clusters,
    const uint32_t* h_offsets, const uint32_t* d_offsets, const uint32_t* d_indices, int perceptual,
    uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid, uint64_t* d_current_err);
/* f2  the same fit at a chosen optimizer quality (BU_ETC_QUALITY_SLOW or _UBER), for basisu_frontend::reoptimize_remapped_endpoints
 *     (frontend.cpp:2996-3104: slow below compression level 6), the backend's call back into the frontend. */
BU_HIP_API int bu_hip_k_refit_endpoints_given_selectors_q(bu_hip_context*, const void* d_pixel_blocks, const void* d_encoded_blocks, uint32_t n_clusters,
    const uint32_t* h_offsets, const uint32_t* d_offsets, const uint32_t* d_indices, int quality, int perceptual,
    uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid, uint64_t* d_current_err);
/* a15 compute_endpoint_subblock_error_vec (frontend.cpp:1006-1091): u64 error of every training vector (block*2+subblock) under the
 *     endpoints of its block's cluster; feeds introduce_new_endpoint_clusters. d_out_err: 2*n_blocks entries. */
BU_HIP_API int bu_hip_k_subblock_errors(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_blocks, const uint32_t* d_block_cluster,
    const uint8_t* d_cluster_params, int perceptual, uint64_t* d_out_err);
/* The stateless part of basisu_backend::create_encoder_blocks (encoder/basisu_backend.cpp:406-617) for one slice of num_blocks_x x num_blocks_y blocks starting at first_block:
 * d_own_err[b] = the block's error as encoded (cur_err of :507 / :841); with_neighbours: d_neighbour_err[b * 3 + p] = its error under the endpoints of its left / upper / upper-left
 * neighbour (g_endpoint_preds order) with its own selectors, ~0u where the walk does not ask for it (edge, a neighbour already shares its endpoints, zero error). The decisions that chain
 * from block to block stay on the host (include/basisu_hip_backend.h). d_cluster_params: r5, g5, b5, intensity table per endpoint cluster. */
BU_HIP_API int bu_hip_k_backend_block_errors(bu_hip_context*, const void* d_pixel_blocks, const void* d_etc_blocks, const uint32_t* d_block_cluster, const uint8_t* d_cluster_params,
    uint32_t first_block, uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t n_clusters, int perceptual, int with_neighbours, uint32_t* d_own_err, uint32_t* d_neighbour_err);
/* a9 for one of `parts` equal shares of the clusters (multi-GPU): the clusters at positions part, part + parts, ... of the
 *     size-descending order. Entries of clusters outside the share are neither read nor written. */
BU_HIP_API int bu_hip_k_generate_endpoint_codebook_part(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_clusters,
    const uint32_t* h_offsets, const uint32_t* d_offsets, const uint32_t* d_indices, int quality, int perceptual, uint32_t step,
    uint8_t* d_params, uint64_t* d_err, uint8_t* d_valid, uint32_t part, uint32_t parts);
/* a10 refine_endpoint_clusterization (frontend.cpp:1648-1917) for BOTH hierarchical (n_parents > 0: candidates are
 *     d_cand_indices[d_cand_offsets[p] .. d_cand_offsets[p+1]) for the block's parent p) and flat codebooks (n_parents == 0). */
BU_HIP_API int bu_hip_k_refine_endpoint_clusterization(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_blocks,
    const uint32_t* d_block_cluster, const uint8_t* d_cluster_params, uint32_t n_clusters, uint32_t n_parents,
    const uint32_t* d_cand_offsets, const uint32_t* d_cand_indices, const uint8_t* d_block_parent, int perceptual, uint32_t* d_out_best_cluster);
/* The path (bu_hip_tuning::refine_unsorted: 0, 1 or 2) a refine call with these arguments takes on this context (NULL: under the process defaults). */
BU_HIP_API int bu_hip_refine_path(const bu_hip_context*, uint32_t n_clusters, uint32_t n_parents, int perceptual);
/* a11 create_initial_packed_texture (frontend.cpp:2014-2096): d_block_cluster may be NULL, then d_color5_inten is per block. */
/* f4  One separable resampling step of mip generation on a resident RGBA8 raster (basis_compressor::generate_mipmaps -> image_resample ->
 *     Resampler, comp.cpp:2146-2230, enc.cpp:1022-1180, resampler.cpp:343-435). The contributor lists of both axes (CSR: first[n+1],
 *     pixel, weight), the pass order and the two value tables (256 floats, 8192 bytes) are HOST arrays computed by the caller
 *     (libbasisu_frontend.so: bu_generate_mipmap_level does that exactly as the reference's host code); the device applies them with the
 *     reference's float operations in the reference's order. d_src: src_w x src_h, d_dst: dst_w x dst_h, tightly packed. num_comps 3
 *     or 4 (3: destination alpha = 255). */
BU_HIP_API int bu_hip_k_resample_rgba8(bu_hip_context*, const void* d_src, uint32_t src_w, uint32_t src_h, void* d_dst, uint32_t dst_w, uint32_t dst_h,
    const uint32_t* x_first, const uint16_t* x_pixel, const float* x_weight, const uint32_t* y_first, const uint16_t* y_pixel, const float* y_weight,
    int x_after_y, int srgb, const float* srgb_to_linear_256, const uint8_t* linear_to_srgb_8192, uint32_t num_comps);
BU_HIP_API int bu_hip_k_determine_selectors(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_blocks,
    const uint8_t* d_color5_inten, const uint32_t* d_block_cluster, int perceptual, void* d_out_etc_blocks);
/* a12 generate_selector_clusters training part (frontend.cpp:2155-2183): 16 floats + u64 weight per block (d_out_vec16 may be NULL). */
BU_HIP_API int bu_hip_k_selector_training_vectors(bu_hip_context*, const void* d_encoded_blocks, uint32_t n_blocks, int perceptual, float* d_out_vec16, uint64_t* d_out_weight);
/* a13 create_optimized_selector_codebook (frontend.cpp:2259-2354): CSR lists of block indices per selector cluster;
 *     rewrites the selector bytes of d_selector_blocks[cluster] (8 B each) for non-empty clusters. */
BU_HIP_API int bu_hip_k_create_optimized_selector_codebook(bu_hip_context*, const void* d_pixel_blocks, const void* d_encoded_blocks,
    uint32_t n_clusters, const uint32_t* d_offsets, const uint32_t* d_block_indices, int perceptual, void* d_selector_blocks);
/* a14 find_optimal_selector_clusters_for_each_block (frontend.cpp:2397-2715), hierarchical or flat; `chunk` reproduces the
 *     reference's "same pixels as the previous block of this job" shortcut (2048; 0 disables). Rewrites the selector bytes
 *     of d_encoded_blocks and writes the chosen cluster per block. */
BU_HIP_API int bu_hip_k_find_optimal_selector_clusters(bu_hip_context*, const void* d_pixel_blocks, void* d_encoded_blocks, uint32_t n_blocks,
    const void* d_selector_blocks, uint32_t n_selectors, uint32_t n_parents, const uint32_t* d_cand_offsets, const uint32_t* d_cand_indices,
    const uint8_t* d_block_parent, int perceptual, uint32_t chunk, uint32_t* d_out_block_selector_cluster);

/* a16-a19 encode_uastc over n_blocks resident tiles -> n_blocks x 16 B (device). Runs four kernels (classify, candidates per
 *     (block, mode job), score per (block, candidate), finish); the candidate workspace lives in the context and is reused. */
BU_HIP_API int bu_hip_k_encode_uastc_blocks(bu_hip_context*, const void* d_pixel_blocks, uint32_t n_blocks, uint32_t flags, void* d_out_uastc_blocks);
/* Bytes of context workspace that call needs (27 candidate slots x 76 B per block at level 2; 170 at level 4). */
BU_HIP_API size_t bu_hip_uastc_workspace_bytes(uint32_t n_blocks, uint32_t flags);
/* ... and what bu_hip_k_uastc_rdo needs for the same blocks cut into total_jobs strips (the two calls share the one workspace; a UASTC pipeline sizes its lanes' for the larger of the two).
 * It is bu_hip_uastc_rdo_slices_workspace_bytes of that one slice: every RDO call has the one workspace layout, so the figure includes the two regions of the strip table
 * (32 + 4 bytes per strip, each region rounded up to 256), which a single-slice call leaves unused. 0 for more than 2^31 - 1 blocks, which bu_hip_k_uastc_rdo refuses. */
BU_HIP_API size_t bu_hip_uastc_rdo_workspace_bytes(uint32_t n_blocks, uint32_t total_jobs);

/* a20 (SURVEY.md 8a "next" row f1): basisu::uastc_rdo (encoder/basisu_uastc_enc.h:139, uastc_enc.cpp:4095-4163) in place over n_blocks
 * resident UASTC blocks and the pixel blocks they were encoded from. `params` mirrors uastc_rdo_params (uastc_enc.h:94-134) field for
 * field; `flags` are the pack flags the blocks were encoded with (the hints of modified blocks are recomputed with them);
 * `total_jobs` has the reference's meaning: 0/1 = one strip, otherwise strips of n_blocks / total_jobs blocks that do not see each
 * other (comp.cpp:2076-2078 passes min(4, threads)). Output is bit-identical to the reference called with the same total_jobs.
 * Synchronises the context's stream; `out_stats` (optional) receives {modified, refined, skipped, strips}. Fails (0) like the reference
 * when a block does not unpack; refuses more than 2^31 - 1 blocks (the walk holds block indices in signed ints). */
typedef struct bu_uastc_rdo_params {
    float m_lambda;
    float m_max_allowed_rms_increase_ratio;
    float m_skip_block_rms_thresh;
    float m_max_smooth_block_std_dev;
    float m_smooth_block_max_error_scale;
    uint32_t m_lz_dict_size;
    uint32_t m_lz_literal_cost;
    uint32_t m_endpoint_refinement;
} bu_uastc_rdo_params;
BU_HIP_API void bu_hip_uastc_rdo_default_params(bu_uastc_rdo_params* out);   /* uastc_rdo_params::clear(), uastc_enc.h:101-112 */
BU_HIP_API int bu_hip_k_uastc_rdo(bu_hip_context*, void* d_uastc_blocks, const void* d_pixel_blocks, uint32_t n_blocks, const bu_uastc_rdo_params* params,
                                  uint32_t flags, uint32_t total_jobs, uint32_t out_stats[4]);
/* The same over every slice of a file in ONE pass (the reference runs uastc_rdo per slice, comp.cpp:2066-2082; the slices' chains are independent). The slices lie
 * back to back in d_uastc_blocks / d_pixel_blocks in the given order, slice s holding slice_blocks[s] blocks; each is cut into strips by total_jobs exactly as
 * bu_hip_k_uastc_rdo cuts it alone, and the strips of all slices walk side by side, the longest started first. Bytes and statistics are those of one
 * bu_hip_k_uastc_rdo call per slice. The host waits for the stream twice per call, however many slices there are. When one slice holds all the blocks the call IS
 * bu_hip_k_uastc_rdo on that slice.
 *   out_stats (may be NULL): n_slices x {modified, refined, skipped, strips}. A slice of 0 blocks does no work and reports {0, 0, 0, 1}.
 *   Refused (0, reason in bu_hip_last_error, nothing enqueued, nothing written): a null pointer, n_slices == 0, more than 2^31 - 1 blocks in all, parameters
 *   bu_hip_k_uastc_rdo refuses. A block that does not unpack fails the call at its end, as there; the error names the lowest slice that holds one.
 * bu_hip_uastc_rdo_slices_workspace_bytes: the context workspace the call needs (0 for arguments it refuses). */
BU_HIP_API int bu_hip_k_uastc_rdo_slices(bu_hip_context*, void* d_uastc_blocks, const void* d_pixel_blocks, const uint32_t* slice_blocks, uint32_t n_slices,
                                         const bu_uastc_rdo_params* params, uint32_t flags, uint32_t total_jobs, uint32_t* out_stats);
BU_HIP_API size_t bu_hip_uastc_rdo_slices_workspace_bytes(const uint32_t* slice_blocks, uint32_t n_slices, uint32_t total_jobs);
/* host-buffer form over the context's resident pixel blocks (bu_hip_set_pixel_blocks): blocks in, blocks out */
BU_HIP_API int bu_hip_uastc_rdo(bu_hip_context*, bu_uastc_block* blocks, const bu_uastc_rdo_params* params, uint32_t flags, uint32_t total_jobs,
                                uint32_t out_stats[4]);

/* encode_uastc (+ uastc_rdo) over a STREAM of images with several in flight on one GPU -- what basis_parallel_compress (comp.cpp:5466-5559) does with a job pool for
 * BASELINE configs[4]'s batch. The RDO walk is one serial chain per strip and leaves most of the chip idle (96 strips of the Kodak batch: 96 of 256 CUs for ~20 ms);
 * the pipeline owns `lanes` private streams + workspaces and ENQUEUES every submission without a host synchronisation, so the next submission's encode kernels and the
 * previous one's hint refit run beside this one's walk. Bytes out = bu_hip_k_encode_uastc_blocks followed (rdo != NULL) by bu_hip_k_uastc_rdo; `flags` as there (callers
 * add cPackUASTCFavorSimplerModes for RDO themselves, as comp.cpp:2016-2018 does).
 *   create : lanes 1..8 (3 fills an MI355X with Kodak-sized batches); max_blocks / max_total_jobs size the workspaces once (they never grow afterwards)
 *   submit : refuses (0, error text on the context, nothing enqueued, the lane as it was) null pointers, n_blocks 0, RDO parameters bu_hip_k_uastc_rdo refuses, and a
 *            submission whose workspace (the larger of bu_hip_uastc_workspace_bytes and, with rdo, bu_hip_uastc_rdo_workspace_bytes) exceeds that of create's arguments
 *   submit : d_px (n_blocks x 64 B) must stay valid and d_out (n_blocks x 16 B) unread until the ticket is waited for; inputs may still be in flight on the context's
 *            stream (the lane waits for them on the device). Blocks only when its lane's previous submission has not finished yet.
 *   wait   : ticket 0 = everything submitted so far; out_stats (may be NULL) = {modified, refined, skipped, strips} of that ticket, as bu_hip_k_uastc_rdo reports them */
typedef struct bu_uastc_pipeline bu_uastc_pipeline;
BU_HIP_API bu_uastc_pipeline* bu_hip_uastc_pipeline_create(bu_hip_context*, uint32_t lanes, uint32_t max_blocks, uint32_t flags, uint32_t max_total_jobs);
BU_HIP_API int  bu_hip_uastc_pipeline_submit(bu_uastc_pipeline*, const void* d_pixel_blocks, uint32_t n_blocks, void* d_out_uastc_blocks, const bu_uastc_rdo_params* rdo_or_null,
                                             uint32_t flags, uint32_t total_jobs, uint64_t* out_ticket);
BU_HIP_API int  bu_hip_uastc_pipeline_wait(bu_uastc_pipeline*, uint64_t ticket, uint32_t out_stats[4]);
BU_HIP_API void bu_hip_uastc_pipeline_destroy(bu_uastc_pipeline*);

/* basisu_lowlevel_uastc_ldr_4x4_transcoder::transcode_slice over resident blocks. target: the reference's
 * transcoder_texture_format value; decode_flags: its cDecodeFlags* (only cDecodeFlagsHighQuality is read);
 * channel0 / channel1: -1 = the reference's defaults (0, 3). row_pitch / rows: RGBA32 only, in pixels, 0 = orig size.
 * Supported targets: cTFBC1_RGB (2), cTFBC3_RGBA (3), cTFBC4_R (4), cTFBC5_RG (5), cTFBC7_RGBA (6), cTFASTC_4x4_RGBA (10), cTFRGBA32 (13); any other fails.
 * One launch on the context's stream; the call synchronises only to read the count of blocks that did not unpack, whose output is zero-filled
 * (the reference stops at the first one). RGBA32 writes exactly orig_width x orig_height pixels (rows cut at `rows`): a padded pitch stays untouched. */
BU_HIP_API int bu_hip_k_transcode_uastc(bu_hip_context*, const void* d_uastc_blocks, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, uint32_t decode_flags, int32_t channel0, int32_t channel1,
        void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t* out_invalid_blocks);
BU_HIP_API size_t bu_hip_transcode_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target);

/* The texel half of basisu_lowlevel_etc1s_transcoder::transcode_slice (transcoder/basisu_transcoder.cpp:8858-9345) over resident palettes and per-block indices, which
 * bu_etc1s_decode_file (basisu_hip_etc1s_decode.h) makes of an ETC1S .basis / .ktx2 file on the host. One lane per block, one launch per image.
 *   d_endpoint_palette: n_endpoints x 4 bytes (r5, g5, b5, intensity table); d_selector_palette: n_selectors x uint32 (texel (x, y) at bits 2 * (y * 4 + x));
 *   d_endpoint_idx / d_selector_idx: num_blocks_x * num_blocks_y uint16 each, raster order; d_alpha_*: the alpha slice's, both NULL = opaque (read by RGBA32 and
 *   RGBA4444 only: alpha is the green channel of the alpha slice's decode).
 * Supported targets (transcoder_texture_format): cTFETC1_RGB (0), cTFBC1_RGB (2), cTFRGBA32 (13), cTFRGB565 (14), cTFBGR565 (15), cTFRGBA4444 (16); any other fails
 * with an error that names it. Block targets write 8 bytes per block in raster order; pixel targets write exactly orig_width x orig_height pixels (little-endian
 * 16-bit words for the 16-bit formats) at out_row_pitch_pixels (0 = orig_width), rows cut at out_rows_pixels (0 = orig_height): a padded pitch stays untouched.
 * bu_hip_k_transcode_etc1s first counts, on the device, the indices that are past their palette; if there is one it fails and the transcode is not launched.
 * bu_hip_k_transcode_etc1s_counted skips that pass (for indices the host decoder has already range-checked): a block with an index past its palette is zero-filled
 * and counted in *out_invalid_blocks, never gathered, and does not stop the others. Both synchronise to read their counter. */
BU_HIP_API int bu_hip_k_transcode_etc1s(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);
BU_HIP_API int bu_hip_k_transcode_etc1s_counted(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t* out_invalid_blocks);
/* The two ETC1S -> BC1 endpoint tables the BC1 target reads ([intensity table 8][base5 32][selector range 6][mapping 10] -> lo | hi << 8 | squared error << 16; 15,360
 * words each, 5-bit and 6-bit endpoints), copied to the host. The library computes them on the device the first time a context needs them; tests compare them with
 * tools/gen_etc1s_transcode_tables.py's host computation. */
BU_HIP_API int bu_hip_etc1s_bc1_endpoint_tables(bu_hip_context*, uint32_t* h_out5, uint32_t* h_out6);
BU_HIP_API size_t bu_hip_etc1s_transcode_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target,
        uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);

/* Both transcoders over EVERY image of a file in one launch: what reading back a texture array, a cubemap or a mip chain (levels x layers x faces, for ETC1S with
 * alpha a second slice per image) would otherwise pay a launch, a stream wait and, for ETC1S, the uploads per image for. One record per image serves both codecs.
 * `slices` is a HOST array of n_slices records. Slice s reads num_blocks_x * num_blocks_y inputs in raster order from first_block on -- UASTC: 16-byte blocks counted
 * from d_uastc_blocks (n_blocks of them, 16-byte aligned); ETC1S: entries of d_endpoint_idx / d_selector_idx (n_indices uint16 each: the file's whole index
 * arrays, bu_etc1s_file_endpoint_indices / _selector_indices), its alpha slice the same two arrays from alpha_first_block on -- and writes at d_out + out_offset
 * byte for byte what bu_hip_k_transcode_uastc / bu_hip_k_transcode_etc1s_counted write for the same inputs, size, pitch, rows, target, flags and channels. A pixel
 * target (RGBA32; ETC1S also the 16-bit formats) writes only orig_width x min(orig_height, rows) pixels: padding, and the gaps between slices, are not touched.
 * bu_hip_transcode_slice_extent is the room a record takes from its out_offset: blocks x bytes per block, or pitch x rows x bytes per pixel.
 * The records and the table of their block counts go up in one stream-ordered copy; `slices` may be released on return. ONE transcode launch on the context's
 * stream (plus, once per context, the build of the ETC1S -> BC1 tables). A UASTC block that does not unpack, or an ETC1S block with an index past its palette, is
 * zero-filled and counted for its slice. With out_invalid_per_slice non-NULL the n_slices counts are read back behind one stream wait, however many slices there
 * are; with NULL nothing is read back and the call does not synchronise.
 * Fails -- nothing copied, nothing launched, nothing written, the reason by name in bu_hip_last_error -- on a null pointer or n_slices == 0; a target the codec's
 * one-image entry refuses (same text); a record with zero blocks or more than 16384 blocks either way; pixels that do not fit the blocks; a pitch below the width;
 * pitch or rows set for a block target; alpha_first_block set for UASTC; an input range (or alpha range) that ends past n_blocks / n_indices; d_out,
 * d_uastc_blocks or an out_offset that is not 16-byte aligned (the RGBA32 rows are stored as 16-byte words where their address allows); an extent that ends past
 * out_bytes; an out_offset before the end of the record before it (outputs ascend in table order and may not overlap, gaps are allowed; inputs may be in any
 * order and may repeat, they are only read); more than 2^30 blocks in all; ETC1S palettes outside 1..65535; a UASTC channel above 3. */
#define BU_HIP_NO_ALPHA_SLICE UINT64_MAX
typedef struct bu_hip_transcode_slice {
    uint64_t first_block;        /* UASTC: the image's first block, counted in 16-byte blocks from d_uastc_blocks. ETC1S: the image's first entry in d_ep_idx / d_sel_idx */
    uint64_t alpha_first_block;  /* ETC1S: first entry of the image's alpha slice, or BU_HIP_NO_ALPHA_SLICE; read only by RGBA32 / RGBA4444. UASTC: must be BU_HIP_NO_ALPHA_SLICE */
    uint64_t out_offset;         /* bytes from d_out where this image's output begins; a multiple of 16 */
    uint32_t num_blocks_x, num_blocks_y;              /* both >= 1 */
    uint32_t orig_width, orig_height;                 /* 0 = 4 * num_blocks */
    uint32_t out_row_pitch_pixels, out_rows_pixels;   /* pixel targets: 0 = orig size; block targets: must be 0 */
} bu_hip_transcode_slice;
BU_HIP_API int bu_hip_k_transcode_uastc_slices(bu_hip_context*, const void* d_uastc_blocks, uint64_t n_blocks, const bu_hip_transcode_slice* slices, uint32_t n_slices,
        uint32_t target, uint32_t decode_flags, int32_t channel0, int32_t channel1, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API int bu_hip_k_transcode_etc1s_slices(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
        void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
/* bytes one record occupies from its out_offset for `target` (0 = target not supported by that codec) */
BU_HIP_API size_t bu_hip_transcode_slice_extent(const bu_hip_transcode_slice*, uint32_t target, int etc1s);

/* The ETC1S transcoder's second entry family: the three entries above with a decode_flags word, and two more targets. The first family keeps its six targets and
 * its refusals; these take
 *   cTFETC1_RGB (0), cTFBC1_RGB (2), cTFRGBA32 (13), cTFRGB565 (14), cTFBGR565 (15), cTFRGBA4444 (16): byte for byte what the first family writes;
 *   cTFETC2_RGBA (1): 16 bytes per block, bytes 0-7 the EAC A8 block of the alpha slice (convert_etc1s_to_etc2_eac_a8, transcoder/basisu_transcoder.cpp:4786), bytes
 *     8-15 the ETC1 block of the colour slice;
 *   cTFBC7_RGBA (6): one mode-5 block (convert_etc1s_to_bc7_m5_color :4310, the chroma filter chroma_filter_bc7_mode5 :4641 with its mode-5 encoder :8102, then
 *     convert_etc1s_to_bc7_m5_alpha :4472), bit for bit the reference's.
 * Without an alpha slice (both alpha pointers NULL, or BU_HIP_NO_ALPHA_SLICE) the two 16-byte targets write the opaque alpha half / opaque alpha fields; with one,
 * its indices are range-checked like the colour slice's. d_out of a 16-byte target must be 16-byte aligned.
 * BC3_RGBA, BC4_R and BC5_RG are refused: their look-up could not be restated as a search. ASTC_4x4_RGBA, ETC2_EAC_R11 and ETC2_EAC_RG11 are refused
 * here and taken by the third family below.
 * decode_flags: 64 (cDecodeFlagsNoETC1SChromaFiltering) turns BC7's chroma filter off; any other bit is refused by name. The filter reads the endpoint indices of
 * the eight blocks around a block; one that is past the palette contributes the centre block's own entry (and is itself zero-filled and counted).
 * The ETC1S -> BC7 colour look-up is built on the device by the first BC7 transcode of a context (bu_hip_etc1s_bc7_color_table copies it, 15,360 words
 * [intensity table 8][base5 32][selector range 6][mapping 10] -> lo | hi << 8 | min(error, 65535) << 16, and the encoder's 128 float midpoints to the host; tests
 * compare them with tools/gen_etc1s_transcode_tables.py's host computation). Everything else is as for the first family, refusals included. */
BU_HIP_API int bu_hip_k_transcode_etc1s_image(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t decode_flags);
BU_HIP_API int bu_hip_k_transcode_etc1s_image_counted(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t decode_flags,
        uint32_t* out_invalid_blocks);
BU_HIP_API int bu_hip_k_transcode_etc1s_images(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
        uint32_t decode_flags, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API size_t bu_hip_etc1s_image_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target,
        uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);
BU_HIP_API size_t bu_hip_etc1s_image_slice_extent(const bu_hip_transcode_slice*, uint32_t target);
BU_HIP_API int bu_hip_etc1s_bc7_color_table(bu_hip_context*, uint32_t* h_out, uint32_t* h_midpoints);
/* A diagnostic, not a transcoding entry: the mode-5 encoder that runs under BC7's chroma filter, on tiles of the caller's choosing instead of the pixels the filter
 * rebuilds. d_tiles: n_tiles tiles of 16 RGBA pixels (64 bytes each, pixel y * 4 + x, alpha ignored); d_out: n_tiles opaque 16-byte blocks. One lane per tile, the
 * same device function and the same midpoint table (this context's) as the filter. Queued on the context's stream like the transcodes. Refused before any launch,
 * d_out untouched: a null pointer, either pointer not 16-byte aligned, more than 2^30 tiles. n_tiles == 0 returns 1 and writes nothing. */
BU_HIP_API int bu_hip_k_bc7_mode5_tiles(bu_hip_context*, const void* d_tiles, uint32_t n_tiles, void* d_out);

/* The ETC1S transcoder's third entry family: the second family's arguments, its eight targets byte for byte, and three more. The first two families keep their
 * targets and their refusals; these also take
 *   cTFASTC_4x4_RGBA (10): 16 bytes per block, convert_etc1s_to_astc_4x4 (transcoder/basisu_transcoder.cpp:5747) as the native build compiles it
 *     (BASISD_SUPPORT_ASTC_HIGHER_OPAQUE_QUALITY = 1): void extent for a constant block; block truncation (CEM 12, 8-bit endpoints, 1-bit weights) when colour
 *     and alpha use at most two selectors each; luminance + alpha (CEM 4) for a grey base colour; RGB over 8-bit endpoints (CEM 8) for an opaque block; else
 *     RGBA over endpoints of BISE range 0..47 in two planes (CEM 12);
 *   cTFETC2_EAC_R11 (20): 8 bytes per block, convert_etc1s_to_etc2_eac_r11 (:5104) on the colour slice's first channel; the alpha slice is not read;
 *   cTFETC2_EAC_RG11 (21): 16 bytes per block, bytes 0-7 that block, bytes 8-15 the same conversion of the alpha slice.
 * Without an alpha slice ASTC's alpha is 255 and RG11's second half the opaque EAC block (base 255, table 13, multiplier 1, every code 4). d_out of a 16-byte
 * target must be 16-byte aligned. decode_flags as in the second family: 64 alone, which only BC7 heeds.
 * Not supported, refused by name: BC3_RGBA, BC4_R, BC5_RG (their look-up could not be restated as a search), PVRTC1, and PVRTC2, ATC, FXT1 (the
 * fourth family below takes ATC RGB, FXT1 and PVRTC2 RGB / RGBA), and
 * cDecodeFlagsTranscodeAlphaDataToOpaqueFormats (R11 from the alpha slice alone).
 * The two ETC1S -> ASTC look-ups are built on the device by the first ASTC transcode of a context. bu_hip_etc1s_astc_tables copies them to the host: twice 15,360
 * words [intensity table 8][base5 32][selector range 6][mapping 10] -> lo | hi << 8 | error << 16, over the 48 BISE codes of range 0..47 and over 8-bit
 * endpoints, and the 48 unquantised values of those codes; tests compare them with tools/gen_etc1s_transcode_tables.py's host computation. */
BU_HIP_API int bu_hip_k_transcode_etc1s_block_format(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t decode_flags);
BU_HIP_API int bu_hip_k_transcode_etc1s_block_format_counted(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette,
        uint32_t n_selectors, const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x,
        uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels,
        uint32_t decode_flags, uint32_t* out_invalid_blocks);
BU_HIP_API int bu_hip_k_transcode_etc1s_block_formats(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
        uint32_t decode_flags, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API size_t bu_hip_etc1s_block_format_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target,
        uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);
BU_HIP_API size_t bu_hip_etc1s_block_format_slice_extent(const bu_hip_transcode_slice*, uint32_t target);
BU_HIP_API int bu_hip_etc1s_astc_tables(bu_hip_context*, uint32_t* h_out_0_47, uint32_t* h_out_0_255, uint32_t* h_unquant48);

/* The ETC1S transcoder's fourth entry family: the third family's arguments, its eleven targets byte for byte through the same kernels, and four more. The first
 * three families keep their targets and their refusals; these also take
 *   cTFATC_RGB (11): 8 bytes per block, convert_etc1s_to_atc (transcoder/basisu_transcoder.cpp:6476): the low colour 555, the high colour 565, 2-bit selectors;
 *   cTFFXT1_RGB (17): 16 bytes per 8x4 texels, CC_MIXED without alpha: convert_etc1s_to_fxt1 (:2573) over convert_etc1s_to_dxt1 (:2271) with three-colour blocks
 *     forbidden. An output block covers two source blocks side by side, so a row holds (num_blocks_x + 1) / 2 blocks, rows in order, and the output takes
 *     (num_blocks_x + 1) / 2 * num_blocks_y * 16 bytes (bu_hip_etc1s_vendor_format_output_bytes, _slice_extent); the lone left half at the end of an odd row fills
 *     both colour pairs and repeats its right column. It reads the ETC1S -> BC1 tables of the context;
 *   cTFPVRTC2_4_RGB (18): 8 bytes per block, convert_etc1s_to_pvrtc2_rgb (:7153): hard (non-interpolated) opaque blocks, the low colour 554, the high colour 555,
 *     the modulation bytes first. Unlike PVRTC1, any image size;
 *   cTFPVRTC2_4_RGBA (19): 8 bytes per block, convert_etc1s_to_pvrtc2_rgba (:7285): hard translucent blocks, colour a 4433 and colour b 4443, re-encoded per pixel
 *     from the colour and the alpha slice's block: a constant alpha >= 250 gives the RGB block; a constant colour with constant alpha the best of modulation 0, 1
 *     and 3; any other block bounds from one of four routes (the 4D incremental PCA in binary32 among them, bit for bit the reference's), quantised, and three
 *     integer thresholds per texel. Without an alpha slice (both alpha pointers NULL, or BU_HIP_NO_ALPHA_SLICE) it is the PVRTC2_4_RGB block. Its alpha indices are
 *     range-checked like the colour slice's, and a bad one is the block's failure too.
 * The alpha slice is not read by the other three. An invalid count is of SOURCE blocks; an FXT1 block with an invalid half is sixteen zero bytes.
 * Not supported, refused by name with the reason: BC3_RGBA, BC4_R, BC5_RG and ATC_RGBA (all need the ETC1S -> BC4 look-up, which could not be restated as a
 * search); PVRTC1 has its own family.
 * The three ETC1S -> ATC / PVRTC2 look-ups are built on the device by the first ATC RGB or PVRTC2 transcode of a context. bu_hip_etc1s_atc_tables copies them
 * to the host: three times 15,360 words [intensity table 8][base5 32][selector range 6][mapping 10] -> lo | hi << 8 | min(error, 65535) << 16, for endpoints of
 * 5 and 5 bits, 5 and 6 bits, and 4 and 5 bits; tests compare them with tools/gen_etc1s_transcode_tables.py's host computation. */
BU_HIP_API int bu_hip_k_transcode_etc1s_vendor_format(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t decode_flags);
BU_HIP_API int bu_hip_k_transcode_etc1s_vendor_format_counted(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette,
        uint32_t n_selectors, const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x,
        uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels,
        uint32_t decode_flags, uint32_t* out_invalid_blocks);
BU_HIP_API int bu_hip_k_transcode_etc1s_vendor_formats(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
        uint32_t decode_flags, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API size_t bu_hip_etc1s_vendor_format_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target,
        uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);
BU_HIP_API size_t bu_hip_etc1s_vendor_format_slice_extent(const bu_hip_transcode_slice*, uint32_t target);
BU_HIP_API int bu_hip_etc1s_atc_tables(bu_hip_context*, uint32_t* h_out_55, uint32_t* h_out_56, uint32_t* h_out_45);

/* The UASTC transcoder's second entry family: bu_hip_k_transcode_uastc and bu_hip_k_transcode_uastc_slices with the targets that consume the ETC1 / EAC hints every
 * UASTC block carries, and the 16-bit rasters. The first family keeps its seven targets and its refusals; these take
 *   cTFBC1_RGB (2), cTFBC3_RGBA (3), cTFBC4_R (4), cTFBC5_RG (5), cTFBC7_RGBA (6), cTFASTC_4x4_RGBA (10), cTFRGBA32 (13): byte for byte what the first family writes;
 *   cTFETC1_RGB (0): 8 bytes per block (transcode_uastc_to_etc1, transcoder/basisu_transcoder.cpp:16720);
 *   cTFETC2_RGBA (1): 16 bytes per block, bytes 0-7 the EAC A8 block from the block's EAC hint (transcode_uastc_to_etc2_eac_a8 :17629), bytes 8-15 the ETC1 block;
 *   cTFETC2_EAC_R11 (20): 8 bytes per block, the EAC block of channel0 (-1 = 0); cTFETC2_EAC_RG11 (21): 16 bytes, channel0's block then channel1's (-1 = 0 and 3).
 *     Channels 0-2 are packed by pack_eac (:18880), with cDecodeFlagsHighQuality by pack_eac_high_quality (:19037); channel 3 goes the hint's way, as in ETC2 RGBA;
 *   cTFRGB565 (14), cTFBGR565 (15), cTFRGBA4444 (16): little-endian 16-bit words, exactly orig_width x orig_height pixels at out_row_pitch_pixels (0 = orig_width),
 *     rows cut at out_rows_pixels (0 = orig_height), as RGBA32: a padded pitch stays untouched.
 * All bit for bit the reference's. Any other target is refused with an error that names it and lists these; PVRTC1 (needs neighbouring blocks), ATC / FXT1 / PVRTC2
 * (the reference has no UASTC route to them) are among the refused.
 * decode_flags: 32 (cDecodeFlagsHighQuality) selects BC1 / BC3's second pass and R11 / RG11's 16-table packer; any other bit is refused by name -- with
 * cDecodeFlagsTranscodeAlphaDataToOpaqueFormats the reference would pack ETC1 from the alpha channel, which is not built here.
 * The blocks must be 16-byte aligned and d_out aligned to the target's unit (2 to 16 bytes; the table form: 16). The one-image entry refuses a pitch or rows for a
 * block target, and returns 1 without a launch (nothing read, nothing written) for a grid of zero blocks. Everything else is as for the first family, refusals
 * included: an invalid block is zero-filled and counted, per slice in the table form. */
BU_HIP_API int bu_hip_k_transcode_uastc_texture(bu_hip_context*, const void* d_uastc_blocks, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, uint32_t decode_flags, int32_t channel0, int32_t channel1,
        void* d_out, uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels, uint32_t* out_invalid_blocks);
BU_HIP_API int bu_hip_k_transcode_uastc_textures(bu_hip_context*, const void* d_uastc_blocks, uint64_t n_blocks, const bu_hip_transcode_slice* slices, uint32_t n_slices,
        uint32_t target, uint32_t decode_flags, int32_t channel0, int32_t channel1, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API size_t bu_hip_uastc_texture_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target,
        uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);
BU_HIP_API size_t bu_hip_uastc_texture_slice_extent(const bu_hip_transcode_slice*, uint32_t target);

/* PVRTC1 4bpp, for both codecs: a family of its own, because it is the one target whose block depends on its neighbours. Every other family above keeps refusing
 * it. target: cTFPVRTC1_4_RGB (8) or cTFPVRTC1_4_RGBA (9); 8 bytes per block, byte for byte what the reference's transcoder writes
 * (transcode_uastc_to_pvrtc1_4_rgb / _rgba, transcoder/basisu_transcoder.cpp:19541-19643; the two PVRTC1 cases of the ETC1S transcode_slice :8901-8987 with
 * fixup_pvrtc1_4_modulation_rgb / _rgba :3621-3977). A block's endpoints are the floor / ceil of its colour bounds; its 32 modulation bits compare each texel with
 * the endpoints of the 3x3 blocks around it, interpolated, and the blocks around an edge block are those of the opposite edge. The blocks are stored in Morton
 * order (for a non-square image over the shorter axis' bits, the longer axis' other bits above), num_blocks_x * num_blocks_y * 8 bytes per image, with no padding
 * of levels under 8x8 pixels. An image is whole or nothing: there is no pitch, no rows, no channel choice.
 * Two launches per call on the context's stream, with no host wait between them: the endpoint words go to a workspace of 4 bytes per block from the context's
 * arenas, the second launch reads them back. The arguments are the texture family's (UASTC) and the block-format family's (ETC1S) without pitch / rows /
 * channels; the table forms take the records of the whole-file transcoders (pitch / rows 0) and make their two launches over every image of the file.
 * cTFPVRTC1_4_RGBA without alpha data -- an ETC1S image without an alpha slice (both alpha pointers NULL; in a table: no record has one) -- writes what
 * cTFPVRTC1_4_RGB writes, as the reference does. Whether a UASTC file has alpha is its header's word, so that choice is the caller's (transcode.py makes it).
 * An invalid block (an ETC1S index past its palette, a UASTC block that does not unpack) is written as eight zero bytes and counted, per slice in the table
 * forms, and never stops the others; its neighbours read its endpoint word as 0. bu_hip_k_transcode_etc1s_pvrtc1 first counts the indices past their palette
 * and fails without a launch if there is one; _counted skips that pass, as in the other ETC1S families.
 * Refused by name before any launch: a target other than 8 or 9; an image whose width, height or block counts are not powers of two ("PVRTC1 only supports power
 * of 2 dimensions"); pixels that do not fit the blocks; zero blocks; a one-image output that is not 8-byte aligned (table forms: 16, and an extent past
 * out_bytes); any decode flag, cDecodeFlagsPVRTCDecodeToNextPow2 and cDecodeFlagsTranscodeAlphaDataToOpaqueFormats (RGB from the alpha data alone) among them;
 * a table in which some records have an alpha slice and others none. */
BU_HIP_API int bu_hip_k_transcode_uastc_pvrtc1(bu_hip_context*, const void* d_uastc_blocks, uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width,
        uint32_t orig_height, uint32_t target, uint32_t decode_flags, void* d_out, uint32_t* out_invalid_blocks);
BU_HIP_API int bu_hip_k_transcode_uastc_pvrtc1_images(bu_hip_context*, const void* d_uastc_blocks, uint64_t n_blocks, const bu_hip_transcode_slice* slices, uint32_t n_slices,
        uint32_t target, uint32_t decode_flags, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API int bu_hip_k_transcode_etc1s_pvrtc1(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t decode_flags);
BU_HIP_API int bu_hip_k_transcode_etc1s_pvrtc1_counted(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette,
        uint32_t n_selectors, const void* d_endpoint_idx, const void* d_selector_idx, const void* d_alpha_endpoint_idx, const void* d_alpha_selector_idx, uint32_t num_blocks_x,
        uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height, uint32_t target, void* d_out, uint32_t decode_flags, uint32_t* out_invalid_blocks);
BU_HIP_API int bu_hip_k_transcode_etc1s_pvrtc1_images(bu_hip_context*, const void* d_endpoint_palette, uint32_t n_endpoints, const void* d_selector_palette, uint32_t n_selectors,
        const void* d_endpoint_idx, const void* d_selector_idx, uint64_t n_indices, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t target,
        uint32_t decode_flags, void* d_out, size_t out_bytes, uint32_t* out_invalid_per_slice);
BU_HIP_API size_t bu_hip_pvrtc1_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y);
BU_HIP_API size_t bu_hip_pvrtc1_slice_extent(const bu_hip_transcode_slice*, uint32_t target);   /* 0 = not a PVRTC1 target */

/* gpu_image::unpack(encoder/basisu_gpu_texture.cpp:1218-1266) over resident blocks: what a GPU samples from a BC1 / BC3 / BC4 / BC5 / BC7 texture, as RGBA8.
 * format: the transcoder_texture_format value the transcoders above take as a target -- cTFBC1_RGB (2), cTFBC3_RGBA (3), cTFBC4_R (4), cTFBC5_RG (5), cTFBC7_RGBA (6);
 * any other fails with an error that names it. d_blocks: num_blocks_x * num_blocks_y blocks of 8 (BC1, BC4) or 16 bytes in raster order, aligned to their size;
 * d_out: 4-byte aligned, room for bu_hip_unpack_output_bytes. orig_width / orig_height: 0 = the padded size; row_pitch / rows: in pixels, 0 = orig size.
 * BC1 decodes with its punch-through alpha (three-colour blocks' index 3 is (0, 0, 0, 0)), BC3's colour half always with four colours; BC4 writes R and BC5 R, G,
 * the other colour channels are 0 and alpha 255. Exactly orig_width x orig_height pixels are written (rows cut at `rows`): ragged blocks are clipped and a padded
 * pitch stays untouched. The only invalid block is a BC7 block whose first byte is 0 (the reserved mode): its texels are zero-filled and it is counted -- the
 * reference leaves the previous block's pixels there. One launch on the context's stream; the call synchronises once to read that count. */
BU_HIP_API int bu_hip_k_unpack_blocks(bu_hip_context*, const void* d_blocks, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t format, void* d_out_rgba, uint32_t out_row_pitch_pixels,
        uint32_t out_rows_pixels, uint32_t* out_invalid_blocks);
BU_HIP_API size_t bu_hip_unpack_output_bytes(uint32_t num_blocks_x, uint32_t num_blocks_y, uint32_t orig_width, uint32_t orig_height,
        uint32_t out_row_pitch_pixels, uint32_t out_rows_pixels);

/* The texture unpacker: gpu_image::unpack over resident blocks of EVERY block format the transcoders above write. A family of its own: bu_hip_k_unpack_blocks keeps
 * its five formats and its refusals. format: the transcoder_texture_format value -- the five BC formats, texel for texel what bu_hip_k_unpack_blocks writes, and
 *   cTFETC1_RGB (0)         8 bytes   individual and differential mode, flip; A = 255
 *   cTFETC2_RGBA (1)       16 bytes   bytes 0-7 EAC A8, bytes 8-15 ETC1
 *   cTFETC2_EAC_R11 (20)    8 bytes   the 11-bit value to 8 bits as (v * 255 + 1023) / 2047; G = B = 0, A = 255
 *   cTFETC2_EAC_RG11 (21)  16 bytes   two R11 blocks into R and G; B = 0, A = 255
 *   cTFASTC_4x4_RGBA (10)  16 bytes   the whole LDR 4x4 format in the L8 (non-sRGB) decode profile -- void extent, every block mode and weight grid from 2x2 to 4x4
 *                                     (infill), bits / trits / quints, one to four partitions, dual plane, the ten LDR endpoint modes; a channel is the top 8
 *                                     bits of the UNORM16 result -- as basisu_astc::astc::decompress_ldr(.., isSRGB = false, 4, 4) decodes it
 *   cTFPVRTC1_4_RGB (8), cTFPVRTC1_4_RGBA (9)   8 bytes, blocks in Morton order as bu_hip_k_transcode_*_pvrtc1 write them; both modulation modes; power-of-two
 *                                     images only ("PVRTC1 only supports power of 2 dimensions")
 * any other fails with an error that names it. Geometry, alignment, clipping, pitch and rows are bu_hip_k_unpack_blocks's; d_out has room for
 * bu_hip_unpack_output_bytes. Invalid blocks are zero-filled (alpha included) and counted, and never stop the others -- the reference returns false and leaves the
 * caller's buffer as it was: BC7's reserved mode; an ETC1 / ETC2 colour half whose differential base leaves 0..31 (ETC2's T / H / planar encodings, which the
 * reference does not decode); an ASTC block the reference's LDR decoder refuses (reserved block modes, a weight grid past 4x4, weight or endpoint bit counts out
 * of range, four partitions with two planes, an HDR endpoint mode in a partition that holds a texel, an HDR or malformed void extent). R11, RG11 and PVRTC1 have
 * no invalid blocks. One launch on the context's stream; the call synchronises once to read the count. */
BU_HIP_API int bu_hip_k_unpack_texture(bu_hip_context*, const void* d_blocks, uint32_t num_blocks_x, uint32_t num_blocks_y,
        uint32_t orig_width, uint32_t orig_height, uint32_t format, void* d_out_rgba, uint32_t out_row_pitch_pixels,
        uint32_t out_rows_pixels, uint32_t* out_invalid_blocks);
BU_HIP_API uint32_t bu_hip_unpack_texture_bytes_per_block(uint32_t format);   /* 0 = not a format that unpacks */

/* The payload of a DX10 .dds file from the resident tile array (64 B per tile: RGBA8, rows of four texels, borders duplicated -- what bu_hip_k_extract_slices
 * writes): pack_slice of the reference tool's `-dds` mode (encoder/basisu_dds_export.cpp:151-267). format: the tool's dds_output_format value, in the order of its
 * -dds_format tokens. BC1 is basist::encode_bc1 with cEncodeBC1HighQuality, BC4 basist::encode_bc4; BC2 = explicit 4-bit alpha + BC1, BC3 = BC4 of alpha + BC1,
 * BC5 = BC4 of red + BC4 of green. The raw formats truncate the channels to their bits (r >> 3, a >= 128, a >> 4), they never round.
 *   bu_hip_k_pack_dds_blocks (BC1-BC5): tile i -> 8 (BC1, BC4) or 16 bytes at d_out + i * that, i < n_tiles. The tile array is in slice order (image outermost,
 *     then level), which is DDS subresource order (layer, face, level): the whole file's payload is this one launch, and there is no slice table.
 *   bu_hip_k_pack_dds_pixels (the seven raw formats): `slices` is a HOST array of n_slices records as the whole-file transcoders take them. Slice s reads its
 *     num_blocks_x * num_blocks_y tiles in raster order from tile first_block on and writes exactly orig_width x orig_height pixels in tight rows at d_out +
 *     out_offset: the padding of the last tiles is cropped and nothing between or behind the slices is written. One launch for all slices.
 *   bu_hip_dds_payload_bytes: what the slices' subresources take, back to back (blocks x bytes per block, or pixels x bytes per pixel); 0 for a format that is
 *     refused or a null / empty table.
 * Both kernels are stream-ordered and neither call synchronises. Both fail -- nothing copied, nothing launched, nothing written, the reason by name in
 * bu_hip_last_error -- on BU_HIP_DDS_BC7 (neither of the reference's two BC7 packers, bc7f and bc7e_scalar, is implemented here); on a format value that is no
 * format; on a raw format given to _blocks or a block format given to _pixels; on a null pointer; on d_tiles or d_out that is not 16-byte aligned; on more than
 * 2^30 tiles. _pixels also fails on n_slices == 0; a record with zero blocks or more than 16384 either way; pixels that do not fit the blocks; a pitch or row count
 * (rows are tight) or an alpha_first_block that is set; tiles that end past n_tiles; an out_offset that is no multiple of the pixel size, lies before the end of the
 * record before it, or whose subresource ends past out_bytes. */
enum { BU_HIP_DDS_BC1 = 0, BU_HIP_DDS_BC2 = 1, BU_HIP_DDS_BC3 = 2, BU_HIP_DDS_BC4 = 3, BU_HIP_DDS_BC5 = 4, BU_HIP_DDS_BC7 = 5, BU_HIP_DDS_A8R8G8B8 = 6,
       BU_HIP_DDS_A8B8G8R8 = 7, BU_HIP_DDS_R8 = 8, BU_HIP_DDS_R8G8 = 9, BU_HIP_DDS_R5G6B5 = 10, BU_HIP_DDS_A1R5G5B5 = 11, BU_HIP_DDS_A4R4G4B4 = 12 };
BU_HIP_API int bu_hip_k_pack_dds_blocks(bu_hip_context*, const void* d_tiles, uint64_t n_tiles, uint32_t format, void* d_out);
BU_HIP_API int bu_hip_k_pack_dds_pixels(bu_hip_context*, const void* d_tiles, uint64_t n_tiles, const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t format,
        void* d_out, size_t out_bytes);
BU_HIP_API size_t bu_hip_dds_payload_bytes(const bu_hip_transcode_slice* slices, uint32_t n_slices, uint32_t format);

/* The counting half of image_metrics::calc (encoder/basisu_enc.cpp:2155-2226) for all eight lines basis_compressor's m_compute_stats stage reports per slice
 * (comp.cpp:4195-4253), in one pass over two resident RGBA8 rasters (4 bytes per pixel, 4-byte aligned; a row pitch in pixels, 0 = the width; each raster reaches
 * to pixel (height - 1) * pitch + width). The region compared is min(width_a, width_b) x min(height_a, height_b), as calc crops; at most 16384 each way.
 *   hist[row][d]: how many values of the region differ by d = |a - b|; rows 0-3 = R, G, B, A, 4 = 709 luma, 5 = 601 luma ((13938 r + 46869 g + 4729 b + 32768) >> 16
 *   and (19595 r + 38470 g + 7471 b + 32768) >> 16, per image, then differenced). sum_a / sum_b: per-channel sums of each image over the region (calc's m_sum_a /
 *   m_sum_b of a channel set are sums of these). Integer counts: exact and the same on every run. bu_image_metrics_reduce (basisu_hip_image_metrics.h, host code)
 *   turns them into Max / Mean / RMS / PSNR in the reference's own expression order.
 * Versioned by size like bu_hip_tuning: the caller sets struct_bytes = sizeof(bu_image_metrics_counts) of its header; at most that many bytes are written (and
 * struct_bytes itself is left alone). One launch on the context's stream (none for an empty region, whose counts are zero); synchronises to copy the counts out.
 * Fails -- nothing launched, *h_out untouched -- on a null pointer, a misaligned raster, a pitch below its width or a region beyond 16384. */
typedef struct bu_image_metrics_counts {
    uint32_t struct_bytes;
    uint32_t width, height;       /* the region compared */
    uint32_t reserved;
    uint32_t hist[6][256];
    uint64_t sum_a[4], sum_b[4];
} bu_image_metrics_counts;
BU_HIP_API int bu_hip_k_image_metrics(bu_hip_context*, const void* d_a, uint32_t width_a, uint32_t height_a, uint32_t pitch_a_pixels, const void* d_b, uint32_t width_b,
        uint32_t height_b, uint32_t pitch_b_pixels, bu_image_metrics_counts* h_out);

/* PSNR-HVS / PSNR-HVS-M as psnr_hvs_compute_metrics computes them (encoder/basisu_enc.cpp:2256-2519; the lines after "PSNR-HVS and PSNR-HVS-M metrics:" of the
 * m_compute_stats stage, comp.cpp:4265-4276, and of `basisu -compare_hvs`), over two resident RGBA8 rasters laid out as for bu_hip_k_image_metrics. The region is
 * min(width_a, width_b) x min(height_a, height_b), at most 16384 each way, cut into ceil(w / 8) x ceil(h / 8) blocks of 8x8; a block's pixel coordinates are clamped
 * to each raster's OWN last column and row (extract_block_clamped), not to the region.
 *   Modes, the index of sum_hvs / sum_hvsm: 0 = BT.601 Y rounded to 8 bits, 1 = BT.601 Y in float, 2-5 = R, G, B, A.
 *   Per block and mode everything up to the 64 + 64 per-coefficient terms is the reference's binary32 arithmetic in its operation order (csrc/psnr_hvs.h), bit for
 *   bit; the block's two doubles are its terms added in index order. sum_hvs / sum_hvsm[mode] are the sums of those doubles over all blocks, added in an order that
 *   depends on the region's size alone (per-workgroup partials, then a fixed tree; no floating-point atomics): the same bits on every run, and within
 *   2 (blocks - 1) 2^-53 relative of the blocks added in raster order. bu_psnr_hvs_reduce (basisu_hip_image_metrics.h, host code) turns them into mseh and dB.
 * Versioned by size like bu_image_metrics_counts. Two launches on the context's stream (none for an empty region, whose sums and block count are zero); synchronises
 * to copy the sums out. Fails -- nothing launched, *h_out untouched -- on a null pointer, a misaligned raster, a pitch below its width or a region beyond 16384.
 * bu_hip_k_psnr_hvs_blocks is the test hook under it: the same launches, and h_out_blocks[block * 2 + 0 / 1] = the HVS / HVS-M double of every block of ONE mode,
 * blocks in raster order; capacity_blocks (the doubles h_out_blocks holds, halved) must be at least the region's block count, which *out_blocks (may be NULL) gets. */
typedef struct bu_psnr_hvs_sums {
    uint32_t struct_bytes;
    uint32_t width, height;       /* the region compared */
    uint32_t blocks;              /* ceil(width / 8) * ceil(height / 8) */
    double sum_hvs[6], sum_hvsm[6];
} bu_psnr_hvs_sums;
BU_HIP_API int bu_hip_k_psnr_hvs(bu_hip_context*, const void* d_a, uint32_t width_a, uint32_t height_a, uint32_t pitch_a_pixels, const void* d_b, uint32_t width_b,
        uint32_t height_b, uint32_t pitch_b_pixels, bu_psnr_hvs_sums* h_out);
BU_HIP_API int bu_hip_k_psnr_hvs_blocks(bu_hip_context*, const void* d_a, uint32_t width_a, uint32_t height_a, uint32_t pitch_a_pixels, const void* d_b, uint32_t width_b,
        uint32_t height_b, uint32_t pitch_b_pixels, uint32_t mode, double* h_out_blocks, uint32_t capacity_blocks, uint32_t* out_blocks);

/* SSIM as compute_ssim computes it (encoder/basisu_ssim.cpp) and `basisu -compare -compare_ssim` prints it (basisu_tool.cpp: "R SSIM" .. "Y 601 SSIM"), over two
 * resident RGBA8 rasters laid out as for bu_hip_k_image_metrics. The region is min(width_a, width_b) x min(height_a, height_b); the filter's coordinates are clamped
 * to the REGION (compute_ssim crops both images first). Three calls of the reference in one: RGBA (r, g, b, a; rgb = (r + g + b) / 3.0f in float) and channel 0 of
 * the 709-luma and the 601-luma call.
 *   Every figure is the reference's binary32 arithmetic in its operation order, bit for bit (csrc/ssim.h): per pixel and channel five 121-tap Gaussian filterings and
 *   the smap formula (csrc/ssim_kernels.hip, one lane per pixel), then the mean as ONE running float sum over the pixels in raster order -- evaluated in chunks with
 *   csrc/fsum_scan.h, with plain float adds wherever a chunk's shortcut is not valid, so the sum's bits are the serial sum's. That includes what the serial sum does
 *   from 2^24 pixels on: an identical pair's sum stops at 16777216, so its figures fall below 1.
 *   chunks / chunks_walked: how many chunks of 256 addends the six sums had, and how many of them had to be added one by one (diagnostic).
 * Versioned by size like bu_image_metrics_counts. Six launches on the context's stream; synchronises to copy the result out. The six float planes of the region
 * (24 bytes per pixel) are reserved from the context for the call and given back after it when they exceed 64 MiB. Fails -- nothing launched, *h_out untouched -- on
 * a null pointer, a misaligned raster, a pitch below its width, an EMPTY region (the reference asserts), a region beyond 16384 each way or beyond 2^25 pixels.
 * bu_hip_k_ssim_map is the test hook under it: the smap values of ONE call in raster order -- mode 0 = RGBA, 4 floats per pixel; 1 / 2 = channel 0 of the 709 / 601
 * luma call, 1 float per pixel; capacity_floats must cover them; *out_pixels (may be NULL) gets the region's pixel count. */
typedef struct bu_ssim_result {
    uint32_t struct_bytes;
    uint32_t width, height;       /* the region compared */
    uint32_t chunks_walked;
    float r, g, b, rgb, a, luma_709, luma_601;
    uint32_t chunks;
} bu_ssim_result;
BU_HIP_API int bu_hip_k_ssim(bu_hip_context*, const void* d_a, uint32_t width_a, uint32_t height_a, uint32_t pitch_a_pixels, const void* d_b, uint32_t width_b,
        uint32_t height_b, uint32_t pitch_b_pixels, bu_ssim_result* h_out);
BU_HIP_API int bu_hip_k_ssim_map(bu_hip_context*, const void* d_a, uint32_t width_a, uint32_t height_a, uint32_t pitch_a_pixels, const void* d_b, uint32_t width_b,
        uint32_t height_b, uint32_t pitch_b_pixels, uint32_t mode, float* h_out, uint64_t capacity_floats, uint32_t* out_pixels);

/* a15 + the list handling inside a9 / a10 / a13 / a14: cluster bookkeeping on the device (basis_universal_amd/csrc/bookkeeping_kernels.hip).
 *     A clustering is two resident per-block arrays, cluster index and position inside the cluster's list; these calls turn distinct-vector level
 *     results into them, rebuild them after a reassignment, apply codebook renumberings to them and produce the CSR lists the per-cluster
 *     kernels read, so that no block-sized array crosses PCIe between the frontend's stages. Stream-ordered; nothing synchronises.
 *   map_blocks_from_groups: groups = the output of bu_hip_k_unique_*_vectors (d_group_offsets[u_total + 1], d_sorted_block_idx[n]); every block of
 *     distinct vector u gets cluster d_leaf_of_unique[u], position d_first_pos[u] + its rank inside the group, parent d_parent_of_unique[u]
 *     (d_first_pos / d_out_pos and d_parent_of_unique / d_out_parent may be NULL).
 *   map_rank_blocks (frontend.cpp:1921-1942, lists rebuilt in block order): d_out_sizes[k + 1] (last entry 0), d_out_offsets[k + 1] (exclusive
 *     sum), d_out_sorted_blocks[n] = block ids grouped by cluster, ascending inside a cluster, d_out_pos[n] (may be NULL) = rank of every block.
 *     More than 2^30 blocks returns 0 with "more than 2^30 in one call" before anything is reserved or written. */
BU_HIP_API int bu_hip_k_map_blocks_from_groups(bu_hip_context*, const uint32_t* d_group_offsets, const uint32_t* d_sorted_block_idx, uint32_t n_blocks, uint32_t u_total,
    const uint32_t* d_leaf_of_unique, const uint32_t* d_first_pos, const uint32_t* d_parent_of_unique, uint32_t* d_out_cluster, uint32_t* d_out_pos, uint8_t* d_out_parent);
BU_HIP_API int bu_hip_k_map_rank_blocks(bu_hip_context*, const uint32_t* d_block_cluster, uint32_t n_blocks, uint32_t n_clusters, uint32_t* d_out_sizes,
    uint32_t* d_out_offsets, uint32_t* d_out_sorted_blocks, uint32_t* d_out_pos);
/*   map_endpoint_csr: d_out_indices[d_offsets[cluster] + 2 * pos] = 2b, 2b + 1 (d_offsets in training-vector units: 2 per block). */
BU_HIP_API int bu_hip_k_map_endpoint_csr(bu_hip_context*, const uint32_t* d_block_cluster, const uint32_t* d_block_pos, uint32_t n_blocks, const uint32_t* d_offsets,
    uint32_t* d_out_indices);
/*   map_remap: cluster[b] = d_new_index[old], pos[b] += d_base[old] (d_block_pos and d_base may be NULL). */
BU_HIP_API int bu_hip_k_map_remap(bu_hip_context*, uint32_t* d_block_cluster, uint32_t* d_block_pos, uint32_t n_blocks, const uint32_t* d_new_index, const uint32_t* d_base);
/*   map_count_differences: *d_out_count = |{ i : a[i] != b[i] }| (device word). map_membership: d_out_flags[parent * n_clusters + cluster] = 1 for
 *     every (parent, cluster) pair that occurs (d_block_parent may be NULL = one parent). map_gather: out[i] = table[index[i]]. */
BU_HIP_API int bu_hip_k_map_count_differences(bu_hip_context*, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, uint32_t* d_out_count);
BU_HIP_API int bu_hip_k_map_membership(bu_hip_context*, const uint8_t* d_block_parent, const uint32_t* d_block_cluster, uint32_t n_blocks, uint32_t n_parents,
    uint32_t n_clusters, uint8_t* d_out_flags);
BU_HIP_API int bu_hip_k_map_gather(bu_hip_context*, const uint32_t* d_table, const uint32_t* d_index, uint32_t n, uint32_t* d_out);

/* f3  Codebook builder FAST MODE (basis_universal_amd/csrc/kmeans_kernels.hip): weighted k-means over the distinct training
 *     vectors with the assignment step on the matrix cores, instead of the TSVQ. NOT bit-identical to the reference (different, deterministic
 *     codebooks); off unless asked for (bu_frontend_set_fast_codebooks), held to the reference's own size / PSNR tolerances by the tests.
 *     kind 0: d_keys = uint32 packed selector vectors + d_weights; kind 1: d_keys = uint64 endpoint colour keys, weights = 2 x group sizes
 *     (d_group_offsets[n + 1]). Writes, per distinct vector, its cluster (empty clusters removed, index order kept) and -- n_parents > 0 -- the
 *     parent group of that cluster (k-means over the centroids); returns the counts. Synchronises. */
BU_HIP_API int bu_hip_kmeans_codebook(bu_hip_context*, int kind, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_group_offsets, uint32_t n_vectors,
    uint32_t max_clusters, uint32_t n_parents, uint32_t iterations, uint32_t* d_out_cluster_of_vector, uint32_t* d_out_parent_of_vector, uint32_t* out_clusters,
    uint32_t* out_parents);
/*     The same steps one at a time, for kernel-level tests (tests/test_gpu_kmeans_kernels.py): the functions bu_hip_kmeans_codebook is made of, on the same
 *     workspace; k <= n_vectors. Stream-ordered; nothing synchronises.
 *   kmeans_seed: d_out_pick[k] = the distinct vector every centroid starts on (the weight quantiles (c + 1/2) / k, made strictly ascending),
 *     d_out_centroids[k * 16] = those vectors as floats.
 *   kmeans_round: one assignment round on the caller's d_centroids[k * 16]: d_out_assign[n] = the centroid of every vector (raw: empty clusters keep
 *     their index), d_out_sums[k * 17] = per cluster the 16 weighted component sums and the weight, d_out_worst[ceil(n / 512)] (may be NULL) = per group of 512
 *     vectors (float bits of the largest error x weight) << 32 | ~index of that vector. d_live[k] (NULL: all live): clusters whose word is 0 are dead and
 *     never assigned. update != 0 (needs d_live): also the centroid update and the re-seeding of empty clusters; d_centroids and d_live are overwritten with
 *     the next round's (live word = the cluster's weight, 1 for a re-seeded cluster, 0 for one left empty). */
BU_HIP_API int bu_hip_k_kmeans_seed(bu_hip_context*, int kind, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_group_offsets, uint32_t n_vectors, uint32_t k,
    uint32_t* d_out_pick, float* d_out_centroids);
BU_HIP_API int bu_hip_k_kmeans_round(bu_hip_context*, int kind, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_group_offsets, uint32_t n_vectors, uint32_t k,
    float* d_centroids, uint64_t* d_live, int update, uint32_t* d_out_assign, uint64_t* d_out_sums, uint64_t* d_out_worst);

/* a8  tree_vector_quant (encoder/basisu_enc.h:1546-2078): the order-dependent TSVQ tree build, split by split, bit-exact.
 *     The host keeps the tree, the variance priority queue and the split order (enc.h:1616-1660); the device executes batches of
 *     independent node splits (split_node, enc.h:1737-1800) on the resident training set. Rows must be the DISTINCT training
 *     vectors in ascending order (what generate_hierarchical_codebook_threaded's std::map yields, enc.h:2233-2290), dim 6 or 16.
 *     Node member lists live in two device index buffers: the root is {buf 0, start 0, count n}; a split of {buf, start, count}
 *     leaves its children at {buf^1, start, l_count} and {buf^1, start+l_count, r_count}. Member lists are ascending. */
typedef struct bu_tsvq bu_tsvq;
/* A node's member list is the span [start, start + count) of index buffer `buf` (0 .. BU_TSVQ_BUFFERS - 1); a split leaves the children's lists (left first) over the
 * same span of buffer (buf + 1) % BU_TSVQ_BUFFERS. */
#define BU_TSVQ_BUFFERS 4u
typedef struct { float origin[16]; uint64_t weight; float var; uint32_t pad; } bu_tsvq_root;      /* prepare_root, enc.h:1708-1735 */
typedef struct { uint32_t buf, start, count, pad; uint64_t weight; float origin[16]; } bu_tsvq_node;
typedef struct { uint32_t ok, l_count, r_count, pad; uint64_t l_weight, r_weight; float l_var, r_var; float l_centroid[16], r_centroid[16]; } bu_tsvq_split;
BU_HIP_API bu_tsvq* bu_hip_tsvq_create(bu_hip_context*, uint32_t dim, const float* h_rows, const uint64_t* h_weights, uint32_t n, bu_tsvq_root* h_out_root);
/* dim 16 with every component in {0,1,2,3} (ETC1S selector vectors): one dword per vector, component 0 in the top two bits. */
BU_HIP_API bu_tsvq* bu_hip_tsvq_create_packed16(bu_hip_context*, const uint32_t* h_keys, const uint64_t* h_weights, uint32_t n, bu_tsvq_root* h_out_root);
/* the same from device arrays (e.g. the outputs of bu_hip_k_unique_selector_vectors), copied on the context's stream */
BU_HIP_API bu_tsvq* bu_hip_tsvq_create_packed16_device(bu_hip_context*, const uint32_t* d_keys, const uint64_t* d_weights, uint32_t n, bu_tsvq_root* h_out_root);
/* dim 6 from the outputs of bu_hip_k_unique_endpoint_vectors: the rows (six floats = key byte * (1 / 255), frontend.cpp:846-851) and the weights (2 per block of the
 * vector's group) are made on the device; nothing is downloaded or uploaded */
BU_HIP_API bu_tsvq* bu_hip_tsvq_create_endpoint_device(bu_hip_context*, const uint64_t* d_unique_keys, const uint32_t* d_group_offsets, uint32_t n, bu_tsvq_root* h_out_root);
/* a12 + the de-duplication in front of the selector TSVQ (frontend.cpp:2140-2189; std::map<vec16F, weight> of
 * generate_hierarchical_codebook_threaded, enc.h:2218-2290) for n resident ETC1S blocks and their u64 training weights
 * (bu_hip_k_selector_training_vectors): distinct selector vectors as packed keys in ascending order = the map's order, their summed
 * weights, and the blocks of every distinct vector (ascending) as d_sorted_block_idx[d_group_offsets[u] .. d_group_offsets[u+1]).
 * All outputs are device arrays of n_blocks entries (offsets: n_blocks + 1). Integer work: exact and order independent. Synchronises. */
/* a7 + its de-duplication (frontend.cpp:825-866, enc.h:2218-2290) for n resident ETC1S blocks: distinct (low rgb, high rgb) block-colour vectors as
 * 48-bit keys (low r,g,b in bits 47..24, high r,g,b in bits 23..0; divide the bytes by 255 for the reference's vec6F) in ascending order, and the
 * blocks of every distinct vector (ascending) as d_sorted_block_idx[d_group_offsets[u] .. d_group_offsets[u+1]). Each block stands for its two
 * sub-block training vectors (ids 2b and 2b+1, weight 1 each). Outputs: device arrays of n_blocks (offsets: n_blocks + 1) entries. Synchronises.
 * Both refuse n_blocks > 2^30: they return 0 with "more than 2^30 in one call" and *out_unique = 0, before any workspace is reserved or any output written. */
BU_HIP_API int bu_hip_k_unique_endpoint_vectors(bu_hip_context*, const void* d_etc1_blocks, uint32_t n_blocks, uint32_t* d_sorted_block_idx, uint64_t* d_unique_keys,
                                                uint32_t* d_group_offsets, uint32_t* out_unique);
BU_HIP_API int bu_hip_k_unique_selector_vectors(bu_hip_context*, const void* d_enc_blocks, const uint64_t* d_weights, uint32_t n_blocks, uint32_t* d_sorted_block_idx,
                                                uint32_t* d_unique_keys, uint64_t* d_unique_weights, uint32_t* d_group_offsets, uint32_t* out_unique);
/* Every record of a batch (here, in a deep round and in bu_hip_tsvq_roots) must be a span of the member buffers: buf < BU_TSVQ_BUFFERS, count >= 1, start + count <= n.
 * Anything else returns 0 with "span outside the training set" before a kernel is launched (the tree driver, tsvq_device.h, only ever queues nodes of two members and more). */
BU_HIP_API int  bu_hip_tsvq_split(bu_hip_context*, bu_tsvq*, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_split* h_out); /* synchronises */
/* A DEEP round: the same, and in the same round trip the splits of the children, grandchildren, ... (`levels` generations, <= BU_TSVQ_BUFFERS - 2) of every node of the batch that went
 * through the one-workgroup kernel -- a split is a pure function of its node, so the caller's replay of the reference's variance queue (enc.h:1636-1655) finds them
 * when it gets there instead of asking for another round; what it never reaches is dropped. Each generation's node records are made ON THE DEVICE from the results of
 * the one before. A descendant is attempted when its parent's split succeeded, it has more than one member, and its variance (with the reference's 1e-4 for a
 * non-positive variance, enc.h:1766-1792) is positive and not below the float whose bits the caller put into h_nodes[i].pad (0 = no floor): a bound on the
 * speculation, never on the result. h_deep: (2^(levels+1) - 2) * n_nodes records; generation g = 1..levels of batch node i, path p (the sides taken, 0 = left, the
 * first step in the top bit of g bits) at h_deep[n_nodes * (2^g - 2) + i * 2^g + p]; ok == 3 there = not attempted. Synchronises. */
BU_HIP_API int  bu_hip_tsvq_split_deep(bu_hip_context*, bu_tsvq*, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_split* h_out, uint32_t levels, bu_tsvq_split* h_deep);
/* prepare_root (enc.h:1708-1735) of n_nodes member spans (buf / start / count of each record; weight and origin are not read): the root records of the
 * independent trees the reference's multi-threaded codebook build runs over the leaves of its first tree (enc.h:2137-2152). Synchronises. */
BU_HIP_API int  bu_hip_tsvq_roots(bu_hip_context*, bu_tsvq*, const bu_tsvq_node* h_nodes, uint32_t n_nodes, bu_tsvq_root* h_out);
BU_HIP_API int  bu_hip_tsvq_read_members(bu_hip_context*, bu_tsvq*, uint32_t buf, uint32_t start, uint32_t count, uint32_t* h_out);
/* Leaves (or cut nodes) as spans of the member buffers -> d_out[vector] = value for every member of every span: the leaf / parent index of
 * every distinct vector without bringing the member lists to the host. h_spans: n_spans records. Stream-ordered after the splits. */
typedef struct { uint32_t buf, start, count, value; } bu_tsvq_span;
BU_HIP_API int  bu_hip_tsvq_scatter_spans(bu_hip_context*, bu_tsvq*, const bu_tsvq_span* h_spans, uint32_t n_spans, uint32_t* d_out);
/* A finished tree in one pass: span i is leaf i and `value` its parent (cut) index -> d_leaf_of[vector], d_parent_of[vector] (may be NULL); with d_group_offsets (the
 * vectors' groups of blocks, bu_hip_k_unique_endpoint_vectors) also d_first_pos[vector] = where the vector's blocks start inside its leaf's block list (the blocks of the
 * members in front of it, in list order) and d_sizes[leaf] = the length of that list. Synchronises. */
BU_HIP_API int  bu_hip_tsvq_finish_spans(bu_hip_context*, bu_tsvq*, const bu_tsvq_span* h_spans, uint32_t n_spans, uint32_t* d_leaf_of, uint32_t* d_parent_of,
                                         const uint32_t* d_group_offsets, uint32_t* d_first_pos, uint32_t* d_sizes);
/* Multi-GPU (nodes of one round split by different ranks): the child member lists and result records of a batch laid end to end in a staging buffer the
 * host application sum-reduces across ranks (all_reduce_u64 of bu_comm): entries of nodes a rank did not split are zero, so the sum is the union.
 *   exchange_pack:   children of the nodes with h_mine[i] != 0 (from the member buffers) and their h_records into the staging buffer, zero elsewhere;
 *                    returns the device pointer and its size in u64 words.   [host: all_reduce_u64(*d_staging, *n_u64)]
 *   exchange_unpack: children of the nodes with h_mine[i] == 0 from the staging buffer into the member buffers, all records into h_records. Synchronises. */
BU_HIP_API int  bu_hip_tsvq_exchange_pack(bu_hip_context*, bu_tsvq*, const bu_tsvq_node* h_nodes, const uint8_t* h_mine, const bu_tsvq_split* h_records, uint32_t n_nodes,
                                          void** d_staging, uint64_t* n_u64);
BU_HIP_API int  bu_hip_tsvq_exchange_unpack(bu_hip_context*, bu_tsvq*, const bu_tsvq_node* h_nodes, const uint8_t* h_mine, bu_tsvq_split* h_records, uint32_t n_nodes);
BU_HIP_API void bu_hip_tsvq_destroy(bu_hip_context*, bu_tsvq*);

#ifdef __cplusplus
}
#endif
#endif /* BASISU_HIP_H */
