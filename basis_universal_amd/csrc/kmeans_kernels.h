// kmeans_kernels.h -- launch interface of kmeans_kernels.hip (internal to libbasisu_hip.so; C ABI: bu_hip_kmeans_codebook in include/basisu_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bu {

struct kmeans_buffers {
    void* vec; uint64_t* weights; void* hi; void* lo; float* cnorm; float* cen; uint64_t* sums; uint32_t k_pad;
    float *err_key, *err_key_sorted; uint32_t *err_idx, *worst, *pick, *empty; uint64_t* cum; void* cub; size_t cub_bytes;
};
size_t kmeans_workspace_bytes(uint32_t n, uint32_t k);
kmeans_buffers kmeans_carve(void* ws, uint32_t n, uint32_t k);
// endpoints == 0: d_keys = uint32 packed selector vectors, d_weights their weights. endpoints != 0: d_keys = uint64 48-bit colour keys, weights
// are 2 x the group sizes (d_goffs). After the call (stream-ordered): d_assign[u] = centroid of distinct vector u, b.sums[c * 17 + 16] = weight of
// cluster c, b.cen = centroids of the last update (k x 16 floats).
hipError_t launch_kmeans(hipStream_t st, int endpoints, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_goffs, uint32_t n, uint32_t k, uint32_t iterations,
                         const kmeans_buffers& b, uint32_t* d_assign);

// The steps launch_kmeans is made of (all stream-ordered), also driven one at a time by bu_hip_k_kmeans_seed / bu_hip_k_kmeans_round:
//   begin:        keys -> b.vec (and b.weights for endpoints), b.cum = inclusive weight sums; *out_weights = the weights the later steps take
//   seed:         b.pick[k] = the distinct vectors at the weight quantiles, b.cen = those vectors
//   flags:        the "two sums per 64-bit accumulator" word behind b.empty
//   assign_round: prepare (have_live: clusters whose b.sums[c * 17 + 16] is 0 are dead), assign, unpack sums -> d_assign[n] (raw), b.sums, and -- want_worst --
//                 one (weighted error, ~index) key per workgroup of 512 vectors at kmeans_wg_worst(b)[0 .. kmeans_workgroups(n))
//   update_round: b.cen = sums / weight, empty clusters onto the workgroups' worst vectors (their b.sums[c * 17 + 16] = 1); needs the keys of assign_round
hipError_t kmeans_begin(hipStream_t st, int endpoints, const void* d_keys, const uint64_t* d_weights, const uint32_t* d_goffs, uint32_t n, const kmeans_buffers& b,
                        const uint64_t** out_weights);
void kmeans_seed(hipStream_t st, uint32_t n, uint32_t k, const kmeans_buffers& b);
void kmeans_flags(hipStream_t st, int endpoints, uint32_t n, uint32_t k, const kmeans_buffers& b);
uint32_t kmeans_workgroups(uint32_t n);
const void* kmeans_wg_worst(const kmeans_buffers& b);
hipError_t kmeans_assign_round(hipStream_t st, int endpoints, const uint64_t* weights, uint32_t n, uint32_t k, const kmeans_buffers& b, bool have_live, bool want_worst,
                               uint32_t* d_assign, uint32_t debug_skip);
// a cluster's live word is the weight word of its sums: caller's array of k words -> b.sums[c * 17 + 16] and back
void kmeans_set_live(hipStream_t st, const uint64_t* d_live, uint32_t k, const kmeans_buffers& b);
void kmeans_get_live(hipStream_t st, uint64_t* d_live, uint32_t k, const kmeans_buffers& b);
hipError_t kmeans_update_round(hipStream_t st, uint32_t n, uint32_t k, const kmeans_buffers& b);

} // namespace bu
