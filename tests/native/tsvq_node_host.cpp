// tsvq_node_host.cpp -- test-only shim over basis_universal_amd/csrc/host/tsvq.h: ONE node of the tree at a time (helpers.tsvq_node_host()).
//   tn_root:  the bu_tsvq_root record of a member list in list order (make_root, enc.h:1708-1735)
//   tn_split: the bu_tsvq_split record of a node (member list, weight, origin) and its two child lists, left first (prep_split + refine_split)
// Both go through the bodies generate() runs (tsvq<N>::root_of / split_of); tests/test_tsvq_node_host.py replays the reference's queue over them and
// compares the tree with bu_host_tsvq, so the per-node records the GPU tests compare against are tied to the tree builder and, through it, to the reference.
// The records have the layout of include/basisu_hip.h (origin / centroid components N..15 and pad are 0). Variances are RAW: split() substitutes 1e-4 afterwards.
// Built and bound by tests/native_libs.py.
#include <cstdint>
#include <cstring>
#include "../../basis_universal_amd/csrc/host/tsvq.h"
#include "host_api.h"

namespace {
struct root_rec { float origin[16]; uint64_t weight; float var; uint32_t pad; };
struct split_rec { uint32_t ok, l_count, r_count, pad; uint64_t l_weight, r_weight; float l_var, r_var; float l_centroid[16], r_centroid[16]; };
static_assert(sizeof(root_rec) == 80 && sizeof(split_rec) == 168, "layout of bu_tsvq_root / bu_tsvq_split");

struct handle {
    int dim;
    bu::tsvq<6> q6;
    bu::tsvq<16> q16;
};

template <int N> void root(const bu::tsvq<N>& q, const uint32_t* members, uint32_t count, root_rec* out) {
    std::memset(out, 0, sizeof(*out));
    float origin[N];
    q.root_of(members, count, origin, out->weight, out->var);
    std::memcpy(out->origin, origin, sizeof(origin));
}

template <int N> void split(const bu::tsvq<N>& q, const uint32_t* members, uint32_t count, uint64_t weight, const float* origin, split_rec* out, uint32_t* children) {
    std::memset(out, 0, sizeof(*out));
    typename bu::tsvq<N>::side L, R;
    if (!q.split_of(members, count, weight, origin, L, R)) return;   // ok = 0
    out->ok = 1;
    out->l_count = (uint32_t)L.members.size(); out->r_count = (uint32_t)R.members.size();
    out->l_weight = L.weight; out->r_weight = R.weight;
    out->l_var = L.var; out->r_var = R.var;
    std::memcpy(out->l_centroid, L.centroid, sizeof(L.centroid));
    std::memcpy(out->r_centroid, R.centroid, sizeof(R.centroid));
    if (out->l_count) std::memcpy(children, L.members.data(), (size_t)out->l_count * 4);
    if (out->r_count) std::memcpy(children + out->l_count, R.members.data(), (size_t)out->r_count * 4);
}
}  // namespace

HOST_API void* tn_open(uint32_t dim, const float* rows, const uint64_t* weights, uint32_t n) {
    if (dim != 6 && dim != 16) return nullptr;
    handle* h = new handle();
    h->dim = (int)dim;
    if (dim == 6) h->q6.set_training(rows, weights, n); else h->q16.set_training(rows, weights, n);
    return h;
}
HOST_API void tn_close(void* p) { delete static_cast<handle*>(p); }
HOST_API void tn_root(void* p, const uint32_t* members, uint32_t count, void* out_root) {
    handle* h = static_cast<handle*>(p);
    if (h->dim == 6) root<6>(h->q6, members, count, static_cast<root_rec*>(out_root));
    else root<16>(h->q16, members, count, static_cast<root_rec*>(out_root));
}
// out_children: room for `count` indices; left list first, then the right one (untouched where ok == 0)
HOST_API void tn_split(void* p, const uint32_t* members, uint32_t count, uint64_t weight, const float* origin, void* out_split, uint32_t* out_children) {
    handle* h = static_cast<handle*>(p);
    if (h->dim == 6) split<6>(h->q6, members, count, weight, origin, static_cast<split_rec*>(out_split), out_children);
    else split<16>(h->q16, members, count, weight, origin, static_cast<split_rec*>(out_split), out_children);
}
