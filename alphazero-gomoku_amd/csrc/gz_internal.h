// gz_internal.h -- what the translation units of libgzero share on the host side: the
// one declaration of every cross-file entry point (each is defined in the file named
// beside it; definer and callers include this header, so the compiler checks them
// against each other) and the error / launch helpers.  Not part of include/gzero.h.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/gzero.h"

namespace gzpv {
struct TreeWs;  // gz_pvnet.h: the carved tree-forward workspace
}

extern "C" {
// the thread's last-error message (gz_selfplay.hip; tools/stamps_stub.cpp for the
// stand-alone instrumented builds)
void gz_internal_set_error(const char* msg);

// gz_plan.hip: gz_plan_search with optional leaf tags (d_leaf_meta, [leaf_cap])
int gz_internal_plan_search(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n,
                            const gz_search_params* p, const gz_planner_params* pp, const float* d_gn_weights,
                            void* d_workspace, void* d_trees, int32_t* d_moves, gz_search_stats* d_stats,
                            uint32_t* d_leaves, int32_t leaf_cap, int32_t* d_leaf_count, int32_t* d_leaf_meta,
                            void* stream);

// gz_selfplay.hip: selfplay_commit_kernel with the optional visit buffers (gz_puct.hip)
int gz_internal_selfplay_commit(void* d_slots, int32_t n_slots, const int32_t* d_moves, const gz_search_stats* d_stats,
                                gz_record* d_records, int32_t record_cap, gz_selfplay_counters* d_counters,
                                const uint16_t* d_pend_visits, uint16_t* d_out_visits, void* stream);

// gz_gnet.hip: the search roots' full forward, maps and policy-conv outputs into slots
// 0..n-1 (d_rec: n record rows of scratch)
int gz_internal_gn_roots(const float* d_weights, const uint32_t* d_rows, int32_t n, void* d_slots, float* d_rec,
                         void* stream);

// gz_gnet.hip: the planner nets over tagged rows (gz_plan.hip's collect kernel)
int gz_internal_gn_forward_tagged(const float* d_weights, const uint32_t* d_rows, int32_t max_rows,
                                  const int32_t* d_count, const int32_t* d_full_list, const int32_t* d_full_count,
                                  const int32_t* d_inc_list, const int32_t* d_inc_count, const void* d_tags,
                                  void* d_slots, float* d_p, float* d_q, float* d_rec, float* d_hscratch,
                                  int32_t* d_queue, void* stream);

// gz_pvsym.hip: row i of d_out = row i of d_in under its symmetry t (d_sym_in[i] & 7, or
// sym_of(seed, row) when d_sym_in is NULL), t into d_sym_out[i]; d_out may be d_in
int gz_internal_sym_boards(const uint32_t* d_in, uint32_t* d_out, int32_t n, const int32_t* d_count,
                           const uint8_t* d_sym_in, uint64_t seed, uint8_t* d_sym_out, void* stream);
// gz_pvsym.hip: the non-NULL 225-wide rows mapped back in place, row i by d_sym[i]
int gz_internal_sym_rows(float* d_logits, float* d_probs, double* d_prior, int32_t n, const int32_t* d_count,
                         const uint8_t* d_sym, void* stream);
}  // extern "C"

// The stages of gz_pv_forward_tree (gz_pvnet.hip) on the carved workspace t.  C++
// linkage: a declaration that drifts from its definition fails to link.
// gz_pvinc.hip: counters and lists (roots, full, children, grandchildren, patch slots)
int gz_internal_tree_classify(const gzpv::TreeWs& t, const uint32_t* d_boards, const int32_t* d_meta, int32_t n,
                              const int32_t* d_count, int32_t root_cap, void* stream);
// gz_pvinc.hip: the root children and the grandchildren (gz_internal_tree_delta)
int gz_internal_tree_children(const gzpv::TreeWs& t, const float* d_weights, const uint32_t* d_boards,
                              const int32_t* d_meta, int32_t n, const int32_t* d_count, int grid, void* stream);
// gz_pvdg.hip: the root children, then the grandchildren, through pv_dg_kernel
int gz_internal_tree_delta(const gzpv::TreeWs& t, const float* d_weights, const uint32_t* d_boards,
                           const int32_t* d_meta, int grid, void* stream);

// set the error message, return the code
inline int gz_fail(int code, const char* msg) {
    gz_internal_set_error(msg);
    return code;
}
inline int gz_fail(int code, const std::string& msg) { return gz_fail(code, msg.c_str()); }

// after kernel launches: GZ_OK, or GZ_ERR_HIP with "what: <the HIP error>"
inline int gz_check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gz_fail(GZ_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return GZ_OK;
}

// the device's CU count (256, the MI355X's, when it cannot be read)
inline int gz_cu_count() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    return cus;
}
