// Shared between select_kernels.hip and bnb.cpp (sgufp_frontier_select): the device state of
// one select and the per-block arrays of its scans.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dd_device.hpp"

namespace sgufp {

constexpr int kSelBlock = 256;        // records per block (one per thread) of the flag / scatter kernels
constexpr int kSelHistBlocks = 1024;  // blocks of the grid-stride histogram at most

// Written by the host before the first launch (rank = k, everything else 0), read back after
// the last one.
struct SelState {
    uint64_t prefix;   // radix select: the digits chosen so far; after 8 passes the threshold key T
    int64_t rank;      // rank still to find among the records matching the prefix; at the end the
                       // number of records == T that are selected
    int64_t gt;        // records with key > T
    int64_t n_sel;     // selected records counted by the flag kernels (== k)
    int64_t non_len;   // solution entries of the non-selected records
    int64_t sol_top;   // solution entries of all records: the top of the compacted arena
    int32_t moved;     // 1: a selected record lies below the top k
    int32_t bad;       // 1: n_sel != k (the scatter then writes nothing)
    int32_t oob;       // 1: the scatter met a destination outside the arrays
    int32_t pad;
};

struct SelBlockCounts {   // [blocks]
    uint32_t *sel_cnt, *sel_len, *non_len;            // per block: selected records, their / the others' entries
    int64_t *sel_cnt_pre, *sel_len_pre, *non_len_pre;   // exclusive prefixes over the blocks
};

hipError_t launch_select(const FrontierDev &src, const FrontierDev &dst, int64_t n, int64_t k, int64_t sol_cap,
                         SelState *state, unsigned long long *hist, uint32_t *cnt_eq, int64_t *eq_above,
                         const SelBlockCounts &bc, hipStream_t st);

}  // namespace sgufp
