// Best-bound node selection on the device frontier (sgufp_frontier_select, bnb.cpp): a stable
// partition of the stack that leaves the k open records with the largest ub on top, so that the
// next sgufp_bnb_step pops them.  (The reference's NodeQueue, DDSolver.h, orders nodes through a
// host priority queue; here the stack stays in HBM.)
//
//   threshold   radix select of the k-th largest ub over an order-preserving uint64 key, 8 passes
//               of one 8-bit digit: k_sel_hist (grid-stride histogram of the records that match
//               the prefix so far) and k_sel_pick (one block: picks the digit, writes the prefix
//               and the remaining rank for the next pass).  It ends with the threshold key T,
//               count(ub > T) and the number of records == T still needed.
//   flags       the records == T that are taken are the topmost ones: k_sel_count_eq per block,
//               k_sel_scan_eq (one block) gives every block the == T records above it;
//               k_sel_count then has each record's flag and counts, per block, the selected
//               records and both groups' solution lengths; k_sel_scan (one block) turns the block
//               totals into offsets and writes the call's results.
//   scatter     k_sel_scatter copies every record's fields and its solution span, compacted to
//               sol_len, into the second set of frontier arrays; the host swaps the two sets.
//
// Every kernel reads what an earlier launch on the stream wrote and finishes on its own: no
// workgroup waits for another one.  Counts and arena offsets across blocks are int64; inside a
// block of kSelBlock records they fit 32 bits (256 records x 65535 entries < 2^24, and a chunk
// of 256 such block totals < 2^32).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dd_device.hpp"
#define SGUFP_MULTI_WAVE_TU 1
#include "wave.hpp"
#include "select_device.hpp"

namespace sgufp {

namespace {

constexpr int kSelWaves = kSelBlock / kWave;

// largest double <-> largest key; -0.0 and 0.0 share one key
__device__ __forceinline__ uint64_t ub_key(double u) {
    uint64_t b = (u == 0.0) ? 0ull : (uint64_t)__double_as_longlong(u);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// exclusive prefix of x over the block's threads (in thread order) and the block's total;
// `tot` is LDS of kSelWaves + 1 entries.  Every thread of the block calls it.
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t x, uint32_t *tot, uint32_t &total) {
    const uint32_t incl = wave_scan_incl(x);
    const int w = (int)threadIdx.x / kWave;
    __syncthreads();   // the previous use of tot is over
    if (lane() == kWave - 1) tot[w] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int i = 0; i < kSelWaves; i++) {
        const uint32_t t = tot[i];
        base += (i < w) ? t : 0u;
        all += t;
    }
    total = all;
    return base + incl - x;
}

// 1 when record i of block b is selected: ub > T, or ub == T and fewer than `need` records == T
// lie above it (eq_higher: those of its own block)
__device__ __forceinline__ bool sel_flag(uint64_t key, uint64_t T, int64_t eq_above, uint32_t eq_higher, int64_t need) {
    return key > T || (key == T && eq_above + (int64_t)eq_higher < need);
}

}  // namespace

// ---- threshold -------------------------------------------------------------------------------
// pass p looks at digit (key >> (56 - 8 p)) & 255 of the records whose higher digits equal the
// prefix chosen so far
__global__ void __launch_bounds__(kSelBlock) k_sel_hist(const double *ub, int64_t n, int pass, const SelState *state,
                                                        unsigned long long *hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const uint64_t prefix = state->prefix;
    for (int64_t i = (int64_t)blockIdx.x * kSelBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSelBlock) {
        const uint64_t key = ub_key(ub[i]);
        if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    const uint32_t c = h[threadIdx.x];
    if (c) atomicAdd(&hist[threadIdx.x], (unsigned long long)c);
}

// one block: the digit d with count(digit > d) < rank <= count(digit >= d); the bins are
// cleared for the next pass
__global__ void __launch_bounds__(kSelBlock) k_sel_pick(int pass, SelState *state, unsigned long long *hist) {
    __shared__ unsigned long long h[256];
    h[threadIdx.x] = hist[threadIdx.x];
    hist[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int64_t rank = state->rank;
    int64_t above = 0;
    int d = 255;
    for (; d > 0; d--) {
        if (above + (int64_t)h[d] >= rank) break;
        above += (int64_t)h[d];
    }
    state->prefix |= (uint64_t)d << (56 - 8 * pass);
    state->rank = rank - above;
    state->gt += above;
}

// ---- flags -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSelBlock) k_sel_count_eq(const double *ub, int64_t n, const SelState *state,
                                                            uint32_t *cnt_eq) {
    __shared__ uint32_t tot[kSelWaves + 1];
    const int64_t i = (int64_t)blockIdx.x * kSelBlock + threadIdx.x;
    const uint32_t eq = (i < n && ub_key(ub[i]) == state->prefix) ? 1u : 0u;
    uint32_t total;
    (void)block_scan_excl(eq, tot, total);
    if (threadIdx.x == 0) cnt_eq[blockIdx.x] = total;
}

// one block: eq_above[b] = sum of cnt_eq over the blocks above b
__global__ void __launch_bounds__(kSelBlock) k_sel_scan_eq(const uint32_t *cnt_eq, int nb, int64_t *eq_above) {
    __shared__ uint32_t tot[kSelWaves + 1];
    int64_t carry = 0;   // records == T in the chunks above this one
    for (int hi = nb; hi > 0; hi -= kSelBlock) {
        // thread t holds block hi - 1 - t: the scan runs from the top of the stack down
        const int b = hi - 1 - (int)threadIdx.x;
        const uint32_t c = b >= 0 ? cnt_eq[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_excl(c, tot, total);
        if (b >= 0) eq_above[b] = carry + (int64_t)ex;
        carry += (int64_t)total;
    }
}

__global__ void __launch_bounds__(kSelBlock) k_sel_count(const double *ub, const uint16_t *sol_len, int64_t n,
                                                         int64_t k, SelState *state, const int64_t *eq_above,
                                                         SelBlockCounts bc) {
    __shared__ uint32_t tot[kSelWaves + 1];
    const int b = blockIdx.x;
    const int64_t i = (int64_t)b * kSelBlock + threadIdx.x;
    const bool in = i < n;
    const uint64_t T = state->prefix;
    const uint64_t key = in ? ub_key(ub[i]) : 0ull;
    const uint32_t len = in ? (uint32_t)sol_len[i] : 0u;
    const uint32_t eq = (in && key == T) ? 1u : 0u;
    uint32_t eq_total, total;
    const uint32_t eq_ex = block_scan_excl(eq, tot, eq_total);
    const bool sel = in && sel_flag(key, T, eq_above[b], eq_total - eq_ex - eq, state->rank);
    if (sel && i < n - k) state->moved = 1;   // a selected record below the top k: the stack changes
    (void)block_scan_excl(sel ? 1u : 0u, tot, total);
    const uint32_t n_sel = total;
    (void)block_scan_excl(sel ? len : 0u, tot, total);
    const uint32_t l_sel = total;
    (void)block_scan_excl((in && !sel) ? len : 0u, tot, total);
    if (threadIdx.x == 0) {
        bc.sel_cnt[b] = n_sel;
        bc.sel_len[b] = l_sel;
        bc.non_len[b] = total;
    }
}

// one block: exclusive prefixes of the block totals in stack order, and the results of the call
__global__ void __launch_bounds__(kSelBlock) k_sel_scan(SelBlockCounts bc, int nb, int64_t n, int64_t k,
                                                        SelState *state) {
    __shared__ uint32_t tot[kSelWaves + 1];
    int64_t c_sel = 0, c_slen = 0, c_nlen = 0;
    for (int lo = 0; lo < nb; lo += kSelBlock) {
        const int b = lo + (int)threadIdx.x;
        const bool in = b < nb;
        uint32_t total;
        uint32_t ex = block_scan_excl(in ? bc.sel_cnt[b] : 0u, tot, total);
        if (in) bc.sel_cnt_pre[b] = c_sel + (int64_t)ex;
        c_sel += (int64_t)total;
        ex = block_scan_excl(in ? bc.sel_len[b] : 0u, tot, total);
        if (in) bc.sel_len_pre[b] = c_slen + (int64_t)ex;
        c_slen += (int64_t)total;
        ex = block_scan_excl(in ? bc.non_len[b] : 0u, tot, total);
        if (in) bc.non_len_pre[b] = c_nlen + (int64_t)ex;
        c_nlen += (int64_t)total;
    }
    if (threadIdx.x == 0) {
        state->n_sel = c_sel;
        state->non_len = c_nlen;
        state->sol_top = c_nlen + c_slen;
        state->bad = c_sel == k ? 0 : 1;
    }
}

// ---- scatter ---------------------------------------------------------------------------------
// Non-selected records go to entries [0, n - k) and the arena from 0 on, selected ones to
// [n - k, n) and the arena behind the others, both in stack order.  One record per thread for
// the fields; then the block's waves take its records in turn and the lanes stride over each
// solution span.  A destination outside the arrays (the counts of the earlier kernels would
// have to be wrong) is not written and raises state->oob.
__global__ void __launch_bounds__(kSelBlock) k_sel_scatter(FrontierDev src, FrontierDev dst, int64_t n, int64_t k,
                                                           int64_t sol_cap, SelState *state, const int64_t *eq_above,
                                                           SelBlockCounts bc) {
    __shared__ uint32_t tot[kSelWaves + 1];
    __shared__ int64_t s_from[kSelBlock], s_to[kSelBlock];
    __shared__ uint32_t s_len[kSelBlock];
    if (state->bad) return;   // written by the launch before this one: the same for every thread
    const int b = blockIdx.x;
    const int t = threadIdx.x;
    const int64_t i = (int64_t)b * kSelBlock + t;
    const bool in = i < n;
    const uint64_t T = state->prefix;
    const uint64_t key = in ? ub_key(src.ub[i]) : 0ull;
    const uint32_t len = in ? (uint32_t)src.sol_len[i] : 0u;
    const uint32_t eq = (in && key == T) ? 1u : 0u;
    uint32_t eq_total, total;
    const uint32_t eq_ex = block_scan_excl(eq, tot, eq_total);
    const bool sel = in && sel_flag(key, T, eq_above[b], eq_total - eq_ex - eq, state->rank);
    const uint32_t sel_ex = block_scan_excl(sel ? 1u : 0u, tot, total);
    const uint32_t slen_ex = block_scan_excl(sel ? len : 0u, tot, total);
    const uint32_t nlen_ex = block_scan_excl((in && !sel) ? len : 0u, tot, total);
    const int64_t sel_pre = bc.sel_cnt_pre[b];
    int64_t e, o;
    if (sel) {
        e = (n - k) + sel_pre + (int64_t)sel_ex;
        o = state->non_len + bc.sel_len_pre[b] + (int64_t)slen_ex;
    } else {
        e = ((int64_t)b * kSelBlock - sel_pre) + (int64_t)(t - (int)sel_ex);
        o = bc.non_len_pre[b] + (int64_t)nlen_ex;
    }
    bool ok = in;
    if (in && (e < 0 || e >= n || o < 0 || o + (int64_t)len > sol_cap)) {
        state->oob = 1;
        ok = false;
    }
    if (ok) {
        dst.gl[e] = src.gl[i];
        dst.lb[e] = src.lb[i];
        dst.ub[e] = src.ub[i];
        dst.mask[e] = src.mask[i];
        dst.valid[e] = src.valid[i];
        dst.sol_off[e] = o;
        dst.sol_len[e] = (uint16_t)len;
    }
    s_from[t] = ok ? src.sol_off[i] : 0;
    s_to[t] = o;
    s_len[t] = ok ? len : 0u;
    __syncthreads();
    for (int r = t / kWave; r < kSelBlock; r += kSelWaves) {
        const uint32_t l = s_len[r];
        const int64_t from = s_from[r], to = s_to[r];
        for (uint32_t x = (uint32_t)lane(); x < l; x += kWave) dst.sol[to + x] = src.sol[from + x];
    }
}

// ---- the launches of one select, back to back on the stream ----------------------------------
hipError_t launch_select(const FrontierDev &src, const FrontierDev &dst, int64_t n, int64_t k, int64_t sol_cap,
                         SelState *state, unsigned long long *hist, uint32_t *cnt_eq, int64_t *eq_above,
                         const SelBlockCounts &bc, hipStream_t st) {
    const int nb = (int)((n + kSelBlock - 1) / kSelBlock);
    const int gh = std::min(nb, kSelHistBlocks);
    for (int pass = 0; pass < 8; pass++) {
        hipLaunchKernelGGL(k_sel_hist, dim3(gh), dim3(kSelBlock), 0, st, src.ub, n, pass, state, hist);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(kSelBlock), 0, st, pass, state, hist);
    }
    hipLaunchKernelGGL(k_sel_count_eq, dim3(nb), dim3(kSelBlock), 0, st, src.ub, n, state, cnt_eq);
    hipLaunchKernelGGL(k_sel_scan_eq, dim3(1), dim3(kSelBlock), 0, st, cnt_eq, nb, eq_above);
    hipLaunchKernelGGL(k_sel_count, dim3(nb), dim3(kSelBlock), 0, st, src.ub, src.sol_len, n, k, state, eq_above, bc);
    hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(kSelBlock), 0, st, bc, nb, n, k, state);
    hipLaunchKernelGGL(k_sel_scatter, dim3(nb), dim3(kSelBlock), 0, st, src, dst, n, k, sol_cap, state, eq_above, bc);
    return hipGetLastError();
}

}  // namespace sgufp
