// Batched branch-and-bound rounds on the device: the replacement of the reference's
// DDSolver master/worker loop (DDSolver.cpp:556-846) around NodeExplorer::process
// (NodeExplorer.cpp:915-986), with the open-node frontier resident in HBM.
//
// One round (sgufp_bnb_step) = what the reference's workers do for a batch of popped nodes,
// as the steps of BnbRound:
//   pop_and_relax     pop the top `b` records of the frontier stack (LIFO like lf_queue::pop);
//                     records with ub <= zOpt are pruned unprocessed (DDSolver.cpp:707-711) inside
//                     k_relax, every other one is processed against the current pools and zOpt
//                     (k_relax + k_emit);
//   classify          the statuses: counters, and the exact DDs that enter their loop;
//   refine            exact DDs run the refinement loop of NodeExplorer.cpp:946-969: argmax path,
//                     stop when the path was seen ({ub, ub}), else the device scenario subproblem,
//                     the new cut is appended to the global pool (Container::add) and applied to
//                     that DD (k_refine); the round's limits cut loops short (deferred);
//   save_deferred     the deferred records and their seen paths are kept on the host;
//   update_incumbent  max(zOpt, lb of closed exact DDs)  (the CAS at DDSolver.cpp:723-731);
//   push_children     cutset children of parents with ub > zOpt are pushed (DDSolver.cpp:744-748),
//                     compacted from the emit buffers onto the stack where the popped batch was;
//   push_deferred     the deferred records go back on top of the children, in their frontier
//                     order and with the bound their loop reached: popped first next round.
// Records processed in one round all see the same zOpt and pools, as concurrent workers
// of the reference may.  Children of a parent keep the reference's cutset order; parents
// keep their frontier order, so the top of the stack is the last parent's first child.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "ctx.hpp"

namespace sgufp {
hipError_t launch_loop_check(const BatchOut &out, const SeenLists &S, const int32_t *act, int na, int m, int32_t *flag,
                             int32_t *chains, hipStream_t st);
hipError_t launch_seen_append(const BatchOut &out, const SeenLists &S, const int32_t *fresh, int nf, int m,
                              hipStream_t st);
hipError_t launch_append_cuts(const int32_t *cut_type, const double *cut_rhs, const double *cut_row, int nf, int stride,
                              int first, double *rows, double *rhs, double *coefT, const int32_t *slot_tab, int L,
                              int us, double *row_ub, int32_t *row_id, uint8_t *is_feas, hipStream_t st);
hipError_t launch_gather_rows(const double *rows, const double *rhs, const int32_t *ids, int k, int stride, double *out,
                              hipStream_t st);
hipError_t launch_frontier_bound(const double *ub, int64_t n, double z, double *pmax, int64_t *pcnt, int *blocks,
                                 hipStream_t st);
}  // namespace sgufp

bool sgufp_ctx::inc_store(double value, const int16_t *src, int32_t len, hipMemcpyKind kind) {
    const size_t cap = (size_t)std::max(std::max(sc.Lcap, net.L), 1);
    if (len < 0 || (size_t)len > cap) {
        err = "incumbent path longer than totalLayers";
        return false;
    }
    if (!d_inc_path && !alloc(d_inc_path, cap, "incumbent path")) return false;
    if (len && !hip_ok(hipMemcpyAsync(d_inc_path, src, (size_t)len * sizeof(int16_t), kind, stream), "incumbent path"))
        return false;
    inc_value = value;
    inc_len = len;
    inc_host_valid = false;
    return true;
}

void sgufp_ctx::decode_states(const uint16_t *gl, const uint32_t *mask, size_t count, int64_t *states_off,
                              int16_t *states) const {
    int64_t ss = 0;
    for (size_t c = 0; c < count; c++) {
        if (states_off) states_off[c] = ss;
        const int u = net.layer_universe[gl[c]];
        for (uint32_t m = mask[c]; m; m &= m - 1) {
            if (states) states[ss] = net.sets[u][__builtin_ctz(m)];
            ss++;
        }
    }
    if (states_off) states_off[count] = ss;
}

void sgufp_ctx::frontier_alt_drop() {
    if (fr_alt.gl) release(fr_alt.gl);
    if (fr_alt.lb) release(fr_alt.lb);
    if (fr_alt.ub) release(fr_alt.ub);
    if (fr_alt.mask) release(fr_alt.mask);
    if (fr_alt.valid) release(fr_alt.valid);
    if (fr_alt.sol_off) release(fr_alt.sol_off);
    if (fr_alt.sol_len) release(fr_alt.sol_len);
    if (fr_alt.sol) release(fr_alt.sol);
    fr_alt = FrontierDev{};
    fr_alt_ready = false;
}

// scratch of one select over n records and the second set of frontier arrays; false (and no
// second set) when device memory does not allow it
bool sgufp_ctx::select_reserve(int64_t n) {
    const size_t nb = (size_t)((n + kSelBlock - 1) / kSelBlock);
    bool ok = (d_sel_state || alloc(d_sel_state, 1, "frontier select")) &&
              (d_sel_hist || alloc(d_sel_hist, 256, "frontier select")) &&
              grow(d_sel_u32, sel_u32_cap, 4 * nb, "frontier select") &&
              grow(d_sel_i64, sel_i64_cap, 4 * nb, "frontier select");
    if (ok && !fr_alt_ready) {
        const size_t cap = (size_t)fr_cap;
        ok = alloc(fr_alt.gl, cap, "frontier select") && alloc(fr_alt.lb, cap, "frontier select") &&
             alloc(fr_alt.ub, cap, "frontier select") && alloc(fr_alt.mask, cap, "frontier select") &&
             alloc(fr_alt.valid, cap, "frontier select") && alloc(fr_alt.sol_off, cap, "frontier select") &&
             alloc(fr_alt.sol_len, cap, "frontier select") && alloc(fr_alt.sol, fr_sol_cap, "frontier select");
        if (ok) fr_alt_ready = true;
        else frontier_alt_drop();
    }
    if (!ok) (void)hipGetLastError();   // the failed hipMalloc is reported here, not by a later launch
    return ok;
}

bool sgufp_ctx::frontier_reserve(int64_t entries, size_t sol_entries) {
    // the second set of sgufp_frontier_select keeps the first set's capacities: it goes when
    // the first set grows, and the next select allocates it again
    if (fr_alt_ready && (entries > fr_cap || sol_entries > fr_sol_cap)) {
        if (!sync()) return false;
        frontier_alt_drop();
    }
    if (entries > fr_cap) {
        const int64_t cap = std::max<int64_t>(entries, std::max<int64_t>(2 * fr_cap, 4096));
        FrontierDev f{};
        if (!alloc(f.gl, cap, "frontier") || !alloc(f.lb, cap, "frontier") || !alloc(f.ub, cap, "frontier") ||
            !alloc(f.mask, cap, "frontier") || !alloc(f.valid, cap, "frontier") ||
            !alloc(f.sol_off, cap, "frontier") || !alloc(f.sol_len, cap, "frontier"))
            return false;
        const size_t k = (size_t)fr_n;
        if (k && (!hip_ok(hipMemcpyAsync(f.gl, fr.gl, k * 2, hipMemcpyDeviceToDevice, stream), "D2D") ||
                  !hip_ok(hipMemcpyAsync(f.lb, fr.lb, k * 8, hipMemcpyDeviceToDevice, stream), "D2D") ||
                  !hip_ok(hipMemcpyAsync(f.ub, fr.ub, k * 8, hipMemcpyDeviceToDevice, stream), "D2D") ||
                  !hip_ok(hipMemcpyAsync(f.mask, fr.mask, k * 4, hipMemcpyDeviceToDevice, stream), "D2D") ||
                  !hip_ok(hipMemcpyAsync(f.valid, fr.valid, k, hipMemcpyDeviceToDevice, stream), "D2D") ||
                  !hip_ok(hipMemcpyAsync(f.sol_off, fr.sol_off, k * 8, hipMemcpyDeviceToDevice, stream), "D2D") ||
                  !hip_ok(hipMemcpyAsync(f.sol_len, fr.sol_len, k * 2, hipMemcpyDeviceToDevice, stream), "D2D")))
            return false;
        if (!sync()) return false;
        release(fr.gl); release(fr.lb); release(fr.ub); release(fr.mask); release(fr.valid);
        release(fr.sol_off); release(fr.sol_len);
        f.sol = fr.sol;
        fr = f;
        fr_cap = cap;
    }
    if (sol_entries > fr_sol_cap) {
        const size_t cap = std::max(sol_entries, std::max<size_t>(2 * fr_sol_cap, 1 << 20));
        int16_t *s = nullptr;
        if (!alloc(s, cap, "frontier sol")) return false;
        if (fr_sol_top && !hip_ok(hipMemcpyAsync(s, fr.sol, (size_t)fr_sol_top * 2, hipMemcpyDeviceToDevice, stream), "D2D"))
            return false;
        if (!sync()) return false;
        release(fr.sol);
        fr.sol = s;
        fr_sol_cap = cap;
    }
    return true;
}

// Seen-path lists of the refinement loops: slots x cap entries of Lcap int16 + len + hash, i.e.
// slots x cap x (2 Lcap + 10) bytes (1 024 slots x 64 x 572 B = 37 MB at 1k arcs).  cap doubles
// when one loop outgrows it and is kept for the search (the longest loop sets it); the lists go
// with sgufp_frontier_clear.
bool sgufp_ctx::loop_reserve(int slots, int cap) {
    const int Lc = std::max(sc.Lcap, 1);
    if (!d_lact) {
        const size_t B = (size_t)std::max(max_batch, 1);
        if (!alloc(d_lact, B, "loop") || !alloc(d_lflag, B, "loop") || !alloc(d_lchain, B, "loop") ||
            !alloc(d_lrowub, B, "loop"))
            return false;
    }
    if (seen.paths && slots <= seen_slots && cap <= seen.cap) return true;
    // grow (keeping the lists: a loop can outgrow the capacity mid-round)
    const int ns = std::max(slots, seen_slots);
    const int nc = std::max(cap, std::max(64, seen.cap ? 2 * seen.cap : 0));
    SeenLists t{};
    t.cap = nc;
    t.Lcap = Lc;
    if (!alloc(t.paths, (size_t)ns * nc * Lc, "seen paths") || !alloc(t.len, (size_t)ns * nc, "seen paths") ||
        !alloc(t.hash, (size_t)ns * nc, "seen paths") || !alloc(t.n, (size_t)ns, "seen paths"))
        return false;
    if (seen.paths) {
        const int oc = seen.cap;
        for (int sl = 0; sl < seen_slots; sl++) {
            if (!hip_ok(hipMemcpyAsync(t.paths + (size_t)sl * nc * Lc, seen.paths + (size_t)sl * oc * Lc,
                                       (size_t)oc * Lc * 2, hipMemcpyDeviceToDevice, stream), "D2D") ||
                !hip_ok(hipMemcpyAsync(t.len + (size_t)sl * nc, seen.len + (size_t)sl * oc, (size_t)oc * 2,
                                       hipMemcpyDeviceToDevice, stream), "D2D") ||
                !hip_ok(hipMemcpyAsync(t.hash + (size_t)sl * nc, seen.hash + (size_t)sl * oc, (size_t)oc * 8,
                                       hipMemcpyDeviceToDevice, stream), "D2D"))
                return false;
        }
        if (!hip_ok(hipMemcpyAsync(t.n, seen.n, (size_t)seen_slots * 4, hipMemcpyDeviceToDevice, stream), "D2D") ||
            !sync())
            return false;
        release(seen.paths); release(seen.len); release(seen.hash); release(seen.n);
    } else if (!hip_ok(hipMemsetAsync(t.n, 0, (size_t)ns * 4, stream), "memset")) {
        return false;
    }
    seen = t;
    seen_slots = ns;
    return true;
}

// the same 64-bit order-free hash as path_hash (bnb_kernels.hip)
static uint64_t mix64h(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

bool sgufp_ctx::seen_upload(int slot, const std::vector<std::vector<int16_t>> &paths) {
    const int cnt = (int)paths.size();
    if (cnt > seen.cap) return false;
    std::vector<int16_t> flat((size_t)cnt * seen.Lcap, 0);
    std::vector<uint16_t> len(cnt);
    std::vector<uint64_t> h(cnt);
    for (int i = 0; i < cnt; i++) {
        const auto &p = paths[i];
        len[i] = (uint16_t)p.size();
        uint64_t x = 0;
        for (size_t t = 0; t < p.size(); t++) {
            flat[(size_t)i * seen.Lcap + t] = p[t];
            x += mix64h(((uint64_t)(uint32_t)t << 16) ^ (uint64_t)(uint16_t)p[t] ^ 0x9E3779B97F4A7C15ull);
        }
        h[i] = x + mix64h((uint64_t)p.size() + 1);
    }
    const size_t e = (size_t)slot * seen.cap;
    const int32_t n32 = cnt;
    return upload(seen.paths + e * seen.Lcap, flat.data(), flat.size()) && upload(seen.len + e, len.data(), len.size()) &&
           upload(seen.hash + e, h.data(), h.size()) && upload(seen.n + slot, &n32, 1) && sync();
}

bool sgufp_ctx::seen_download(int slot, int count, std::vector<std::vector<int16_t>> &paths) {
    const size_t e = (size_t)slot * seen.cap;
    std::vector<int16_t> flat((size_t)count * seen.Lcap);
    std::vector<uint16_t> len(count);
    if (!download(flat.data(), seen.paths + e * seen.Lcap, flat.size()) || !download(len.data(), seen.len + e, len.size()) ||
        !sync())
        return false;
    paths.resize(count);
    for (int i = 0; i < count; i++)
        paths[i].assign(flat.begin() + (size_t)i * seen.Lcap, flat.begin() + (size_t)i * seen.Lcap + len[i]);
    return true;
}

static double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" {

int sgufp_bnb_set_trace(sgufp_ctx *ctx, int enabled) {
    if (!ctx) return SGUFP_ERR_ARG;
    ctx->trace = enabled != 0;
    for (auto &t : ctx->trace_items) t.clear();
    return SGUFP_OK;
}

int sgufp_bnb_trace(sgufp_ctx *ctx, int kind, int64_t *count, int64_t *path_entries, int32_t *record, int32_t *code,
                    int32_t *row, double *value, int64_t *path_off, int16_t *paths) {
    if (!ctx || kind < 0 || kind > 3) return SGUFP_ERR_ARG;
    const auto &items = ctx->trace_items[kind];
    int64_t pe = 0;
    for (size_t i = 0; i < items.size(); i++) {
        if (record) record[i] = items[i].record;
        if (code) code[i] = items[i].code;
        if (row) row[i] = items[i].row;
        if (value) value[i] = items[i].value;
        if (path_off) path_off[i] = pe;
        if (paths && !items[i].path.empty())
            std::memcpy(paths + pe, items[i].path.data(), items[i].path.size() * sizeof(int16_t));
        pe += (int64_t)items[i].path.size();
    }
    if (path_off) path_off[items.size()] = pe;
    if (count) *count = (int64_t)items.size();
    if (path_entries) *path_entries = pe;
    return SGUFP_OK;
}

int sgufp_bnb_set_limits(sgufp_ctx *ctx, int max_refine_iters, double round_seconds) {
    if (!ctx || max_refine_iters < 0 || !(round_seconds >= 0.0)) return SGUFP_ERR_ARG;
    ctx->bnb_max_iters = max_refine_iters;
    ctx->bnb_seconds = round_seconds;
    return SGUFP_OK;
}

void sgufp_ctx::make_record_key(uint16_t gl, uint32_t mask, const int16_t *sol, size_t len, std::string &key) {
    key.resize(6 + 2 * len);
    std::memcpy(&key[0], &gl, 2);
    std::memcpy(&key[2], &mask, 4);
    if (len) std::memcpy(&key[6], sol, 2 * len);
}

std::string FrontierRecords::key(int k) const {
    std::string key;
    sgufp_ctx::make_record_key(gl[k], mask[k], sol.data() + off[k], len[k], key);
    return key;
}

void FrontierRecords::append(const FrontierRecords &r, int k) {
    gl.push_back(r.gl[k]);
    lb.push_back(r.lb[k]);
    ub.push_back(r.ub[k]);
    mask.push_back(r.mask[k]);
    valid.push_back(r.valid[k]);
    len.push_back(r.len[k]);
    off.push_back((int64_t)sol.size());
    sol.insert(sol.end(), r.sol.begin() + r.off[k], r.sol.begin() + r.off[k] + r.len[k]);
}

bool sgufp_ctx::read_frontier(int64_t lo, int n, FrontierRecords &r) {
    r.gl.resize(n); r.lb.resize(n); r.ub.resize(n); r.mask.resize(n); r.valid.resize(n); r.len.resize(n);
    // arena span of the entries: offsets increase with the entry index, up to the next entry's
    // offset or, at the top of the stack, the top of the arena
    const bool top = lo + n >= fr_n;
    r.off.assign((size_t)n + 1, fr_sol_top);
    if (!download(r.gl.data(), fr.gl + lo, n) || !download(r.lb.data(), fr.lb + lo, n) ||
        !download(r.ub.data(), fr.ub + lo, n) || !download(r.mask.data(), fr.mask + lo, n) ||
        !download(r.valid.data(), fr.valid + lo, n) || !download(r.len.data(), fr.sol_len + lo, n) ||
        !download(r.off.data(), fr.sol_off + lo, (size_t)n + (top ? 0 : 1)) || !sync())
        return false;
    const int64_t s_lo = r.off[0];
    r.sol.resize((size_t)(r.off[n] - s_lo));
    if (!download(r.sol.data(), fr.sol + s_lo, r.sol.size()) || !sync()) return false;
    r.off.pop_back();
    for (auto &o : r.off) o -= s_lo;
    return true;
}

bool sgufp_ctx::write_frontier(int64_t e0, int64_t s0, const FrontierRecords &r) {
    const size_t n = r.gl.size();
    if (!frontier_reserve(e0 + (int64_t)n, (size_t)s0 + r.sol.size())) return false;
    std::vector<int64_t> off(r.off);
    for (auto &o : off) o += s0;
    return upload(fr.gl + e0, r.gl.data(), n) && upload(fr.lb + e0, r.lb.data(), n) &&
           upload(fr.ub + e0, r.ub.data(), n) && upload(fr.mask + e0, r.mask.data(), n) &&
           upload(fr.valid + e0, r.valid.data(), n) && upload(fr.sol_len + e0, r.len.data(), n) &&
           upload(fr.sol_off + e0, off.data(), n) && upload(fr.sol + s0, r.sol.data(), r.sol.size()) && sync();
}

int sgufp_frontier_clear(sgufp_ctx *ctx) {
    if (!ctx) return SGUFP_ERR_ARG;
    ctx->fr_n = 0;
    ctx->fr_sol_top = 0;
    ctx->deferred_seen.clear();
    ctx->inc_drop();
    if (ctx->seen.paths) {   // a new search starts with small seen-path lists again
        if (!ctx->sync()) return SGUFP_ERR_HIP;
        ctx->release(ctx->seen.paths);
        ctx->release(ctx->seen.len);
        ctx->release(ctx->seen.hash);
        ctx->release(ctx->seen.n);
        ctx->seen = SeenLists{};
        ctx->seen_slots = 0;
    }
    return SGUFP_OK;
}

int sgufp_frontier_size(const sgufp_ctx *ctx, int64_t *n, int64_t *sol_entries) {
    if (!ctx) return SGUFP_ERR_ARG;
    if (n) *n = ctx->fr_n;
    if (sol_entries) *sol_entries = ctx->fr_sol_top;
    return SGUFP_OK;
}

int sgufp_frontier_push(sgufp_ctx *ctx, int n, const uint16_t *gl, const double *lb, const double *ub,
                        const int64_t *states_off, const int16_t *states, const int64_t *sol_off, const int16_t *sol) {
    if (!ctx || n < 0 || (n && (!gl || !lb || !ub || !states_off || !sol_off))) return SGUFP_ERR_ARG;
    if (n == 0) return SGUFP_OK;
    FrontierRecords e;
    ctx->encode_records(n, gl, states_off, states, sol_off, sol, e);
    e.gl.assign(gl, gl + n);
    e.lb.assign(lb, lb + n);
    e.ub.assign(ub, ub + n);
    if (!ctx->write_frontier(ctx->fr_n, ctx->fr_sol_top, e)) return SGUFP_ERR_HIP;
    ctx->fr_n += n;
    ctx->fr_sol_top += (int64_t)e.sol.size();
    return SGUFP_OK;
}

// the frontier entries [lo, lo + n) for a caller: r, decoded to the caller's arrays (states,
// solutions re-based to 0)
static int read_records(sgufp_ctx *ctx, int64_t lo, int n, uint16_t *gl, double *lb, double *ub, int64_t *states_off,
                        int16_t *states, int64_t *sol_off, int16_t *sol, FrontierRecords &r) {
    if (!ctx->read_frontier(lo, n, r)) return SGUFP_ERR_HIP;
    if (gl) std::copy(r.gl.begin(), r.gl.end(), gl);
    if (lb) std::copy(r.lb.begin(), r.lb.end(), lb);
    if (ub) std::copy(r.ub.begin(), r.ub.end(), ub);
    ctx->decode_states(r.gl.data(), r.mask.data(), (size_t)n, states_off, states);
    int64_t o = 0;
    for (int k = 0; k < n; k++) {
        if (sol_off) sol_off[k] = o;
        if (sol) std::memcpy(sol + o, r.sol.data() + r.off[k], r.len[k] * sizeof(int16_t));
        o += r.len[k];
    }
    if (sol_off) sol_off[n] = o;
    return SGUFP_OK;
}

static int records_size(sgufp_ctx *ctx, int64_t lo, int n, int64_t *n_states, int64_t *n_sol) {
    std::vector<uint32_t> mask(n);
    std::vector<uint16_t> len(n);
    if (!ctx->download(mask.data(), ctx->fr.mask + lo, n) || !ctx->download(len.data(), ctx->fr.sol_len + lo, n) ||
        !ctx->sync())
        return SGUFP_ERR_HIP;
    int64_t ns = 0, nl = 0;
    for (int k = 0; k < n; k++) {
        ns += __builtin_popcount(mask[k]);
        nl += len[k];
    }
    if (n_states) *n_states = ns;
    if (n_sol) *n_sol = nl;
    return SGUFP_OK;
}

int sgufp_frontier_take_size(sgufp_ctx *ctx, int n, int from_bottom, int64_t *n_states, int64_t *n_sol) {
    if (!ctx || n < 0 || n > ctx->fr_n) return SGUFP_ERR_ARG;
    return records_size(ctx, from_bottom ? 0 : ctx->fr_n - n, n, n_states, n_sol);
}

int sgufp_frontier_peek_size(sgufp_ctx *ctx, int64_t first, int n, int64_t *n_states, int64_t *n_sol) {
    if (!ctx || n < 0 || first < 0 || first + n > ctx->fr_n) return SGUFP_ERR_ARG;
    return records_size(ctx, first, n, n_states, n_sol);
}

int sgufp_frontier_peek(sgufp_ctx *ctx, int64_t first, int n, uint16_t *gl, double *lb, double *ub,
                        int64_t *states_off, int16_t *states, int64_t *sol_off, int16_t *sol) {
    if (!ctx || n < 0 || first < 0 || first + n > ctx->fr_n) return SGUFP_ERR_ARG;
    FrontierRecords r;
    return read_records(ctx, first, n, gl, lb, ub, states_off, states, sol_off, sol, r);
}

int sgufp_frontier_take(sgufp_ctx *ctx, int n, int from_bottom, uint16_t *gl, double *lb, double *ub,
                        int64_t *states_off, int16_t *states, int64_t *sol_off, int16_t *sol) {
    if (!ctx || n < 0 || n > ctx->fr_n) return SGUFP_ERR_ARG;
    if (n == 0) {
        if (states_off) states_off[0] = 0;
        if (sol_off) sol_off[0] = 0;
        return SGUFP_OK;
    }
    const int64_t total = ctx->fr_n;
    const int64_t lo = from_bottom ? 0 : total - n;
    FrontierRecords r;
    const int rc = read_records(ctx, lo, n, gl, lb, ub, states_off, states, sol_off, sol, r);
    if (rc != SGUFP_OK) return rc;
    // a taken record leaves this context (another shard, or the caller): its deferred loop's
    // seen list goes no further (the receiver restarts the loop; re-solving a path only
    // re-adds a valid cut)
    for (int k = 0; k < n && !ctx->deferred_seen.empty(); k++) ctx->deferred_seen.erase(r.key(k));
    if (!from_bottom || n == total) {
        int64_t s_lo = 0;
        if (!ctx->download(&s_lo, ctx->fr.sol_off + lo, 1) || !ctx->sync()) return SGUFP_ERR_HIP;
        ctx->fr_n -= n;
        ctx->fr_sol_top = ctx->fr_n ? s_lo : 0;
        return SGUFP_OK;
    }
    // from the bottom: the remaining entries move down (frontier_drop_bottom, shard.cpp)
    return ctx->frontier_drop_bottom(n) ? SGUFP_OK : SGUFP_ERR_HIP;
}

int sgufp_cuts_rows(sgufp_ctx *ctx, int is_feasibility, int first, int count, double *rhs, double *rows) {
    if (!ctx || first < 0 || count < 0) return SGUFP_ERR_ARG;
    const auto &v = is_feasibility ? ctx->f_rows : ctx->o_rows;
    if (first + count > (int)v.size()) return SGUFP_ERR_ARG;
    if (count == 0) return SGUFP_OK;
    // one gather kernel ({rhs, row} blocks) and one download instead of a copy per row
    const size_t stride = (size_t)ctx->net.n_slots + 1, blk = stride + 1;
    if (!ctx->grow(ctx->d_rowbuf, ctx->rowbuf_cap, (size_t)count * blk, "cut rows") ||
        !ctx->grow(ctx->d_rowids, ctx->rowids_cap, (size_t)count, "cut rows"))
        return SGUFP_ERR_HIP;
    std::vector<double> buf((size_t)count * blk);
    if (!ctx->upload(ctx->d_rowids, v.data() + first, (size_t)count) ||
        !ctx->hip_ok(launch_gather_rows(ctx->d_rows, ctx->d_rhs, ctx->d_rowids, count, (int)stride, ctx->d_rowbuf,
                                        ctx->stream), "k_gather_rows") ||
        !ctx->download(buf.data(), ctx->d_rowbuf, buf.size()) || !ctx->sync())
        return SGUFP_ERR_HIP;
    for (int c = 0; c < count; c++) {
        if (rhs) rhs[c] = buf[(size_t)c * blk];
        if (rows) std::memcpy(rows + (size_t)c * stride, &buf[(size_t)c * blk + 1], stride * sizeof(double));
    }
    return SGUFP_OK;
}

int sgufp_bnb_incumbent(sgufp_ctx *ctx, double *value, int16_t *path, int32_t *len) {
    if (!ctx) return SGUFP_ERR_ARG;
    if (path && ctx->inc_len && !ctx->inc_host_valid) {
        ctx->inc_host.resize((size_t)ctx->inc_len);
        if (!ctx->download(ctx->inc_host.data(), ctx->d_inc_path, (size_t)ctx->inc_len) || !ctx->sync())
            return SGUFP_ERR_HIP;
        ctx->inc_host_valid = true;
    }
    if (value) *value = ctx->inc_value;
    if (len) *len = ctx->inc_len;
    if (path && ctx->inc_len) std::memcpy(path, ctx->inc_host.data(), (size_t)ctx->inc_len * sizeof(int16_t));
    return SGUFP_OK;
}

int sgufp_incumbent_set(sgufp_ctx *ctx, double value, const int16_t *path, int32_t len) {
    if (!ctx || len < 0 || len > ctx->net.L || (len && !path)) return SGUFP_ERR_ARG;
    if (!ctx->inc_store(value, path, len, hipMemcpyHostToDevice) || !ctx->sync()) return SGUFP_ERR_HIP;
    ctx->inc_host.assign(path, path + len);
    ctx->inc_host_valid = true;
    return SGUFP_OK;
}

int sgufp_frontier_bound(sgufp_ctx *ctx, double incumbent, double *max_ub, int64_t *open) {
    if (!ctx) return SGUFP_ERR_ARG;
    double mx = -__DBL_MAX__;
    int64_t cnt = 0;
    if (ctx->fr_n > 0) {   // an empty stack launches nothing
        if (!ctx->d_fb_max &&
            (!ctx->alloc(ctx->d_fb_max, kBoundBlocks, "frontier bound") || !ctx->alloc(ctx->d_fb_cnt, kBoundBlocks, "frontier bound")))
            return SGUFP_ERR_HIP;
        int g = 0;
        if (!ctx->hip_ok(launch_frontier_bound(ctx->fr.ub, ctx->fr_n, incumbent, ctx->d_fb_max, ctx->d_fb_cnt, &g, ctx->stream),
                         "k_frontier_bound"))
            return SGUFP_ERR_HIP;
        std::vector<double> pm((size_t)g);
        std::vector<int64_t> pc((size_t)g);
        if (!ctx->download(pm.data(), ctx->d_fb_max, (size_t)g) || !ctx->download(pc.data(), ctx->d_fb_cnt, (size_t)g) ||
            !ctx->sync())
            return SGUFP_ERR_HIP;
        for (int i = 0; i < g; i++) {
            mx = std::max(mx, pm[i]);
            cnt += pc[i];
        }
    }
    if (max_ub) *max_ub = mx;
    if (open) *open = cnt;
    return SGUFP_OK;
}

// the double whose order-preserving key (ub_key, select_kernels.hip) is `key`; 0.0 for either zero
static double key_to_ub(uint64_t key) {
    const uint64_t b = (key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key;
    double u;
    std::memcpy(&u, &b, sizeof u);
    return u;
}

int sgufp_frontier_select(sgufp_ctx *ctx, int k, int policy, int64_t *selected, double *threshold) {
    if (!ctx || (policy != SGUFP_SELECT_LIFO && policy != SGUFP_SELECT_BEST_BOUND)) return SGUFP_ERR_ARG;
    const int64_t n = ctx->fr_n;
    const int64_t kk = k <= 0 ? ctx->max_batch : std::min(k, ctx->max_batch);
    if (policy == SGUFP_SELECT_LIFO || n == 0 || kk >= n) {
        // the top min(k, n) records as they lie: no kernel; their smallest ub comes down only
        // when the caller asks for it
        const int64_t m = std::min(kk, n);
        if (selected) *selected = m;
        if (threshold) {
            std::vector<double> ub((size_t)m);
            if (!ctx->download(ub.data(), ctx->fr.ub + (n - m), (size_t)m) || !ctx->sync()) return SGUFP_ERR_HIP;
            *threshold = m ? *std::min_element(ub.begin(), ub.end()) : -__DBL_MAX__;
        }
        return SGUFP_OK;
    }
    if (!ctx->select_reserve(n)) return SGUFP_ERR_CAPACITY;
    const size_t nb = (size_t)((n + kSelBlock - 1) / kSelBlock);
    SelBlockCounts bc{};
    uint32_t *cnt_eq = ctx->d_sel_u32;
    bc.sel_cnt = ctx->d_sel_u32 + nb;
    bc.sel_len = ctx->d_sel_u32 + 2 * nb;
    bc.non_len = ctx->d_sel_u32 + 3 * nb;
    int64_t *eq_above = ctx->d_sel_i64;
    bc.sel_cnt_pre = ctx->d_sel_i64 + nb;
    bc.sel_len_pre = ctx->d_sel_i64 + 2 * nb;
    bc.non_len_pre = ctx->d_sel_i64 + 3 * nb;
    SelState s{};
    s.rank = kk;
    if (!ctx->upload(ctx->d_sel_state, &s, 1) ||
        !ctx->hip_ok(hipMemsetAsync(ctx->d_sel_hist, 0, 256 * sizeof(unsigned long long), ctx->stream), "memset") ||
        !ctx->hip_ok(launch_select(ctx->fr, ctx->fr_alt, n, kk, (int64_t)ctx->fr_sol_cap, ctx->d_sel_state,
                                   ctx->d_sel_hist, cnt_eq, eq_above, bc, ctx->stream), "frontier select") ||
        !ctx->download(&s, ctx->d_sel_state, 1) || !ctx->sync())
        return SGUFP_ERR_HIP;
    if (s.bad || s.oob || s.sol_top > ctx->fr_sol_top) {   // the stack is as it was: nothing is swapped
        ctx->err = "frontier select: inconsistent counts";
        return SGUFP_ERR_STATE;
    }
    if (s.moved) {
        std::swap(ctx->fr, ctx->fr_alt);
        ctx->fr_sol_top = s.sol_top;   // the spans were compacted to sol_len
        ctx->relaxed = false;          // a staged batch that aliased the frontier is gone
        ctx->dd_built = false;
    }
    if (selected) *selected = kk;
    if (threshold) *threshold = key_to_ub(s.prefix);
    return SGUFP_OK;
}

}  // extern "C"

namespace {

// One round of sgufp_bnb_step: the steps of the header comment as methods, in the order they
// run, over the host state of the round.  Every step returns an SGUFP_* code.
struct BnbRound {
    sgufp_ctx &c;
    double &incumbent;           // in: the round's zOpt; out: update_incumbent
    const double z;
    const int b;                 // popped records (batch slots 0 .. b-1)
    const int64_t base;          // their first frontier entry
    const std::chrono::steady_clock::time_point t_round = std::chrono::steady_clock::now();
    BatchOut &o;
    sgufp_bnb_stats S{};

    // per batch slot
    std::vector<int32_t> st;
    std::vector<double> ub, lbv;
    std::vector<uint32_t> nch, need, dn, da, sw;
    std::vector<int32_t> nseen;                  // paths on the slot's seen list
    int64_t sol_start = 0;                       // arena position of the popped slice
    // host copy of the popped slice: read before the relaxation when deferred loops exist (their
    // keys) or the round is traced, else by save_deferred when it has records to save
    FrontierRecords popped;
    std::vector<std::string> keys;               // per slot, when deferred loops exist
    std::vector<int> exact, closed, deferred;    // slots that entered their loop / closed it / were cut short
    std::vector<std::vector<std::vector<int16_t>>> seen_host;   // the deferred records' seen lists
    FrontierRecords kept;                        // the deferred records (save_deferred -> push_deferred)
    double znew = 0.0;

    // refinement loop: k_loop_check's answers for the records still in their loop, and the fresh
    // records of the previous iteration, whose cuts (pool rows prev_first ...) file_rows files
    std::vector<int32_t> flag, chains, ptype;
    std::vector<int> prev;
    int prev_first = 0;
    std::vector<double> pub, pobj;               // their rows' bounds; trace: their sum_s obj_s / S
    std::vector<size_t> prev_trace;              // trace: their items of kind 1
    std::vector<uint16_t> tlen;                  // trace: the argmax paths the loop check saw
    std::vector<int16_t> tpath;

    BnbRound(sgufp_ctx &ctx, double &inc, int n)
        : c{ctx}, incumbent{inc}, z{inc}, b{n}, base{ctx.fr_n - n}, o{ctx.out} {
        S.popped = b;
    }

    // ---- trace (sgufp_bnb_set_trace): kinds 0 popped, 1 subproblems, 2 closed loops, 3 waves ----
    int trace_popped() {
        std::vector<uint64_t> ticks(b);
        std::vector<uint32_t> redo(b);
        if (!c.download(ticks.data(), o.ticks, b) || !c.download(redo.data(), o.redo, b) || !c.sync())
            return SGUFP_ERR_HIP;
        const bool stamped = relax_has_phases();
        for (int k = 0; k < b; k++) {
            c.trace_items[0].push_back({k, st[k], -1, popped.ub[k], {}});
            c.trace_items[3].push_back({k, (int32_t)(redo[k] & 0xFF), (int32_t)sw[k], stamped ? (double)ticks[k] : 0.0, {}});
        }
        return SGUFP_OK;
    }
    bool trace_paths() {   // the argmax paths as the loop check saw them
        tlen.resize((size_t)b);
        tpath.resize((size_t)b * c.sc.Lcap);
        return c.download(tlen.data(), o.path_len, (size_t)b) && c.download(tpath.data(), o.path, tpath.size()) &&
               c.sync();
    }
    std::vector<int16_t> slot_path(int k) const {
        const size_t Lc = (size_t)c.sc.Lcap;
        return std::vector<int16_t>(tpath.begin() + (long)(k * Lc), tpath.begin() + (long)(k * Lc + tlen[k]));
    }
    void trace_closed(int k) {
        c.trace_items[2].push_back({k, 0, -1, 0.0, slot_path(k)});   // value: the bound after the loop
    }
    void trace_subproblems(const std::vector<int> &fresh) {
        prev_trace.clear();
        for (int k : fresh) {
            prev_trace.push_back(c.trace_items[1].size());
            c.trace_items[1].push_back({k, -1, -1, 0.0, slot_path(k)});   // code, row, value: file_rows
        }
    }

    // ---- 1: pop the top b records and relax them in place (k_relax prunes by bound) ----
    int pop_and_relax() {
        for (auto &t : c.trace_items) t.clear();
        if ((!c.deferred_seen.empty() || c.trace) && !c.read_frontier(base, b, popped)) return SGUFP_ERR_HIP;
        if (!c.deferred_seen.empty())
            for (int k = 0; k < b; k++) keys.push_back(popped.key(k));
        c.n = b;
        c.cur = c.frontier_slice(base, b);
        c.restricted_done = false;
        if (!c.relax_current(z)) return SGUFP_ERR_HIP;
        st.resize(b); ub.resize(b); nch.resize(b); need.resize(b); dn.resize(b); da.resize(b); sw.resize(b);
        lbv.assign(b, -__DBL_MAX__);
        if (!c.download(st.data(), o.status, b) || !c.download(ub.data(), o.ub, b) ||
            !c.download(nch.data(), o.nchild, b) || !c.download(need.data(), o.sol_need, b) ||
            !c.download(dn.data(), o.dd_nodes, b) || !c.download(da.data(), o.dd_arcs, b) ||
            !c.download(sw.data(), o.sweeps, b) || !c.download(&sol_start, c.fr.sol_off + base, 1) || !c.sync())
            return SGUFP_ERR_HIP;
        if (c.timing) hipEventElapsedTime(&c.ms_relax, c.ev[0], c.ev[1]);
        S.ms_relax = c.timing ? c.ms_relax : 0.0;
        return SGUFP_OK;
    }

    // ---- 2: the statuses: counters, the records that enter the refinement loop ----
    int classify() {
        for (int k = 0; k < b; k++) {
            switch (st[k]) {
                case SGUFP_PRUNED_BY_BOUND: S.pruned_bound++; continue;
                case SGUFP_PRUNED_BY_FEASIBILITY_CUT: S.pruned_feasibility++; break;
                case SGUFP_PRUNED_BY_OPTIMALITY_CUT: S.pruned_optimality++; break;
                case SGUFP_NEEDS_SUBPROBLEM: exact.push_back(k); break;
                case SGUFP_SUCCESS: break;
                default: {
                    char msg[128];
                    std::snprintf(msg, sizeof msg, "B&B round: frontier record %lld failed with node status %d",
                                  (long long)(base + k), st[k]);
                    c.err = msg;
                    return SGUFP_ERR_STATE;
                }
            }
            S.relaxed++;
            S.children += nch[k];
            S.dd_nodes += dn[k];
            S.dd_arcs += da[k];
            S.sweeps += sw[k];
        }
        S.exact = (int64_t)exact.size();
        if (c.trace && trace_popped() != SGUFP_OK) return SGUFP_ERR_HIP;
        // a popped record that left its deferred loop without re-entering it (pruned by bound
        // or by a cut of the grown pool) drops its seen list
        if (!keys.empty())
            for (int k = 0; k < b; k++)
                if (st[k] != SGUFP_NEEDS_SUBPROBLEM) c.deferred_seen.erase(keys[k]);
        return SGUFP_OK;
    }

    // ---- 3: the refinement loop of the exact DDs, device-resident: per iteration k_loop_check
    // (argmax path seen? -> {ub, ub}; else fresh), one synchronisation, then k_seen_append, the
    // scenario subproblem on the fresh paths read in place, k_append_cuts (Container::add on the
    // device) and k_refine, back to back on the stream.  The host files the appended rows under
    // the F / O lists at the next synchronisation.  The loop of one record is a chain of
    // dependent subproblems (one new cut per iteration); a round stops it after bnb_max_iters
    // iterations or bnb_seconds.  A record deferred so rebuilds its DD when popped again, applies
    // the pool (its own new cuts included, so its bound is where the loop left it) and resumes
    // with its seen list: it ends exactly where the uninterrupted loop would (a path repeats). ----
    int refine() {
        if (exact.empty()) return SGUFP_OK;
        int rc = resume_loops();
        if (rc != SGUFP_OK) return rc;
        std::vector<int> act = exact;   // the records still in their loop, as in d_lact
        if (!c.upload(c.d_lact, act.data(), act.size())) return SGUFP_ERR_HIP;
        while (!act.empty()) {
            const int na = (int)act.size();
            if (!c.hip_ok(launch_loop_check(o, c.seen, c.d_lact, na, c.net.m, c.d_lflag, c.d_lchain, c.stream),
                          "k_loop_check"))
                return SGUFP_ERR_HIP;
            flag.resize(na);
            chains.resize(na);
            if (!c.download(flag.data(), c.d_lflag, (size_t)na) || !c.download(chains.data(), c.d_lchain, (size_t)na))
                return SGUFP_ERR_HIP;
            if ((rc = file_rows()) != SGUFP_OK) return rc;   // the one sync
            if (c.trace && !trace_paths()) return SGUFP_ERR_HIP;
            std::vector<int> fresh;
            int nct = 1;
            for (int a = 0; a < na; a++) {
                const int k = act[a];
                if (flag[a] == 1) {                 // {ub, ub, {}, SUCCESS}
                    closed.push_back(k);
                    S.exact_closed++;
                    if (c.trace) trace_closed(k);
                } else if (flag[a] == 2) {
                    fresh.push_back(k);
                    nct = std::max(nct, chains[a]);
                } else {
                    st[k] = flag[a] - 3;
                    if (st[k] == SGUFP_PRUNED_BY_FEASIBILITY_CUT) S.pruned_feasibility++;
                    else if (st[k] == SGUFP_PRUNED_BY_OPTIMALITY_CUT) S.pruned_optimality++;
                }
            }
            if (fresh.empty()) break;
            if ((c.bnb_max_iters > 0 && S.refine_iters >= c.bnb_max_iters) ||
                (c.bnb_seconds > 0 && S.refine_iters > 0 && seconds_since(t_round) >= c.bnb_seconds)) {
                // (every round runs at least one iteration: a batch whose relaxation alone
                // outlasts round_seconds still makes progress)
                deferred.swap(fresh);    // their current path is unseen: solved when resumed
                break;
            }
            std::vector<int> rest;
            if (c.bnb_seconds > 0) rest = split_chunk(fresh, nct);
            S.refine_iters++;
            const int nf = (int)fresh.size();
            int most = 0;
            for (int k : fresh) most = std::max(most, ++nseen[k]);
            if (!c.sub_init()) return c.sub_rc;
            if (!c.loop_reserve(b, most) || !c.upload(c.d_lact, fresh.data(), (size_t)nf) ||
                !c.hip_ok(launch_seen_append(o, c.seen, c.d_lact, nf, c.net.m, c.stream), "k_seen_append") ||
                !c.sub_grow(nf, 1) || !c.grow_rows(c.n_rows + nf))
                return SGUFP_ERR_HIP;
            SubIO io;
            if (!sub_io(nf, nct, io) || !c.hip_ok(launch_subproblem(c.sn, io, c.stream), "subproblem launch"))
                return SGUFP_ERR_HIP;
            c.sub_last_n = nf;
            if (c.sub_stats) c.sub_stats_add(nf);
            const int first = c.n_rows;
            if (!c.hip_ok(launch_append_cuts(io.cut_type, io.cut_rhs, io.cut_row, nf, c.net.n_slots + 1, first, c.d_rows,
                                             c.d_rhs, c.d_coefT, c.nd.slot_tab, c.net.L, c.ustride, c.d_lrowub, c.d_rcuts,
                                             c.d_rfeas, c.stream), "k_append_cuts") ||
                !c.hip_ok(launch_refine(c.nd, c.sc, c.batch(), c.pool(), o, c.d_lact, c.d_rcuts, c.d_rfeas, nf, z, c.ex,
                                        c.stream), "k_refine"))
                return SGUFP_ERR_HIP;
            c.n_rows += nf;
            S.subproblems += nf;
            prev = fresh;
            prev_first = first;
            if (c.trace) trace_subproblems(fresh);
            act = fresh;
            act.insert(act.end(), rest.begin(), rest.end());
            if (!c.upload(c.d_lact + nf, rest.data(), rest.size())) return SGUFP_ERR_HIP;
        }
        if (!prev.empty() && (rc = file_rows()) != SGUFP_OK) return rc;
        // bounds after the loop: closed records' lb (the incumbent candidates) and the
        // deferred records' bound
        if (!c.download(ub.data(), o.ub, b) || !c.sync()) return SGUFP_ERR_HIP;
        for (int k : closed) lbv[k] = ub[k];
        for (auto &t : c.trace_items[2]) t.value = ub[t.record];
        for (int k : deferred) {
            seen_host.emplace_back();
            if (!c.seen_download(k, nseen[k], seen_host.back())) return SGUFP_ERR_HIP;
        }
        return SGUFP_OK;
    }

    // empty seen lists for the batch slots; a record whose loop an earlier round deferred gets
    // its list back
    int resume_loops() {
        if (!c.loop_reserve(b, 64)) return SGUFP_ERR_HIP;
        nseen.assign(b, 0);
        if (!c.hip_ok(hipMemsetAsync(c.seen.n, 0, (size_t)b * 4, c.stream), "memset")) return SGUFP_ERR_HIP;
        if (keys.empty()) return SGUFP_OK;
        for (int k : exact) {
            auto it = c.deferred_seen.find(keys[k]);
            if (it == c.deferred_seen.end()) continue;
            const int cnt = (int)it->second.size();
            if (!c.loop_reserve(b, cnt + 1) || !c.seen_upload(k, it->second)) return SGUFP_ERR_HIP;
            nseen[k] = cnt;
            c.deferred_seen.erase(it);
            S.resumed++;
        }
        return SGUFP_OK;
    }

    // Container::add for the cuts of the previous iteration's subproblems: their types and row
    // bounds come down behind whatever the caller queued, one synchronisation, then the rows go
    // under the feasibility list and the optimality list
    int file_rows() {
        const size_t np = prev.size();
        ptype.resize(np);
        pub.resize(np);
        pobj.resize(np);
        if (!c.download(ptype.data(), c.sio.cut_type, np) || !c.download(pub.data(), c.d_lrowub, np) ||
            (c.trace && !c.download(pobj.data(), c.sio.obj_mean, np)) || !c.sync())
            return SGUFP_ERR_HIP;
        for (size_t i = 0; i < np; i++) {
            if (ptype[i] < 0) {
                // the rows of that launch leave the pool again (they were appended and
                // applied on the device before the host saw the type); the batch's results
                // are not used past the error
                c.n_rows = prev_first;
                c.err = "scenario subproblem failed (invalid path or numerical failure)";
                return SGUFP_ERR_STATE;
            }
        }
        c.row_ub.resize((size_t)c.n_rows);
        for (int want = 1; want >= 0; want--)
            for (size_t i = 0; i < np; i++) {
                if (ptype[i] != want) continue;
                auto &list = want ? c.f_rows : c.o_rows;
                if (c.trace) {
                    auto &t = c.trace_items[1][prev_trace[i]];
                    t.code = want;
                    t.row = (int32_t)list.size();
                    t.value = pobj[i];
                }
                list.push_back(prev_first + (int)i);
                c.row_ub[(size_t)prev_first + i] = pub[i];
                (want ? S.new_feasibility_cuts : S.new_optimality_cuts)++;
            }
        c.order_dirty = true;
        prev.clear();
        return SGUFP_OK;
    }

    // With a round deadline, one iteration solves at most chunk_lps scenario LPs (a 1024-leaf
    // iteration of the 512-scenario C5 network would take minutes): the fresh records past the
    // chunk are returned -- they stay in the loop unchanged (path not yet seen) for the next
    // iteration, or are deferred at the deadline -- and nct is recomputed over the kept ones
    // (fresh holds the flag-2 records in loop order)
    std::vector<int> split_chunk(std::vector<int> &fresh, int &nct) const {
        const size_t chunk = (size_t)std::max<int64_t>(1, c.chunk_lps / std::max(1, c.net.S));
        if (fresh.size() <= chunk) return {};
        const std::vector<int> rest(fresh.begin() + (long)chunk, fresh.end());
        fresh.resize(chunk);
        nct = 1;
        size_t kept_n = 0;
        for (size_t a = 0; a < flag.size() && kept_n < chunk; a++)
            if (flag[a] == 2) {
                nct = std::max(nct, chains[a]);
                kept_n++;
            }
        return rest;
    }

    // the subproblem launch on the nf fresh paths, read in place from the batch's outputs
    bool sub_io(int nf, int nct, SubIO &io) {
        io = c.sio;
        io.n_paths = nf;
        io.nct_cap = nct;
        io.path_slot = c.d_lact;
        io.path_len = o.path_len;
        io.path_stride = c.sc.Lcap;
        io.paths = o.path;
        io.path_off = nullptr;
        // warm starts: every path starts from the stored state of the closest path solved
        // before (the record's own previous path, a sibling's, ...) and leaves its own state
        // in the ring for the next ones (k_warm_pick, k_sub_scenario<..., WARM>)
        if (!c.warm_reserve()) return true;
        if (!c.hip_ok(launch_warm_pick(io, c.wring, c.warm_ptr, c.stream), "k_warm_pick")) return false;
        io.warm_src = c.wring.src;
        io.warm_dst = c.wring.dst;
        io.wst_x = c.d_wx;
        io.wst_a = c.d_wa;
        io.wst_ok = c.d_wok;
        c.warm_ptr = (c.warm_ptr + nf) % c.wring.R;
        return true;
    }

    // ---- 4: the deferred records, saved before the children overwrite the popped slice, and
    // their seen lists under the records' keys ----
    int save_deferred() {
        S.deferred = (int64_t)deferred.size();
        if (deferred.empty()) return SGUFP_OK;
        if (popped.gl.empty() && !c.read_frontier(base, b, popped)) return SGUFP_ERR_HIP;
        for (size_t i = 0; i < deferred.size(); i++) {
            kept.append(popped, deferred[i]);
            kept.ub.back() = ub[deferred[i]];   // the bound the loop reached (every pool cut is valid)
            c.deferred_seen[kept.key((int)i)] = std::move(seen_host[i]);
        }
        return SGUFP_OK;
    }

    // ---- 5: incumbent (DDSolver.cpp:723-731) ----
    int update_incumbent() {
        znew = z;
        int best = -1;   // the first slot in batch order that reaches the maximum (strict >)
        for (int k = 0; k < b; k++)
            if (lbv[k] > znew) {
                znew = lbv[k];
                best = k;
            }
        S.improved = znew > z ? 1 : 0;
        incumbent = znew;
        if (best < 0) return SGUFP_OK;
        // the stored solution: that leaf's argmax path, copied on the device before the
        // children overwrite anything (only an improving round pays the length's round trip)
        uint16_t len = 0;
        if (!c.download(&len, o.path_len + best, 1) || !c.sync() ||
            !c.inc_store(znew, o.path + (size_t)best * c.sc.Lcap, (int32_t)len, hipMemcpyDeviceToDevice))
            return SGUFP_ERR_HIP;
        return SGUFP_OK;
    }

    // ---- 6: push the children of parents with ub > zOpt (DDSolver.cpp:744-748) ----
    int push_children() {
        std::vector<int32_t> par;
        std::vector<int64_t> dchild, dsol;
        int64_t nc = 0, ns = 0;
        for (int k = 0; k < b; k++) {
            if (st[k] != SGUFP_SUCCESS || nch[k] == 0 || !(ub[k] > znew)) continue;
            par.push_back(k);
            dchild.push_back(base + nc);
            dsol.push_back(sol_start + ns);
            nc += nch[k];
            ns += need[k];
        }
        c.relaxed = false;   // the popped slice is overwritten below
        c.dd_built = false;
        if (!c.frontier_reserve(base + nc, (size_t)(sol_start + ns))) return SGUFP_ERR_HIP;
        const int np = (int)par.size();
        if (np > c.max_batch) return SGUFP_ERR_STATE;
        if (np && (!c.upload(c.d_bidx, par.data(), np) || !c.upload(c.d_boff, dchild.data(), np) ||
                   !c.upload(c.d_bsol, dsol.data(), np) ||
                   !c.hip_ok(launch_push_children(c.children_view(), o, c.d_bidx, c.d_boff, c.d_bsol, np, c.fr, c.stream),
                             "k_push_children") ||
                   !c.sync()))
            return SGUFP_ERR_HIP;
        c.fr_n = base + nc;
        c.fr_sol_top = c.fr_n ? sol_start + ns : 0;
        S.pushed = nc;
        return SGUFP_OK;
    }

    // ---- 7: the deferred records on top, in their frontier order: popped first next round ----
    int push_deferred() {
        if (!kept.gl.empty()) {
            if (!c.write_frontier(c.fr_n, c.fr_sol_top, kept)) return SGUFP_ERR_HIP;
            c.fr_n += (int64_t)kept.gl.size();
            c.fr_sol_top += (int64_t)kept.sol.size();
        }
        S.frontier = c.fr_n;
        return SGUFP_OK;
    }
};

}  // namespace

extern "C" int sgufp_bnb_step(sgufp_ctx *ctx, int max_nodes, double *incumbent, sgufp_bnb_stats *stats) {
    if (!ctx || !incumbent) return SGUFP_ERR_ARG;
    if (ctx->fr_n == 0) {
        if (stats) *stats = sgufp_bnb_stats{};
        return SGUFP_OK;
    }
    int b = ctx->max_batch;
    if (max_nodes > 0) b = std::min(b, max_nodes);
    BnbRound r(*ctx, *incumbent, (int)std::min<int64_t>(b, ctx->fr_n));
    int rc;
    if ((rc = r.pop_and_relax()) != SGUFP_OK || (rc = r.classify()) != SGUFP_OK || (rc = r.refine()) != SGUFP_OK ||
        (rc = r.save_deferred()) != SGUFP_OK || (rc = r.update_incumbent()) != SGUFP_OK ||
        (rc = r.push_children()) != SGUFP_OK || (rc = r.push_deferred()) != SGUFP_OK)
        return rc;
    if (stats) *stats = r.S;
    return SGUFP_OK;
}
