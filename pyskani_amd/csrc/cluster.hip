// The cluster stage (psk_cluster_records): representatives and clusters from the psk_hit_min records of an all-vs-all (Database.triangle_records, or a full run).
//
// A record (q = query & 0x7FFFFFFF, r = ref_index) QUALIFIES iff q != r, ani >= (float)min_ani and the aligned-fraction rule holds, every comparison in float (a NaN
// fails each). The unordered pair {q, r} is an EDGE iff one of its records qualifies; its weight is the largest ani among them. Genome a PRECEDES b iff
// priority[a] > priority[b], or the priorities are equal and a < b (no priorities: a < b).
//   greedy: the lexicographically-first maximal independent set of the edge graph under that order are the representatives; every other genome is a member of the
//           adjacent representative of largest weight (ties: the earlier one in the order) - ANY adjacent representative, also one that comes after the member.
//   single: connected components; a component's representative is its first genome in the order.
// Nothing here depends on the order atomics arrive in: the edge list is a sort, the row starts are binary searches, a greedy decision is taken from FINAL states of
// better-ranked neighbours only (a vertex leaves `undecided` once and never changes again: a stale read delays a decision, it cannot change one), hooking ends with a
// partition that is the components' whatever the labels are, and a component's representative is a minimum.
//
// Stages, all on the lane's stream with scratch from the context's block pool (as locality.hip takes its own):
//   clu_edges    a lane per record: two directed entries (key = u << 32 | v, value = the ani's bits - ani is positive, unsigned order is float order), or two copies
//                of the sentinel key n << 32 that the sort parks behind every edge; an index >= n raises the error word (vector atomicOr)
//   radix sort   of the entries over the 32 + bit_width(n) key bits in use
//   clu_heads / exclusive sum / clu_scatter   the first entry of every run of equal keys is the directed edge: adj[] = v, w[] = the run's maximum
//   clu_rows     row_start[v] = edges before the lower bound of v << 32 in the sorted keys
//   rank         stable radix sort of ~priority with the index as value: vertex_of_rank[], rank[] (the identity without priorities)
//   clu_round    a wave per vertex, four launches to a synchronisation, each with a flag of its own; clu_assign: a wave per member, arg-max by wave reduction
//   clu_hook / clu_jump / clu_best / clu_single_out   single linkage
// The linkage forest (psk_cluster_forest) starts from the same rows; its rule and stages stand above forest_keys_kernel below.
#include "common.h"
#include <hipcub/hipcub.hpp>

namespace {

constexpr uint32_t CLU_UNDECIDED = 0u, CLU_REP = 1u, CLU_MEMBER = 2u;
constexpr int CLU_SWEEPS = 4;      // times a wave looks at its vertex in one launch of clu_round_kernel: states decided by other waves of the launch are seen through agent-scope loads
inline size_t clu_al256(size_t x) { return (x + 255) & ~(size_t)255; }

__global__ __launch_bounds__(256) void clu_edges_kernel(const psk_hit_min* __restrict__ recs, uint32_t n_recs, uint32_t n, float min_ani, float min_af, int use_af, int either,
                                                        unsigned long long* __restrict__ key, uint32_t* __restrict__ val, uint32_t* err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_recs) return;
    const psk_hit_min h = recs[i];
    const uint32_t q = h.query & 0x7FFFFFFFu, r = h.ref_index;      // (bit 31 of `query`: the regression model produced the ani)
    const unsigned long long none = (unsigned long long)n << 32;
    unsigned long long a = none, b = none;
    if (q >= n || r >= n) atomicOr(err, 1u);
    else {
        const bool af_ok = !use_af || (either ? (h.af_query >= min_af || h.af_ref >= min_af) : (h.af_query >= min_af && h.af_ref >= min_af));      // (= max / min of the two >= min_af; a NaN fails its comparison)
        if (q != r && h.ani >= min_ani && af_ok) { a = ((unsigned long long)q << 32) | r; b = ((unsigned long long)r << 32) | q; }
    }
    const size_t o = 2 * (size_t)i;
    key[o] = a; key[o + 1] = b;
    val[o] = val[o + 1] = __float_as_uint(h.ani);
}
// flag[i] = 1 where a run of equal edge keys begins (N + 1 entries, the last one 0: its exclusive sum is the number of directed edges)
__global__ __launch_bounds__(256) void clu_heads_kernel(const unsigned long long* __restrict__ key, uint32_t N, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > N) return;
    uint32_t f = 0u;
    if (i < N) { const unsigned long long k = key[i]; f = ((uint32_t)(k >> 32) < n && (i == 0 || key[i - 1] != k)) ? 1u : 0u; }
    flag[i] = f;
}
// the head of a run writes the directed edge: its target and the largest weight of the run (a run is the records of one pair in one direction: one or two entries, more only for repeated records)
__global__ __launch_bounds__(256) void clu_scatter_kernel(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ val, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ pos, uint32_t N, uint32_t* __restrict__ adj, uint32_t* __restrict__ w) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const unsigned long long k = key[i];
    uint32_t m = val[i];
    for (uint32_t j = i + 1; j < N && key[j] == k; j++) m = max(m, val[j]);
    const uint32_t p = pos[i];      // (< N: an exclusive sum of N flags)
    adj[p] = (uint32_t)k; w[p] = m;
}
__global__ __launch_bounds__(256) void clu_rows_kernel(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ pos, uint32_t N, uint32_t n, uint32_t* __restrict__ row) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v > n) return;
    const unsigned long long want = (unsigned long long)v << 32;
    uint32_t lo = 0, hi = N;      // first entry with key >= want, in [0, N]
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (key[mid] < want) lo = mid + 1; else hi = mid; }
    row[v] = pos[lo];
}
__global__ __launch_bounds__(256) void clu_prio_kernel(const unsigned long long* __restrict__ prio, uint32_t n, unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) { key[v] = ~prio[v]; val[v] = v; }
}
__global__ __launch_bounds__(256) void clu_rank_kernel(const uint32_t* __restrict__ vertex_of_rank, uint32_t n, uint32_t* __restrict__ rank) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) rank[vertex_of_rank[i]] = i;      // (a permutation of [0, n): the sort's values are the indices)
}
__global__ __launch_bounds__(256) void clu_iota_kernel(uint32_t n, uint32_t* __restrict__ a, uint32_t* __restrict__ b) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) { a[v] = v; if (b) b[v] = v; }
}

// One greedy round: a wave per vertex strides its row. A neighbour of better rank that is a representative makes the vertex a member; all of them members (or none
// there) makes it a representative; else it waits. Only final states decide, so the states other waves write during the launch may be read as they come.
__global__ __launch_bounds__(256) void clu_round_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ adj, const uint32_t* __restrict__ rank, uint32_t n,
                                                        uint32_t* state, uint32_t* changed) {
    const uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (v >= n) return;      // (wave-uniform)
    if (state[v] != CLU_UNDECIDED) return;
    const uint32_t b = row[v], e = row[v + 1], rv = rank[v];
    for (int sweep = 0; sweep < CLU_SWEEPS; sweep++) {
        bool rep = false, und = false;
        for (uint32_t k = b + lane; k < e; k += 64u) {
            const uint32_t u = adj[k];
            if (rank[u] < rv) {
                const uint32_t s = __hip_atomic_load(&state[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                rep |= s == CLU_REP; und |= s == CLU_UNDECIDED;
            }
        }
        const bool any_rep = __ballot(rep) != 0ull, any_und = __ballot(und) != 0ull;
        if (any_rep || !any_und) {
            if (lane == 0) { __hip_atomic_store(&state[v], any_rep ? CLU_MEMBER : CLU_REP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); *changed = 1u; }
            return;
        }
    }
}
// a wave per member: the adjacent representative of largest (weight, then better rank)
__global__ __launch_bounds__(256) void clu_assign_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ adj, const uint32_t* __restrict__ w, const uint32_t* __restrict__ rank,
                                                         const uint32_t* __restrict__ vertex_of_rank, const uint32_t* __restrict__ state, uint32_t n,
                                                         uint32_t* __restrict__ rep_of, float* __restrict__ rep_ani) {
    const uint32_t v = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (v >= n) return;
    if (state[v] != CLU_MEMBER) { if (lane == 0) { rep_of[v] = v; rep_ani[v] = 1.0f; } return; }
    unsigned long long best = 0ull;      // weight << 32 | ~rank: a weight is a positive float's bits, never 0
    for (uint32_t k = row[v] + lane, e = row[v + 1]; k < e; k += 64u) {
        const uint32_t u = adj[k];
        if (state[u] == CLU_REP) { const unsigned long long c = ((unsigned long long)w[k] << 32) | (0xFFFFFFFFu - rank[u]); best = c > best ? c : best; }
    }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(best, d, 64); best = o > best ? o : best; }
    if (lane == 0) {      // (a member has a representative neighbour: best != 0; were it 0, the index below would leave the table)
        rep_of[v] = best ? vertex_of_rank[0xFFFFFFFFu - (uint32_t)best] : v; rep_ani[v] = best ? __uint_as_float((uint32_t)(best >> 32)) : 1.0f;
    }
}

// single linkage: a lane per sorted entry, the head of a run with u < v hooks (each undirected edge once). label[x] is always a vertex of x's component and only decreases.
__global__ __launch_bounds__(256) void clu_hook_kernel(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ flag, uint32_t N, uint32_t* label, uint32_t* changed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const unsigned long long k = key[i];
    const uint32_t a = (uint32_t)(k >> 32), b = (uint32_t)k;
    if (a >= b) return;
    const uint32_t la = label[a], lb = label[b];
    if (la == lb) return;
    const uint32_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
    atomicMin(&label[hi], lo);
    atomicMin(&label[la < lb ? b : a], lo);
    *changed = 1u;
}
__global__ __launch_bounds__(256) void clu_jump_kernel(uint32_t* label, uint32_t n) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const uint32_t l = label[v];
    const uint32_t ll = label[l];
    if (ll < l) atomicMin(&label[v], ll);
}
__global__ __launch_bounds__(256) void clu_best_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ rank, uint32_t n, uint32_t* best) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) atomicMin(&best[label[v]], rank[v]);
}
__global__ __launch_bounds__(256) void clu_single_out_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ best, const uint32_t* __restrict__ vertex_of_rank,
                                                             const uint32_t* __restrict__ row, const uint32_t* __restrict__ adj, const uint32_t* __restrict__ w, uint32_t n,
                                                             uint32_t* __restrict__ rep_of, float* __restrict__ rep_ani) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n) return;
    const uint32_t rep = vertex_of_rank[best[label[v]]];
    rep_of[v] = rep;
    float a = 1.0f;
    if (rep != v) {      // the direct edge to the representative, if there is one: a row's targets ascend
        uint32_t lo = row[v], hi = row[v + 1];
        const uint32_t end = hi;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (adj[mid] < rep) lo = mid + 1; else hi = mid; }
        a = (lo < end && adj[lo] == rep) ? __uint_as_float(w[lo]) : 0.0f;
    }
    rep_ani[v] = a;
}

inline dim3 clu_grid(uint64_t items) { return dim3((unsigned)((items + 255u) / 256u)); }

psk_status cluster_impl(Lane* ctx, const psk_hit_min* recs, uint32_t n_recs, uint32_t n, const uint64_t* priority, float min_ani, float min_af, int use_af, int either, int linkage,
                        uint32_t* rep_of, float* rep_ani) {
    hipStream_t st = ctx->stream;
    const uint32_t N = 2u * n_recs;      // (n_recs < 2^30)
    int n_bits = 0; while (n_bits < 32 && (n >> n_bits)) n_bits++;      // bit width of n: the sentinel's high word
    size_t ts1 = 0, ts2 = 0, ts3 = 0;
    PSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, ts1, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)N, 0, 32 + n_bits, st));
    PSK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, ts2, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(N + 1u), st));
    if (priority) PSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, ts3, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 64, st));
    const size_t ts = std::max(ts1, std::max(ts2, ts3));
    PoolScratch tmp;      // back to the pool on every exit
    const size_t N8 = 8 * (size_t)N, N4 = 4 * (size_t)N + 4, n4 = 4 * (size_t)n + 4, n8 = priority ? 8 * (size_t)n : 0;
    const size_t o_flag = 0, o_recs = clu_al256(o_flag + 64), o_k0 = clu_al256(o_recs + sizeof(psk_hit_min) * (size_t)n_recs), o_k1 = clu_al256(o_k0 + N8), o_v0 = clu_al256(o_k1 + N8),
                 o_v1 = clu_al256(o_v0 + N4), o_hd = clu_al256(o_v1 + N4), o_pos = clu_al256(o_hd + N4), o_adj = clu_al256(o_pos + N4), o_w = clu_al256(o_adj + N4),
                 o_row = clu_al256(o_w + N4), o_rank = clu_al256(o_row + n4), o_vor = clu_al256(o_rank + n4), o_state = clu_al256(o_vor + n4), o_best = clu_al256(o_state + n4),
                 o_rep = clu_al256(o_best + n4), o_ani = clu_al256(o_rep + n4), o_p0 = clu_al256(o_ani + n4), o_p1 = clu_al256(o_p0 + n8), o_pv = clu_al256(o_p1 + n8),
                 o_t = clu_al256(o_pv + n4), o_end = o_t + ts;
    PSK_TRY(tmp.reserve(ctx->dev, o_end + 256));
    char* T = (char*)tmp.p;
    uint32_t* d_flag = (uint32_t*)(T + o_flag);      // [0..3]: a round's / hook pass's "changed"; [4]: an index was out of range
    psk_hit_min* d_recs = (psk_hit_min*)(T + o_recs);
    unsigned long long *k0 = (unsigned long long*)(T + o_k0), *k1 = (unsigned long long*)(T + o_k1), *p0 = (unsigned long long*)(T + o_p0), *p1 = (unsigned long long*)(T + o_p1);
    uint32_t *v0 = (uint32_t*)(T + o_v0), *v1 = (uint32_t*)(T + o_v1), *head = (uint32_t*)(T + o_hd), *pos = (uint32_t*)(T + o_pos), *adj = (uint32_t*)(T + o_adj), *w = (uint32_t*)(T + o_w),
             *row = (uint32_t*)(T + o_row), *rank = (uint32_t*)(T + o_rank), *vor = (uint32_t*)(T + o_vor), *state = (uint32_t*)(T + o_state), *best = (uint32_t*)(T + o_best),
             *d_rep = (uint32_t*)(T + o_rep), *pv = (uint32_t*)(T + o_pv);
    float* d_ani = (float*)(T + o_ani);
    void* hp;
    PSK_TRY(ctx->pinned(64, &hp));
    uint32_t* h_flag = (uint32_t*)hp;      // [0..4] as d_flag, [8]: directed edges

    // edges -> rows
    PSK_HIP(hipMemsetAsync(d_flag, 0, 32, st));
    PSK_HIP(hipMemcpyAsync(d_recs, recs, sizeof(psk_hit_min) * (size_t)n_recs, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(clu_edges_kernel, clu_grid(n_recs), dim3(256), 0, st, (const psk_hit_min*)d_recs, n_recs, n, min_ani, min_af, use_af, either, k0, v0, d_flag + 4);
    size_t t1 = ts;
    PSK_HIP(hipcub::DeviceRadixSort::SortPairs(T + o_t, t1, (const unsigned long long*)k0, k1, (const uint32_t*)v0, v1, (int)N, 0, 32 + n_bits, st));
    hipLaunchKernelGGL(clu_heads_kernel, clu_grid((uint64_t)N + 1), dim3(256), 0, st, (const unsigned long long*)k1, N, n, head);
    size_t t2 = ts;
    PSK_HIP(hipcub::DeviceScan::ExclusiveSum(T + o_t, t2, (const uint32_t*)head, pos, (int)(N + 1u), st));
    hipLaunchKernelGGL(clu_scatter_kernel, clu_grid(N), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)v1, (const uint32_t*)head, (const uint32_t*)pos, N, adj, w);
    hipLaunchKernelGGL(clu_rows_kernel, clu_grid((uint64_t)n + 1), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)pos, N, n, row);
    PSK_HIP(hipMemcpyAsync(h_flag + 8, row + n, 4, hipMemcpyDeviceToHost, st));
    // rank
    if (priority) {
        PSK_HIP(hipMemcpyAsync(p1, priority, 8 * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(clu_prio_kernel, clu_grid(n), dim3(256), 0, st, (const unsigned long long*)p1, n, p0, pv);
        size_t t3 = ts;
        PSK_HIP(hipcub::DeviceRadixSort::SortPairs(T + o_t, t3, (const unsigned long long*)p0, p1, (const uint32_t*)pv, vor, (int)n, 0, 64, st));      // (stable: equal priorities keep ascending indices)
        hipLaunchKernelGGL(clu_rank_kernel, clu_grid(n), dim3(256), 0, st, (const uint32_t*)vor, n, rank);
    } else {
        hipLaunchKernelGGL(clu_iota_kernel, clu_grid(n), dim3(256), 0, st, n, rank, vor);
    }
    const char* range_msg = "cluster_records: a record's query or ref_index is n_genomes (%u) or more";
    const uint64_t max_batches = (uint64_t)n / 4 + 2;
    uint64_t passes = 0;
    bool done = false;
    if (linkage == 0) {
        // rounds, four to a synchronisation: every round decides at least the best-ranked undecided vertex, so one that changed nothing found none left
        PSK_HIP(hipMemsetAsync(state, 0, 4 * (size_t)n, st));
        const dim3 gw = clu_grid(64 * (uint64_t)n);
        for (uint64_t batch = 0; batch < max_batches && !done; batch++) {
            PSK_HIP(hipMemsetAsync(d_flag, 0, 16, st));
            for (int k = 0; k < 4; k++)
                hipLaunchKernelGGL(clu_round_kernel, gw, dim3(256), 0, st, (const uint32_t*)row, (const uint32_t*)adj, (const uint32_t*)rank, n, state, d_flag + k);
            PSK_HIP(hipMemcpyAsync(h_flag, d_flag, 32, hipMemcpyDeviceToHost, st));
            PSK_HIP(hipStreamSynchronize(st));
            if (h_flag[4]) { psk_set_error(range_msg, n); return PSK_EINVAL; }
            for (int k = 0; k < 4; k++) { if (h_flag[k]) passes++; else done = true; }
        }
        if (!done) { psk_set_error("cluster_records: the greedy rounds did not end after %llu launches", (unsigned long long)(4 * max_batches)); return PSK_EHIP; }
        hipLaunchKernelGGL(clu_assign_kernel, gw, dim3(256), 0, st, (const uint32_t*)row, (const uint32_t*)adj, (const uint32_t*)w, (const uint32_t*)rank, (const uint32_t*)vor,
                           (const uint32_t*)state, n, d_rep, d_ani);
        ctx->dev->cl_rounds = passes; ctx->dev->cl_hooks = 0;
    } else {
        uint32_t* label = state;
        hipLaunchKernelGGL(clu_iota_kernel, clu_grid(n), dim3(256), 0, st, n, label, (uint32_t*)nullptr);
        PSK_HIP(hipMemsetAsync(best, 0xFF, 4 * (size_t)n, st));
        // passes of (hook, jump, jump) until a hook pass joins nothing: every edge then has one label at both ends
        for (uint64_t batch = 0; batch < (uint64_t)n + 64 && !done; batch++) {
            PSK_HIP(hipMemsetAsync(d_flag, 0, 16, st));
            for (int k = 0; k < 4; k++) {
                hipLaunchKernelGGL(clu_hook_kernel, clu_grid(N), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)head, N, label, d_flag + k);
                hipLaunchKernelGGL(clu_jump_kernel, clu_grid(n), dim3(256), 0, st, label, n);
                hipLaunchKernelGGL(clu_jump_kernel, clu_grid(n), dim3(256), 0, st, label, n);
            }
            PSK_HIP(hipMemcpyAsync(h_flag, d_flag, 32, hipMemcpyDeviceToHost, st));
            PSK_HIP(hipStreamSynchronize(st));
            if (h_flag[4]) { psk_set_error(range_msg, n); return PSK_EINVAL; }
            for (int k = 0; k < 4; k++) { if (h_flag[k]) passes++; else done = true; }
        }
        if (!done) { psk_set_error("cluster_records: hooking did not converge"); return PSK_EHIP; }
        hipLaunchKernelGGL(clu_best_kernel, clu_grid(n), dim3(256), 0, st, (const uint32_t*)label, (const uint32_t*)rank, n, best);
        hipLaunchKernelGGL(clu_single_out_kernel, clu_grid(n), dim3(256), 0, st, (const uint32_t*)label, (const uint32_t*)best, (const uint32_t*)vor, (const uint32_t*)row,
                           (const uint32_t*)adj, (const uint32_t*)w, n, d_rep, d_ani);
        ctx->dev->cl_rounds = 0; ctx->dev->cl_hooks = passes;
    }
    ctx->dev->cl_edges = h_flag[8] / 2;
    PSK_HIP(hipMemcpyAsync(rep_of, d_rep, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (rep_ani) PSK_HIP(hipMemcpyAsync(rep_ani, d_ani, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    PSK_HIP(hipStreamSynchronize(st));
    return PSK_OK;
}

// ---- the linkage forest (psk_cluster_forest): the maximum spanning forest of the same edge graph, pinned uniquely. The semantics are the header's; in short: write an
// edge as (a, b, w) with a < b; e PRECEDES f iff w_e > w_f, or the weights are bit-equal and (a_e, b_e) < (a_f, b_f); the forest is what Kruskal keeps walking the edges
// in that order, and it comes out in that order. The order is strict and total (edges are deduplicated), so the forest is unique and Boruvka finds the same set.
//
// The front half is cluster_impl's, kept here as a SECOND COPY of its launch sequence (the same kernels, the same arguments): cluster_impl itself is untouched.
//   forest_keys  the head of every run writes its key to ekey[pos]: the deduplicated directed edges, ascending in (u, v) - position p of ekey[] is position p of adj[] / w[]
//   forest_mate  a lane per directed edge: (u, v) with u < v has id = its own position; (u, v) with u > v finds the position of (v, u) by binary search in v's row. Both
//                directions carry one eid, and ascending eid is ascending (a, b)
//   a pick is one integer: w_bits << 32 | (0xFFFFFFFF - eid); the largest is the first edge in the order (ani > 0: bit order is float order); 0 means none
//   rounds (Boruvka), label[] = the root of every vertex's component, the identity at first:
//     forest_pick  a wave per vertex strides its row over the neighbours of another label, reduces the maximum by shuffles, one lane does a 64-bit atomicMax on
//                  best[label[u]] (a maximum does not depend on the order of arrival)
//     forest_hook  a lane per vertex. A root r with best[r] != 0 decodes the edge, flags it (a plain store of 1, whoever picked it stores the same) and takes
//                  s = the label of the end outside its component as its parent - unless s picked the same edge and r < s: then r stays the root. Every other vertex's
//                  parent is its label. Reads label[] and best[], writes parent[] and the flags only.
//                  Picks form no cycle longer than 2: let C_1 -> C_2 -> ... -> C_k -> C_1 be components each hooking to the next by its pick e_i. e_i also leaves
//                  C_(i+1), whose pick e_(i+1) is its FIRST outgoing edge in the order: e_(i+1) precedes e_i or is e_i. Around the cycle every pick precedes or equals
//                  the one before it and the chain returns to e_1, so under a strict order all are one edge - which joins two components only: k <= 2, the mutual pick.
//     forest_jump  out[v] = in[in[v]], from one array into the other (a launch reads nothing it writes), bit_width(n) + 2 launches behind the hook, each with a flag of
//                  its own and each returning at once unless the launch before it changed something. A hooking chain is at most n - 1 deep, so ceil(log2(n)) launches
//                  flatten it and the next one changes nothing; after that one both arrays are equal and the rest leave them alone.
//   one synchronisation per round; the first round that hooks nothing ends the loop, bounded by bit_width(n) + 2 rounds (every hooking round at least halves the
//   components that still have an outgoing edge).
//   output: exclusive sum of the flags, keys ~w_bits << 32 | eid of the flagged edges, a radix sort of those (ascending = the edge order), a gather of (a, b, w).
// What one step needs from another always crosses a launch boundary: no kernel here reads what another wave of its own launch stored.
__global__ __launch_bounds__(256) void forest_keys_kernel(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos, uint32_t N,
                                                          unsigned long long* __restrict__ ekey) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N || !flag[i]) return;
    ekey[pos[i]] = key[i];      // (pos[i] < N: an exclusive sum of N flags)
}
__global__ __launch_bounds__(256) void forest_mate_kernel(const unsigned long long* __restrict__ ekey, const uint32_t* __restrict__ row, uint32_t E, uint32_t n,
                                                          uint32_t* __restrict__ eid, uint32_t* err) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= E) return;
    const unsigned long long k = ekey[p];
    const uint32_t u = (uint32_t)(k >> 32), v = (uint32_t)k;
    uint32_t id = p;
    if (u > v) {      // the position of (v, u) in v's row (v < n: clu_edges_kernel let no other index through)
        const unsigned long long want = ((unsigned long long)v << 32) | u;
        uint32_t lo = row[v], hi = row[v + 1];
        const uint32_t end = hi;
        while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (ekey[mid] < want) lo = mid + 1; else hi = mid; }
        if (lo < end && ekey[lo] == want) id = lo;
        else atomicOr(err, 1u);      // (every record wrote both directions: the mate is there)
    }
    eid[p] = id;
}
__global__ __launch_bounds__(256) void forest_pick_kernel(const uint32_t* __restrict__ row, const uint32_t* __restrict__ adj, const uint32_t* __restrict__ w, const uint32_t* __restrict__ eid,
                                                          const uint32_t* __restrict__ label, uint32_t n, unsigned long long* best) {
    const uint32_t u = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (u >= n) return;      // (wave-uniform)
    const uint32_t lu = label[u];
    unsigned long long m = 0ull;
    for (uint32_t k = row[u] + lane, e = row[u + 1]; k < e; k += 64u) {
        if (label[adj[k]] != lu) { const unsigned long long c = ((unsigned long long)w[k] << 32) | (0xFFFFFFFFu - eid[k]); m = c > m ? c : m; }
    }
    for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(m, d, 64); m = o > m ? o : m; }
    if (lane == 0 && m) atomicMax(&best[lu], m);      // (lu < n: a label is a vertex)
}
__global__ __launch_bounds__(256) void forest_hook_kernel(const unsigned long long* __restrict__ ekey, const uint32_t* __restrict__ label, const unsigned long long* __restrict__ best,
                                                          uint32_t n, uint32_t E, uint32_t* __restrict__ parent, uint32_t* in_forest, uint32_t* hooked) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    uint32_t p = label[r];
    const unsigned long long c = p == r ? best[r] : 0ull;
    if (c) {
        const uint32_t id = 0xFFFFFFFFu - (uint32_t)c;
        if (id < E) {      // (it is: a pick names a directed edge's position)
            const unsigned long long k = ekey[id];
            const uint32_t la = label[(uint32_t)(k >> 32)], lb = label[(uint32_t)k];
            const uint32_t s = la == r ? lb : la;      // the root of the component at the other end
            in_forest[id] = 1u;
            if (!(best[s] == c && r < s)) p = s;       // a mutual pick keeps the smaller root
            *hooked = 1u;
        }
    }
    parent[r] = p;
}
// *gate != 0: out[v] = in[in[v]]; else the launch before changed nothing (or the round hooked nothing), in[] and out[] are equal already and stay
__global__ __launch_bounds__(256) void forest_jump_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, const uint32_t* __restrict__ gate, uint32_t* changed) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= n || !*gate) return;
    const uint32_t p = in[v], pp = in[p];      // (p < n: a parent is a vertex)
    out[v] = pp;
    if (pp != p) *changed = 1u;
}
__global__ __launch_bounds__(256) void forest_outkeys_kernel(const uint32_t* __restrict__ in_forest, const uint32_t* __restrict__ opos, const uint32_t* __restrict__ w, uint32_t E,
                                                             uint32_t cap, unsigned long long* __restrict__ okey) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= E || !in_forest[p]) return;
    const uint32_t o = opos[p];
    if (o < cap) okey[o] = ((unsigned long long)(~w[p]) << 32) | p;      // (a forest has at most n - 1 = cap edges; the host refuses a larger count)
}
__global__ __launch_bounds__(256) void forest_gather_kernel(const unsigned long long* __restrict__ okey, const unsigned long long* __restrict__ ekey, const uint32_t* __restrict__ w,
                                                            uint32_t F, uint32_t E, uint32_t* __restrict__ oa, uint32_t* __restrict__ ob, uint32_t* __restrict__ ow) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= F) return;
    const uint32_t id = (uint32_t)okey[i];
    if (id >= E) return;
    const unsigned long long k = ekey[id];
    oa[i] = (uint32_t)(k >> 32); ob[i] = (uint32_t)k; ow[i] = w[id];
}

psk_status forest_impl(Lane* ctx, const psk_hit_min* recs, uint32_t n_recs, uint32_t n, float min_ani, float min_af, int use_af, int either,
                       uint32_t* edge_a, uint32_t* edge_b, float* edge_ani, uint32_t* n_edges) {
    hipStream_t st = ctx->stream;
    const uint32_t N = 2u * n_recs;      // (n_recs < 2^30)
    int n_bits = 0; while (n_bits < 32 && (n >> n_bits)) n_bits++;      // bit width of n: the sentinel's high word
    const int max_jumps = n_bits + 2, max_rounds = n_bits + 2;         // (<= 34)
    size_t ts1 = 0, ts2 = 0, ts3 = 0;
    PSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, ts1, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)N, 0, 32 + n_bits, st));
    PSK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, ts2, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(N + 1u), st));
    PSK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, ts3, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, 0, 64, st));
    const size_t ts = std::max(ts1, std::max(ts2, ts3));
    PoolScratch tmp;      // back to the pool on every exit
    const size_t N8 = 8 * (size_t)N, N4 = 4 * (size_t)N + 4, n4 = 4 * (size_t)n + 4, n8 = 8 * (size_t)n;
    const size_t o_flag = 0, o_recs = clu_al256(o_flag + 256), o_k0 = clu_al256(o_recs + sizeof(psk_hit_min) * (size_t)n_recs), o_k1 = clu_al256(o_k0 + N8), o_v0 = clu_al256(o_k1 + N8),
                 o_v1 = clu_al256(o_v0 + N4), o_hd = clu_al256(o_v1 + N4), o_pos = clu_al256(o_hd + N4), o_adj = clu_al256(o_pos + N4), o_w = clu_al256(o_adj + N4),
                 o_row = clu_al256(o_w + N4), o_la = clu_al256(o_row + n4), o_lb = clu_al256(o_la + n4), o_best = clu_al256(o_lb + n4), o_ok0 = clu_al256(o_best + n8),
                 o_ok1 = clu_al256(o_ok0 + n8), o_oa = clu_al256(o_ok1 + n8), o_ob = clu_al256(o_oa + n4), o_ow = clu_al256(o_ob + n4), o_t = clu_al256(o_ow + n4), o_end = o_t + ts;
    PSK_TRY(tmp.reserve(ctx->dev, o_end + 256));
    char* T = (char*)tmp.p;
    uint32_t* d_flag = (uint32_t*)(T + o_flag);      // [0]: the round hooked; [1 .. max_jumps]: a jump launch changed a parent; [40]: an index was out of range; [41]: an edge without its mate
    psk_hit_min* d_recs = (psk_hit_min*)(T + o_recs);
    unsigned long long *k0 = (unsigned long long*)(T + o_k0), *k1 = (unsigned long long*)(T + o_k1), *best = (unsigned long long*)(T + o_best), *ok0 = (unsigned long long*)(T + o_ok0),
                       *ok1 = (unsigned long long*)(T + o_ok1);
    uint32_t *v0 = (uint32_t*)(T + o_v0), *v1 = (uint32_t*)(T + o_v1), *head = (uint32_t*)(T + o_hd), *pos = (uint32_t*)(T + o_pos), *adj = (uint32_t*)(T + o_adj), *w = (uint32_t*)(T + o_w),
             *row = (uint32_t*)(T + o_row), *la = (uint32_t*)(T + o_la), *lb = (uint32_t*)(T + o_lb), *oa = (uint32_t*)(T + o_oa), *ob = (uint32_t*)(T + o_ob), *ow = (uint32_t*)(T + o_ow);
    void* hp;
    PSK_TRY(ctx->pinned(256, &hp));
    uint32_t* h_flag = (uint32_t*)hp;      // [0 .. 41] as d_flag, [48]: directed edges, [49]: forest edges

    // edges -> rows: cluster_impl's launches
    PSK_HIP(hipMemsetAsync(d_flag, 0, 256, st));
    PSK_HIP(hipMemcpyAsync(d_recs, recs, sizeof(psk_hit_min) * (size_t)n_recs, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(clu_edges_kernel, clu_grid(n_recs), dim3(256), 0, st, (const psk_hit_min*)d_recs, n_recs, n, min_ani, min_af, use_af, either, k0, v0, d_flag + 40);
    size_t t1 = ts;
    PSK_HIP(hipcub::DeviceRadixSort::SortPairs(T + o_t, t1, (const unsigned long long*)k0, k1, (const uint32_t*)v0, v1, (int)N, 0, 32 + n_bits, st));
    hipLaunchKernelGGL(clu_heads_kernel, clu_grid((uint64_t)N + 1), dim3(256), 0, st, (const unsigned long long*)k1, N, n, head);
    size_t t2 = ts;
    PSK_HIP(hipcub::DeviceScan::ExclusiveSum(T + o_t, t2, (const uint32_t*)head, pos, (int)(N + 1u), st));
    hipLaunchKernelGGL(clu_scatter_kernel, clu_grid(N), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)v1, (const uint32_t*)head, (const uint32_t*)pos, N, adj, w);
    hipLaunchKernelGGL(clu_rows_kernel, clu_grid((uint64_t)n + 1), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)pos, N, n, row);
    // the deduplicated keys, into the sort's input buffer (free now)
    unsigned long long* ekey = k0;
    hipLaunchKernelGGL(forest_keys_kernel, clu_grid(N), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)head, (const uint32_t*)pos, N, ekey);
    PSK_HIP(hipMemcpyAsync(h_flag + 48, row + n, 4, hipMemcpyDeviceToHost, st));
    PSK_HIP(hipMemcpyAsync(h_flag, d_flag, 192, hipMemcpyDeviceToHost, st));
    PSK_HIP(hipStreamSynchronize(st));
    if (h_flag[40]) { psk_set_error("cluster_forest: a record's query or ref_index is n_genomes (%u) or more", n); return PSK_EINVAL; }
    const uint32_t E = h_flag[48];      // directed edges: <= N
    if (E > N || (E & 1u)) { psk_set_error("cluster_forest: %u directed edges from %u entries", E, N); return PSK_EHIP; }
    ctx->dev->fo_edges = E / 2; ctx->dev->fo_rounds = 0; ctx->dev->fo_jumps = 0;
    *n_edges = 0;
    if (E == 0) return PSK_OK;
    // edge ids; the flags of the forest's edges take the place of the heads (E + 1 <= N + 1 entries, the last one stays 0 for the sum)
    uint32_t *eid = v0, *in_forest = head, *opos = pos;
    hipLaunchKernelGGL(forest_mate_kernel, clu_grid(E), dim3(256), 0, st, (const unsigned long long*)ekey, (const uint32_t*)row, E, n, eid, d_flag + 41);
    PSK_HIP(hipMemsetAsync(in_forest, 0, 4 * (size_t)E + 4, st));
    hipLaunchKernelGGL(clu_iota_kernel, clu_grid(n), dim3(256), 0, st, n, la, (uint32_t*)nullptr);
    uint64_t rounds = 0, jumps = 0;
    bool done = false;
    for (int round = 0; round < max_rounds && !done; round++) {
        PSK_HIP(hipMemsetAsync(d_flag, 0, 160, st));
        PSK_HIP(hipMemsetAsync(best, 0, n8, st));
        hipLaunchKernelGGL(forest_pick_kernel, clu_grid(64 * (uint64_t)n), dim3(256), 0, st, (const uint32_t*)row, (const uint32_t*)adj, (const uint32_t*)w, (const uint32_t*)eid,
                           (const uint32_t*)la, n, best);
        hipLaunchKernelGGL(forest_hook_kernel, clu_grid(n), dim3(256), 0, st, (const unsigned long long*)ekey, (const uint32_t*)la, (const unsigned long long*)best, n, E, lb, in_forest, d_flag);
        for (int j = 0; j < max_jumps; j++)      // lb -> la, la -> lb, ...: launch j runs iff flag j is set (0: the hook's, j: the launch before's)
            hipLaunchKernelGGL(forest_jump_kernel, clu_grid(n), dim3(256), 0, st, (const uint32_t*)((j & 1) ? la : lb), (j & 1) ? lb : la, n, (const uint32_t*)(d_flag + j), d_flag + j + 1);
        PSK_HIP(hipMemcpyAsync(h_flag, d_flag, 192, hipMemcpyDeviceToHost, st));
        PSK_HIP(hipStreamSynchronize(st));
        if (h_flag[41]) { psk_set_error("cluster_forest: a directed edge without its reverse"); return PSK_EHIP; }
        if (!h_flag[0]) { done = true; break; }
        rounds++;
        for (int j = 0; j < max_jumps && h_flag[j]; j++) jumps++;      // the launches that found their gate open
        if (h_flag[max_jumps]) { psk_set_error("cluster_forest: pointer jumping did not end after %d launches", max_jumps); return PSK_EHIP; }
    }
    if (!done) { psk_set_error("cluster_forest: the rounds did not end after %d", max_rounds); return PSK_EHIP; }
    ctx->dev->fo_rounds = rounds; ctx->dev->fo_jumps = jumps;
    // the flagged edges in the edge order
    size_t t3 = ts;
    PSK_HIP(hipcub::DeviceScan::ExclusiveSum(T + o_t, t3, (const uint32_t*)in_forest, opos, (int)(E + 1u), st));
    PSK_HIP(hipMemcpyAsync(h_flag + 49, opos + E, 4, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(forest_outkeys_kernel, clu_grid(E), dim3(256), 0, st, (const uint32_t*)in_forest, (const uint32_t*)opos, (const uint32_t*)w, E, n - 1u, ok0);
    PSK_HIP(hipStreamSynchronize(st));
    const uint32_t F = h_flag[49];
    if (F == 0 || F > n - 1u) { psk_set_error("cluster_forest: %u forest edges over %u genomes", F, n); return PSK_EHIP; }
    size_t t4 = ts;
    PSK_HIP(hipcub::DeviceRadixSort::SortKeys(T + o_t, t4, (const unsigned long long*)ok0, ok1, (int)F, 0, 64, st));
    hipLaunchKernelGGL(forest_gather_kernel, clu_grid(F), dim3(256), 0, st, (const unsigned long long*)ok1, (const unsigned long long*)ekey, (const uint32_t*)w, F, E, oa, ob, ow);
    PSK_HIP(hipMemcpyAsync(edge_a, oa, 4 * (size_t)F, hipMemcpyDeviceToHost, st));
    PSK_HIP(hipMemcpyAsync(edge_b, ob, 4 * (size_t)F, hipMemcpyDeviceToHost, st));
    PSK_HIP(hipMemcpyAsync(edge_ani, ow, 4 * (size_t)F, hipMemcpyDeviceToHost, st));      // (the input's bits)
    PSK_HIP(hipStreamSynchronize(st));
    *n_edges = F;
    return PSK_OK;
}

}  // namespace

extern "C" {

psk_status psk_cluster_records(psk_ctx* ctx, const psk_hit_min* recs, uint64_t n_recs, uint32_t n_genomes, const uint64_t* priority, const psk_cluster_opts* opts,
                               uint32_t* rep_of, float* rep_ani, uint32_t* n_reps) {
    if (!ctx || !opts || !rep_of) { psk_set_error("cluster_records: NULL ctx, opts or rep_of"); return PSK_EINVAL; }
    if (!recs && n_recs) { psk_set_error("cluster_records: NULL recs with n_recs = %llu", (unsigned long long)n_recs); return PSK_EINVAL; }
    if (opts->af_rule != 0 && opts->af_rule != 1) { psk_set_error("cluster_records: af_rule %d (0: both fractions, 1: either)", (int)opts->af_rule); return PSK_EINVAL; }
    if (opts->linkage != 0 && opts->linkage != 1) { psk_set_error("cluster_records: linkage %d (0: greedy representatives, 1: single linkage)", (int)opts->linkage); return PSK_EINVAL; }
    if (n_recs >= (1ull << 30)) { psk_set_error("cluster_records: %llu records (the limit is 2^30 - 1: their directed entries are one radix sort)", (unsigned long long)n_recs); return PSK_ELIMIT; }
    if (n_genomes >= (1u << 31)) { psk_set_error("cluster_records: %u genomes (the limit is 2^31 - 1)", n_genomes); return PSK_ELIMIT; }
    if (n_genomes == 0 && n_recs) { psk_set_error("cluster_records: a record's query or ref_index is n_genomes (%u) or more", n_genomes); return PSK_EINVAL; }
    if (n_recs == 0) {      // no edge: every genome represents itself (nothing for the device to do)
        for (uint32_t v = 0; v < n_genomes; v++) { rep_of[v] = v; if (rep_ani) rep_ani[v] = 1.0f; }
        if (n_reps) *n_reps = n_genomes;
        return PSK_OK;
    }
    const double ma = opts->min_ani <= 0 ? 0.95 : opts->min_ani, mf = opts->min_af < 0 ? 0.5 : opts->min_af;
    PSK_LANE(lg, ctx);
    PSK_TRY(cluster_impl(lg.lane, recs, (uint32_t)n_recs, n_genomes, priority, (float)ma, (float)mf, mf != 0 ? 1 : 0, opts->af_rule, opts->linkage, rep_of, rep_ani));
    if (n_reps) { uint32_t c = 0; for (uint32_t v = 0; v < n_genomes; v++) c += rep_of[v] == v; *n_reps = c; }
    return PSK_OK;
}

psk_status psk_ctx_cluster_stats(psk_ctx* c, uint64_t* edges, uint64_t* rounds, uint64_t* hook_passes) {
    if (!c) { psk_set_error("NULL ctx"); return PSK_EINVAL; }
    if (edges) *edges = c->cl_edges.load();
    if (rounds) *rounds = c->cl_rounds.load();
    if (hook_passes) *hook_passes = c->cl_hooks.load();
    return PSK_OK;
}

psk_status psk_cluster_forest(psk_ctx* ctx, const psk_hit_min* recs, uint64_t n_recs, uint32_t n_genomes, const psk_cluster_opts* opts,
                              uint32_t* edge_a, uint32_t* edge_b, float* edge_ani, uint32_t* n_edges) {
    if (!ctx || !opts || !n_edges) { psk_set_error("cluster_forest: NULL ctx, opts or n_edges"); return PSK_EINVAL; }
    if (n_genomes > 1 && (!edge_a || !edge_b || !edge_ani)) { psk_set_error("cluster_forest: NULL edge_a, edge_b or edge_ani with n_genomes = %u", n_genomes); return PSK_EINVAL; }
    if (!recs && n_recs) { psk_set_error("cluster_forest: NULL recs with n_recs = %llu", (unsigned long long)n_recs); return PSK_EINVAL; }
    if (opts->af_rule != 0 && opts->af_rule != 1) { psk_set_error("cluster_forest: af_rule %d (0: both fractions, 1: either)", (int)opts->af_rule); return PSK_EINVAL; }
    if (opts->linkage != 0 && opts->linkage != 1) { psk_set_error("cluster_forest: linkage %d (0 or 1; the forest ignores it)", (int)opts->linkage); return PSK_EINVAL; }
    if (n_recs >= (1ull << 30)) { psk_set_error("cluster_forest: %llu records (the limit is 2^30 - 1: their directed entries are one radix sort)", (unsigned long long)n_recs); return PSK_ELIMIT; }
    if (n_genomes >= (1u << 31)) { psk_set_error("cluster_forest: %u genomes (the limit is 2^31 - 1)", n_genomes); return PSK_ELIMIT; }
    if (n_genomes == 0 && n_recs) { psk_set_error("cluster_forest: a record's query or ref_index is n_genomes (%u) or more", n_genomes); return PSK_EINVAL; }
    *n_edges = 0;
    if (n_recs == 0) return PSK_OK;      // no edge, no forest edge (nothing for the device to do)
    const double ma = opts->min_ani <= 0 ? 0.95 : opts->min_ani, mf = opts->min_af < 0 ? 0.5 : opts->min_af;
    PSK_LANE(lg, ctx);
    return forest_impl(lg.lane, recs, (uint32_t)n_recs, n_genomes, (float)ma, (float)mf, mf != 0 ? 1 : 0, opts->af_rule, edge_a, edge_b, edge_ani, n_edges);
}

psk_status psk_ctx_forest_stats(psk_ctx* c, uint64_t* edges, uint64_t* rounds, uint64_t* jump_passes) {
    if (!c) { psk_set_error("NULL ctx"); return PSK_EINVAL; }
    if (edges) *edges = c->fo_edges.load();
    if (rounds) *rounds = c->fo_rounds.load();
    if (jump_passes) *jump_passes = c->fo_jumps.load();
    return PSK_OK;
}

}  // extern "C"
