// The database's locality order (psk_db::slot_of / ref_of): an internal order of the references in which relatives are neighbours, so that the blocks of the seed
// index (2^BSI_BLOG consecutive SLOTS each) hold a query's relatives together whatever order the references were added in.
//
// Relatives are found from what the database already holds, in O(markers): a reference's markers are sorted and unique, so its first LOC_S markers are a bottom-s
// min-hash of its marker set. Every (marker, reference) of those is sorted by marker (stable: a run of equal markers lists its references in ascending order); every
// reference of a run but the first makes one EDGE (first reference of the run, itself); the edges are sorted, and a pair of references that LOC_T or more markers
// made an edge of is linked. One shared marker is no evidence: a given 21-mer sits in a random 5 Mb genome with probability 2 L / 4^21 ~ 2.3e-6, so two unrelated
// genomes share one of their 128 bottom markers with probability 6e-4 - and 10 000 genomes are 5e7 pairs. Three by chance: 4e-11 per pair.
// (128, not 64: a member 10 % from its family's ancestor keeps 11 % of the ancestor's markers; with 64, one in ten of those found no partner with three edges.)
// Connected components by hooking (atomicMin of labels) and pointer jumping until no edge joins two labels; a component's label ends as its smallest reference index,
// whatever order the atomics arrive in. The order is the stable sort of the references by (label, index): singletons and ties keep insertion order, and a database
// whose groups are contiguous already gets the identity - then nothing downstream translates anything.
#include "query_parts.h"
#include <hipcub/hipcub.hpp>
#include <algorithm>

constexpr uint32_t LOC_S = 128;     // bottom markers per reference
constexpr uint32_t LOC_T = 3;       // shared bottom markers (with the same first holder) that link two references
constexpr unsigned long long LOC_NO_MARKER = 1ull << (2 * K_MARKER);      // (markers are 2 K_MARKER-bit k-mers: sorts behind every marker)
constexpr unsigned long long LOC_NO_EDGE = ~0ull;

__global__ __launch_bounds__(256) void loc_gather_kernel(const MarkerSet* __restrict__ refs, uint32_t n_refs, unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t r = t / LOC_S, i = t % LOC_S;
    if (r >= n_refs) return;
    const MarkerSet m = refs[r];
    key[t] = i < m.n ? (unsigned long long)m.p[i] : LOC_NO_MARKER;
    val[t] = r;
}
// head[i] = i where a run of equal markers begins, 0 elsewhere: its inclusive max-scan is every entry's run start
__global__ __launch_bounds__(256) void loc_heads_kernel(const unsigned long long* __restrict__ key, uint32_t n, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || key[i] != key[i - 1]) ? i : 0u;
}
__global__ __launch_bounds__(256) void loc_edges_kernel(const unsigned long long* __restrict__ key, const uint32_t* __restrict__ val, const uint32_t* __restrict__ start, uint32_t n,
                                                        unsigned long long* __restrict__ edge) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = start[i];
    edge[i] = (s == i || key[i] == LOC_NO_MARKER) ? LOC_NO_EDGE : ((unsigned long long)val[s] << 32) | val[i];      // (val[s] < val[i]: the sort is stable and a reference's markers are distinct)
}
__global__ __launch_bounds__(256) void loc_init_kernel(uint32_t* __restrict__ label, uint32_t n) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < n) label[r] = r;
}
// a lane per sorted edge; the FIRST of a run of at least LOC_T equal edges hooks. label[x] <= x, always a member of x's component, and only ever decreases.
__global__ __launch_bounds__(256) void loc_hook_kernel(const unsigned long long* __restrict__ edge, uint32_t n, uint32_t* __restrict__ label, uint32_t* __restrict__ changed) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || (uint64_t)i + LOC_T - 1 >= n) return;
    const unsigned long long e = edge[i];
    if (e == LOC_NO_EDGE || edge[i + LOC_T - 1] != e || (i && edge[i - 1] == e)) return;
    const uint32_t a = (uint32_t)(e >> 32), b = (uint32_t)e;
    const uint32_t la = label[a], lb = label[b];
    if (la == lb) return;
    const uint32_t lo = la < lb ? la : lb, hi = la < lb ? lb : la;
    atomicMin(&label[hi], lo);
    atomicMin(&label[la < lb ? b : a], lo);
    *changed = 1u;
}
__global__ __launch_bounds__(256) void loc_jump_kernel(uint32_t* __restrict__ label, uint32_t n) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t l = label[r];
    const uint32_t ll = label[l];
    if (ll < l) atomicMin(&label[r], ll);
}
struct LocMax { __host__ __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };

// label[r] = smallest index of r's group, on the host. Called with the database locked exclusively. The order is an optimisation: where the grouping cannot run (no room
// for its 28 bytes per gathered marker, more than one radix sort's worth of markers, no convergence) every reference is its own group - the insertion order - and the
// call that asked goes on as it would have without the order.
static psk_status locality_labels(Lane* ctx, psk_db* db, std::vector<uint32_t>& label) {
    const uint32_t n = (uint32_t)db->refs.size();
    label.resize(n);
    if (n == 0) return PSK_OK;
    auto ungrouped = [&]() -> psk_status { for (uint32_t i = 0; i < n; i++) label[i] = i; return PSK_OK; };
    if ((uint64_t)n * LOC_S >= 0x7FFFFF00ull) return ungrouped();      // (one radix sort: 16 M references)
    hipStream_t st = ctx->stream;
    PSK_TRY(upload_marker_table(ctx, db));
    const uint32_t N = n * LOC_S, gN = (N + 255u) / 256u, gn = (n + 255u) / 256u;
    size_t ts1 = 0, ts2 = 0, ts3 = 0;
    PSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, ts1, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)N, 0, 2 * K_MARKER + 1, st));
    PSK_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, ts2, (const uint32_t*)nullptr, (uint32_t*)nullptr, LocMax(), (int)N, st));
    PSK_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, ts3, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)N, 0, 64, st));
    const size_t ts = std::max(ts1, std::max(ts2, ts3));
    PoolScratch tmp;      // back to the pool when the labels are on the host
    const size_t o_k0 = 0, o_k1 = al256(o_k0 + 8 * (size_t)N), o_v0 = al256(o_k1 + 8 * (size_t)N), o_v1 = al256(o_v0 + 4 * (size_t)N), o_h = al256(o_v1 + 4 * (size_t)N),
                 o_lab = al256(o_h + 4 * (size_t)N), o_flag = al256(o_lab + 4 * (size_t)n), o_t = al256(o_flag + 64), o_end = o_t + ts;
    { const psk_status rc = tmp.reserve(ctx->dev, o_end + 256); if (rc == PSK_ENOMEM) return ungrouped(); PSK_TRY(rc); }
    char* T = (char*)tmp.p;
    unsigned long long *k0 = (unsigned long long*)(T + o_k0), *k1 = (unsigned long long*)(T + o_k1);
    uint32_t *v0 = (uint32_t*)(T + o_v0), *v1 = (uint32_t*)(T + o_v1), *head = (uint32_t*)(T + o_h), *d_label = (uint32_t*)(T + o_lab), *d_flag = (uint32_t*)(T + o_flag);
    hipLaunchKernelGGL(loc_gather_kernel, dim3(gN), dim3(256), 0, st, (const MarkerSet*)db->d_marker_ptr.p, n, k0, v0);
    size_t t1 = ts;
    PSK_HIP(hipcub::DeviceRadixSort::SortPairs(T + o_t, t1, (const unsigned long long*)k0, k1, (const uint32_t*)v0, v1, (int)N, 0, 2 * K_MARKER + 1, st));
    hipLaunchKernelGGL(loc_heads_kernel, dim3(gN), dim3(256), 0, st, (const unsigned long long*)k1, N, head);
    size_t t2 = ts;
    PSK_HIP(hipcub::DeviceScan::InclusiveScan(T + o_t, t2, (const uint32_t*)head, v0, LocMax(), (int)N, st));      // v0: every entry's run start
    hipLaunchKernelGGL(loc_edges_kernel, dim3(gN), dim3(256), 0, st, (const unsigned long long*)k1, (const uint32_t*)v1, (const uint32_t*)v0, N, k0);
    size_t t3 = ts;
    PSK_HIP(hipcub::DeviceRadixSort::SortKeys(T + o_t, t3, (const unsigned long long*)k0, k1, (int)N, 0, 64, st));
    hipLaunchKernelGGL(loc_init_kernel, dim3(gn), dim3(256), 0, st, d_label, n);
    // rounds of (hook, jump, jump), four to a synchronisation, each with a flag of its own: done when a hook pass found no edge between two labels
    void* hp;
    PSK_TRY(ctx->pinned(4 * (size_t)n + 64, &hp));
    uint32_t* h_flag = (uint32_t*)hp;
    bool done = false;
    for (int batch = 0; batch < 64 && !done; batch++) {
        PSK_HIP(hipMemsetAsync(d_flag, 0, 16, st));
        for (int k = 0; k < 4; k++) {
            hipLaunchKernelGGL(loc_hook_kernel, dim3(gN), dim3(256), 0, st, (const unsigned long long*)k1, N, d_label, d_flag + k);
            hipLaunchKernelGGL(loc_jump_kernel, dim3(gn), dim3(256), 0, st, d_label, n);
            hipLaunchKernelGGL(loc_jump_kernel, dim3(gn), dim3(256), 0, st, d_label, n);
        }
        PSK_HIP(hipMemcpyAsync(h_flag, d_flag, 16, hipMemcpyDeviceToHost, st));
        PSK_HIP(hipStreamSynchronize(st));
        done = h_flag[3] == 0;
    }
    if (!done) return ungrouped();      // (256 rounds: every round with a change lowers a label)
    PSK_HIP(hipMemcpyAsync(hp, d_label, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    PSK_HIP(hipStreamSynchronize(st));
    memcpy(label.data(), hp, 4 * (size_t)n);
    return PSK_OK;
}

// Called with the database locked exclusively, wherever its device tables are (re)built; loc_state 1 = the order is that of the references now in the database.
// $PSK_LOCALITY=0: insertion order. A database of one index block has nothing to order.
psk_status ensure_locality(Lane* ctx, psk_db* db, bool want_groups) {      // (declared in common.h)
    const uint32_t n = (uint32_t)db->refs.size();
    const bool have_order = db->loc_state == 1;
    if (have_order && (!want_groups || db->loc_groups_known)) return PSK_OK;
    if (!have_order) {
        db->loc_identity = true; db->ref_of.clear(); db->slot_of.clear(); db->d_ref_of.release(); db->d_slot_of.release();
        db->loc_groups_known = false; db->loc_groups = 0;
    }
    const bool keep = have_order || Switches::read().locality.off() || n <= (1u << BSI_BLOG);      // the order stands / stays the insertion order: the groups are only counted, for psk_db_locality
    if (keep && !want_groups) { db->loc_state = 1; return PSK_OK; }
    std::vector<uint32_t> label;
    PSK_TRY(locality_labels(ctx, db, label));
    uint32_t groups = 0;
    for (uint32_t r = 0; r < n; r++) groups += label[r] == r;
    db->loc_groups = groups; db->loc_groups_known = true;
    if (keep) { db->loc_state = 1; return PSK_OK; }
    // stable counting sort by label (a group's label is its first member: the groups keep the order of their first members)
    std::vector<uint32_t> first(n + 1, 0);
    for (uint32_t r = 0; r < n; r++) first[label[r] + 1]++;
    for (uint32_t r = 0; r < n; r++) first[r + 1] += first[r];
    std::vector<uint32_t> ref_of(n), slot_of(n);
    bool identity = true;
    for (uint32_t r = 0; r < n; r++) { const uint32_t s = first[label[r]]++; ref_of[s] = r; slot_of[r] = s; identity = identity && s == r; }
    if (!identity) {
        psk_status rc = db->d_ref_of.reserve(ctx->dev, 4 * (size_t)n + 256);
        if (rc == PSK_OK) rc = db->d_slot_of.reserve(ctx->dev, 4 * (size_t)n + 256);
        if (rc == PSK_ENOMEM) { db->d_ref_of.release(); db->d_slot_of.release(); db->loc_state = 1; return PSK_OK; }      // (no room for the two tables: insertion order)
        PSK_TRY(rc);
        PSK_HIP(hipMemcpyAsync(db->d_ref_of.p, ref_of.data(), 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        PSK_HIP(hipMemcpyAsync(db->d_slot_of.p, slot_of.data(), 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        PSK_HIP(hipStreamSynchronize(ctx->stream));      // (the host vectors are this frame's until they are moved below)
        db->ref_of.swap(ref_of); db->slot_of.swap(slot_of);
        db->loc_identity = false;
    }
    db->loc_state = 1;
    return PSK_OK;
}

// the pass matrix of a round, columns from insertion order into slot order: out[q][s] = in[q][ref_of[s]]
__global__ __launch_bounds__(256) void pass_to_slots_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n_refs, const uint32_t* __restrict__ ref_of) {
    const uint8_t* __restrict__ src = in + (size_t)blockIdx.y * n_refs;
    uint8_t* __restrict__ dst = out + (size_t)blockIdx.y * n_refs;
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_refs; s += gridDim.x * 256u) dst[s] = src[ref_of[s]];
}
void pass_to_slots_launch(const uint8_t* in, uint8_t* out, uint32_t n_queries, uint32_t n_refs, const uint32_t* ref_of, hipStream_t st) {
    for (uint32_t q0 = 0; q0 < n_queries; q0 += 65535u)      // (grid.y holds 65 535)
        hipLaunchKernelGGL(pass_to_slots_kernel, dim3(std::min(64u, (n_refs + 255u) / 256u), std::min(65535u, n_queries - q0)), dim3(256), 0, st,
                           in + (size_t)q0 * n_refs, out + (size_t)q0 * n_refs, n_refs, ref_of);
}
