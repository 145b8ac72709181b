// Chain stage 5 (only when a call asks for it): the bootstrap interval of every pair's ANI - skani's --ci. The per-chunk values the reduce stage averaged
// are resampled B times with replacement; the bounds are order statistics of the B resample means. The rule (include/pyskani_amd.h, psk_ci_opts) is a function of
// the pair's values, B and the seed alone: the draw stream (chain_stages.h: ci_key / ci_hash / ci_index) does not know the pair, so neither batch, lane, round nor
// slot can move a bound. Launched after the reduce and the learned-ANI regression, whose record says whether the bounds are shifted.
//
// Three tiers, cut like the reduce's:
//   interval_wave_kernel    chunk tables of up to 64 RW_PER rows (pairs of ~5 Mb genomes: ~250): one wave per pair, four pairs per workgroup, no workgroup barrier;
//                           values and resample means in the wave's own LDS; a lane owns resample b, b + 64, ...
//   interval_group_kernel   longer tables with up to RED_CAP kept values: one workgroup per pair, values in LDS, 256 lanes own the resamples
//   interval_global_kernel  more kept values than that (Gb-scale pairs: ~150 000 rows): the values compacted into global scratch (one double per chunk row)
// In every tier a resample is ONE lane's sequential double sum in draw order - the order the rule states - so the tiers agree to the bit, and the bounds are found
// by rank (values below + equal values at lower resample index: a permutation, so exactly one mean has each rank; equal means are equal floats).
#include "chain_stages.h"
#include <cmath>

namespace {

__device__ __forceinline__ double chunk_value(const ChunkOut& c, int k) {      // the expression of pair_reduce_*: m == 1 gives the pair's ani_raw bit for bit
    double ratio = (double)c.anchors / (double)(c.seeds > 1 ? c.seeds - 1 : 1);
    if (ratio > 1.0) ratio = 1.0;
    return pow(ratio, 1.0 / (double)k);
}

// mean of resample b over v[0..m): two draws per hash, summed in draw order
template <class V>
__device__ __forceinline__ double resample_mean(const V v, uint32_t m, uint64_t seed, uint32_t b) {
    const uint64_t key = ci_key(seed, b);
    double sum = 0.0;
    const uint32_t half = m >> 1;
#pragma unroll 4
    for (uint32_t jj = 0; jj < half; jj++) {
        const uint64_t h = ci_hash(key, jj);
        sum += v[ci_index((uint32_t)h, m)];
        sum += v[ci_index((uint32_t)(h >> 32), m)];
    }
    if (m & 1u) sum += v[ci_index((uint32_t)ci_hash(key, half), m)];
    return sum / (double)m;
}

// the float a caller sees for the order statistic x: shifted with the regression's ANI, clamped like it
__device__ __forceinline__ float bound_of(double x, const psk_hit& h) {
    float f = (float)x;
    if (h.learned) { f = f + (h.ani - h.ani_raw); f = f < 0.0f ? 0.0f : (f > 1.0f ? 1.0f : f); }
    return f;
}

// ranks of means[0..B) by the lanes [t, t + T, ...): the mean of rank lo_rank / hi_rank writes its bound
__device__ __forceinline__ void write_bounds(const double* means, const IntervalArgs& A, uint32_t p, uint32_t t, uint32_t T) {
    for (uint32_t b = t; b < A.B; b += T) {
        const double x = means[b];
        uint32_t rank = 0;
        for (uint32_t y = 0; y < A.B; y++) { const double o = means[y]; rank += (o < x) || (o == x && y < b); }
        if (rank == A.lo_rank) A.out[p].x = bound_of(x, A.hits[p]);
        if (rank == A.hi_rank) A.out[p].y = bound_of(x, A.hits[p]);
    }
}

// one (pairs, draws) pair of atomics per workgroup: a counter every wave bumps serialises the launch on one L2 line
__device__ __forceinline__ void count_work(const IntervalArgs& A, unsigned long long pairs, unsigned long long draws) {
    __shared__ unsigned long long s_w[2];
    if (threadIdx.x == 0) { s_w[0] = 0; s_w[1] = 0; }
    __syncthreads();
    if (pairs) { atomicAdd(&s_w[0], pairs); atomicAdd(&s_w[1], draws); }
    __syncthreads();
    if (threadIdx.x == 0 && s_w[0]) { atomicAdd(&A.work[0], s_w[0]); atomicAdd(&A.work[1], s_w[1]); }
}

}  // namespace

// pairs without a chunk table (batches that carry the live list: no tier visits them)
__global__ __launch_bounds__(256) void interval_empty_kernel(IntervalArgs A, uint32_t n_pairs) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_pairs && A.n_chunks[p] == 0) A.out[p] = make_float2(-1.0f, -1.0f);
}

__global__ __launch_bounds__(256) void interval_wave_kernel(IntervalArgs A, uint32_t n_pairs) {
    extern __shared__ double s_dyn[];      // per wave: 64 RW_PER values, then b_pad resample means
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* sv = s_dyn + (size_t)wave * (64u * RW_PER + A.b_pad);
    double* sm = sv + 64u * RW_PER;
    const uint32_t n = A.live ? *A.n_live : n_pairs;
    unsigned long long w_pairs = 0, w_draws = 0;
    for (uint32_t k = blockIdx.x * 4 + wave; k < n; k += gridDim.x * 4) {
        const uint32_t p = A.live ? A.live[k] : k;
        const uint32_t nc = A.n_chunks[p];
        if (nc > 64u * RW_PER) continue;      // the workgroup tiers
        if (nc == 0 || A.hits[p].ani_raw < 0.0f) {      // no chunk table (a launch without the live list), no kept chain, or below min_aligned_frac
            if (lane == 0) A.out[p] = make_float2(-1.0f, -1.0f);
            continue;
        }
        const ChunkOut* co = A.chunks + (size_t)A.cbase[p];
        lds_wave_sync();      // the previous pair's ranks have been read
        uint32_t m = 0;
        for (uint32_t r0 = 0; r0 < nc; r0 += 64u) {      // the values of the chunks that kept a chain, compacted in chunk order
            const uint32_t r = r0 + lane;
            ChunkOut c{};
            if (r < nc) c = co[r];
            const bool valid = r < nc && c.n_intervals != 0;
            const unsigned long long vm = __ballot(valid);
            if (valid) sv[m + (uint32_t)__popcll(vm & ((1ull << lane) - 1))] = chunk_value(c, A.k);
            m += (uint32_t)__popcll(vm);
        }
        lds_wave_sync();
        for (uint32_t b = lane; b < A.B; b += 64u) sm[b] = resample_mean((const double*)sv, m, A.seed, b);
        lds_wave_sync();
        write_bounds(sm, A, p, lane, 64u);
        if (lane == 0) { w_pairs++; w_draws += (unsigned long long)A.B * m; }
    }
    count_work(A, w_pairs, w_draws);
}

// one workgroup per pair of more than 64 RW_PER rows; GLOBAL: the pairs with more than RED_CAP kept values, else the others
template <bool GLOBAL>
__device__ __forceinline__ void interval_group(const IntervalArgs& A, uint32_t n_pairs) {
    __shared__ double s_v[GLOBAL ? 1 : RED_CAP];
    __shared__ double s_mean[CI_MAX_ITER];
    __shared__ uint32_t s_wt[2][4];
    __shared__ uint32_t s_m;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t n = A.live ? *A.n_live : n_pairs;
    unsigned long long w_pairs = 0, w_draws = 0;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t p = A.live ? A.live[k] : k;
        const uint32_t nc = A.n_chunks[p];
        if (nc <= 64u * RW_PER) continue;      // the wave tier
        if (!GLOBAL && A.hits[p].ani_raw < 0.0f) {
            if (threadIdx.x == 0) A.out[p] = make_float2(-1.0f, -1.0f);
            continue;
        }
        if (GLOBAL && A.hits[p].ani_raw < 0.0f) continue;
        const ChunkOut* co = A.chunks + (size_t)A.cbase[p];
        __syncthreads();      // the previous pair's LDS has been read
        if (threadIdx.x == 0) s_m = 0;
        __syncthreads();
        uint32_t t_m = 0;
        for (uint32_t i = threadIdx.x; i < nc; i += 256u) t_m += co[i].n_intervals != 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t_m += __shfl_xor(t_m, o);
        if (lane == 0) atomicAdd(&s_m, t_m);
        __syncthreads();
        const uint32_t m = s_m;
        if (GLOBAL ? m <= (uint32_t)RED_CAP : m > (uint32_t)RED_CAP) continue;      // the other workgroup tier's pair (uniform: every thread read the same s_m)
        double* gv = GLOBAL ? A.big_vals + (size_t)A.cbase[p] : s_v;      // m <= nc values in the pair's own nc slots
        // the kept rows' values compacted in chunk order, 256 rows per step: ballot ranks inside a wave, the four wave totals through LDS (pair_reduce_pair)
        uint32_t run = 0;
        for (uint32_t i0 = 0, it = 0; i0 < nc; i0 += 256u, it++) {
            const uint32_t i = i0 + threadIdx.x;
            ChunkOut c{};
            if (i < nc) c = co[i];
            const bool f = i < nc && c.n_intervals != 0;
            const unsigned long long bal = __ballot(f);
            if (lane == 0) s_wt[it & 1][w] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t before = 0, tot = 0;
            for (uint32_t x = 0; x < 4; x++) { const uint32_t cx = s_wt[it & 1][x]; if (x < w) before += cx; tot += cx; }
            if (f) gv[run + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1))] = chunk_value(c, A.k);
            run += tot;
        }
        __syncthreads();      // (orders the workgroup's global writes too)
        for (uint32_t b = threadIdx.x; b < A.B; b += 256u) s_mean[b] = resample_mean((const double*)gv, m, A.seed, b);
        __syncthreads();
        write_bounds(s_mean, A, p, threadIdx.x, 256u);
        if (threadIdx.x == 0) { w_pairs++; w_draws += (unsigned long long)A.B * m; }
    }
    __syncthreads();
    count_work(A, w_pairs, w_draws);
}
__global__ __launch_bounds__(256) void interval_group_kernel(IntervalArgs A, uint32_t n_pairs) { interval_group<false>(A, n_pairs); }
__global__ __launch_bounds__(256) void interval_global_kernel(IntervalArgs A, uint32_t n_pairs) { interval_group<true>(A, n_pairs); }

// the launches of one batch (chain.hip: chain_run, after the reduce and the regression)
void interval_launch(const IntervalArgs& A, uint32_t n_pairs, uint32_t rows_pair_max, bool use_live, std::atomic<uint64_t>* tier_launches, hipStream_t st) {
    if (use_live) hipLaunchKernelGGL(interval_empty_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, st, A, n_pairs);
    const size_t lds = 4 * sizeof(double) * (64u * RW_PER + (size_t)A.b_pad);
    tier_launches[0]++;
    hipLaunchKernelGGL(interval_wave_kernel, dim3(std::min<uint32_t>((n_pairs + 3) / 4, 16384u)), dim3(256), lds, st, A, n_pairs);
    if (rows_pair_max > 64u * RW_PER) { tier_launches[1]++; hipLaunchKernelGGL(interval_group_kernel, dim3(std::min<uint32_t>(n_pairs, 8192u)), dim3(256), 0, st, A, n_pairs); }
    if (rows_pair_max > (uint32_t)RED_CAP) { tier_launches[2]++; hipLaunchKernelGGL(interval_global_kernel, dim3(std::min<uint32_t>(n_pairs, 512u)), dim3(256), 0, st, A, n_pairs); }
}
