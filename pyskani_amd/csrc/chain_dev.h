// Device helpers shared by the translation units that chain anchors (join.hip / dp.hip / select.hip / reduce.hip: the batched path; small_query.hip: the
// one-launch-sequence query of a small genome). Header-only: every translation unit gets its own copy (no relocatable device code).
#pragma once
#include "common.h"

struct MarkerSet { const uint64_t* p; uint32_t n; uint32_t pad; };

// LDS hand-off between lanes of ONE wave: order the ds ops, no workgroup barrier
__device__ __forceinline__ void lds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The slice join's 8-byte anchor (slice_join.hip emits it, the DP kernels read it): lo = q_rel | (ref contig << 1 | strand) << 16, hi = r pos, where
// q_rel = q pos - the q pos of the head of the anchor's chunk (row_q0). A chunk spans at most FRAGMENT_LENGTH query bases and the blocked seed index the slice
// join walks holds references of at most 2^GSI_CONTIG_BITS contigs (seed_index.hip), so no input of that join overflows it; the DP uses q only as differences
// within one chunk. What the 16-byte record carries beside it - the q contig - is per chunk row too (row_q0).
static_assert(FRAGMENT_LENGTH < (1u << 16), "q_rel fills the low 16 bits of a packed anchor");
static_assert(GSI_CONTIG_BITS + 1 <= 16, "ref contig << 1 | strand fills the high 16 bits of a packed anchor");
__device__ __forceinline__ uint2 pk_anchor(uint32_t q_rel, uint32_t r, uint32_t m) { return make_uint2((q_rel & 0xFFFFu) | (m << 16), r); }
// (q_rel, r pos, ref contig << 1 | strand, -): one mask and one shift
__device__ __forceinline__ uint4 pk_unpack(uint2 a) { return make_uint4(a.x & 0xFFFFu, a.y, a.x >> 16, 0u); }
// The DP kernels read either form through this: PK = the slice join's 8-byte anchors (q relative to the row's head), else the 16-byte records
// (q pos, r pos, ref contig << 1 | strand, q contig). Both hand out (q, r pos, ref contig << 1 | strand, -).
template <bool PK> struct AncRd {
    const void* a;
    __device__ __forceinline__ uint4 operator[](size_t i) const { return PK ? pk_unpack(((const uint2*)a)[i]) : ((const uint4*)a)[i]; }
    // anchors i .. i + 3 (i a multiple of four): W4 16-byte words, and what the words hold - loads and decoding apart, so that a caller can load ahead and
    // keep the raw words (two registers per 8-byte anchor) until it needs the fields
    static constexpr int W4 = PK ? 2 : 4;
    __device__ __forceinline__ void load4w(size_t i, uint4 (&w)[W4]) const {
        const uint4* p = PK ? (const uint4*)((const uint2*)a + i) : (const uint4*)a + i;
#pragma unroll
        for (int k = 0; k < W4; k++) w[k] = p[k];
    }
    static __device__ __forceinline__ void unpack4(const uint4 (&w)[W4], uint4 (&o)[4]) {
        if (PK) {
#pragma unroll
            for (int k = 0; k < 2; k++) { o[2 * k] = pk_unpack(make_uint2(w[k].x, w[k].y)); o[2 * k + 1] = pk_unpack(make_uint2(w[k].z, w[k].w)); }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = w[k % W4];
        }
    }
    __device__ __forceinline__ void load4(size_t i, uint4 (&o)[4]) const { uint4 w[W4]; load4w(i, w); unpack4(w, o); }
};

// u = q - r', r' the strand-signed reference position (-r on the reverse strand): the anchor's diagonal. With it the gap of a
// pair is |ux - uy| and dr = dq - (ux - uy): three instructions fewer per (anchor, predecessor) pair than from q and r.
struct LaneAnchor { uint32_t q, u, m; int32_t f; };
__device__ __forceinline__ uint32_t lane_diag(uint32_t qx, uint32_t rx, uint32_t sg) { return qx - ((rx ^ sg) - sg); }

// key of predecessor y for anchor x at distance d, NEGATIVE when y is not chainable; same rule as the wave kernel and the oracle.
// The DP kernel's time is its VALU instruction count (profiles/r3/r3a_chain_lane20_counters.md: 65 % of all issue cycles at three
// waves per SIMD, the rest waits), so the step is written for it: a predecessor is kept as (q + 1, diagonal, contig | strand,
// score - 1) - the two "- 1" of the range tests are paid once per anchor instead of once per pair -, every requirement is a sign
// bit, and the verdict is the key's own sign (one v_and_or) so that the running maximum, taken signed, skips what is not chainable.
// ISA per (anchor, predecessor) pair: 8 v_sub, 3 v_or3, v_xor, v_lshl_add, v_and_or, 2 v_max = 17 instructions / 46 issue cycles;
// the first version had 20 / 70 (its mask came out as v_cmp + v_cndmask, the slowest VALU instruction there is: 32.8 -> 29.3 ms).
struct LanePred { uint32_t q1, u, m; int32_t f1; };
__device__ __forceinline__ int32_t lane_eval2(uint32_t qx, uint32_t ux, uint32_t mx, const LanePred& y, int d) {
    const int32_t a = (int32_t)(qx - y.q1);                               // dq - 1
    const int32_t t = (int32_t)(ux - y.u), nt = (int32_t)(y.u - ux);      // dq - dr (strand -: dr = ry - rx)
    const int32_t gap = t > nt ? t : nt;
    const int32_t b = a - t;                                              // dr - 1
    const int32_t s1 = y.f1 - gap;                                        // score - ANCHOR_SCORE2 - 1
    const uint32_t z = y.m ^ mx;
    // 1 <= dq <= 2500, dr >= 1, gap <= 300, score > 40, same ref contig and strand
    const uint32_t bad = (uint32_t)a | (uint32_t)(BP_CHAIN_BAND - 1 - a) | (uint32_t)b | (uint32_t)(MAX_GAP_LENGTH - gap) | (uint32_t)s1 | z | (0u - z);
    const uint32_t key = ((uint32_t)s1 << 7) + ((((uint32_t)ANCHOR_SCORE2 + 1u) << 7) | (127u - (uint32_t)d));      // scores stay below 2^20 (a chunk holds < 16 384 anchors): the key's sign bit is free
    return (int32_t)(key | (bad & 0x80000000u));
}
// The same for the slice join's 8-byte anchors: wx = q | m << 16, the anchor's own low word (m = ref contig << 1 | strand), and y.q1 = (q + 1) | m << 16.
// Equal m: wx - y.q1 is dq - 1 as before. Different m: the high halves differ by at least 2^16 and the low ones by at most FRAGMENT_LENGTH + 1, so the
// difference is below -(BP_CHAIN_BAND) or above BP_CHAIN_BAND - 1 and one of the two range tests on a fails: no test on m of its own, and y.m is not read.
static_assert(FRAGMENT_LENGTH + 1u < (1u << 16) && (1u << 16) - (FRAGMENT_LENGTH + 1u) > (uint32_t)BP_CHAIN_BAND, "q + 1 stays in the low half; another contig or strand is out of the q range");
__device__ __forceinline__ int32_t lane_eval2_qm(uint32_t wx, uint32_t ux, const LanePred& y, int d) {
    const int32_t a = (int32_t)(wx - y.q1);                               // dq - 1, or out of range
    const int32_t t = (int32_t)(ux - y.u), nt = (int32_t)(y.u - ux);
    const int32_t gap = t > nt ? t : nt;
    const int32_t b = a - t;
    const int32_t s1 = y.f1 - gap;
    const uint32_t bad = (uint32_t)a | (uint32_t)(BP_CHAIN_BAND - 1 - a) | (uint32_t)b | (uint32_t)(MAX_GAP_LENGTH - gap) | (uint32_t)s1;
    const uint32_t key = ((uint32_t)s1 << 7) + ((((uint32_t)ANCHOR_SCORE2 + 1u) << 7) | (127u - (uint32_t)d));
    return (int32_t)(key | (bad & 0x80000000u));
}
// q + 1 of a window entry (QM: the low half of its first register)
template <bool QM> __device__ __forceinline__ uint32_t lane_q1(const LanePred& y) { return QM ? y.q1 & 0xFFFFu : y.q1; }
