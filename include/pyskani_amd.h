/* include/pyskani_amd.h — C-ABI of the MI355X-native ANI engine (libpyskani_amd.so).
 *
 * The drop-in boundary for pyskani's Database.sketch()/Database.query() hot path. pyskani
 * has no FFI today: its PyO3 crate calls the Rust crate `skani` directly. Each entry point
 * below replaces one of those call sites (paths are relative to /root/reference):
 *
 *   psk_sketch_host / psk_sketch_batch_device
 *        <- the per-contig loop over skani::seeding::fmh_seeds in Database::_sketch,
 *           src/pyskani/_skani/lib.rs:140-185 (contig filter :156, metadata :157-161,
 *           fmh_seeds :165-171) and skani::types::Sketch::get_markers_only at :495
 *   psk_db_add  <- self.markers.push(marker) + sketches.store(sketch)   lib.rs:501-508
 *   psk_screen  <- skani::screen::check_markers_quickly loop            lib.rs:617-637
 *   psk_chain   <- skani::chain::map_params_from_sketch + chain_seeds   lib.rs:646-653
 *   psk_query   <- the whole allow_threads closure of Database::query   lib.rs:569-659
 *                  (screen_val default :603-609, learned rule :611-614, ani>0.1 filter :654)
 *   psk_hit     <- the fields of skani::types::AniEstResult that Hit exposes, hit.rs:77-104
 *   psk_model_* <- skani::regression::{use_learned_ani, get_model}      lib.rs:611-614 and the
 *                  `&model_opt` argument of map_params_from_sketch      lib.rs:646-651
 *   psk_db_add  also implements the name-keyed store of lib.rs:51-55: queries shortlist NAMES
 *                  (lib.rs:616-637), so a name sketched twice yields one hit, against its last sketch
 *
 * Conventions: plain pointers and sizes, opaque handles, no exceptions cross the ABI.
 * Every function returns a psk_status; psk_last_error() gives the thread-local message.
 * Inputs are borrowed for the duration of the call only. Outputs returned through `**`
 * are library-allocated and released with the matching psk_*_free / psk_free.
 * Threading: every call runs on one of the context's execution lanes (own HIP stream, scratch and pinned
 * staging; at most $PSK_LANES = 8 at a time, further callers wait), so psk_query / psk_screen / psk_chain /
 * psk_sketch_host from different host threads overlap on the device, as `&self` + the released GIL allow in
 * lib.rs:551,569. A database is held shared by queries and exclusively by psk_db_add (`&mut self`, lib.rs:479)
 * and by whatever (re)builds its device tables.
 * A missing GPU is an error (PSK_EHIP) — there is no CPU fallback in this library.
 */
#ifndef PYSKANI_AMD_H
#define PYSKANI_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PSK_OK = 0,
    PSK_EINVAL = 1,   /* bad argument (k > 16, c == 0, NULL, ...)  -> ValueError          */
    PSK_ENOMEM = 2,   /* host or device allocation failed          -> MemoryError         */
    PSK_EHIP = 3,     /* HIP runtime error / no device             -> RuntimeError        */
    PSK_ENOMODEL = 4, /* learned-ANI requested, no model loaded    -> RuntimeError        */
    PSK_EKEY = 5,     /* unknown reference name                    -> KeyError            */
    PSK_ELIMIT = 6,   /* input exceeds a documented limit          -> OverflowError       */
    PSK_ERCCL = 7     /* RCCL missing or a collective failed       -> RuntimeError        */
} psk_status;

typedef struct psk_ctx psk_ctx;       /* one GPU: device id, stream, scratch arenas         */
typedef struct psk_sketch psk_sketch; /* one genome's seeds+index+markers, resident in HBM  */
typedef struct psk_db psk_db;         /* ordered reference set (insertion order = lib.rs:501) */
typedef struct psk_model psk_model;   /* learned-ANI regression model (gradient-boosted trees), device resident */

/* SketchParams::new(marker_c, c, k, false, false)  lib.rs:416 */
typedef struct {
    int32_t c;        /* compression, default 125        */
    int32_t marker_c; /* marker compression, default 1000 */
    int32_t k;        /* k-mer size, default 15, <= 16    */
} psk_params;

/* kwargs of Database.query, lib.rs:549, and the CommandParams literal lib.rs:573-601 */
typedef struct {
    int32_t learned_ani;     /* -1 = default rule (lib.rs:611-613), 0 = off, 1 = on            */
    int32_t median;          /* lib.rs:583 */
    int32_t robust;          /* lib.rs:582 */
    int32_t faster_small;    /* rescue_small = !faster_small, lib.rs:597 */
    double cutoff;           /* 0 = SEARCH_ANI_CUTOFF_DEFAULT (0.80), lib.rs:603-609 */
    double min_aligned_frac; /* 0 = D_FRAC_COVER_CUTOFF/100 = 0.15, lib.rs:589-590   */
    const psk_model* model;  /* `model_opt` of lib.rs:614/:650. The regression runs when learned_ani == 1, or when
                                learned_ani == -1, c >= 70, !median (lib.rs:611-613) AND a model is given; learned_ani == 1
                                without a model is PSK_ENOMODEL, learned_ani == -1 without one returns the raw chain ANI */
} psk_query_opts;

typedef struct {
    float ani;        /* AniEstResult.ani                   hit.rs:78  */
    float af_query;   /* AniEstResult.align_fraction_query  hit.rs:90  */
    float af_ref;     /* AniEstResult.align_fraction_ref    hit.rs:102 */
    uint32_t ref_index; /* insertion index in the db; name via psk_db_name */
    /* integer intermediates (bit-exact parity checks against the oracle) */
    uint32_t n_chunks, n_intervals;
    uint64_t n_anchors, covered_query, covered_ref, sum_chain_anchors, sum_chunk_seeds;
    float ani_raw;      /* chain ANI before the regression (== ani when learned == 0)      */
    float ani_std;      /* sample standard deviation of the per-chunk ANI estimates        */
    uint32_t learned;   /* 1 iff the regression model produced `ani`                       */
    uint32_t reserved;
} psk_hit;

/* What the reference's Hit holds (hit.rs:77-104: identity, query_fraction, reference_fraction, the two names) and nothing else, in 20 bytes: the record of
 * psk_query_many_min and psk_gather_hits_min - what crosses PCIe and xGMI when the caller did not ask for the chaining integers. */
typedef struct {
    float ani, af_query, af_ref;
    uint32_t ref_index; /* insertion index in the db (sharded runs: the global index) */
    uint32_t query;     /* index of the query within the call (sharded runs: the global index); bit 31: the regression model produced `ani` */
} psk_hit_min;

/* psk_hit_min and the bootstrap interval of `ani` (psk_query_many_ci), 28 bytes; `query` as in psk_hit_min */
typedef struct {
    float ani, af_query, af_ref;
    uint32_t ref_index;
    uint32_t query;
    float ci_lo, ci_hi; /* the 5 % and 95 % points of the resample means, around `ani` */
} psk_hit_ci;
/* Options of the interval calls; a NULL pointer means {0, 0, 0}. */
typedef struct {
    uint32_t iterations; /* resamples B: 0 = 100, else 20 <= B <= 1024 */
    uint32_t reserved;   /* must be 0 */
    uint64_t seed;       /* of the draw stream */
} psk_ci_opts;

typedef struct { uint32_t kmer, pos, contig, canon; } psk_seed; /* export record (parity tests) */

const char* psk_last_error(void);
const char* psk_version(void);
/* The C-ABI's revision: raised whenever an entry point's parameters or a structure's layout change (4: psk_sketch_unpack takes the extent of its source buffer as third
 * argument; 5: psk_hit_min / psk_query_many_min / psk_gather_hits_min / psk_ctx_join_work added;
 * 6: psk_db_locality added; 7: psk_ctx_rerun_stats added). psk_query_many_tri and psk_query_many_tri_min came after 7 WITHOUT raising it: no existing argument
 * list or structure moved, and a binding that wants them detects them by their presence (dlsym); psk_cluster_records, psk_ctx_cluster_stats, psk_ctx_tier_stats, psk_cluster_forest, psk_ctx_forest_stats, psk_screen_many, psk_ctx_screen_stats and the interval calls (psk_chain_ci, psk_query_many_ci, psk_ctx_interval_stats, psk_ci_draw, psk_ci_ranks) likewise. A binding compares psk_abi_version() with the PSK_ABI_VERSION it was
 * written against before it calls anything else: an argument list that moved is a memory error, not a link error. */
#define PSK_ABI_VERSION 7
int psk_abi_version(void);
/* Releases an array the library returned (hit lists, gathered lists). Never release such an array with free(): large hit arrays are
 * huge-page blocks the library keeps one of for its next call ($PSK_HIT_CACHE=0: returned to the system at once). */
void psk_free(void* p);

psk_status psk_ctx_create(int device, psk_ctx** out);
void psk_ctx_destroy(psk_ctx* ctx);
psk_status psk_ctx_synchronize(psk_ctx* ctx);
/* Measurement: bracket the named kernels' launches with HIP events on the ctx stream.
 * kernel in {"sketch_scan","sketch_emit","sketch_sort","screen","anchor","chain_chunk",
 * "select","pair_reduce","anchor_emit","interval"}; "reset" clears the accumulators. psk_ctx_timing synchronises the stream. */
psk_status psk_ctx_set_timing(psk_ctx* ctx, int on);
/* Shader clock the device holds under an integer-VALU load: a fixed ~1 ms micro-kernel (v_alignbit_b32 chains, 4 cycles per
 * wave64 instruction on gfx950) timed with HIP events; *mhz = cycles / duration, *ms = the duration (may be NULL). */
psk_status psk_ctx_clock_probe(psk_ctx* ctx, double* mhz, double* ms);
psk_status psk_ctx_timing(psk_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches);
/* Work of the chain stage since the last reset: pairs that reached chain_seeds (lib.rs:652-653), (pair, query seed) items joined,
 * anchors emitted. The per-kernel algorithmic bytes of bench.py are counted from these. Any pointer may be NULL. */
psk_status psk_ctx_work(psk_ctx* ctx, uint64_t* pairs, uint64_t* items, uint64_t* anchors, int reset);
/* ... and of the joins that go through the database-wide seed index (metagenome contigs, all-vs-all of genomes): query seeds looked up per walk of the index and index
 * entries in the runs the lookups found (what those kernels' algorithmic bytes are counted from: 12 B per lookup, 12 B per entry, 16 B per anchor); while the timers
 * are on (psk_ctx_set_timing) also the candidate chains the selection read and the chunk-table rows the reduce read. Any pointer may be NULL. */
psk_status psk_ctx_join_work(psk_ctx* ctx, uint64_t* lookups, uint64_t* visited, uint64_t* candidates, uint64_t* rows, int reset);
/* Measurement: psk_query_host calls since the context was created that ran as one launch sequence (`taken`), that exceeded one of its
 * capacities and were rerun on the general path (`rerun`), and that went to the general path at once (`general`, which includes `rerun`). */
psk_status psk_ctx_small_query_stats(psk_ctx* ctx, uint64_t* taken, uint64_t* rerun, uint64_t* general);
/* Measurement: batches of the chain stage that were sent round again since the last reset, by cause. `cap`: the anchor total exceeded the optimistically sized
 * anchor arrays; `wide`: a seed with 255 or more matches (or a contig number of 2^23 or more) asked for the wide join format; `onepass`: a pair outgrew its room
 * in the one-walk index join and the batch took the count pass; `refit`: a batch of the two-lane pipeline was handed back to the one-chain loop (a wide request,
 * too many anchors for one launch, or no memory). Read-only: no decision depends on them. Any pointer may be NULL. */
psk_status psk_ctx_rerun_stats(psk_ctx* ctx, uint64_t* cap, uint64_t* wide, uint64_t* onepass, uint64_t* refit, int reset);
/* Measurement: which size tiers of the chain selection and of the per-pair reduce the chain stage launched since the last reset, and how many pairs its selection
 * lists held. out[0..n) receives, in this order (entries beyond the eleventh are zero): launches of select_tiny_kernel, pair_empty_kernel, pair_reduce_tiny_kernel,
 * pair_reduce_small_kernel, pair_reduce_wave_kernel, pair_reduce_kernel and pair_reduce_large_kernel (a batch that is sent round again launches again); then, summed
 * over the completed batches, the pairs in the live list, the pairs the lane-per-pair selection left to the wave kernels, the pairs passed to the second selection tier
 * (more than 512 candidate chains) and to the workgroup tier (more than 1024). Read-only: no decision depends on them. Added after ABI 7 without raising it: a binding
 * detects it by its presence. */
psk_status psk_ctx_tier_stats(psk_ctx* ctx, uint64_t* out, int n, int reset);
/* Measurement: sub-launches of the marker screen since the last reset, by path. out[0..n) receives, in this order (entries beyond the sixth are zero): a workgroup per
 * pair; sliced queries (marker sets above 65 536); the inverted marker index with the count row in LDS, looked up by waves; the same by one lane per marker; the
 * inverted index with the count matrix in HBM; the single query's kernel (psk_screen). Read-only: no decision depends on them. Added after ABI 7 without raising it:
 * a binding detects it by its presence. */
psk_status psk_ctx_screen_stats(psk_ctx* ctx, uint64_t* out, int n, int reset);
/* Host-side 2-bit packing of the ingest pipeline (csrc/pack_host.cpp), exposed for tests: n ASCII bases -> ceil(n / 16) words, the first base in a
 * word's highest two bits; A 0, C 1, G 2, T 3, case-insensitive, every other byte 0 (the codes of the sketch kernels). mode 0: the best
 * implementation the CPU has (AVX-512BW), 1: the scalar one. */
void psk_pack2bit_host(const uint8_t* src, uint64_t n, uint32_t* dst, int mode);
/* device bump allocator for callers that stage genomes in HBM themselves (bench, multi-GPU) */
psk_status psk_device_alloc(psk_ctx* ctx, size_t bytes, void** dptr);
psk_status psk_device_free(psk_ctx* ctx, void* dptr);
psk_status psk_memcpy_h2d(psk_ctx* ctx, void* dst, const void* src, size_t bytes);

/* Sketch one genome from host ASCII contigs. Contigs shorter than 500 are ignored (lib.rs:156). */
psk_status psk_sketch_host(psk_ctx* ctx, const psk_params* p, const uint8_t* const* contigs,
                           const uint64_t* lens, uint32_t n_contigs, int want_seeds,
                           psk_sketch** out);

/* Sketch n_genomes genomes from host ASCII in one call: genome g owns contigs [genome_first_contig[g],
 * genome_first_contig[g+1]) of contigs[]/lens[] (ordinary pageable memory, borrowed for the call). The call is a
 * three-stage pipeline — worker threads copy into pinned staging slots, a copy stream moves the slots over PCIe, the
 * sketch kernels run on the previous sub-batch — so the sustained rate is the host->device link's, not one memcpy
 * thread's ($PSK_INGEST_THREADS, default min(16, cores / 2)). Same result as n_genomes x psk_sketch_host. */
psk_status psk_sketch_many_host(psk_ctx* ctx, const psk_params* p, const uint8_t* const* contigs, const uint64_t* lens,
                                const uint32_t* genome_first_contig, uint32_t n_genomes, int want_seeds,
                                psk_sketch** out);

/* Sketch n_genomes genomes whose ASCII already sits in HBM. d_bases is a device pointer;
 * contig i is bytes [contig_off[i], contig_off[i]+contig_len[i]) of it, contig_off[i] % 16 == 0
 * and the allocation must extend 16 bytes past the last contig. genome g owns contigs
 * [genome_first_contig[g], genome_first_contig[g+1]). out[] receives n_genomes handles. */
psk_status psk_sketch_batch_device(psk_ctx* ctx, const psk_params* p, const uint8_t* d_bases,
                                   const uint64_t* contig_off, const uint64_t* contig_len,
                                   const uint32_t* genome_first_contig, uint32_t n_genomes,
                                   int want_seeds, psk_sketch** out);

void psk_sketch_free(psk_sketch* s);
/* n x psk_sketch_free in one call (a host in an interpreted language pays per call: 100 000 contig sketches) */
void psk_sketch_free_many(psk_sketch* const* sketches, uint32_t n);
psk_status psk_sketch_info(const psk_sketch* s, psk_params* p, uint64_t* n_seeds,
                           uint64_t* n_markers, uint64_t* total_len, uint32_t* n_contigs);
/* copy the sketch back to the host: seeds in (contig,pos) order, markers sorted unique */
psk_status psk_sketch_export(const psk_sketch* s, psk_seed* seeds, uint64_t* markers);

/* kept-contig lengths (n_contigs from psk_sketch_info), needed to serialise a sketch */
psk_status psk_sketch_contig_lens(const psk_sketch* s, uint32_t* lens);
/* Inverse of psk_sketch_export (+ contig lengths): rebuilds a device-resident sketch, e.g. from the records
 * Database.open/load read back (lib.rs:95-122, 249-337). seeds in (contig,pos) order, markers sorted distinct.
 * has_seeds = 0 builds a marker-only sketch (skani::types::Sketch::get_markers_only, lib.rs:495).
 * Markers are 42-bit values (21-mers, two bits a base): one of 2^42 or more is PSK_EINVAL, the message names its index. */
psk_status psk_sketch_import(psk_ctx* ctx, const psk_params* p, const uint32_t* contig_lens, uint32_t n_contigs,
                             const psk_seed* seeds, uint64_t n_seeds, const uint64_t* markers, uint64_t n_markers,
                             int has_seeds, psk_sketch** out);

/* ---- learned-ANI regression (lib.rs:611-614; skani::regression, crate gbdt 0.1.3 at Cargo.lock:1608) ----
 * skani embeds its trained GBDT weights inside the crate, which is not part of the reference tree; a model
 * therefore comes from the caller: either as flat arrays (what a Rust host holding a gbdt::GBDT would pass) or
 * as the serde-JSON text of a gbdt::gradient_boost::GBDT. Inference runs on the GPU, one lane per hit.
 * Tree semantics (gbdt 0.1.3 DecisionTree::predict_one): at an inner node go LEFT iff x[feature] < threshold;
 * a feature equal to PSK_FEATURE_UNKNOWN follows `missing` (-1 left, 0 stop and use this node's value, +1 right);
 * prediction = bias + shrinkage * sum over trees of the reached node's value, accumulated in tree order in f32. */
#define PSK_FEATURE_UNKNOWN (-3.402823466e+38F)   /* gbdt VALUE_TYPE_UNKNOWN = f32::MIN */
typedef struct {
    int32_t feature;    /* index into the model's feature vector */
    float threshold;    /* DTNode.feature_value */
    int32_t left, right;/* node indices relative to the tree's first node */
    float value;        /* DTNode.pred */
    int32_t missing;    /* -1 / 0 / +1 */
    int32_t is_leaf;
    int32_t reserved;
} psk_tree_node;
/* What a model's feature vector is made of. The default vector (features == NULL) is
 * {ANI100, STD100, Q90_QUERY, Q50_QUERY, Q10_QUERY, Q90_REF, Q50_REF, Q10_REF, AVG_CHAIN_LEN}: the fields skani's
 * AniEstResult carries beside the three fractions, as recalled — UNVERIFIED against the absent crate; a model file
 * may name its own order with a top-level "psk_features": ["ani100", "std100", ...] array. */
typedef enum {
    PSK_F_ANI100 = 0,       /* raw chain ANI x 100 */
    PSK_F_STD100 = 1,       /* sample std of the per-chunk ANI estimates x 100 */
    PSK_F_Q90_QUERY = 2, PSK_F_Q50_QUERY = 3, PSK_F_Q10_QUERY = 4,   /* contig-length quantiles: sorted lengths at n*9/10, n/2, n/10 */
    PSK_F_Q90_REF = 5, PSK_F_Q50_REF = 6, PSK_F_Q10_REF = 7,
    PSK_F_AVG_CHAIN_LEN = 8,/* covered bases / kept chains */
    PSK_F_AF_QUERY = 9, PSK_F_AF_REF = 10, PSK_F_N_CHUNKS = 11,
    PSK_F_TOTAL_LEN_QUERY = 12, PSK_F_TOTAL_LEN_REF = 13, PSK_F_N_CONTIGS_QUERY = 14, PSK_F_N_CONTIGS_REF = 15,
    PSK_F_COUNT = 16
} psk_feature;
psk_status psk_model_create(psk_ctx* ctx, const psk_tree_node* nodes, uint64_t n_nodes, const uint32_t* tree_first_node,
                            uint32_t n_trees, float bias, float shrinkage, const int32_t* features, uint32_t n_features,
                            psk_model** out);
psk_status psk_model_load_json(psk_ctx* ctx, const char* json, size_t len, psk_model** out);
psk_status psk_model_load_file(psk_ctx* ctx, const char* path, psk_model** out);
void psk_model_free(psk_model* m);
psk_status psk_model_info(const psk_model* m, uint32_t* n_trees, uint64_t* n_nodes, uint32_t* n_features);
/* evaluate the model on n_rows host rows of n_features floats (GPU evaluation; parity tests and model checks) */
psk_status psk_model_predict(const psk_model* m, const float* rows, uint32_t n_rows, float* out);

/* ---- device-side sketch records: the exchange step of a multi-GPU all-vs-all. A packed sketch is one
 * self-contained, 16-byte aligned byte range of HBM that an RCCL all-gather can move between GPUs as it is;
 * psk_sketch_unpack turns n received records (d_src + offsets[i]) into n sketches sharing one store. Nothing
 * passes through host memory except the 64-byte headers and the contig tables. */
psk_status psk_sketch_pack_size(const psk_sketch* s, uint64_t* bytes);
psk_status psk_sketch_pack(const psk_sketch* s, void* d_dst, uint64_t capacity);
psk_status psk_sketch_unpack(psk_ctx* ctx, const void* d_src, uint64_t capacity, const uint64_t* offsets, uint32_t n, psk_sketch** out);
/* n sketches (of one context) -> n records at d_dst + offsets[i] (16-byte aligned, inside `capacity` bytes): one header upload,
 * one copy launch and one synchronisation for the whole batch */
psk_status psk_sketch_pack_many(const psk_sketch* const* sketches, uint32_t n, void* d_dst, const uint64_t* offsets, uint64_t capacity);

/* ---- multi-GPU exchange. One process per GPU; a psk_comm is this rank's end of an RCCL communicator bound to its
 * context ("one ani_ctx owns its devices and its RCCL communicator", §8b threading row). The path shards by reference
 * (lib.rs:617-657: every (query, ref) pair is independent), so the only collectives are the all-gather of the per-shard hit lists and,
 * for an all-vs-all, the all-gather of the shards' sketches as the query side. librccl.so is loaded at run time: without it every
 * call below returns PSK_ERCCL and the library is otherwise complete (replicas only).
 * Bootstrap: rank 0 calls psk_comm_unique_id, the host program hands the PSK_COMM_ID_BYTES bytes to every rank over any channel
 * it has (MPI, a file, torch.distributed), every rank calls psk_comm_create (collective: returns when all ranks have joined). */
typedef struct psk_comm psk_comm;
#define PSK_COMM_ID_BYTES 128
psk_status psk_comm_unique_id(void* id);
psk_status psk_comm_create(psk_ctx* ctx, int rank, int world, const void* id, psk_comm** out);
void psk_comm_destroy(psk_comm* comm);
/* rank, world, bytes this rank has sent through the communicator and the number of collectives (any may be NULL) */
psk_status psk_comm_info(const psk_comm* comm, int* rank, int* world, uint64_t* bytes_sent, uint64_t* collectives);
/* All-gather of ragged per-shard hit lists (host arrays). Records travel as they are: the caller has put the GLOBAL reference
 * index in ref_index and the global query index in `reserved`. *all (psk_free) = every rank's list in rank order, identical on
 * every rank; counts (world entries, may be NULL) = the ranks' list lengths. */
psk_status psk_gather_hits(psk_comm* comm, const psk_hit* local, uint64_t n_local, psk_hit** all, uint64_t* n_all, uint64_t* counts);
/* ... the same for 20-byte records (the caller has put the global indices in ref_index / query): a quarter of the bytes per link */
psk_status psk_gather_hits_min(psk_comm* comm, const psk_hit_min* local, uint64_t n_local, psk_hit_min** all, uint64_t* n_all, uint64_t* counts);
/* All-gather of device-resident sketches as packed records, HBM -> xGMI -> HBM (no host hop): every rank contributes n sketches
 * and receives everybody's as sketches on ITS GPU. *all (psk_free; each entry psk_sketch_free) = the ranks' sketches in rank
 * order; counts[r] (world entries) = how many came from rank r. */
psk_status psk_gather_sketches(psk_comm* comm, const psk_sketch* const* mine, uint32_t n, psk_sketch*** all, uint32_t* counts);

psk_status psk_db_create(psk_ctx* ctx, const psk_params* p, psk_db** out);
void psk_db_destroy(psk_db* db);
/* takes ownership of s (also on failure) */
psk_status psk_db_add(psk_db* db, const char* name, psk_sketch* s);
/* n x psk_db_add in one call; ownership moves only on PSK_OK */
psk_status psk_db_add_batch(psk_db* db, const char* const* names, psk_sketch* const* sketches, uint32_t n);
uint32_t psk_db_size(const psk_db* db);
const char* psk_db_name(const psk_db* db, uint32_t index);
const psk_sketch* psk_db_sketch(const psk_db* db, uint32_t index);

/* The database's locality order: an internal order of the references in which relatives are neighbours (found on the GPU from the references' marker sets; the seed
 * indexes are laid out by it, so the speed of the index joins does not depend on the order the references were added in). Nothing at this boundary is in that
 * order - indices, names and hits stay in insertion order; this call computes the order if references were added since it was last computed and reports it:
 * slot_of[i] = position of reference i (psk_db_size entries, or NULL), *n_groups = groups of relatives found, *is_identity = 1 when the order is the insertion
 * order (the references' groups were contiguous already, the database fits one index block of 256 references, or $PSK_LOCALITY=0). Any pointer may be NULL. */
psk_status psk_db_locality(psk_db* db, uint32_t* slot_of, uint32_t* n_groups, uint32_t* is_identity);
/* Measurement: the layout of the database's blocked seed index (the index the all-vs-all join walks), as it stands: *bits = width of a block's bucket table (2^bits
 * buckets), *shift = k-mer bits below the bucket (2k - bits), *tagged = 1 when the buckets are fine enough for the walks of the all-vs-all join to match an entry by the
 * k-mer's low byte in its value and read no key (8 bytes per visited entry instead of 12). Builds nothing: all zero until a query has built the index. Any pointer may be
 * NULL. Added after ABI 7 without raising it: a binding detects it by its presence. */
psk_status psk_db_seed_index_info(psk_db* db, int* bits, int* shift, int* tagged);
/* The bucket rule behind it, on the host alone (exposed for tests): for k-mers of 2k bits, a largest block of max_block entries, n_blocks blocks and n_entries entries
 * in all, the bucket-table width and whether the index is tagged. mode: 1 forces tagging, 0 forbids it ($PSK_BSI_TAG), anything else lets the sizes decide: tagged
 * when the bucket tables of max(today's width, 2k - 8) bits are no larger than the 4-byte key array the walks stop reading. Tagged implies 2k - *bits <= 8. */
void psk_bsi_plan(int k, uint64_t max_block, uint32_t n_blocks, uint64_t n_entries, int mode, int* bits, int* tagged);

/* check_markers_quickly(query, ref_i, screen_val, rescue_small) for every ref of the db.
 * pass[i] in {0,1}; shared[i] = |markers(q) ∩ markers(ref_i)| (may be NULL). */
psk_status psk_screen(psk_db* db, const psk_sketch* query, double screen_val, int rescue_small,
                      uint8_t* pass, uint32_t* shared);
/* The screen step of psk_query_many alone: pass[i * psk_db_size + r] in {0,1} for query i and reference r (a host array of n_queries x psk_db_size bytes, insertion
 * order), by the path and the sub-launches psk_query_many would take for these queries ($PSK_SCREEN, $PSK_SCREEN_WAVE, $PSK_SCREEN_GLOBAL as there). Nothing behind
 * the screen runs (no duplicate-name rule, no triangle mask, no seed prefilter), so markers-only sketches are fine. More than 2^30 cells: PSK_ELIMIT. An empty
 * database or n_queries = 0 writes nothing. Added after ABI 7 without raising it: a binding detects it by its presence. */
psk_status psk_screen_many(psk_db* db, const psk_sketch* const* queries, uint32_t n_queries, double screen_val, int rescue_small, uint8_t* pass);

/* chain_seeds(ref, query, map_params) for n_refs references against one query. */
psk_status psk_chain(psk_ctx* ctx, const psk_sketch* const* refs, uint32_t n_refs,
                     const psk_sketch* query, const psk_query_opts* o, psk_hit* out);

/* Database.query: screen, chain the shortlist, keep ani > 0.1. hits in ref insertion order. */
psk_status psk_query(psk_db* db, const psk_sketch* query, const psk_query_opts* o,
                     psk_hit** hits, uint64_t* n_hits);

/* Database.query from the caller's host bytes, as the reference's pymethod runs it (lib.rs:549-660: `_sketch` of the query at
 * :571 - not stored - then the screen / chain closure): contigs[i] is lens[i] ASCII bytes, borrowed for the call; contigs shorter
 * than 500 are ignored (lib.rs:156); seed = the `seed` kwarg (lib.rs:553). Same hits as psk_sketch_host + psk_query + psk_sketch_free.
 * A small genome (one or a few contigs, up to ~90 kb at c = 30 / ~380 kb at c = 125) runs as ONE launch sequence with ONE
 * synchronisation (csrc/small_query.hip); $PSK_SMALL_QUERY=0 keeps every call on the general path (tests, A/B). */
psk_status psk_query_host(psk_db* db, const uint8_t* const* contigs, const uint64_t* lens, uint32_t n_contigs, int seed,
                          const psk_query_opts* o, psk_hit** hits, uint64_t* n_hits);

/* n_queries x Database.query against one database (all-vs-all and metagenome-bin workloads, BASELINE
 * configs[2]/[3]); offsets has n_queries+1 entries, hits of query i are hits[offsets[i]..offsets[i+1]). */
psk_status psk_query_many(psk_db* db, const psk_sketch* const* queries, uint32_t n_queries,
                          const psk_query_opts* o, psk_hit** hits, uint64_t* offsets);
/* psk_query_many returning psk_hit_min records: same hits, same order; `query` of a record = the index of its query in `queries`. The chaining integers of
 * psk_hit stay on the device (what a parity test reads through psk_query_many); a metagenome step's 9.5 M hits are 190 MB instead of 763 MB over PCIe. */
psk_status psk_query_many_min(psk_db* db, const psk_sketch* const* queries, uint32_t n_queries,
                              const psk_query_opts* opts, psk_hit_min** hits, uint64_t* offsets);

/* Triangle mode of the two calls above: one signed 64-bit key per query and one reference base for the database. The pair (query i, reference r - insertion index)
 * is chained iff query_key[i] < 0 or ref_base + r > query_key[i]; a negative key leaves that query as psk_query_many treats it. A database's own triangle - every
 * unordered pair once, no genome against itself, what skani's `triangle` reports - is queries = its sketches in insertion order, query_key[i] = i, ref_base = 0:
 * genome i is the query of every pair (i, j) with j > i. A sharded job passes the queries' GLOBAL indices and its shard's first global index. The mask is laid over
 * the screen's pass matrix on the device (after the duplicate-name rule), so the pairs it removes are never chained, and a hit that remains is the very record of
 * the unmasked call: same order (ascending query, then ref_index), offsets of n_queries + 1 entries. query_key == NULL with n_queries > 0: PSK_EINVAL;
 * ref_base + the database's size beyond 2^63: PSK_ELIMIT. */
psk_status psk_query_many_tri(psk_db* db, const psk_sketch* const* queries, uint32_t n_queries, const int64_t* query_key, uint64_t ref_base,
                              const psk_query_opts* opts, psk_hit** hits, uint64_t* offsets);
psk_status psk_query_many_tri_min(psk_db* db, const psk_sketch* const* queries, uint32_t n_queries, const int64_t* query_key, uint64_t ref_base,
                                  const psk_query_opts* opts, psk_hit_min** hits, uint64_t* offsets);

/* ---- the cluster stage: representatives and clusters from the records of an all-vs-all (csrc/cluster.hip). Dereplication as it is done with skani's `triangle` output:
 * one representative per group of genomes above an ANI / aligned-fraction threshold, every other genome assigned to a representative.
 * Input: n_recs records over n_genomes genomes - a triangle or a full all-vs-all; a pair may appear in either direction, in both, or repeatedly. q = query & 0x7FFFFFFF
 * (bit 31 is the `learned` flag), r = ref_index; an index of n_genomes or more is PSK_EINVAL. A record QUALIFIES iff q != r, ani >= (float)min_ani and the aligned-fraction
 * rule holds - af_rule 0: af_query >= (float)min_af and af_ref >= (float)min_af, 1: one of the two - every comparison in float; a NaN fails its comparison. The unordered
 * pair {q, r} is an EDGE iff one of its records qualifies, and its weight is the largest ani among those.
 * Order: genome a precedes b iff priority[a] > priority[b], or the priorities are equal and a < b; priority == NULL: insertion order, genome 0 first.
 * linkage 0 (greedy): walk the genomes in that order; one with an edge to a representative is a member, any other becomes a representative (the lexicographically-first
 *   maximal independent set). Then every member goes to its adjacent representative of largest weight - any adjacent one, also one that comes after the member in the
 *   order; ties to the earlier representative. rep_of[rep] = rep, rep_ani[rep] = 1; a member's rep_ani is the weight of the edge to its representative.
 * linkage 1 (single): the connected components; rep_of[v] = the component's first genome in the order, rep_ani[v] = 1 for it, else the weight of the direct edge to it, 0
 *   without one.
 * The result is a function of the input alone. recs, priority and the outputs are host memory (rep_of, rep_ani: n_genomes entries); *n_reps = genomes with rep_of[v] == v.
 * n_recs >= 2^30 or n_genomes >= 2^31: PSK_ELIMIT. n_recs == 0: every genome represents itself, without a device call. */
typedef struct {
    double  min_ani;   /* <= 0: 0.95 */
    double  min_af;    /* < 0: 0.5; 0: no aligned-fraction condition */
    int32_t af_rule;   /* 0: both fractions, 1: either */
    int32_t linkage;   /* 0: greedy representatives, 1: single linkage */
} psk_cluster_opts;
psk_status psk_cluster_records(psk_ctx* ctx, const psk_hit_min* recs, uint64_t n_recs, uint32_t n_genomes,
                               const uint64_t* priority /* n_genomes values or NULL */, const psk_cluster_opts* opts,
                               uint32_t* rep_of, float* rep_ani /* may be NULL */, uint32_t* n_reps /* may be NULL */);
/* Measurement: the context's last psk_cluster_records call that reached the device - undirected edges of its graph, greedy rounds that decided a vertex (linkage 0),
 * hook passes that joined two labels (linkage 1). Any pointer may be NULL. */
psk_status psk_ctx_cluster_stats(psk_ctx* ctx, uint64_t* edges, uint64_t* rounds, uint64_t* hook_passes);

/* ---- the linkage forest: the maximum spanning forest of the same ANI graph (csrc/cluster.hip). Its edges in descending weight are the merge sequence of single-linkage
 * agglomeration, and dropping the edges below t leaves exactly the single-linkage clusters at t: one call answers every cut from its floor up.
 * Edges
 *  - Records, qualification, edges and weights are exactly those of psk_cluster_records. q = query & 0x7FFFFFFF, r = ref_index.
 *  - A record qualifies iff q != r, ani >= (float)min_ani and the aligned-fraction rule holds. All comparisons are in float. A NaN fails.
 *  - The unordered pair is an edge iff one of its records qualifies. Its weight is the largest qualifying ani.
 *  - psk_cluster_opts is reused with its defaults (min_ani <= 0: 0.95, min_af < 0: 0.5, min_af == 0: no fraction rule).
 *  - linkage must be 0 or 1 and is otherwise ignored.
 *  - Here min_ani is the FLOOR: the lowest cut the forest can later answer.
 * Edge order
 *  - Write an edge as (a, b, w) with a < b.
 *  - Edge e PRECEDES f iff w_e > w_f, or the weights are bit-equal and (a_e, b_e) < (a_f, b_f) lexicographically.
 *  - This is a strict total order. Edges are deduplicated, so no two share (a, b).
 * The forest
 *  - Walk the edges in that order and keep an edge iff its ends are not yet connected (Kruskal). The edges kept are the forest.
 *  - Under a strict total order the forest is unique. Any correct parallel algorithm returns the same set.
 * Output
 *  - The forest's edges IN THAT ORDER, as three host arrays edge_a[], edge_b[] (with a < b) and edge_ani[].
 *  - edge_ani[] holds the input's float bits. It is never computed.
 *  - Also *n_edges = n_genomes - components.
 *  - The caller provides room for n_genomes - 1 entries each. NULL arrays are allowed when n_genomes <= 1.
 * Refusals and limits
 *  - These are as in psk_cluster_records.
 *  - An index >= n_genomes is PSK_EINVAL with the same message shape, and the context stays usable.
 *  - n_recs >= 2^30 or n_genomes >= 2^31 is PSK_ELIMIT.
 *  - n_recs == 0 gives *n_edges = 0 without a device call. */
psk_status psk_cluster_forest(psk_ctx* ctx, const psk_hit_min* recs, uint64_t n_recs, uint32_t n_genomes,
                              const psk_cluster_opts* opts, uint32_t* edge_a, uint32_t* edge_b, float* edge_ani, uint32_t* n_edges);
/* Measurement: the context's last psk_cluster_forest call that reached the device - undirected edges of its graph, Boruvka rounds that hooked at least one component,
 * pointer-jump launches (those that found something left to do; the launches behind them return at once). Any pointer may be NULL. */
psk_status psk_ctx_forest_stats(psk_ctx* ctx, uint64_t* edges, uint64_t* rounds, uint64_t* jump_passes);

/* ---- confidence intervals of the ANI: skani's --ci, a 5 % - 95 % bootstrap interval resampled from the per-chunk estimates whose mean the ANI is (csrc/interval.hip).
 * The rule is a function of the pair's chunk values, the options and nothing else - not of the batch, lane, round or slot the pair was computed in.
 * Values
 *  - v[0..m) are the values of the chunks that kept a chain, in chunk order, as doubles: pow(min(1, anchors / max(1, seeds - 1)), 1 / k), the reduce stage's own expression.
 * Resampling, for resample b in [0, B) and draw j in [0, m)
 *  - h = mm_hash64(seed + ((uint64)b << 32) + (j >> 1)), a wrap-around 64-bit sum; w = the high word of h for an odd j, the low word for an even one.
 *  - idx = (uint32)(((uint64)w * m) >> 32), and mean_b = (v[idx_0] + v[idx_1] + ... + v[idx_(m-1)]) / m in double, added in draw order.
 * Bounds
 *  - With s the B means in ascending order: ci_lo = (float)s[B / 20], ci_hi = (float)s[B - 1 - B / 20] - s[5] and s[94] for B = 100.
 *  - A pair whose ani_raw is negative (no chunk kept a chain, or below min_aligned_frac): ci_lo = ci_hi = -1.
 *  - Where the regression model produced `ani` (learned == 1), both bounds are moved by ani - ani_raw in float and clamped to [0, 1]: the interval sits around the
 *    number the caller sees. m == 1 gives ci_lo == ci_hi == ani_raw.
 * Refusals, before any device work, PSK_EINVAL: a NULL argument (the options may be NULL), iterations outside {0} and [20, 1024], reserved != 0, and median or robust
 * set in the query options - the interval is defined for the mean estimator. The context stays usable.
 * A call that does not ask for intervals launches nothing of this and returns what it returned before. */
/* psk_chain and the bounds of every pair: out[] is bit-equal to psk_chain's, ci_lo[] / ci_hi[] have n_refs entries. */
psk_status psk_chain_ci(psk_ctx* ctx, const psk_sketch* const* refs, uint32_t n_refs, const psk_sketch* query, const psk_query_opts* o, const psk_ci_opts* ci,
                        psk_hit* out, float* ci_lo, float* ci_hi);
/* psk_query_many_min (query_key == NULL) or psk_query_many_tri_min (query_key given) with psk_hit_ci records: same hits, same order, the five shared fields bit-equal. */
psk_status psk_query_many_ci(psk_db* db, const psk_sketch* const* queries, uint32_t n_queries, const int64_t* query_key, uint64_t ref_base,
                             const psk_query_opts* opts, const psk_ci_opts* ci, psk_hit_ci** hits, uint64_t* offsets);
/* Measurement, since the last reset: pairs that received bounds and draws made for them (summed over the completed batches), and launches of the three size tiers -
 * tier_launches[0] one wave per pair (chunk tables of up to 512 rows), [1] one workgroup per pair (up to 4096 kept values), [2] values in global memory (beyond).
 * Any pointer may be NULL. */
psk_status psk_ctx_interval_stats(psk_ctx* ctx, uint64_t* pairs, uint64_t* draws, uint64_t* tier_launches /* 3 entries */, int reset);
/* Host only, exposed for tests: the draw and the ranks of the rule above, from the inline functions the kernels use. psk_ci_draw: idx of draw j of resample b among m
 * values (m == 0: 0). psk_ci_ranks: *n = the resamples `iterations` stands for (0 -> 100), *lo_rank = n / 20, *hi_rank = n - 1 - n / 20; NULL pointers are skipped. */
uint32_t psk_ci_draw(uint64_t seed, uint32_t b, uint32_t j, uint32_t m);
void psk_ci_ranks(uint32_t iterations, uint32_t* n, uint32_t* lo_rank, uint32_t* hi_rank);

#ifdef __cplusplus
}
#endif
#endif
