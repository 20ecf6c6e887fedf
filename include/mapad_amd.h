/* mapad_amd.h — C ABI of the MI355X-native mapAD read-mapping hot path (libmapad_amd.so).
 *
 * Drop-in boundary for `mapad map` (mpieva/mapAD v0.45.0).  The reference has no FFI today; its internal seam for this
 * path is the generic call k_mismatch_search::<SDM, MB>() made from run_inner (src/map/mapping.rs:153-271) and from
 * Worker::run (src/distributed/worker.rs:80-198), i.e. exactly the worker side of its dispatcher/worker split.  Each
 * entry point below names the reference interface it replaces.  INTEGRATION.md shows the Rust `extern "C"` block a
 * maintainer would add.
 *
 * Conventions: plain pointers and sizes, POD structs, caller-owned inputs, library-owned results released with the
 * matching *_free.  Every function returns 0 on success or a negative mapad_status_t; no exceptions cross the boundary.
 * A context is bound to one GPU and is not re-entrant; use one context per GPU / per host thread.
 * There is NO CPU fallback: without a usable gfx950 device mapad_ctx_create() fails with MAPAD_ERR_NO_DEVICE.
 */
#ifndef MAPAD_AMD_H
#define MAPAD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mapad_status {
    MAPAD_OK = 0,
    MAPAD_ERR_INVALID = -1,      /* bad argument                                  (errors.rs: Error::InvalidInput) */
    MAPAD_ERR_IO = -2,           /* file could not be read / written              (errors.rs: Error::Io)           */
    MAPAD_ERR_INDEX_VERSION = -3,/* on-disk index version != 5                    (versioned_index.rs:31-40)       */
    MAPAD_ERR_PARSE = -4,        /* malformed index / FASTA                       (errors.rs: Error::ParseError)   */
    MAPAD_ERR_NO_DEVICE = -5,    /* no gfx950 GPU / HIP runtime failure (there is no CPU path)                     */
    MAPAD_ERR_DEVICE = -6,       /* a HIP call failed                                                              */
    MAPAD_ERR_NOMEM = -7,
    MAPAD_ERR_READ_TOO_LONG = -8,/* read longer than MAPAD_MAX_READ_LEN = i16::MAX   (record.rs:144-150)             */
    MAPAD_ERR_UNSUPPORTED = -9   /* input beyond a documented limit of this entry point; another entry point takes it */
} mapad_status_t;

#define MAPAD_MAX_READ_LEN 32767

/* ---- parameters: AlignmentParameters + the two plugin enums (src/map/mod.rs:21-31,
 *      sequence_difference_models.rs:67-72, mismatch_bounds.rs:26-30) ------------------------------------------------ */
enum { MAPAD_MODEL_SIMPLE_ADNA = 0, MAPAD_MODEL_VINDIJA_PWM = 1, MAPAD_MODEL_TEST = 2 };
enum { MAPAD_LIBRARY_SINGLE_STRANDED = 0, MAPAD_LIBRARY_DOUBLE_STRANDED = 1 };
enum { MAPAD_BOUND_DISCRETE = 0, MAPAD_BOUND_CONTINUOUS = 1, MAPAD_BOUND_TEST = 2 };

typedef struct mapad_params {
    int32_t model_kind;
    int32_t library_prep;
    float five_prime_overhang, three_prime_overhang; /* double_stranded: five_prime_overhang is the overhang */
    float ds_deamination_rate, ss_deamination_rate;
    float divergence;                                /* already divided by 3 (main.rs:452)                   */
    int32_t ignore_base_quality;
    float deam_score, mm_score, match_score;         /* TestDifferenceModel                                   */
    int32_t bound_kind;
    float poisson_threshold, base_error_rate;        /* Discrete                                              */
    float cutoff, exponent;                          /* Continuous (cutoff already negated, main.rs:467-470)  */
    float threshold, repr_mm_bound;                  /* TestBound                                             */
    float penalty_gap_open, penalty_gap_extend;
    int32_t gap_dist_ends, max_num_gaps_open;
    int32_t stack_limit_abort;
    uint32_t stack_limit, edit_tree_limit;           /* 0 = reference constants 2 000 000 / 10 000 000        */
    uint64_t chunk_size;                             /* --batch_size, default 250 000                         */
} mapad_params_t;

/* build_alignment_parameters (src/main.rs:418-499): CLI-level values -> derived parameters.
 * poisson_prob < 0 selects the Continuous bound with (as_cutoff, as_cutoff_exponent). */
int mapad_params_from_cli(mapad_params_t* out, int library_prep, float five_prime_overhang, float three_prime_overhang,
                          float ds_deamination_rate, float ss_deamination_rate, float divergence, float poisson_prob,
                          float as_cutoff, float as_cutoff_exponent, float indel_rate, float gap_extension_penalty,
                          int gap_dist_ends, int max_num_gaps_open, int ignore_base_quality, int no_search_limit_recovery,
                          uint64_t chunk_size);

/* trait SequenceDifferenceModel (sequence_difference_models.rs:14-62) */
float mapad_sdm_get(const mapad_params_t* p, uint64_t i, uint64_t read_length, uint8_t from, uint8_t to, uint8_t base_quality);
float mapad_sdm_representative_mismatch_penalty(const mapad_params_t* p);
float mapad_sdm_min_penalty(const mapad_params_t* p, uint64_t i, uint64_t read_length, uint8_t to, uint8_t base_quality, int only_mismatches);
int32_t mapad_sdm_alignment_start(const mapad_params_t* p, uint64_t pattern_length);
/* trait MismatchBound (mismatch_bounds.rs:10-20) */
int mapad_mb_reject(const mapad_params_t* p, float value, uint64_t read_length);
int mapad_mb_reject_iterative(const mapad_params_t* p, float value, float reference);
float mapad_mb_remaining_frac_of_repr_mm(const mapad_params_t* p, float value, uint64_t read_length);

/* ---- index: RtFmdIndex + SampledSuffixArray + FastaIdPositions + OriginalSymbols (src/index/mod.rs) ------------------ */
typedef struct mapad_index mapad_index_t;

/* `mapad index` (src/index/indexing.rs:29-212) on an in-memory FASTA-like input: n_contigs sequences (any case, IUPAC).
 * Ambiguous bases in runs shorter than 20 are replaced by a random compatible base drawn like the reference draws it — rand 0.9
 * StdRng::seed_from_u64(seed) + slice.choose(): ChaCha12 keyed through PCG32, index by Canon's method, restated in host_index.hpp and
 * checked against the one draw the reference's integration test pins —, longer runs become 'X'; originals are kept. */
int mapad_index_build(const char* const* names, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n_contigs,
                      uint64_t seed, mapad_index_t** out);
/* The same products (src/index/indexing.rs:163-195: suffix array -> BWT, SA sample, Less, rank structure) with the suffix sorting done on
 * the MI355X `device_id` (prefix doubling over radix sorts, mapad_amd/csrc/index_gpu.hip); byte-identical to mapad_index_build for every
 * input.  Texts up to 2^40 symbols; MAPAD_ERR_NO_DEVICE without a GPU (mapad_index_build is the host path of this offline step). */
int mapad_index_build_gpu(const char* const* names, const uint8_t* const* seqs, const uint64_t* lens, uint32_t n_contigs,
                          uint64_t seed, int device_id, mapad_index_t** out);
/* What the prefix doubling of the most recent mapad_index_build_gpu call of this process did (all zero before the first; a call that
 * failed leaves what it had counted): [0] doubling rounds, [1] unresolved rows before round 1, [2] chunks sorted, [3] chunks cut at the
 * last group head within the chunk limit, [4] chunks cut at the first group head behind it (one group larger than the limit), [5] chunks
 * that took the rest of the list because no head followed, [6] chunks that were the whole remaining list at once, [7] largest chunk
 * in rows, [8] pieces in which the unresolved rows were collected, [9] rows per chunk and [10] elements per sort call in force.
 * The two limits are 2^28 and 2^30; MAPAD_INDEX_DBL_CHUNK / MAPAD_INDEX_SORT_CAP in the environment lower them for one build (test
 * hooks: 64 <= chunk < cap <= 2^30, chunk <= 2^28; anything else fails the build with MAPAD_ERR_PARSE). */
int mapad_last_index_build_info(uint64_t out[16]);
/* load_index_from_path + load_suffix_array/.tpi/.tos (src/index/mod.rs:212-239): reads the 7 files <prefix>.{tbw,tle,toc,trt,tsa,tpi,tos} */
int mapad_index_open(const char* prefix, mapad_index_t** out);
/* writers of indexing.rs:110-208 (snappy frame stream of bincode 1.3, version byte 5) */
int mapad_index_save(const mapad_index_t* idx, const char* prefix);
void mapad_index_free(mapad_index_t* idx);
uint64_t mapad_index_text_len(const mapad_index_t* idx);           /* n = 2|G| + 2 */
int mapad_index_copy_bwt(const mapad_index_t* idx, uint8_t* out);  /* n rank bytes ($=0 A=1 C=2 G=3 T=4 X=5) */
uint32_t mapad_index_n_contigs(const mapad_index_t* idx);
int mapad_index_contig(const mapad_index_t* idx, uint32_t i, const char** name, uint64_t* start, uint64_t* end);
/* SampledSuffixArray pieces, for cross-checks: sizes then copies */
uint64_t mapad_index_sa_sample_len(const mapad_index_t* idx);
uint64_t mapad_index_sa_extra_len(const mapad_index_t* idx);
int mapad_index_copy_sa(const mapad_index_t* idx, uint64_t* sample, uint64_t* extra_rows, uint64_t* extra_vals);

/* the rank structure as the GPU sees it: 64-byte blocks (8 x u64 per 96 BWT rows; layout in mapad_amd/csrc/fmd_device.hpp),
 * less[8] (reference ranks) and the two sentinel rows */
int mapad_index_device_view(const mapad_index_t* idx, const uint64_t** blocks, uint64_t* n_blocks, uint64_t less[8], uint64_t sentinel[2]);
/* SampledSuffixArray::get (src/index/mod.rs:160-187) */
int mapad_index_sa_get(const mapad_index_t* idx, uint64_t row, uint64_t* out);
/* the same for n rows on one host thread (UINT64_MAX for rows past the text): the CPU side of mapad_sa_locate() */
int mapad_index_sa_get_batch(const mapad_index_t* idx, const uint64_t* rows, uint64_t n, uint64_t* out);

/* ---- mapping context: one GPU, index resident in HBM ---------------------------------------------------------------- */
typedef struct mapad_ctx mapad_ctx_t;

int mapad_ctx_create(const mapad_index_t* idx, const mapad_params_t* params, int device_id, mapad_ctx_t** out);
/* MAPAD_GENERAL_DIRECTION=1 (read when a context is created): launch the general search step even for the simple_adna model, whose searches only ever extend
 * backward and which by default gets the kernel compiled for that direction alone (csrc/search_core.hpp: search_step<.., BWD>).  Same results, bit for bit; for
 * comparing the two kernels from one build (tests/test_gpu_bwd.py). */
void mapad_ctx_destroy(mapad_ctx_t* ctx);
/* run every launch on this HIP stream (a hipStream_t; NULL = the default stream) */
int mapad_ctx_set_stream(mapad_ctx_t* ctx, void* hip_stream);

/* Leave the last `n_cus` compute units of the device free of this context's launches (its batch slots' streams get a CU mask; pipeline depth >= 2 only: depth 1
 * runs on the caller's stream).  A search launch fills every CU it may use; RCCL's transfer kernels (248-256 VGPRs, 37.6 KB of LDS per block) only fit on CUs it
 * does not use.  For one-process-per-GPU runs that gather results over xGMI beside the next search; before the first batch.  MAPAD_RESERVED_CUS sets the default. */
int mapad_ctx_set_reserved_cus(mapad_ctx_t* ctx, int n_cus);
/* The heavy tail.  The reference absorbs the reads that run into STACK_LIMIT / EDIT_TREE_LIMIT (src/map/mapping.rs:52-54,1358-1380) on its rayon threads; here a
 * read is handed — by the kernel, while it runs, through host-coherent page-locked memory — to the library's host threads when (a) it has made `pops` pops on the
 * GPU while the host threads keep up (default 2^20; MAPAD_TAIL_POPS; 0 = the host tail is off; MAPAD_TAIL_BACKLOG_BUDGET) — or MAPAD_TAIL_POPS_IDLE pops while a host
 * thread is idle —, (b) it needs a grown arena of a class the GPU has few of and every one is taken, while the host
 * threads have little waiting (MAPAD_TAIL_MIN_CLASS, MAPAD_TAIL_BACKLOG), or (c) no growable arena can hold it (the reads the full-limit stage would restart).
 * The host threads map it from scratch with the kernel's own search step compiled for the host (csrc/host_tail.hpp; MAPAD_TAIL_THREADS threads, default this
 * process's share of the CPUs, divided by LOCAL_WORLD_SIZE when several ranks share a node).  Their results join the batch before its order-preserving collect:
 * nothing a caller sees depends on where a read was finished. */
int mapad_ctx_set_tail_pops(mapad_ctx_t* ctx, uint32_t pops);
/* "This process is one rank of `local_world` on its node": the host tail's worker threads that take reads from now on are this rank's part of the node's CPU share
 * (what LOCAL_WORLD_SIZE / MAPAD_LOCAL_WORLD_SIZE set at start; 0 = back to those).  Process-wide like the worker pool itself; returns the number of workers.
 * The reference's workers each own a whole machine (src/distributed/worker.rs:80-198); eight ranks on one node share its CPUs, and bench.py measures C5 as such a
 * rank on a one-GPU box with this call (`secondary.c5_rank_of_8`). */
uint32_t mapad_tail_set_local_world(uint32_t local_world);
/* the batch selected by mapad_ctx_select_batch, after its collect / fetch: {reads finished on the host, pops the GPU had spent on them, pops on the host,
 * host wall-clock microseconds from the first hand-over to the last result, host threads, pop budget, and the host reads' E_search, N_push, N_node sums
 * (SURVEY 8d events the kernel did not execute), microseconds the host threads spent inside these reads, summed over the threads,
 * [10] hand-overs the host saw while the launch was still running, [11] reads handed over for reason (b), [12] for reason (c), [13] smallest class of (b) | reads handed over below `pops` because a host thread was idle << 32,
 * [14] reads a host thread CONTINUED from the GPU's state (heap and nodes copied out of the read's grown arena) instead of mapping them from scratch, [15] reads
 * the kernel handed over with their state.  For continued reads the pop / event figures above count the host's share only.} */
int mapad_last_tail_info(mapad_ctx_t* ctx, uint64_t out[16]);
/* Duplicate collapsing (default off; MAPAD_COLLAPSE_DUPLICATES=1 sets the default of new contexts).  On: reads of a batch with the same length, the same bases
 * and — unless the parameters ignore base qualities — the same qualities are found on the GPU (a 64-bit key per read, an open-addressing table, then a
 * byte-for-byte comparison: csrc/collapse_core.hpp), only the lowest-indexed read of every such group gets a D array and a search, and its results are copied
 * to the others before the order-preserving collect.  Everything a caller can fetch is bit-identical to what it fetches with collapsing off (the search is
 * deterministic per read); only mapad_last_collapse_info and the kernel times tell the difference.  Within one batch only.  Changing the setting waits for the
 * batches in flight; it holds from the next batch on. */
int mapad_ctx_set_collapse_duplicates(mapad_ctx_t* ctx, int on);
/* the batch selected by mapad_ctx_select_batch: {reads, groups (= reads searched), reads that had a twin (duplicates and their representatives), reads whose
 * key collided with another read's and that the byte comparison kept apart, pops executed (representatives only), microseconds of the grouping kernels,
 * microseconds of the fan-out kernel, 0} — times from HIP events on the batch's stream; [4] and [6] are known once the batch has been collected (fetch /
 * compact), 0 before.  With collapsing off: groups == reads, the rest 0.  Waits for the batch's launch. */
int mapad_last_collapse_info(mapad_ctx_t* ctx, uint64_t out[8]);
/* whether mapad_fetch_result()/mapad_map_batch() also copy the D arrays back (default on; bench.py turns it off) */
int mapad_ctx_set_fetch_d_arrays(mapad_ctx_t* ctx, int on);
/* Score tables are built lazily per read length.  mapad_map_batch() does this itself; before mapad_map_batch_device()
 * (where the host never sees the reads) announce the lengths that will occur. */
int mapad_ctx_prepare_lengths(mapad_ctx_t* ctx, const uint32_t* lens, uint32_t n);

/* HitInterval (src/map/mod.rs:34-61) with the edit track flattened; 40 bytes. */
typedef struct mapad_hit {
    uint64_t lower, lower_rev, size; /* RtBiInterval */
    float alignment_score;
    uint32_t n_ops;                  /* EditOperationsTrack length */
    uint32_t ops_offset;             /* first op in the batch's ops array */
    uint32_t reserved;
} mapad_hit_t;
/* packed EditOperation (src/map/record.rs:225-237): kind<<24 | reference base (ASCII)<<16 | read position;
 * kind 0 Insertion, 1 Deletion, 2 Match, 3 Mismatch */

typedef struct mapad_read_counters { /* algorithm events per read; identical on the CPU oracle */
    uint32_t e_search, e_darray, n_push, n_pop, n_node, n_hits;
} mapad_read_counters_t;

/* Result of one batch == Vec<BinaryHeap<HitInterval>> of run_inner's par_iter (mapping.rs:153-271), order-preserving.
 * hits of read i are hits[hit_begin[i] .. hit_begin[i+1]) in BinaryHeap array order. */
typedef struct mapad_batch_result {
    uint64_t n_reads;
    uint64_t n_hits, n_ops;
    const uint64_t* hit_begin;             /* n_reads + 1 */
    const mapad_hit_t* hits;               /* n_hits */
    const uint32_t* ops;                   /* n_ops */
    const uint32_t* status;                /* per read: 0 ok, 2 stopped by --no_search_limit_recovery */
    const mapad_read_counters_t* counters; /* per read */
    const float* d_arrays;                 /* concatenated BiDArray::d_composite, same offsets as the reads (debug/parity) */
    uint64_t n_second_pass;                /* arena migrations: times a read slot outgrew its arena and moved into a larger size class */
    uint64_t n_third_pass;                 /* reads re-run by the pass that holds the reference's full STACK_LIMIT / EDIT_TREE_LIMIT */
} mapad_batch_result_t;

/* k_mismatch_search over a chunk of reads (host buffers): seqs/quals concatenated, read i = [offsets[i], offsets[i+1]).
 * quals are raw Phred values (no +33). */
int mapad_map_batch(mapad_ctx_t* ctx, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads,
                    mapad_batch_result_t** out);
void mapad_batch_result_free(mapad_batch_result_t* r);

/* Asynchronous variant for a chunk loop that keeps the GPU busy (run_inner's loop, src/map/mapping.rs:151-294, with the next chunk
 * submitted before the previous one is collected): stages the reads (the host buffers may be reused on return), launches on the next of the
 * context's batch slots (mapad_ctx_set_pipeline_depth) and returns.  Collect with mapad_ctx_select_batch + mapad_fetch_result; a fetch that
 * returns MAPAD_ERR_NOMEM (hit pools too small for that chunk) is repaired by running the chunk through mapad_map_batch. */
int mapad_submit_batch(mapad_ctx_t* ctx, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads);
/* page-locked host memory: reads placed here reach the GPU by DMA at link speed (pageable memory goes through the driver's staging copies).
 * Freed blocks are kept for reuse (power-of-two sizes, up to 8 GB): pinning costs milliseconds and hipHostFree waits for the device, which a
 * chunk loop that allocates per chunk cannot afford. */
void* mapad_host_alloc(size_t bytes);
void mapad_host_free(void* p);
/* CPUs this process may really use: the visible CPUs capped by the cgroup's CPU-time quota (cpu.max); MAPAD_HOST_CPUS overrides.  What the library's own host
 * thread pools (host tail, record strings, index preparation) size themselves by, and what a caller's pools beside them should (csrc/host_cpus.hpp). */
unsigned mapad_host_cpus(void);

/* Device-resident variant used by bench.py and the multi-GPU driver: inputs already in HBM (device pointers), results stay
 * in the context's device buffers until fetched.  Asynchronous on the context's stream.
 * The three input buffers are read in place, not copied: they must stay untouched until the batch has been collected (mapad_fetch_result,
 * mapad_compact_result_device, mapad_records_device) and, while an accumulator stage is on (damage profile or score, coverage, pileup, ...), until it has
 * been converted — the stages read the reads at conversion time.
 * Ordering: work queued on the context's stream (mapad_ctx_set_stream) before a submission — the uploads of these very buffers, a consumer of the results of
 * the batch that used the same batch slot before — is complete before that slot's launch begins, at every pipeline depth. */
int mapad_map_batch_device(mapad_ctx_t* ctx, const void* d_seqs, const void* d_quals, const void* d_offsets, uint64_t n_reads,
                           uint32_t max_read_len);
/* Batches in flight.  With depth d > 1 the context keeps d sets of batch buffers and streams of its own: mapad_map_batch_device rotates
 * through them and returns as soon as the batch is enqueued (it waits only for the batch that used the same set d calls ago), so the serial
 * tail of batch k — its few heaviest reads, each a chain of dependent memory accesses — runs beside the bulk of batch k + 1, the way the
 * reference's worker threads start the next chunk while stragglers finish (src/map/mapping.rs:151-156).  Inputs are ordered behind the
 * context's stream (mapad_ctx_set_stream) at submission.  Default 1 (MAPAD_PIPELINE_DEPTH overrides): everything runs on the context's stream.
 * Changing the depth waits for all batches and drops their results. */
int mapad_ctx_set_pipeline_depth(mapad_ctx_t* ctx, int depth);
/* Allocates, for every batch slot, the device buffers of batches of up to n_reads reads / total_bases bases / reads up to max_read_len long
 * (host_inputs != 0: also the staging buffers of mapad_map_batch / mapad_submit_batch).  Optional: buffers grow on demand, but an allocation in
 * the middle of a pipeline waits for the kernels that are running. */
int mapad_ctx_reserve(mapad_ctx_t* ctx, uint64_t n_reads, uint64_t total_bases, uint32_t max_read_len, int host_inputs);
/* result accessors (fetch, compact, counters, kernel times, device pointers) read the batch submitted `age` calls before the most recent
 * one (0 = most recent; reset to 0 by every submission) */
int mapad_ctx_select_batch(mapad_ctx_t* ctx, int age);
/* HIP-event time stamps of every launch since the last call (waits for all batches): 4 floats per launch = ms from the start of the first
 * launch to {start of the D-array kernel, end of D arrays + ordering, end of the growable search stages, end of the full-limit stage}.
 * Returns the number of launches in *n (at most `cap` are written). */
int mapad_kernel_history(mapad_ctx_t* ctx, float* out, uint32_t cap, uint32_t* n);
/* after synchronising the stream: copy the last device batch's results to the host */
int mapad_fetch_result(mapad_ctx_t* ctx, mapad_batch_result_t** out);
/* Order-preserving collect (src/map/mapping.rs:288) on the device: lays the last batch's hits and edit operations out in read order and
 * returns device pointers to hit_begin (u64[n_reads + 1], exclusive prefix sums), the hit records (mapad_hit_t[n_hits], ops_offset into
 * the ops array) and the ops (u32[n_ops]) — the arrays mapad_fetch_result copies out and the multi-GPU gather sends to rank 0.
 * Valid until the next batch.  Launches on the context's stream; returns without waiting for it. */
int mapad_compact_result_device(mapad_ctx_t* ctx, void** d_hit_begin, void** d_hits, void** d_ops, uint64_t* n_hits, uint64_t* n_ops);
/* device pointers of the last batch's raw result buffers (for the RCCL gather): per-read hit counts (u32[n_reads]),
 * per-read first-hit index (u32[n_reads]), hit pool (mapad_hit_t[]), ops pool (u32[]), 2 x u64 cursors {n_hits, n_ops}.
 * With duplicate collapsing on the pools and cursors hold the representatives' hits only: after the collect a duplicate's count and first-hit index alias
 * its representative's pool entries, before it they are undefined.
 * This call orders nothing: it returns addresses.  The contents are the batch's once its launch has finished — synchronise the context's stream (depth 1) or
 * collect the batch first; work queued on the context's stream is NOT ordered behind the launch by this call, as it is by mapad_compact_result_device. */
int mapad_device_result_ptrs(mapad_ctx_t* ctx, void** d_hit_count, void** d_hit_first, void** d_hits, void** d_ops, void** d_cursors);
/* sums of the per-read counters of the last batch (after a fetch or a stream sync): {e_search, e_darray, n_push, n_pop, n_node, n_hits}.
 * With duplicate collapsing on these stay sums over all reads as fetched, duplicates included: the events of the work the batch stands for (what bench.py
 * derives algorithmic bytes from), not of the work done — that is mapad_last_collapse_info's [4]. */
int mapad_last_batch_counters(mapad_ctx_t* ctx, uint64_t out[6]);
/* HIP-event durations (ms) of the last batch's launches on the context's stream: {darray_kernel + the two ordering kernels,
 * search_kernel over every read + its (normally empty) retry launches, full-limit search_kernel}.  Synchronises on the last event. */
int mapad_last_kernel_ms(mapad_ctx_t* ctx, float out[3]);
/* launch geometry of the last batch, for bench.py's report: {darray grid, block, LDS bytes, search grid, block, full-limit grid,
 * base arena node capacity, base arena KiB per read slot} */
int mapad_last_launch_info(mapad_ctx_t* ctx, uint32_t out[8]);

/* ---- post-search: intervals_to_bam minus BAM byte encoding (mapping.rs:402-718, record.rs:269-449) ------------------- */
typedef struct mapad_record {
    uint16_t flags;
    uint8_t mapq;
    uint8_t mapped, reverse;
    int32_t tid;
    int64_t pos;          /* 0-based leftmost position, -1 if unmapped */
    float as_score, xs_score;
    int32_t nm, x0, x1;
    uint8_t has_xs;
    char xt;
    uint32_t cigar_off, cigar_len, md_off, md_len, xa_off, xa_len; /* into the text blob */
} mapad_record_t;
typedef struct mapad_records {
    uint64_t n;
    const mapad_record_t* recs;
    const char* text;
    uint64_t text_len;
} mapad_records_t;
/* in_flags: input BAM flags per read (NULL = 0, i.e. FASTQ input, record.rs:207-213); seed: stands in for rand::rng()
 * (mapping.rs:273,605; only matters for hits with >= 3 SA rows) */
int mapad_hits_to_records(const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                          const uint8_t* quals, const uint64_t* offsets, const uint16_t* in_flags, uint64_t seed, mapad_records_t** out);
void mapad_records_free(mapad_records_t* r);
/* The seed to pass for a slice of a chunk that starts at read `first_read_index`, such that every read draws the same stand-in for
 * rng.next_u32() (src/map/mapping.rs:605-607) as it would if the whole chunk were converted by one call with `seed`. */
uint64_t mapad_records_seed_at(uint64_t seed, uint64_t first_read_index);

/* ---- SA locate on the device ---------------------------------------------------------------------------
 * SampledSuffixArray::get (src/index/mod.rs:160-187) for a batch of BWT rows: LF walk to the next sampled row (or '$' row) in a
 * kernel, one quad per row, against the index blocks already resident in HBM.  rows / out are host arrays; out[i] = suffix-array
 * value, UINT64_MAX for a row >= text length.  Results are identical to mapad_index_sa_get(). */
int mapad_sa_locate(mapad_ctx_t* ctx, const uint64_t* rows, uint64_t n, uint64_t* out);
/* kernel time (HIP events on the context's stream), rows and LF steps of the last locate call */
int mapad_last_locate_info(mapad_ctx_t* ctx, float* kernel_ms, uint64_t* rows, uint64_t* lf_steps);
/* mapad_hits_to_records() with the suffix-array lookups of all hit intervals of <= 8 rows done by mapad_sa_locate's kernel first
 * (interval2coordinate, mapping.rs:590-649, is the second random-access loop of the reference); same records, uses the context's
 * index and parameters.  `res` may be a result of this context that has not been freed (its hits are then read where the collect left them
 * on the device), a result of another context, or a struct the caller has filled in itself (hit_begin, hits, ops: they are uploaded first). */
int mapad_hits_to_records_gpu(mapad_ctx_t* ctx, const mapad_batch_result_t* res, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets,
                              const uint16_t* in_flags, uint64_t seed, mapad_records_t** out);

/* The same in two calls, for a chunk loop whose GPU thread should not spend its time on strings: mapad_hits_to_coords_gpu() is the device half
 * (which hit is reported, its coordinate, the XA candidates, X0 / X1: one kernel over the hits that are still resident on the device, one small copy back);
 * mapad_coords_to_records() is the host half (flags, CIGAR / MD / XA text, XS / XT, mapping quality) — it needs no context and may run on any thread
 * while the GPU thread goes on submitting and fetching.  Together they return exactly what mapad_hits_to_records_gpu() returns. */
/* The same products left on the device, for the batch selected by mapad_ctx_select_batch (its collect is done first): per read one 88-byte record
 * {i64 pos; i32 tid; u32 mapped, reverse; f32 as, xs; i32 nm, x0, x1; u32 has_xs, xt, text_off, cigar_len, md_len, xa_len; f32 best_size; u32 read_len, mq_off, mq_n, error}
 * (csrc/text_core.hpp: DevRecord), the text pool ([CIGAR][MD][XA] of a read behind its text_off) and the pool of (score, size) f32 pairs the mapping
 * quality is computed from (mq_n pairs behind mq_off) — what a rank sends to rank 0 in the multi-GPU gather (<= 128 bytes per read; the
 * reference's ResultSheet return path, src/distributed/dispatcher.rs:223-247).  Valid until the batch slot is launched again.  Flags and MAPQ are
 * finished on the host (mapad_coords_to_records' arithmetic: glibc exp2f / log10f). */
int mapad_records_device(mapad_ctx_t* ctx, uint64_t seed, void** d_records, void** d_text, void** d_pairs, uint64_t* text_bytes, uint64_t* n_pairs);
typedef struct mapad_coords mapad_coords_t;
int mapad_hits_to_coords_gpu(mapad_ctx_t* ctx, const mapad_batch_result_t* res, uint64_t seed, mapad_coords_t** out);
int mapad_coords_to_records(const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint16_t* in_flags,
                            const mapad_coords_t* coords, mapad_records_t** out);
void mapad_coords_free(mapad_coords_t* c);

/* ---- damage profile: reference base -> read base counts by distance from the read's ends (csrc/damage_core.hpp) ----------------
 * Opt-in; with it off (the default) nothing is launched or allocated.  On: every records call on a batch whose hits AND reads are still on the
 * device (mapad_hits_to_records_gpu / mapad_hits_to_coords_gpu on a result this context fetched and has not launched over since, mapad_records_device)
 * also runs damage_kernel behind records_kernel and adds the batch into a table the context keeps on the device.  A read counts iff it is reported
 * mapped (mode 2: and X0 == 1, i.e. XT:U); of its reported alignment every match / mismatch column with both bases in ACGT adds 1 to
 * counts[0][p][ref][read] (p = 0-based distance from the 5' end, if < 32) and to counts[1][L - 1 - p][ref][read] (distance from the 3' end, if < 32),
 * bases in read orientation, on the text as searched (ambiguity codes restored in MD are not consulted).  A batch counts once however often it is
 * converted.  After mapad_map_batch_device the caller's read buffers must stay valid until the batch has been converted.
 * With the profile on, a records call on hits that have to be uploaded (an older or foreign result: their reads are not on the device) returns
 * MAPAD_ERR_UNSUPPORTED instead of leaving the batch uncounted; mapad_damage_profile_host takes such results. */
#define MAPAD_DAMAGE_POSITIONS 32
typedef struct mapad_damage_profile {
    uint64_t counts[2][MAPAD_DAMAGE_POSITIONS][4][4]; /* [0 = from 5', 1 = from 3'][distance][ref A,C,G,T][read A,C,G,T] */
    uint64_t reads;         /* reads counted */
    uint64_t reads_seen;    /* reads of the batches counted */
    uint64_t aligned_bases; /* columns counted, whatever their distance from the ends */
    uint64_t skipped_bases; /* match / mismatch columns with a base outside ACGT */
    uint64_t insertions, deletions, batches;
    double kernel_ms;       /* HIP-event time of damage_kernel, summed over the batches */
} mapad_damage_profile_t;
/* 0 off (default; MAPAD_DAMAGE_PROFILE sets the default of new contexts), 1 all mapped reads, 2 X0 == 1 only.  Changing the mode waits for the batches in
 * flight and starts an empty table. */
int mapad_ctx_set_damage_profile(mapad_ctx_t* ctx, int mode);
/* waits for the batches in flight, copies the table */
int mapad_ctx_damage_profile(mapad_ctx_t* ctx, mapad_damage_profile_t* out);
/* zeroes the table: nothing has been counted (a batch still resident counts again if it is converted again) */
int mapad_ctx_damage_profile_reset(mapad_ctx_t* ctx);
/* host path, no GPU: the same core over a result, with the host's record_coords under `seed` (the seed of the records call); mode 1 or 2; ADDS into *acc
 * (zero it first; kernel_ms is left alone) */
int mapad_damage_profile_host(const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                              const uint64_t* offsets, uint64_t seed, int mode, mapad_damage_profile_t* acc);

/* ---- depth of coverage: per-base depth and per-contig breadth of the reported alignments (csrc/coverage_core.hpp) -----------------------------
 * Opt-in like the damage profile, and counted at the same place: with it off (the default) nothing is launched or allocated.  On: every records call on a
 * batch whose hits are still on the device also runs coverage_kernel behind records_kernel and adds the batch into an int32 difference array over the
 * forward strand's text positions (4 bytes per position, n / 2 + 1 of them) that the context keeps on the device.  A read counts iff it is reported mapped
 * (mode 2: and X0 == 1, i.e. XT:U); of its reported alignment every match / mismatch column covers its reference base, deleted reference bases are not
 * covered, insertions touch nothing (samtools depth without -J).  A batch counts once however often it is converted.  The summary (per-contig covered
 * bases, depth sum and maximum; the depth histogram over all contig positions) and the per-base depth of a window are computed on the device on demand and
 * leave the array as it is.  With coverage on, a records call on hits that have to be uploaded returns MAPAD_ERR_UNSUPPORTED (whether that batch was counted
 * before cannot be known); mapad_coverage_host_add takes such results. */
#define MAPAD_COVERAGE_BINS 256
typedef struct mapad_coverage_contig {
    uint64_t length, reads, covered_bases, depth_sum, max_depth; /* reads: counted reads reported on it; covered_bases: positions of depth >= 1 */
} mapad_coverage_contig_t;
typedef struct mapad_coverage {
    uint32_t n_contigs;               /* in: entries `contigs` has room for (>= mapad_index_n_contigs); out: entries filled */
    uint32_t pad;
    mapad_coverage_contig_t* contigs; /* caller-provided, index order */
    uint64_t hist[MAPAD_COVERAGE_BINS]; /* contig positions by depth; the last bin is depth >= 255 */
    uint64_t reads;                   /* reads counted */
    uint64_t reads_seen;              /* reads of the batches counted */
    uint64_t covered_columns;         /* match / mismatch operations counted (= the sum of depth_sum over the contigs) */
    uint64_t deleted_columns, insertions, batches;
    double accumulate_ms;             /* HIP-event time of coverage_kernel, summed over the batches (the host path leaves it 0) */
    double summary_ms;                /* HIP-event time of this summary's finishing pass */
} mapad_coverage_t;
/* 0 off (default; MAPAD_COVERAGE sets the default of new contexts), 1 all mapped reads, 2 X0 == 1 only.  Changing the mode waits for the batches in flight and
 * starts an empty table.  The array is allocated at the first switch-on: MAPAD_ERR_NOMEM if it does not fit. */
int mapad_ctx_set_coverage(mapad_ctx_t* ctx, int mode);
/* waits for the batches in flight, runs the finishing pass (contigs cut into segments of MAPAD_COVERAGE_SEGMENT positions, a test hook; default 16384).
 * MAPAD_ERR_DEVICE if the array violates its invariants (depth negative, not 0 outside the contigs, or a total other than 0) instead of a wrong table. */
int mapad_ctx_coverage(mapad_ctx_t* ctx, mapad_coverage_t* out);
/* per-base depth of [from, from + n) of contig tid (0-based) into out[n] */
int mapad_ctx_coverage_depth(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, uint32_t* out);
/* zeroes the table: nothing has been counted (a batch still resident counts again if it is converted again) */
int mapad_ctx_coverage_reset(mapad_ctx_t* ctx);
/* adds src's accumulator into dst's (same index, same non-zero mode: MAPAD_ERR_INVALID otherwise); src keeps its own.  How the tables of several devices become
 * one: the summary is not additive, the difference array is. */
int mapad_ctx_coverage_merge(mapad_ctx_t* dst, mapad_ctx_t* src);
/* host path, no GPU: the same core over fetched results, with the host's record_coords under `seed` (the seed of the records call); mode 1 or 2 */
typedef struct mapad_coverage_host mapad_coverage_host_t;
int mapad_coverage_host_new(const mapad_index_t* idx, int mode, mapad_coverage_host_t** acc);
int mapad_coverage_host_add(mapad_coverage_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, uint64_t seed);
int mapad_coverage_host_summary(const mapad_coverage_host_t* acc, mapad_coverage_t* out);
int mapad_coverage_host_depth(const mapad_coverage_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, uint32_t* out);
void mapad_coverage_host_free(mapad_coverage_host_t* acc);

/* ---- pileup: A/C/G/T counts per reference position and consensus calls of the reported alignments (csrc/pileup_core.hpp) -------------------------------
 * Opt-in like the damage profile and the coverage, and counted at the same place: with it off (the default) nothing is launched or allocated.  On: every
 * records call on a batch whose hits AND reads are still on the device also runs pileup_kernel behind records_kernel and adds the batch into
 * uint32 counts[n / 2][4] (A, C, G, T; forward-strand bases; 16 bytes per forward-strand text position: 48 GB at 3 Gbp) that the context keeps on the device
 * while the mode is non-zero.  A read counts iff it is reported mapped (mode 2: and X0 == 1, i.e. XT:U); of its reported alignment every match / mismatch
 * column goes to exactly one of columns_not_acgt (the read's base is none of ACGT), columns_masked (within mask5 bases of the read's 5' end or mask3 of its
 * 3' end, the read as given), columns_low_quality (raw Phred below min_base_quality) or the cell of its position and forward-strand base
 * (columns_counted); deleted reference bases and insertions count in deleted_columns / insertions only.  A cell wraps at 2^32 (not checked).  A batch counts
 * once however often it is converted.  The call of a position, with d the sum of its four counts and best the largest: that base iff d >= min_depth,
 * best * 100 >= min_percent * d and the maximum is unique, else N — integers only, computed on the device on demand; the counts stay as they are.
 * With the pileup on, a records call on hits that have to be uploaded (their reads are not on the device) returns MAPAD_ERR_UNSUPPORTED;
 * mapad_pileup_host_add takes such results.  After mapad_map_batch_device the caller's read buffers must stay valid until the batch has been converted. */
typedef struct mapad_pileup_contig {
    uint64_t length;
    uint64_t sites_covered; /* positions of depth >= 1 */
    uint64_t sites_deep;    /* positions of depth >= min_depth */
    uint64_t sites_called;  /* positions whose call is not N */
    uint64_t called[4];     /* calls by base: A, C, G, T */
    uint64_t base_sum[4];   /* the sum of the counts by base: A, C, G, T */
    uint64_t max_depth;
} mapad_pileup_contig_t;
typedef struct mapad_pileup {
    uint32_t n_contigs;             /* in: entries `contigs` has room for (>= mapad_index_n_contigs); out: entries filled */
    uint32_t pad;
    mapad_pileup_contig_t* contigs; /* caller-provided, index order */
    uint32_t mode, min_base_quality, mask5, mask3; /* out: what the counts were taken under (mode 0: the pileup is off, everything else is 0) */
    uint32_t min_depth, min_percent;               /* out: the call rule of this summary */
    uint64_t reads;                 /* reads counted */
    uint64_t reads_seen;            /* reads of the batches counted */
    uint64_t columns_counted;       /* = the sum of base_sum over the contigs */
    uint64_t columns_not_acgt, columns_masked, columns_low_quality;
    uint64_t deleted_columns, insertions, batches;
    double accumulate_ms;           /* HIP-event time of pileup_kernel, summed over the batches (the host path leaves it 0) */
    double summary_ms;              /* HIP-event time of this summary's pileup_call_kernel launches */
} mapad_pileup_t;
/* mode 0 off (default) — frees the array —, 1 all mapped reads, 2 X0 == 1 only; min_base_quality 0..255, mask5 / mask3 0..65535.  MAPAD_PILEUP=1|2 with
 * MAPAD_PILEUP_MIN_BQ, MAPAD_PILEUP_MASK5 and MAPAD_PILEUP_MASK3 set the default of new contexts.  Changing the mode or a filter waits for the batches in
 * flight and starts an empty table (a table holds the counts of one setting).  The array is allocated at the switch-on: MAPAD_ERR_NOMEM if it does not fit. */
int mapad_ctx_set_pileup(mapad_ctx_t* ctx, int mode, uint32_t min_base_quality, uint32_t mask5, uint32_t mask3);
/* waits for the batches in flight, runs pileup_call_kernel over every contig; min_depth >= 1, min_percent 0..100 (MAPAD_ERR_INVALID otherwise).  Off: zeroes.
 * MAPAD_ERR_DEVICE if pileup_kernel met an alignment that leaves the text. */
int mapad_ctx_pileup(mapad_ctx_t* ctx, uint32_t min_depth, uint32_t min_percent, mapad_pileup_t* out);
/* the counts of [from, from + n) of contig tid (0-based) into out[n][4]: A, C, G, T */
int mapad_ctx_pileup_counts(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, uint32_t* out);
/* the calls of [from, from + n) of contig tid into out[n]: 'A', 'C', 'G', 'T' or 'N' */
int mapad_ctx_pileup_consensus(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, uint32_t min_depth, uint32_t min_percent, uint8_t* out);
/* zeroes the table: nothing has been counted (a batch still resident counts again if it is converted again) */
int mapad_ctx_pileup_reset(mapad_ctx_t* ctx);
/* adds src's counts into dst's (same index, same non-zero mode, same filters: MAPAD_ERR_INVALID otherwise); src keeps its own.  How the tables of several
 * devices become one before the calls are made. */
int mapad_ctx_pileup_merge(mapad_ctx_t* dst, mapad_ctx_t* src);
/* host path, no GPU: the same core over fetched results and the reads they are of, with the host's record_coords under `seed` (the seed of the records
 * call); mode 1 or 2.  16 bytes of host memory per forward-strand text position. */
typedef struct mapad_pileup_host mapad_pileup_host_t;
int mapad_pileup_host_new(const mapad_index_t* idx, int mode, uint32_t min_base_quality, uint32_t mask5, uint32_t mask3, mapad_pileup_host_t** acc);
int mapad_pileup_host_add(mapad_pileup_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                          const uint8_t* quals, const uint64_t* offsets, uint64_t seed);
int mapad_pileup_host_summary(const mapad_pileup_host_t* acc, uint32_t min_depth, uint32_t min_percent, mapad_pileup_t* out);
int mapad_pileup_host_counts(const mapad_pileup_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, uint32_t* out);
int mapad_pileup_host_consensus(const mapad_pileup_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, uint32_t min_depth, uint32_t min_percent, uint8_t* out);
void mapad_pileup_host_free(mapad_pileup_host_t* acc);

/* ---- PCR duplicates by alignment coordinates (csrc/dedup_core.hpp) ---------------------------------------------------------------------------------
 * Opt-in like the three analyses above and run at the same place, in front of them: with it off (the default) nothing is launched or allocated and every
 * output is what it was.  On: every records call on a batch whose hits are still on the device also runs dedup_insert_kernel and dedup_mark_kernel behind
 * records_kernel.  A read is eligible iff it is reported mapped; its key is (absolute start, reference span, strand) of the reported alignment — exact, no
 * hash.  Every read has an ordinal: the reads of the batches marked before its own (batches are marked in the order in which they are converted) plus its
 * index in the batch.  Of all eligible reads seen so far under one key the lowest ordinal is the original, every other one a duplicate: its
 * mapad_record_t.flags get 0x400 on top of in_flags.  The flagged set does not depend on how the input is cut into batches.  The keys live in an
 * open-addressing table on the device (32 bytes per slot, at most half full: 8 GiB at 100 M fragments) that grows by rehashing; growing waits for the
 * batches in flight, and MAPAD_ERR_NOMEM leaves the old table intact.  MAPAD_DEDUP_SLOTS (a test hook) sets the initial slot count; default: sized for the
 * first batch.  A batch converted again gets the flags of its first conversion and changes nothing.  With the mode on, a records call on hits that have to
 * be uploaded returns MAPAD_ERR_UNSUPPORTED; mapad_dedup_host_add takes such results.  mapad_records_device (the multi-GPU gather) marks but does not
 * carry the flags: a table per device cannot see the other devices' reads. */
#define MAPAD_DUPLICATES_BINS 256
typedef struct mapad_duplicates {
    uint64_t reads_seen;      /* reads of the batches marked */
    uint64_t reads_eligible;  /* ... that are reported mapped */
    uint64_t duplicates;      /* ... that are flagged */
    uint64_t fragments;       /* distinct keys = occupied slots (reads_eligible - duplicates) */
    uint64_t slots;           /* the table's size */
    uint64_t grows;           /* times it was rehashed into a larger one */
    uint64_t batches;
    uint64_t histogram[MAPAD_DUPLICATES_BINS]; /* bin k: fragments seen k times; the last bin is >= 255 */
    double mark_ms;           /* HIP-event time of dedup_insert_kernel + dedup_mark_kernel, summed over the batches (a growth's rehash is not in it; the host path leaves it 0) */
    double summary_ms;        /* HIP-event time of this read-out's dedup_hist_kernel */
} mapad_duplicates_t;
/* 0 off (default; MAPAD_MARK_DUPLICATES=1|2 sets the default of new contexts), 1 marks, 2 marks and leaves the duplicates out of the damage profile, the
 * coverage and the pileup (they still count in those tables' reads_seen).  Changing the mode waits for the batches in flight and starts an empty table;
 * mode 0 frees it. */
int mapad_ctx_set_mark_duplicates(mapad_ctx_t* ctx, int mode);
/* waits for the batches in flight, runs dedup_hist_kernel.  Off: zeroes.  MAPAD_ERR_DEVICE if a kernel met a coordinate that does not fit the key. */
int mapad_ctx_duplicates(mapad_ctx_t* ctx, mapad_duplicates_t* out);
/* empties the table (it keeps its size): nothing has been seen, ordinals start at 0 (a batch still resident is marked again if it is converted again) */
int mapad_ctx_duplicates_reset(mapad_ctx_t* ctx);
/* host path, no GPU: the same core over fetched results in the order in which they are added, with the host's record_coords under `seed` (the seed of the
 * records call).  _add writes the batch's flags (1 = duplicate) into flags[res->n_reads]. */
typedef struct mapad_dedup_host mapad_dedup_host_t;
int mapad_dedup_host_new(mapad_dedup_host_t** acc);
int mapad_dedup_host_add(mapad_dedup_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, uint64_t seed, uint8_t* flags);
int mapad_dedup_host_summary(const mapad_dedup_host_t* acc, mapad_duplicates_t* out);
void mapad_dedup_host_free(mapad_dedup_host_t* acc);
/* the three host accumulators with a per-read skip array (1 = leave the read out, as mode 2 does on the device; NULL = none): what the functions without
 * _skip call */
int mapad_damage_profile_host_skip(const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                                   const uint64_t* offsets, uint64_t seed, int mode, const uint8_t* skip, mapad_damage_profile_t* acc);
int mapad_coverage_host_add_skip(mapad_coverage_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, uint64_t seed,
                                 const uint8_t* skip);
int mapad_pileup_host_add_skip(mapad_pileup_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                               const uint8_t* quals, const uint64_t* offsets, uint64_t seed, const uint8_t* skip);

/* ---- damage score: per-read log-likelihood ratio of the damage model against the same model without damage (csrc/dscore_core.hpp) --------------------
 * Opt-in like the analyses above and run at the same place, behind the duplicate marking and in front of the three tables: with it off (the default) nothing
 * is launched, allocated or built and every output is what it was.  On: every records call on a batch whose hits are still on the device also runs
 * dscore_kernel behind records_kernel.  A read is scored iff it is reported mapped; its score is the sum, over the aligned columns of the reported alignment
 * whose (reference base, read base) is C->C, C->T, G->G or G->A in read orientation, of sdm_get - sdm_get_null at that position and base quality, each term
 * rounded ON THE HOST to 1/256 bit (int16, saturating) when the read length's table is built.  score_q is that integer sum, the score score_q / 256 bits;
 * device and host agree bit for bit.  Positive: the read's C->T / G->A pattern is better explained with damage (-f / -t / -d / -s) than without.
 * Mode 2 leaves the scored reads with score_q < threshold_q = (int32)ceilf(threshold * 256) out of the damage profile, the coverage and the pileup (they
 * still count in those tables' reads_seen); with mark-duplicates mode 2 the duplicates are left out as well.  The score needs no state across reads: every
 * device of a multi-GPU run scores its own reads, the summaries add.  A batch converted again returns the same scores and adds nothing to the summary.  With
 * the mode on, a records call on hits that have to be uploaded returns MAPAD_ERR_UNSUPPORTED; mapad_damage_score_host takes such results.
 * mapad_records_device (the multi-GPU gather) scores but does not carry the scores. */
#define MAPAD_DAMAGE_SCORE_BINS 128
typedef struct mapad_damage_scores {
    uint64_t reads_seen;           /* reads of the batches scored */
    uint64_t reads_scored;         /* ... that are reported mapped */
    uint64_t reads_below;          /* ... with score_q < threshold_q (whatever the mode) */
    uint64_t informative_columns;  /* C->C, C->T, G->G, G->A columns of the scored reads */
    int64_t score_sum;             /* sum of score_q over the scored reads */
    uint64_t batches;
    int32_t threshold_q;
    int32_t pad;
    uint64_t histogram[MAPAD_DAMAGE_SCORE_BINS]; /* scored reads by score, half a bit per bin: bin = (clamp(score_q, -8192, 8191) + 8192) >> 7; bin 64 starts at 0 */
    double kernel_ms;              /* HIP-event time of dscore_kernel, summed over the batches (the host path leaves it 0) */
} mapad_damage_scores_t;
/* 0 off (default; MAPAD_DAMAGE_SCORE=1|2 and MAPAD_DAMAGE_SCORE_MIN=x set the defaults of new contexts), 1 scores, 2 scores and filters the three tables.
 * Changing the mode or the threshold waits for the batches in flight and zeroes the summary; switching on builds the tables of the read lengths prepared so
 * far.  MAPAD_ERR_INVALID: a mode outside 0..2, a threshold that is not a number. */
int mapad_ctx_set_damage_score(mapad_ctx_t* ctx, int mode, float threshold);
/* waits for the batches in flight.  Off: zeroes. */
int mapad_ctx_damage_scores(mapad_ctx_t* ctx, mapad_damage_scores_t* out);
int mapad_ctx_damage_scores_reset(mapad_ctx_t* ctx);
/* the scores that travel beside the records of mapad_hits_to_records_gpu / mapad_coords_to_records: score_q[n] and scored[n] (1 = the read has a score), owned
 * by `recs`.  Both NULL when the records carry none (the mode was off; mapad_hits_to_records). */
int mapad_records_damage_scores(const mapad_records_t* recs, const int32_t** score_q, const uint8_t** scored);
/* host path, no GPU: the same core over a fetched result, with the host's record_coords under `seed` (the seed of the records call).  Writes score_q[n] and
 * scored[n] (either may be NULL) and ADDS the batch to *acc (may be NULL; zero it before the first batch; threshold_q is set). */
int mapad_damage_score_host(const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs, const uint8_t* quals,
                            const uint64_t* offsets, uint64_t seed, float threshold, int32_t* score_q, uint8_t* scored, mapad_damage_scores_t* acc);
/* one read length's table as the device gets it: out[len][*nq][4] int16 (C->C, C->T, G->G, G->A), *nq = 256 for the quality-aware model, else 1.  out == NULL
 * returns *nq only. */
int mapad_damage_score_table(const mapad_params_t* params, uint32_t len, int16_t* out, int* nq);

/* ---- quality rescaling: base qualities marked down at likely-damaged bases (csrc/rescale_core.hpp) ---------------------------------------------------
 * Opt-in like the damage score and run directly behind it, in front of the pileup: with it off (the default) nothing is launched, allocated or built and
 * every output is what it was.  On: every records call on a batch whose hits AND reads are still on the device also copies the batch's qualities into a
 * buffer of the batch slot and runs rescale_kernel over it behind records_kernel.  A read is rescaled iff it is reported mapped.  Its candidate columns are the
 * Mismatch operations of the reported alignment whose (reference base, read base) is C->T or G->A in read orientation; a candidate at read position p with
 * quality byte q != 255 gets q' = table[p][q][cell], a table the HOST builds in double per read length from the damage model the search scores with
 * (-f / -t / -d / -s): pd = clamp((P_dam - P_null) / P_dam, 0, 1), the posterior that the mismatch is damage, from the model's linear probabilities of the
 * column with and without the damage term; e = 10^(-q/10); e' = 1 - (1 - e)(1 - pd); q' = min(q, floor(-10 log10(e') + 0.5)), 0 where e' >= 1.  This is
 * mapDamage's rescaling rule.  q' <= q always; without damage the table is the identity; every other base, every unmapped read and a missing quality (255)
 * stay as they are.  Device and host agree bit for bit.
 * Mode 1 rescales the qualities that travel with the records (mapad_records_rescaled_quals).  Mode 2 does the same and additionally lets the pileup's
 * min_base_quality filter see the rescaled byte, so that a count-based consensus stops counting likely-damaged bases.  The allele and the genotype
 * likelihoods always read the raw qualities: they model damage themselves.  The search never sees a rescaled quality.
 * Rescaling needs no state across reads: every device of a multi-GPU run rescales its own reads, the summaries add.  A batch converted again returns the same
 * bytes and adds nothing to the summary.  With the mode on, a records call on hits that have to be uploaded returns MAPAD_ERR_UNSUPPORTED;
 * mapad_quality_rescale_host takes such results.  mapad_records_device (the multi-GPU gather) rescales but does not carry the bytes. */
#define MAPAD_RESCALE_BINS 64
typedef struct mapad_rescale {
    uint64_t reads_seen;            /* reads of the batches rescaled */
    uint64_t reads_rescaled;        /* ... that are reported mapped */
    uint64_t candidate_columns[2];  /* C->T, G->A mismatch columns of the rescaled reads (a missing quality included) */
    uint64_t bases_changed;         /* ... whose quality changed: q' != q */
    uint64_t quality_drop_sum;      /* sum of q - q' over them */
    uint64_t new_quality[MAPAD_RESCALE_BINS]; /* changed bases by min(q', 63) */
    uint64_t batches;
    double kernel_ms;               /* HIP-event time of the copy of the qualities and rescale_kernel, summed over the batches (the host path leaves it 0) */
} mapad_rescale_t;
/* 0 off (default; MAPAD_RESCALE=1|2 sets the default of new contexts), 1 rescales, 2 rescales and feeds the pileup's base-quality filter.  A change waits for
 * the batches in flight and zeroes the summary; switching on builds the tables of the read lengths prepared so far (512 bytes per read position).
 * MAPAD_ERR_INVALID: a mode outside 0..2. */
int mapad_ctx_set_quality_rescale(mapad_ctx_t* ctx, int mode);
/* waits for the batches in flight.  Off: zeroes. */
int mapad_ctx_quality_rescale(mapad_ctx_t* ctx, mapad_rescale_t* out);
int mapad_ctx_quality_rescale_reset(mapad_ctx_t* ctx);
/* the rescaled qualities that travel beside the records of mapad_hits_to_records_gpu / mapad_coords_to_records (both text paths): quals[*n], the batch's
 * qualities in read orientation at the caller's own `offsets` (*n = offsets[n_reads]), owned by `recs`.  NULL and 0 when the records carry none (the mode was
 * off; mapad_hits_to_records). */
int mapad_records_rescaled_quals(const mapad_records_t* recs, const uint8_t** quals, uint64_t* n);
/* host path, no GPU: the same core over a fetched result, with the host's record_coords under `seed` (the seed of the records call).  Writes the batch's
 * rescaled qualities to out_quals[offsets[n_reads]] (may be NULL) and ADDS the batch to *acc (may be NULL; zero it before the first batch). */
int mapad_quality_rescale_host(const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs, const uint8_t* quals,
                               const uint64_t* offsets, uint64_t seed, uint8_t* out_quals, mapad_rescale_t* acc);
/* one read length's table as the device gets it: out[len][256][2] uint8 (C->T, G->A); the row of quality 255 holds 255. */
int mapad_quality_rescale_table(const mapad_params_t* params, uint32_t len, uint8_t* out);

/* ---- allele likelihoods: damage-aware haploid consensus (csrc/allele_core.hpp) ------------------------------------------------------------------------
 * Opt-in like the pileup and summed at the same place, behind it: with it off (the default) nothing is launched, allocated or built.  On: every records call
 * on a batch whose hits AND reads are still on the device also runs allele_kernel behind records_kernel and adds the batch into int32 ll[n / 2][4] (forward-
 * strand alleles A, C, G, T; units of 1/256 bit) and uint32 depth[n / 2] — 20 bytes per forward-strand text position, 60 GB at 3 Gbp — that the context keeps
 * on the device while the mode is non-zero.  Reads and columns count by the pileup's rule under this table's own filters (all 0 by default).  A counted column
 * of read base b at read position p with quality q adds, for every allele a, the mapper's own log2 P(b | true base a, p, q) — the sequence difference model
 * of -f / -t / -d / -s / -D that the search scores with, read from the search's table and rounded to 1/256 bit (saturating at int16) — to ll[pos][a], and 1
 * to depth[pos]: integers, so device and host agree bit for bit.  A cell can wrap only beyond 65 536 columns of depth (not checked).  The call of a position,
 * with best and second the largest two of its four cells (equal maxima: margin 0) and margin_q = best - second: the best allele iff depth >= min_depth and
 * margin_q >= min_margin_q = max(1, (int32)ceilf(min_margin_bits * 256)), else N; its quality is min(margin_q >> 8, 255) whole bits, 0 for N.  A batch counts
 * once however often it is converted.  With the mode on, a records call on hits that have to be uploaded returns MAPAD_ERR_UNSUPPORTED;
 * mapad_allele_host_add takes such results. */
typedef struct mapad_allele_contig {
    uint64_t length;
    uint64_t sites_covered; /* positions of depth >= 1 */
    uint64_t sites_deep;    /* positions of depth >= min_depth */
    uint64_t sites_called;  /* positions whose call is not N */
    uint64_t called[4];     /* calls by allele: A, C, G, T */
    uint64_t max_depth;
    uint64_t margin_sum_q;  /* the sum of margin_q over the called positions, units of 1/256 bit */
} mapad_allele_contig_t;
typedef struct mapad_allele {
    uint32_t n_contigs;             /* in: entries `contigs` has room for (>= mapad_index_n_contigs); out: entries filled */
    uint32_t pad;
    mapad_allele_contig_t* contigs; /* caller-provided, index order */
    uint32_t mode, min_base_quality, mask5, mask3; /* out: what the sums were taken under (mode 0: off, everything else is 0) */
    uint32_t min_depth;                            /* out: the call rule of this summary */
    int32_t min_margin_q;
    uint64_t reads;                 /* reads counted */
    uint64_t reads_seen;            /* reads of the batches counted */
    uint64_t columns_counted;       /* = the sum of depth over all positions */
    uint64_t columns_not_acgt, columns_masked, columns_low_quality;
    uint64_t deleted_columns, insertions, batches;
    double accumulate_ms;           /* HIP-event time of allele_kernel, summed over the batches (the host path leaves it 0) */
    double summary_ms;              /* HIP-event time of this summary's allele_call_kernel launches */
} mapad_allele_t;
/* mode 0 off (default) — frees the arrays —, 1 all mapped reads, 2 X0 == 1 only; min_base_quality 0..255, mask5 / mask3 0..65535.  MAPAD_ALLELE_LIK=1|2 sets
 * the default of new contexts (filters 0).  Changing any argument waits for the batches in flight and starts an empty table.  The arrays are allocated at the
 * switch-on: MAPAD_ERR_NOMEM if they do not fit. */
int mapad_ctx_set_allele_likelihoods(mapad_ctx_t* ctx, int mode, uint32_t min_base_quality, uint32_t mask5, uint32_t mask3);
/* waits for the batches in flight, runs allele_call_kernel over every contig; min_depth >= 1, min_margin_bits a number (MAPAD_ERR_INVALID otherwise).  Off:
 * zeroes.  MAPAD_ERR_DEVICE if allele_kernel met an alignment that leaves the text or a read length without a table. */
int mapad_ctx_allele_summary(mapad_ctx_t* ctx, uint32_t min_depth, float min_margin_bits, mapad_allele_t* out);
/* the cells of [from, from + n) of contig tid (0-based) into ll[n][4] (A, C, G, T) and depth[n] */
int mapad_ctx_allele_cells(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, int32_t* ll, uint32_t* depth);
/* the calls of [from, from + n) of contig tid: bases[n] ('A', 'C', 'G', 'T' or 'N') and quals[n] (whole bits, 0..255); either may be NULL, not both.
 * MAPAD_ALLELE_PIECE (a test hook) sets the positions per launch; default 2^24. */
int mapad_ctx_allele_consensus(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, uint32_t min_depth, float min_margin_bits, uint8_t* bases, uint8_t* quals);
/* zeroes the table: nothing has been counted (a batch still resident counts again if it is converted again) */
int mapad_ctx_allele_reset(mapad_ctx_t* ctx);
/* adds src's cells, depths and scalars into dst's (same index, same non-zero mode, same filters: MAPAD_ERR_INVALID otherwise); src keeps its own */
int mapad_ctx_allele_merge(mapad_ctx_t* dst, mapad_ctx_t* src);
/* host path, no GPU: the same core over fetched results and the reads they are of, with the host's record_coords under `seed` and the score tables built
 * from `params` as a context builds them (every batch of one accumulator under the same params: MAPAD_ERR_INVALID otherwise); mode 1 or 2.  skip: as for
 * mapad_pileup_host_add_skip.  20 bytes of host memory per forward-strand text position. */
typedef struct mapad_allele_host mapad_allele_host_t;
int mapad_allele_host_new(const mapad_index_t* idx, int mode, uint32_t min_base_quality, uint32_t mask5, uint32_t mask3, mapad_allele_host_t** acc);
int mapad_allele_host_add(mapad_allele_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                          const uint8_t* quals, const uint64_t* offsets, uint64_t seed);
int mapad_allele_host_add_skip(mapad_allele_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                               const uint8_t* quals, const uint64_t* offsets, uint64_t seed, const uint8_t* skip);
int mapad_allele_host_summary(const mapad_allele_host_t* acc, uint32_t min_depth, float min_margin_bits, mapad_allele_t* out);
int mapad_allele_host_cells(const mapad_allele_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, int32_t* ll, uint32_t* depth);
int mapad_allele_host_consensus(const mapad_allele_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, uint32_t min_depth, float min_margin_bits, uint8_t* bases,
                                uint8_t* quals);
void mapad_allele_host_free(mapad_allele_host_t* acc);
/* what a counted column of read base `to` (0..3 = A, C, G, T, read orientation) at 0-based read position pos of a read of len bases with raw Phred `qual`
 * adds, by true base in read orientation: out[4] = A, C, G, T, units of 1/256 bit — the table row as the kernels round it */
int mapad_allele_quantized_row(const mapad_params_t* params, uint32_t len, uint32_t pos, uint32_t qual, uint32_t to, int16_t* out);

/* ---- diploid genotype likelihoods, on top of the allele likelihoods (csrc/genotype_core.hpp) ----------------------------------------------------------
 * Ten unordered pairs of forward-strand alleles in the fixed order AA CC GG TT AC AG AT CG CT GT (0..9).  The four homozygous values of a position are the
 * allele cells ll[pos][4] as they are, and depth[pos] is theirs; this switch adds the six heterozygous cells int32 het[n / 2][6] (AC AG AT CG CT GT, units of
 * 1/256 bit; 24 bytes per forward-strand position, 72 GB at 3 Gbp), allocated only while it is on, and genotype_kernel behind allele_kernel.  It rides on the
 * allele likelihoods: the same mode, filters, reads and columns, so ll, depth and het always describe the same columns.  A counted column of read base b at
 * read position p with quality q adds to het[pos][{x, y}] the value log2(0.5 * P(b | x, p, q) + 0.5 * P(b | y, p, q)) under the same damage model, evaluated
 * on the host in double from the two f32 model values, rounded to 1/256 bit (saturating int16, ties to even) into a table the device only loads from: device
 * and host agree bit for bit.  For a backward record both alleles are complemented (AC <-> GT, AG <-> CT; AT and CG stay).
 * Call rule, integers (int64): g[0..3] = ll, g[4..9] = het - het_penalty_q with het_penalty_q = (int32)ceilf(het_penalty_bits * 256) >= 0 (a NaN or a
 * negative value: MAPAD_ERR_INVALID), applied at the call and never stored.  best is the FIRST maximum in genotype order, second the largest of the other
 * nine, margin_q = best - second; the call is the best genotype iff depth >= min_depth and margin_q >= min_margin_q (as for the allele calls: at least one
 * unit, so a tie is no call), else 255.  GQ = min(margin_q * 301 / 25600, 99), 0 for a no-call; PL_k = min((best - g_k) * 301 / 25600, 255).
 * Consistency: switching this on or off starts BOTH tables (ll / depth and het) empty; any change of the allele settings empties both; allele mode 0 switches
 * this off and frees het and its table; mapad_ctx_allele_reset also zeroes het while this is on; with it on (allele mode already implies it) a records call
 * on hits that have to be uploaded returns MAPAD_ERR_UNSUPPORTED. */
typedef struct mapad_genotype_contig {
    uint64_t length;
    uint64_t sites_covered; /* positions of depth >= 1 */
    uint64_t sites_deep;    /* positions of depth >= min_depth */
    uint64_t sites_called;  /* positions with a genotype call */
    uint64_t called[10];    /* calls by genotype: AA CC GG TT AC AG AT CG CT GT */
    uint64_t max_depth;
    uint64_t margin_sum_q;  /* the sum of margin_q over the called positions, units of 1/256 bit */
} mapad_genotype_contig_t;
typedef struct mapad_genotype {
    uint32_t n_contigs;               /* in: entries `contigs` has room for (>= mapad_index_n_contigs); out: entries filled */
    uint32_t on;                      /* out: 1 while the feature is on (0: everything else below is 0 but the rule) */
    mapad_genotype_contig_t* contigs; /* caller-provided, index order */
    uint32_t min_depth;               /* out: the call rule of this summary */
    int32_t min_margin_q;
    int32_t het_penalty_q;
    uint32_t pad;
    uint64_t batches;
    double accumulate_ms;             /* HIP-event time of genotype_kernel, summed over the batches (the host path leaves it 0) */
    double summary_ms;                /* HIP-event time of this summary's genotype_call_kernel launches */
} mapad_genotype_t;
/* on != 0 only while mapad_ctx_set_allele_likelihoods has a non-zero mode (MAPAD_ERR_INVALID otherwise); allocates het at the switch-on (MAPAD_ERR_NOMEM if
 * it does not fit).  MAPAD_GENOTYPE_LIK=1 sets the default of new contexts, honoured only where MAPAD_ALLELE_LIK is non-zero. */
int mapad_ctx_set_genotype_likelihoods(mapad_ctx_t* ctx, int on);
/* waits for the batches in flight, runs genotype_call_kernel over every contig; min_depth >= 1.  Off: zeroes.  MAPAD_ERR_DEVICE as for the allele summary. */
int mapad_ctx_genotype_summary(mapad_ctx_t* ctx, uint32_t min_depth, float min_margin_bits, float het_penalty_bits, mapad_genotype_t* out);
/* the het cells of [from, from + n) of contig tid (0-based) into het[n][6] (AC AG AT CG CT GT); the homozygous four are mapad_ctx_allele_cells' */
int mapad_ctx_genotype_cells(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, int32_t* het);
/* the calls of [from, from + n) of contig tid: gt[n] (0..9, 255 = no call) and gq[n] (0..99); either may be NULL, not both.  MAPAD_ALLELE_PIECE applies. */
int mapad_ctx_genotype_calls(mapad_ctx_t* ctx, uint32_t tid, uint64_t from, uint64_t n, uint32_t min_depth, float min_margin_bits, float het_penalty_bits, uint8_t* gt,
                             uint8_t* gq);
/* adds src's het cells into dst's — the het cells only: mapad_ctx_allele_merge adds the rest.  Both contexts have the feature on and equal allele settings, the
 * same index and dst != src: MAPAD_ERR_INVALID otherwise, and dst is unchanged. */
int mapad_ctx_genotype_merge(mapad_ctx_t* dst, mapad_ctx_t* src);
/* what a counted column of read base `to` (0..3, read orientation) at 0-based read position pos of a read of len bases with raw Phred `qual` adds, by pair of
 * true bases in read orientation: out[6] = AC AG AT CG CT GT, units of 1/256 bit — the table row as the kernel loads it */
int mapad_genotype_quantized_row(const mapad_params_t* params, uint32_t len, uint32_t pos, uint32_t qual, uint32_t to, int16_t* out);
/* host path: before the first add of a host allele accumulator (MAPAD_ERR_INVALID afterwards); mapad_allele_host_add[_skip] then also fill the het cells
 * (24 more bytes of host memory per forward-strand position) */
int mapad_allele_host_set_genotypes(mapad_allele_host_t* acc, int on);
int mapad_allele_host_genotype_summary(const mapad_allele_host_t* acc, uint32_t min_depth, float min_margin_bits, float het_penalty_bits, mapad_genotype_t* out);
int mapad_allele_host_genotype_cells(const mapad_allele_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, int32_t* het);
int mapad_allele_host_genotype_calls(const mapad_allele_host_t* acc, uint32_t tid, uint64_t from, uint64_t n, uint32_t min_depth, float min_margin_bits, float het_penalty_bits,
                                     uint8_t* gt, uint8_t* gq);

/* ---- SNP panel: strand-split A/C/G/T counts at a fixed panel of biallelic SNPs and one pseudo-haploid call per panel row (csrc/panel_core.hpp) ----------
 * Opt-in like the pileup and counted at the same place, behind the genotype likelihoods: with it off (the default) nothing is launched, allocated or built.
 * On: every records call on a batch whose hits AND reads are still on the device also runs panel_kernel behind records_kernel and adds the batch into
 * uint32 counts[n_slots][2][4] (strand: 0 forward, 1 reverse; forward-strand bases A, C, G, T; 32 bytes per distinct panel position) on the device.  The
 * panel is n_rows rows (tid, pos0, ref, alt): pos0 0-based on contig tid, ref / alt ASCII.  A row is placed iff 0 <= tid < n_contigs and pos0 < the contig's
 * length; an unplaced row, and a row whose alleles are not two different letters of ACGT (either case), is always called missing.  Rows at one position share
 * their counts.  A read counts iff it is reported mapped (mode 2: and X0 == 1, i.e. XT:U) and is not left out by mark-duplicates mode 2 / damage-score mode 2;
 * of its reported alignment every match / mismatch column on a panel position goes to exactly one of columns_not_acgt, columns_masked, columns_low_quality
 * (the pileup's classes under this table's own filters; quality-rescale mode 2 feeds the quality filter as it feeds the pileup's) or its cell
 * (columns_counted); a deleted reference base on a panel position counts in columns_deleted.  A cell wraps at 2^32 (not checked).  A batch counts once
 * however often it is converted.  A mapping-quality threshold is not part of this (MAPQ is computed on the host behind the stages); mode 2 is the filter the
 * device has.
 * The call of row i under a rule, integers only (device and host cannot differ): missing ('9') if the row is unplaced, has invalid alleles, or is a
 * transition ({C,T} or {A,G}) under transitions == 1.  Strands used: both; under transitions == 2 a {C,T} row uses the reverse strand only and an {A,G} row
 * the forward strand only.  n_ref / n_alt: the counts of the row's alleles over the used strands; n = n_ref + n_alt < min_depth: missing.  The draw:
 * z = seed + (i + 1) * 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; u = z ^ z >> 31; ref iff the high
 * 64 bits of u * n are < n_ref.  call 0: the draw; call 1: the majority, the draw on a tie.  '2' for ref, '0' for alt (EIGENSTRAT .geno, pseudo-haploid).
 * i is the row's index as given: a call depends neither on batch sizes nor on the number of devices nor on the order of reads.
 * With the panel on, a records call on hits that have to be uploaded returns MAPAD_ERR_UNSUPPORTED; mapad_snp_panel_host_add takes such results. */
typedef struct mapad_snp_panel_rule {
    uint32_t call;        /* 0 random draw, 1 majority */
    uint32_t min_depth;   /* >= 1 */
    uint32_t transitions; /* 0 keep, 1 missing, 2 single strand */
    uint64_t seed;
} mapad_snp_panel_rule_t;
typedef struct mapad_snp_panel {
    uint32_t mode, min_base_quality, mask5, mask3; /* out: what the counts were taken under (mode 0: the panel is off, everything below but the rule is 0) */
    mapad_snp_panel_rule_t rule;                   /* out: the rule of this summary */
    uint64_t n_rows, n_slots;                      /* rows as given; distinct positions of the placed rows */
    uint64_t reads_seen;                           /* reads of the batches counted */
    uint64_t reads;                                /* reads counted */
    uint64_t reads_on_panel;                       /* ... with at least one panel position inside their reference span */
    uint64_t columns_counted, columns_not_acgt, columns_masked, columns_low_quality, columns_deleted; /* columns on panel positions only */
    uint64_t rows, rows_unplaced;
    uint64_t rows_bad_alleles;   /* placed rows with invalid alleles */
    uint64_t rows_transition;    /* placed rows with valid alleles that are transitions */
    uint64_t rows_covered;       /* placed, valid rows with at least one observation (of any base) on their used strands */
    uint64_t rows_called, called_ref, called_alt, transitions_called;
    uint64_t obs_ref, obs_alt, obs_other; /* observations over the placed, valid rows, used strands */
    uint64_t max_depth;          /* the largest number of observations of one such row */
    uint64_t batches;
    double accumulate_ms;        /* HIP-event time of panel_kernel, summed over the batches (the host path leaves it 0) */
    double summary_ms;           /* HIP-event time of this summary's panel_call_kernel launch */
} mapad_snp_panel_t;
/* mode 0 off (default) — frees the panel and its table; the other arguments are ignored —, 1 all mapped reads, 2 X0 == 1 only; n_rows >= 1
 * (MAPAD_ERR_INVALID for 0 rows with a non-zero mode, and for 2^32 - 1 rows or more); min_base_quality 0..255, mask5 / mask3 0..65535.  Setting a panel —
 * also the same one again — or changing a filter waits for the batches in flight and starts an empty table. */
int mapad_ctx_set_snp_panel(mapad_ctx_t* ctx, int mode, uint64_t n_rows, const int32_t* tid, const uint64_t* pos0, const uint8_t* ref, const uint8_t* alt,
                            uint32_t min_base_quality, uint32_t mask5, uint32_t mask3);
/* waits for the batches in flight, runs panel_call_kernel over every row.  Off: zeroes.  MAPAD_ERR_DEVICE if panel_kernel met an alignment that leaves the text. */
int mapad_ctx_snp_panel(mapad_ctx_t* ctx, const mapad_snp_panel_rule_t* rule, mapad_snp_panel_t* out);
/* the counts of rows [row_from, row_from + n) into out[n][2][4]: strand, then A, C, G, T; zeroes for an unplaced row */
int mapad_ctx_snp_panel_counts(mapad_ctx_t* ctx, uint64_t row_from, uint64_t n, uint32_t* out);
/* the calls of rows [row_from, row_from + n) into out[n]: '2', '0' or '9' */
int mapad_ctx_snp_panel_calls(mapad_ctx_t* ctx, uint64_t row_from, uint64_t n, const mapad_snp_panel_rule_t* rule, uint8_t* out);
/* zeroes the table: nothing has been counted (a batch still resident counts again if it is converted again) */
int mapad_ctx_snp_panel_reset(mapad_ctx_t* ctx);
/* adds src's counts into dst's (same index, same non-zero mode, same filters, the same panel row for row: MAPAD_ERR_INVALID otherwise); src keeps its own */
int mapad_ctx_snp_panel_merge(mapad_ctx_t* dst, mapad_ctx_t* src);
/* host path, no GPU: the same core over fetched results and the reads they are of, with the host's record_coords under `seed`; mode 1 or 2.  `skip`: one byte
 * per read, non-zero = left out (NULL: none), as for mapad_pileup_host_add_skip. */
typedef struct mapad_snp_panel_host mapad_snp_panel_host_t;
int mapad_snp_panel_host_new(const mapad_index_t* idx, int mode, uint64_t n_rows, const int32_t* tid, const uint64_t* pos0, const uint8_t* ref, const uint8_t* alt,
                             uint32_t min_base_quality, uint32_t mask5, uint32_t mask3, mapad_snp_panel_host_t** acc);
int mapad_snp_panel_host_add(mapad_snp_panel_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res, const uint8_t* seqs,
                             const uint8_t* quals, const uint64_t* offsets, uint64_t seed);
int mapad_snp_panel_host_add_skip(mapad_snp_panel_host_t* acc, const mapad_index_t* idx, const mapad_params_t* params, const mapad_batch_result_t* res,
                                  const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t seed, const uint8_t* skip);
int mapad_snp_panel_host_summary(const mapad_snp_panel_host_t* acc, const mapad_snp_panel_rule_t* rule, mapad_snp_panel_t* out);
int mapad_snp_panel_host_counts(const mapad_snp_panel_host_t* acc, uint64_t row_from, uint64_t n, uint32_t* out);
int mapad_snp_panel_host_calls(const mapad_snp_panel_host_t* acc, uint64_t row_from, uint64_t n, const mapad_snp_panel_rule_t* rule, uint8_t* out);
void mapad_snp_panel_host_free(mapad_snp_panel_host_t* acc);

/* ---- the accumulator stages over existing alignments (no search) ----
 * Every stage above reads of a batch only the reported hit's edit operations, the CoordRec fields mapped / error / best / x0 / first and the reads.  A BAM
 * record's contig, POS, strand, CIGAR, MD:Z and SEQ determine all of that (mapad_amd/csrc/align_core.hpp: the rule, the classes, the strand convention), so a
 * batch of alignments — mapped by this library earlier, by the reference, by bwa aln — can be counted by the switched-on stages without being mapped again.
 * align_count_kernel and align_build_kernel (one wavefront per read) build on the device what a search and records_kernel would have left there; the stages then
 * run in the order and on the stream the records path runs them, and count into the same context tables: every accessor, summary, merge and reset above works
 * unchanged.  Reads and qualities are given as mapad_map_batch takes them: as sequenced, so a 0x10 record's SEQ and QUAL un-reversed.
 * A read gets exactly one status class, the first that applies:
 *   0 ok, 1 unmapped (0x4, tid < 0 or pos0 < 0), 2 below_min_mapq, 3 no_md (md_len == 0), 4 bad_contig (tid >= the index's contigs), 5 unsupported_cigar (any of
 *   S H N P, no CIGAR, 2^31 columns or more), 6 length_mismatch (CIGAR query length != read length), 7 md_mismatch (MD's reference length != CIGAR's, an MD
 *   mismatch or deletion token where the CIGAR has none or the other, an unparsable MD), 8 off_contig (pos0 + span beyond the contig's end).
 * A read of any class but 0 is seen, not counted, by every stage, exactly like an unmapped read of a search.  On this path MAPQ comes with the input, so
 * min_mapq is the mapping-quality filter the stages behind a search cannot have.
 * v1: one device per context, synchronous per call (the call returns when the batch has been counted); batches in flight and several devices are not part of
 * it.  A batch accumulated this way has no search result: mapad_fetch_result, the records calls, mapad_compact_result_device, mapad_last_batch_counters and
 * mapad_device_result_ptrs return MAPAD_ERR_UNSUPPORTED for its slot.  A call that fails leaves the slot empty (mapad_ctx_alignment_tracks: MAPAD_ERR_INVALID). */
#define MAPAD_ALN_CLASSES 9
typedef struct mapad_alignment {
    int64_t pos0;            /* 0-based leftmost position on the contig */
    uint64_t x0;             /* X0:i; 0 = the record has none, taken as 1 */
    uint64_t cigar_off;      /* first of the record's n_cigar words in cigar_words (BAM's encoding: len << 4 | op) */
    uint64_t md_off;         /* first of the record's md_len bytes in md_bytes (MD:Z without the terminator); md_len == 0: no MD */
    int32_t tid;
    uint32_t n_cigar, md_len;
    float as_score;          /* AS; becomes the hit's score (no stage reads it) */
    uint16_t flags;          /* 0x4 unmapped, 0x10 reverse; the other bits are ignored */
    uint8_t mapq, pad0;
    uint32_t pad1;
} mapad_alignment_t;
typedef struct mapad_aln_result {
    uint64_t n_reads;
    const uint8_t* status_class;   /* [n_reads] */
    const uint8_t* duplicate;      /* [n_reads], 1 = a duplicate (0x400); NULL while mark-duplicates is off */
    const uint8_t* scored;         /* [n_reads] and score_q [n_reads] (units of 1/256 bit); NULL while the damage score is off */
    const int32_t* score_q;
    const uint8_t* rescaled_quals; /* [n_quals] at the caller's offsets; NULL while the quality rescaling is off */
    uint64_t n_quals;
    uint64_t class_counts[MAPAD_ALN_CLASSES]; /* of this batch */
    float build_ms;                /* HIP-event time of the count kernel, the scan and the build kernel */
} mapad_aln_result_t;
/* Stages the reads into the next batch slot as mapad_submit_batch does (and builds the score tables of their lengths), builds the tracks, runs the switched-on
 * stages (duplicates -> damage score -> rescaling -> the rest).  May be called batch after batch: the tables and the duplicate table persist as they do for
 * mapping.  alns[n_reads]; cigar_words / md_bytes: the two arrays the records point into.  min_mapq 0..255. */
int mapad_ctx_accumulate_alignments(mapad_ctx_t* ctx, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads, const mapad_alignment_t* alns,
                                    const uint32_t* cigar_words, const uint8_t* md_bytes, uint32_t min_mapq, mapad_aln_result_t** out);
void mapad_aln_result_free(mapad_aln_result_t* r);
/* The arrays the stages read, one hit per read (hit_begin[r] = r): of the batch accumulated last (copied from the device), or built on the host with the same
 * core.  ops[hits[r].ops_off .. + hits[r].n_ops) is read r's track; a read that fails only at md_mismatch or off_contig keeps its room in `ops`, unwritten
 * (unspecified words), with n_ops == 0. */
typedef struct mapad_tracks {
    uint64_t n_reads, n_ops;
    const uint64_t* hit_begin;     /* [n_reads + 1] */
    const mapad_hit_t* hits;       /* [n_reads]: lower = lower_rev = 0, size = x0, score = as_score */
    const uint32_t* ops;           /* [n_ops] */
    const uint8_t* status_class;   /* [n_reads] */
    const uint32_t* mapped;        /* the CoordRec fields the stages read, [n_reads] each */
    const uint32_t* error;
    const uint32_t* best;
    const uint64_t* x0;
    const int32_t* tid;
    const uint64_t* rel;
    const uint64_t* abs;
    const uint32_t* backward;
    uint64_t class_counts[MAPAD_ALN_CLASSES];
} mapad_tracks_t;
int mapad_ctx_alignment_tracks(mapad_ctx_t* ctx, mapad_tracks_t** out);
/* host path, no GPU: offsets give the read lengths (a track does not depend on the bases); params: whether the model starts an alignment at the read's end
 * (the position a Deletion carries) */
int mapad_alignment_tracks_host(const mapad_index_t* idx, const mapad_params_t* params, const uint64_t* offsets, uint64_t n_reads, const mapad_alignment_t* alns,
                                const uint32_t* cigar_words, const uint8_t* md_bytes, uint32_t min_mapq, mapad_tracks_t** out);
void mapad_tracks_free(mapad_tracks_t* t);

/* ---- adapter trimming and read-pair merging (the step in front of mapping) -----------------------------------------------------------------------------------
 * The rule is DESIGN.md section 4 "Trim and merge" (csrc/merge_core.hpp): integers only, so that the kernels and the host path agree byte for byte.  The stage
 * needs no index: it has its own object.  Reads are packed as mapad_map_batch takes them (bases upper-cased, raw Phred bytes, 255 = no quality; offsets[n + 1]);
 * mates as sequenced, 5'->3'.  mode 0: pairs (mate 1 with adapter1 behind the fragment, mate 2 with adapter2).  mode 1: single-end trimming — adapter1 only,
 * min_adapter_overlap in the place of min_overlap, the classes read trimmed / too_short / untouched, and an untouched read is written out whole. */
#define MAPAD_MERGE_MAX_MATE_LEN 512
#define MAPAD_MERGE_MAX_ADAPTER 64
#define MAPAD_MERGE_CLASSES 5        /* 0 merged (trimmed), 1 too_short, 2 unmerged (untouched), 3 empty_mate, 4 too_long */
#define MAPAD_MERGE_HIST_BINS 1025   /* lengths of the reads written, 0 .. 1024 */
typedef struct mapad_merge_params {
    uint32_t min_overlap;            /* 11 */
    uint32_t min_adapter_overlap;    /* 3 */
    uint32_t max_mismatch_permille;  /* 166 */
    uint32_t min_length;             /* 15 */
    uint32_t max_quality;            /* 41 */
    uint32_t adapter1_len, adapter2_len;
    uint32_t mode;
    uint8_t adapter1[MAPAD_MERGE_MAX_ADAPTER], adapter2[MAPAD_MERGE_MAX_ADAPTER];
} mapad_merge_params_t;
typedef struct mapad_merge_counts {
    uint64_t pairs_seen;
    uint64_t class_counts[MAPAD_MERGE_CLASSES];
    uint64_t bases_in, bases_out;
    uint64_t histogram[MAPAD_MERGE_HIST_BINS];
    uint64_t calls;
} mapad_merge_counts_t;
typedef struct mapad_merge_result {
    uint64_t n_pairs, total_bases;
    const uint8_t* cls;          /* [n_pairs] */
    const int32_t* frag_len;     /* [n_pairs]: the chosen candidate, -1 for none */
    const uint16_t* matches;     /* [n_pairs]: m and x of the chosen candidate, 0 for none */
    const uint16_t* mismatches;
    const uint8_t* seqs;         /* [total_bases] */
    const uint8_t* quals;
    const uint64_t* offsets;     /* [n_pairs + 1]; a pair that yields no read has a zero-length slot */
    mapad_merge_counts_t counts; /* of this call */
    float kernel_ms[2];          /* HIP-event time of merge_decide_kernel and of merge_write_kernel (0 on the host path) */
} mapad_merge_result_t;
typedef struct mapad_merger mapad_merger_t;
/* no GPU needed */
void mapad_merge_params_default(mapad_merge_params_t* out);
/* MAPAD_ERR_INVALID: an adapter longer than 64 or with a byte outside ACGT, min_overlap or min_adapter_overlap < 1, max_quality > 93,
 * max_mismatch_permille > 1000, a mode outside 0..1 */
int mapad_merge_params_check(const mapad_merge_params_t* params);
int mapad_merger_create(int device_id, const mapad_merge_params_t* params, mapad_merger_t** out);
/* A merger works on a non-blocking stream of its own unless it is given another; NULL gives it its own back. */
int mapad_merger_set_stream(mapad_merger_t* m, void* hip_stream);
void mapad_merger_free(mapad_merger_t* m);
/* mode 0 mergers only / mode 1 mergers only (MAPAD_ERR_INVALID otherwise) */
int mapad_merge_pairs(mapad_merger_t* m, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offsets1, const uint8_t* seqs2, const uint8_t* quals2,
                      const uint64_t* offsets2, uint64_t n_pairs, mapad_merge_result_t** out);
int mapad_trim_reads(mapad_merger_t* m, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n, mapad_merge_result_t** out);
void mapad_merge_result_free(mapad_merge_result_t* r);
/* the running sums over the calls of this merger (mapad_merge_pairs, mapad_trim_reads, mapad_merge_pairs_device) */
int mapad_merger_totals(mapad_merger_t* m, mapad_merge_counts_t* out);
/* dst += src, field by field (how the counts of several calls or mergers become one report; no GPU) */
void mapad_merge_counts_add(mapad_merge_counts_t* dst, const mapad_merge_counts_t* src);
int mapad_merger_reset(mapad_merger_t* m);
/* Inputs and outputs stay in device memory, on the merger's stream.  The outputs belong to the merger and hold until its next call; the offsets are complete
 * when the call returns (it waits for them to learn total_bases), the bases and qualities are ordered on the stream: mapad_map_batch_device on the same stream
 * takes the three as they are.  Single-end mergers take NULL for mate 2. */
int mapad_merge_pairs_device(mapad_merger_t* m, const void* d_seqs1, const void* d_quals1, const void* d_offsets1, const void* d_seqs2, const void* d_quals2,
                             const void* d_offsets2, uint64_t n_pairs, void** d_seqs, void** d_quals, void** d_offsets, uint64_t* total_bases);
/* the same core on host threads, no GPU */
int mapad_merge_pairs_host(const mapad_merge_params_t* params, const uint8_t* seqs1, const uint8_t* quals1, const uint64_t* offsets1, const uint8_t* seqs2,
                           const uint8_t* quals2, const uint64_t* offsets2, uint64_t n_pairs, mapad_merge_result_t** out);
int mapad_trim_reads_host(const mapad_merge_params_t* params, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n, mapad_merge_result_t** out);

/* ---- read clean-up (between the adapter step and the mapper) ------------------------------------------------------------------------------------------------
 * The rule is DESIGN.md section 4 "Clean" (csrc/clean_core.hpp): integers only, so that the kernels and the host path agree byte for byte.  The stage needs no
 * index: it has its own object.  Reads are packed as mapad_map_batch takes them (bases upper-cased, raw Phred bytes, 255 = no quality; offsets[n + 1]).  The
 * steps whose bit is set in `ops` run in this order on every read of 1 .. MAPAD_CLEAN_MAX_LEN bases:
 *   MAPAD_CLEAN_POLY       a tail of poly_base at the 3' end is cut off: the longest run of >= poly_min_len bases from the end that begins with poly_base and in
 *                          which, counted from the end, no prefix of >= poly_min_len bases has more than one other base in poly_one_in and none more than
 *                          poly_max_mismatch;
 *   MAPAD_CLEAN_TRIM_N     bases outside ACGT are removed from the 3' end, then from the 5' end, together with
 *   MAPAD_CLEAN_TRIM_QUAL  bases of quality <= min_quality (255 is no quality and stays);
 *   (always)               what is left is too_short below min_length;
 *   MAPAD_CLEAN_DUST       the complexity score of what is left — over windows of 64 bases every 32, 2000 S / (T (T - 1)) with T the window's triplets of ACGT
 *                          and S the pairs of equal ones, the maximum over the windows: 1000 for a homopolymer, about 20 for random bases — above max_dust
 *                          makes the read low_complexity.
 * A read of class 0, 1 or 5 is written out (a too_long one whole and unscored), every other leaves a zero-length slot. */
#define MAPAD_CLEAN_MAX_LEN 1024
#define MAPAD_CLEAN_CLASSES 6          /* 0 kept, 1 trimmed, 2 too_short, 3 low_complexity, 4 empty, 5 too_long */
#define MAPAD_CLEAN_LEN_BINS 1025      /* lengths of the reads written, 0 .. 1024 */
#define MAPAD_CLEAN_DUST_BINS 101      /* dust / 10 of the reads scored */
#define MAPAD_CLEAN_POLY 1u
#define MAPAD_CLEAN_TRIM_N 2u
#define MAPAD_CLEAN_TRIM_QUAL 4u
#define MAPAD_CLEAN_DUST 8u
typedef struct mapad_clean_params {
    uint32_t ops;                /* 0: the length test alone */
    uint32_t poly_base;          /* 'G' */
    uint32_t poly_min_len;       /* 10 */
    uint32_t poly_one_in;        /* 8 */
    uint32_t poly_max_mismatch;  /* 5 */
    uint32_t min_quality;        /* 2 */
    uint32_t min_length;         /* 15 */
    uint32_t max_dust;           /* permille; 1000 (nothing is above it) — 70 is a usual choice */
} mapad_clean_params_t;
typedef struct mapad_clean_counts {
    uint64_t reads_seen;
    uint64_t class_counts[MAPAD_CLEAN_CLASSES];
    uint64_t bases_in, bases_out;
    uint64_t bases_poly, bases_trim5, bases_trim3;  /* removed as poly tail / at the 5' end / at the 3' end behind the poly tail, over all reads of classes 0 to 3 */
    uint64_t length_histogram[MAPAD_CLEAN_LEN_BINS];
    uint64_t dust_histogram[MAPAD_CLEAN_DUST_BINS];  /* with MAPAD_CLEAN_DUST: the reads of classes 0, 1 and 3 */
    uint64_t calls;
} mapad_clean_counts_t;
typedef struct mapad_clean_result {
    uint64_t n_reads, total_bases;
    const uint8_t* cls;          /* [n_reads] */
    const uint16_t* trim5;       /* [n_reads]: bases removed at the 5' end */
    const uint16_t* trim3;       /* [n_reads]: bases removed at the 3' end, the poly tail among them */
    const uint16_t* poly_len;    /* [n_reads] */
    const uint16_t* dust;        /* [n_reads]: 0 where the read was not scored */
    const uint8_t* seqs;         /* [total_bases] */
    const uint8_t* quals;
    const uint64_t* offsets;     /* [n_reads + 1]; a read that is not written has a zero-length slot */
    mapad_clean_counts_t counts; /* of this call */
    float kernel_ms[2];          /* HIP-event time of clean_decide_kernel and of clean_write_kernel (0 on the host path) */
} mapad_clean_result_t;
typedef struct mapad_cleaner mapad_cleaner_t;
/* no GPU needed.  The defaults have ops == 0: the caller names the steps */
void mapad_clean_params_default(mapad_clean_params_t* out);
/* MAPAD_ERR_INVALID: a poly_base outside ACGT, poly_min_len < 1, poly_one_in < 1, min_quality > 93, max_dust > 1000, an unknown bit in ops */
int mapad_clean_params_check(const mapad_clean_params_t* params);
int mapad_cleaner_create(int device_id, const mapad_clean_params_t* params, mapad_cleaner_t** out);
/* A cleaner works on a non-blocking stream of its own unless it is given another; NULL gives it its own back. */
int mapad_cleaner_set_stream(mapad_cleaner_t* c, void* hip_stream);
void mapad_cleaner_free(mapad_cleaner_t* c);
/* from host memory and back to it.  A call that fails waits for the stream before it returns. */
int mapad_clean_reads(mapad_cleaner_t* c, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads, mapad_clean_result_t** out);
void mapad_clean_result_free(mapad_clean_result_t* r);
/* the running sums over the calls of this cleaner (mapad_clean_reads, mapad_clean_reads_device) */
int mapad_cleaner_totals(mapad_cleaner_t* c, mapad_clean_counts_t* out);
/* dst += src, field by field (no GPU) */
void mapad_clean_counts_add(mapad_clean_counts_t* dst, const mapad_clean_counts_t* src);
int mapad_cleaner_reset(mapad_cleaner_t* c);
/* Inputs and outputs stay in device memory, on the cleaner's stream.  The outputs belong to the cleaner and hold until its next call; the offsets are complete
 * when the call returns (it waits for them to learn total_bases), the bases and qualities are ordered on the stream: mapad_map_batch_device on the same stream
 * takes the three as they are, and the outputs of mapad_merge_pairs_device on this stream are valid inputs.  As with the merger's outputs, a read that was
 * dropped is a zero-length slot, and nothing in the mapper has been tested with zero-length reads: a caller whose batch may hold dropped reads compacts it
 * before it goes to the mapper. */
int mapad_clean_reads_device(mapad_cleaner_t* c, const void* d_seqs, const void* d_quals, const void* d_offsets, uint64_t n_reads, void** d_out_seqs, void** d_out_quals,
                             void** d_out_offsets, uint64_t* total_bases);
/* the same core on host threads, no GPU */
int mapad_clean_reads_host(const mapad_clean_params_t* params, const uint8_t* seqs, const uint8_t* quals, const uint64_t* offsets, uint64_t n_reads,
                           mapad_clean_result_t** out);

/* ---- mappability: at how many places of the reference each of its k-mers can be put (csrc/mappability_core.hpp) ----------------------------------
 * For the start p of a contig, c(p) = the sum of loci(N) over all strings N at Hamming distance <= e from the k-mer seq[p, p + k), where loci(N) is N's FMD
 * interval size in the index's own text (forward strand, '$', reverse complement, '$'; a short ambiguity run is the bases the index drew for it, a long
 * one 'X'), halved when N is its own reverse complement.  A start is valid when p + k <= len and seq has only A, C, G, T (either case) in [p, p + k); an
 * invalid start counts 0, a valid one min(c, 255) >= 1.  cover(x) = the starts s in [max(0, x - k + 1), x] with c(s) == 1.  With possible(x) = the starts of
 * that range with s + k <= len, the masks are: start c(x) == 1; majority 2 cover(x) > possible(x); strict possible(x) > 0 and cover(x) == possible(x).
 * k in 1..255, e in {0, 1}.  `seq` is the whole contig as the FASTA has it and `len` the index's length of contig `tid` (MAPAD_ERR_INVALID otherwise, and
 * for an unknown tid or a window that passes the contig's end).  With e = 0 a start's search ends as soon as one place is left, which is right for the
 * index's own reference only; MAPAD_MAPPABILITY_VERIFY runs every search to its end and returns MAPAD_ERR_INVALID if a valid start counts 0 — the sequence
 * is not the index's reference.  Without it the counts of a foreign sequence mean nothing. */
#define MAPAD_MAPPABILITY_BINS 9
#define MAPAD_MAPPABILITY_VERIFY 1u
typedef struct mapad_mappability_contig {
    uint64_t length, valid_starts, unique_starts;  /* unique: c == 1 */
    uint64_t hist[MAPAD_MAPPABILITY_BINS];         /* valid starts by c: 1, 2, 3-4, 5-8, 9-16, 17-32, 33-64, 65-128, >= 129 */
    uint64_t majority, strict;                     /* positions in the two masks */
} mapad_mappability_contig_t;
typedef struct mapad_mappability {
    uint32_t n_contigs;                   /* in: entries `contigs` has room for (>= mapad_index_n_contigs); out: entries filled */
    uint32_t k, e, pad;
    mapad_mappability_contig_t* contigs;  /* caller-provided, index order */
    mapad_mappability_contig_t total;
    uint64_t starts, steps;               /* starts searched; extension steps taken (two rank queries each) */
    double kernel_ms;                     /* HIP-event time of the count kernels (the host path leaves it 0) */
} mapad_mappability_t;
/* counts and cover of the starts / positions [from, from + n) of contig tid into out_counts[n] and out_cover[n] (either may be NULL).  Runs on the context's
 * stream in tiles of at most 2^22 starts (MAPAD_MAPPABILITY_TILE lowers that: a test hook, read per call; not a number in [1, 2^22]: MAPAD_ERR_PARSE), in
 * device buffers of its own: batches in flight are left alone.  Fetches the counts in front of `from` that the cover needs by itself.  Returns when done. */
int mapad_ctx_mappability(mapad_ctx_t* ctx, uint32_t tid, const uint8_t* seq, uint64_t len, uint64_t from, uint64_t n, uint32_t k, uint32_t e, uint32_t flags,
                          uint8_t* out_counts, uint8_t* out_cover);
/* the figures of every contig and their total, reduced on the device; seqs[i] / lens[i]: contig i of the index */
int mapad_ctx_mappability_summary(mapad_ctx_t* ctx, const uint8_t* const* seqs, const uint64_t* lens, uint32_t k, uint32_t e, uint32_t flags, mapad_mappability_t* out);
/* of the latest of the two calls above: HIP-event time of its count kernels, starts searched, extension steps taken */
int mapad_last_mappability_info(mapad_ctx_t* ctx, double* kernel_ms, uint64_t* starts, uint64_t* steps);
/* the same rule on host threads, no GPU: byte for byte what the device calls return */
int mapad_mappability_host(const mapad_index_t* idx, uint32_t tid, const uint8_t* seq, uint64_t len, uint64_t from, uint64_t n, uint32_t k, uint32_t e, uint32_t flags,
                           uint8_t* out_counts, uint8_t* out_cover);
int mapad_mappability_summary_host(const mapad_index_t* idx, const uint8_t* const* seqs, const uint64_t* lens, uint32_t k, uint32_t e, uint32_t flags,
                                   mapad_mappability_t* out);

const char* mapad_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MAPAD_AMD_H */
