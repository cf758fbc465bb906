/* bamm_em.h -- C ABI of the MI355X (gfx950) EM-refinement hot path of BaMMmotif2.
 *
 * The reference has no FFI layer: the seam is the C++ class `EM` (src/refinement/EM.h:11-69)
 * and `ScoreSeqSet` (src/seq_scoring/ScoreSeqSet.h:14-53), which read
 * `Sequence::getKmer()/getL()` (src/init/Sequence.h:26,36), `Motif::getV/getA/getK/getW/getQ`
 * (src/init/Motif.h:30-38) and `BackgroundModel::getV/getOrder` (src/init/BackgroundModel.h:34-35)
 * and mutate the caller's Motif in place.  This header is what a binding for that seam binds:
 * plain pointers and sizes, no C++ / torch types.  INTEGRATION.md shows the reference-side
 * glue (an `EM` whose methods forward to these entry points).
 *
 * Conventions
 *   - every function returns BAMM_OK (0) or a negative error code; bamm_last_error() gives
 *     the message of the last failure on the calling thread.  Nothing calls exit().
 *     (the reference only ever `exit(1)`s after a std::cerr line, e.g. Global.cpp:127-131.)
 *   - all host buffers are caller-owned and only read/written during the call.
 *   - handles are not thread-safe individually; distinct handles may be used from distinct
 *     threads (FDR.cpp:37 runs folds concurrently).
 *   - flat tensor layouts (identical to oracle/bamm_oracle.h):
 *       v, n, p : [k][y][j] row-major, orders concatenated, order k at W*(4^(k+1)-4)/3
 *       vbg     : [k][y], order k at (4^(k+1)-4)/3
 *       A       : [k][j], (K+1) x W          (Motif.cpp:43-46)
 *       s       : [y][j], 4^(K+1) x W
 *       r       : per sequence L floats, reference's reversed index: r[L-W-i] <-> window
 *                 start i, slots >= L-W+1 are zero (EM.cpp:173,190-192)
 *       sites   : the windows whose r reaches a cut-off, as (sequence, window start i, r) in ascending
 *                 (sequence, i) order -- what EM::write lists in .positions (EM.cpp:577-601); found on
 *                 the device, no window-sized array crosses to the host (bamm_em_sites)
 */
#ifndef BAMM_EM_H_
#define BAMM_EM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BAMM_OK              0
#define BAMM_ERR_ARG        -1   /* bad argument (null, size, order > BAMM_MAX_ORDER, L < W ...) */
#define BAMM_ERR_HIP        -2   /* HIP runtime failure (message carries hipGetErrorString)      */
#define BAMM_ERR_NO_DEVICE  -3   /* no gfx950 device / extension built for another arch         */
#define BAMM_ERR_UNSUPPORTED -4  /* shape outside the kernels' envelope         */
#define BAMM_ERR_STATE      -5   /* call order (e.g. MStep before any EStep)                    */
#define BAMM_ERR_COMM       -6   /* the caller's all-reduce callback failed                     */

#define BAMM_MAX_ORDER      10   /* kmer_ spans 11 bases (Sequence.cpp:37)                      */
#define BAMM_MAX_SEQ_POSITIONS 8192u /* per sequence (reverse strand and separator included): up to
                                      * here a sequence lives in the registers of one wavefront; longer
                                      * ones are accepted and walked window by window (long_seq.hip)  */

typedef struct bamm_ctx  bamm_ctx;   /* one device + one stream                                   */
typedef struct bamm_seqs bamm_seqs;  /* a sequence set resident in HBM (2-bit packed)             */
typedef struct bamm_em   bamm_em;    /* one EM run; replaces `class EM` (EM.h:11-69)              */
typedef struct bamm_comm bamm_comm;  /* one rank of an RCCL communicator, bound to a context       */

const char* bamm_last_error(void);
const char* bamm_version(void);

/* ------------------------------------------------------------------ packing (host only) --
 * Replaces what EM/ScoreSeqSet read through Sequence::getKmer() (EM.cpp:152, :233,
 * ScoreSeqSet.cpp:44): `kmer_[i]` = up to 11 bases ending at i, newest base least
 * significant (Sequence.cpp:35-41).  The packed form keeps 2 bits per position (digit 0 of
 * kmer_[i]) in big-endian order inside 32-bit words, 16 positions per word, every sequence
 * starting on a word boundary, plus an exception list for the positions whose 11-mer cannot
 * be rebuilt from those bits (the reference randomises an unknown base independently per
 * (position, digit), Sequence.cpp:38, and lets the byte 'N' leak into reverse complements,
 * Alphabet.cpp:50).  Pure CPU code: usable and testable without a GPU.                       */
typedef struct bamm_packed {
    uint64_t  n_seqs;
    uint64_t  n_words;
    uint64_t  n_exc;
    uint64_t  total_len;     /* sum of L                                                     */
    uint32_t  max_len;
    uint32_t  min_len;
    uint32_t* words;         /* [n_words]                                                    */
    uint64_t* word_off;      /* [n_seqs+1] first word of each sequence                       */
    uint32_t* len;           /* [n_seqs]   L                                                 */
    uint64_t* exc_off;       /* [n_seqs+1]                                                   */
    uint32_t* exc_pos;       /* [n_exc] position inside its sequence, ascending              */
    uint32_t* exc_kmer;      /* [n_exc] kmer_[pos] mod 4^11 as the reference holds it        */
    uint32_t* exc_clean;     /* [n_exc] what the 2-bit stream alone would give               */
} bamm_packed;

/* kmer: concatenated kmer_ arrays, off[n_seqs+1] (positions).  Values are taken mod 4^11.    */
int  bamm_pack_kmers(const uint64_t* kmer, const uint64_t* off, uint64_t n_seqs, bamm_packed** out);
/* same input as the reference holds it: one pointer per Sequence (getKmer()) + getL()        */
int  bamm_pack_kmer_ptrs(const uint64_t* const* kmer_ptrs, const uint64_t* L, uint64_t n_seqs,
                         bamm_packed** out);
/* from the alphabet codes of FASTA records (0 = N, 1..4 = A,C,G,T; off[n_seqs+1]) -- restates
 * Sequence::Sequence (Sequence.cpp:4-43,91-99): appends the reverse complement unless
 * single_strand and draws libc rand()%4 for unknown bases in the reference's order, so after
 * the caller's srand(42) (mainBaMM.cpp:22) the result equals packing the reference's kmer_.   */
int  bamm_pack_codes(const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int single_strand,
                     bamm_packed** out);
/* the same when the libc stream starts at srand(seed) (the reference seeds once, mainBaMM.cpp:22, and its positives
 * are read first): glibc's generator is restated and checked against the running libc, so the draws are taken on all
 * host threads (each jumps to its share of the one stream) instead of one after the other; falls back to
 * srand(seed) + rand() where the check fails.  Same packing as srand(seed); bamm_pack_codes(...).  Postcondition on
 * either path: libc's stream stands at srand(seed), NOT advanced past the draws (the reference's later consumers all
 * reseed: SeqGenerator.cpp:35, FDR.cpp:153); a caller that continues the one stream behind the positives uses
 * bamm_pack_codes, which draws from libc's rand() itself.                                                       */
int  bamm_pack_codes_seeded(const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int single_strand,
                            uint32_t seed, bamm_packed** out);
/* host threads the packing helpers may use (0 = a default of at most 8); the result never depends
 * on it: the rand() draws are taken serially, in the reference's order                        */
void bamm_set_host_threads(uint32_t n);
/* inverse (host): rebuild kmer_[i] mod 4^(K+1) for every position -- used by tests          */
int  bamm_unpack_y(const bamm_packed* p, uint32_t K, uint32_t* y_out /* [total_len] */);
void bamm_packed_free(bamm_packed* p);

/* contiguous shard [begin,end) of rank `rank` of `world`, balanced by sum(L-W+1) */
int  bamm_shard_range(const uint32_t* len, uint64_t n_seqs, uint32_t W, uint32_t rank,
                      uint32_t world, uint64_t* begin, uint64_t* end);

/* ------------------------------------------------------------------ context ------------- */
/* stream: a hipStream_t created by the caller (e.g. torch's current stream), or NULL to let
 * the context create its own.  Fails with BAMM_ERR_NO_DEVICE when no gfx950 GPU is visible. */
int  bamm_ctx_create(int device, void* hip_stream, bamm_ctx** out);
int  bamm_ctx_destroy(bamm_ctx* ctx);
int  bamm_ctx_sync(bamm_ctx* ctx);
int  bamm_ctx_device_name(bamm_ctx* ctx, char* buf, size_t cap);
/* launch geometry of the sequence kernels (0 = default); exposed for tuning/benchmarks      */
int  bamm_ctx_set_launch(bamm_ctx* ctx, uint32_t blocks, uint32_t threads_per_block);

/* kernel-selection switches, applied to EM handles created afterwards (benchmarks and the tests that
 * compare one kernel with another; results agree within the parity bar whatever is chosen):
 *   "grouped"      1/0  grouped-column kernel for K <= 3 (default 1; 0 = one column at a time)
 *   "group_size"   0 = planner's choice, 2..4 = columns per table row
 *   "group_layout" -1 = planner's choice, 0..3 = table layout of the uniform rows (csrc/grouped.hip:
 *                       grp_geometry), 8 = mixed rows only (csrc/mixed_kernel.h; where they do not apply
 *                       the sequences go one column at a time)
 *   "mix_anchor"   1/0  mixed rows: a sequence whose rows fit a shorter length class with the windows anchored at
 *                       their start runs there (default 1; 0 = every sequence in the class of its length).  The
 *                       two flavours differ in the last bits of r (the summation order of Z), nowhere else
 *   "sparse"      1/0  compacted lists of the non-zero windows in the M-step (default 1)
 *   "e_fused"      1/0  sliced path: whole-table E pass when the odds table fits LDS (default 1)
 *   "e_list"       1/0  sliced path: the E pass hands the M slices compacted lists of the non-zero
 *                       windows instead of all responsibilities (default 1)
 *   "adaptive_lists" 1/0  sliced path: per pass, lists or dense r between the E pass and the M slices, chosen on the
 *                       device from the previous pass's count of non-zero windows (default 1; 0 = always lists)
 *   "list_threshold_pct" 0..100  ... lists when fewer than this percentage of the windows was non-zero (default 45)
 *   "fused_update" 1/0 inside iterate() / optimize() the model update of pass p runs in the block prologue of
 *                       pass p+1's first kernel instead of a launch of its own (default 1; K <= 2-sized tables)
 *   "update_blocks" 1/0 tables beyond the update's LDS form (k >= 3 at usual widths): the model update spread over
 *                       blocks in three short launches instead of one block (default 1; same model bits)
 *   "score_tiles"  1/0  the scorer (bamm_logodds*, bamm_occurrences, bamm_fdr_add_set) takes sequences longer than
 *                       BAMM_MAX_SEQ_POSITIONS tile by tile through the register-resident kernel (default 1; 0 = window by
 *                       window, one workgroup per sequence; the same bits); read at the scoring call
 *   "score_slices" 1/0  the scorer takes a log-odds table beyond one CU's LDS (W * (4^(K+1) + 1) * 4 > 160 KiB) through the same
 *                       register-resident kernels, a slice of motif columns per launch (bamm_score_slice_geometry; orders up
 *                       to 6), instead of window by window with the table in global memory; the same bits; read at the
 *                       scoring call.  Default 0: the library routes as it always has, and the BaMMmotif driver turns the
 *                       key on for its contexts.  Making 1 the library's default is a one-line change (csrc/handles.h)
 *                       together with the tests that pin the default plan (tests/test_score_tiles_gpu.py)
 *   "em_tiles"     1/0  EM passes, getR and bamm_em_sites take sequences longer than BAMM_MAX_SEQ_POSITIONS tile by tile
 *                       (csrc/em_tiles.hip) while the handle's odds and count tables fit one CU's LDS unsliced (default 1;
 *                       0 = window by window, one workgroup per sequence: r and counts within a few ulps, see
 *                       bamm_em_tile_plan); read at bamm_em_create
 *   "scratch_cache_mb" n  idle set-sized scratch blocks (dense r, lists, logs) a context keeps for its next handle
 *                       instead of freeing them (default: a quarter of the device's memory; 0 = keep nothing)
 *   "scratch_poison" 1/0 tests: fill every such block with 0xFF bytes when it is handed out (default 0)
 *   "sites_chunk_positions" n  bamm_em_sites: positions of dense r the call keeps on the device at a time (whole
 *                       sequences; 0 = the default, 2^27 positions = 512 MiB); read at the call, not at handle creation
 *   "neg_segment_positions" n  bamm_sample_negatives: positions per segment of a negative longer than
 *                       BAMM_MAX_SEQ_POSITIONS (16..2^20, rounded down to a multiple of 16; 0 = the default,
 *                       bamm_neg_segment_geometry); the same negatives whatever the cut; for measurements
 *   "kmer_segment_positions" n  bamm_kmer_counts[_gapped]: positions per segment of a record longer than that (16..2^20, rounded
 *                       down to a multiple of 16; 0 = the default, BAMM_MAX_SEQ_POSITIONS); the same table whatever the cut
 *   "kmer_flush_windows" n  bamm_kmer_counts[_gapped]: a workgroup flushes its LDS table once it has added n windows (0 = the
 *                       default, 2^31); the same table whatever the threshold; for tests
 * There are no environment variables that change what the library computes or launches.          */
int  bamm_ctx_set_tuning(bamm_ctx* ctx, const char* key, int value);
/* Device blocks the library has handed to an owner (a sequence set, a handle, a call's temporaries) and not yet taken
 * back, over the whole process; blocks that wait idle in a context's scratch pool are not counted.  For the tests' check
 * that destroying a handle returns all it allocated -- nothing else reads it.                                     */
long long bamm_device_blocks_live(void);

/* ------------------------------------------------------------------ sequences ----------- */
/* Uploads sequences [begin,end) of `p`; they stay resident and are shared (ref-counted) by
 * any number of EM handles -- CV folds pass a mask instead of copying (FDR.cpp:49-57).
 * Any length: sequences up to BAMM_MAX_SEQ_POSITIONS go through the register-resident kernels.  Longer ones are cut
 * into overlapping tiles, one wavefront per tile on the whole GPU: by EM passes, getR and bamm_em_sites while the handle's
 * tables fit one CU's LDS unsliced (bamm_em_tile_geometry, bamm_em_tile_plan: up to order 3 at usual widths; beyond that
 * window by window, one workgroup per sequence), and by the scorer (bamm_score_tile_geometry) while the log-odds table
 * fits the LDS (W * (4^(K+1) + 1) * 4 <= 160 KiB: every width up to order 3, K = 4 up to W = 39, K = 5 up to W = 9,
 * K = 6 up to W = 2; beyond that window by window, or under "score_slices" a slice of columns at a time;
 * bamm_score_plan reports the split) -- the scorer's results are identical on every path, the EM's tile path sums a
 * sequence's partition function in another order (r within 3 ulps of the window-by-window path, deterministic);
 * bamm_seed_from_pwm and bamm_em_mask keep per-wave arrays over one sequence: in LDS up to about
 * 10 000 / 16 000 positions, in a global scratch region per wave beyond (same arithmetic, slower;
 * bamm_em_mask's window lists are 32 bits wide there, and from order 7 on its counts go straight into
 * the accumulator: no limit on length or order short of BAMM_MAX_ORDER, as in the reference).     */
int  bamm_seqs_upload(bamm_ctx* ctx, const bamm_packed* p, uint64_t begin, uint64_t end,
                      bamm_seqs** out);
int  bamm_seqs_destroy(bamm_seqs* s);
int  bamm_seqs_info(const bamm_seqs* s, uint64_t* n_seqs, uint64_t* total_len, uint32_t* max_len,
                    uint64_t* hbm_bytes);

/* ------------------------------------------------------------------ EM ------------------ */
typedef struct bamm_em_params {
    uint32_t K;              /* motif order             (Motif::getK)                        */
    uint32_t W;              /* motif width             (Motif::getW)                        */
    uint32_t bg_order;       /* BackgroundModel::getOrder(); EM uses min(bg_order,K) EM.cpp:23 */
    float    q;              /* Motif::getQ()           (EM.cpp:12)                          */
    int32_t  optimize_q;     /* EM ctor arg; q re-estimated in the first 5 passes of every
                              * optimize() / iterate() call (`iteration` is local to
                              * EM::optimize, EM.cpp:75-99); hand-driven accumulate/update
                              * passes: the handle's first 5                                  */
    float    epsilon;        /* EM.h:62  (0.01)                                              */
    uint32_t max_iterations; /* EM.h:63  (1000)                                              */
    uint64_t n_seqs_global;  /* N used by optimize_q (EM.cpp:515); 0 = this handle's own N   */
    uint64_t n_seqs_bound;   /* upper bound on the sequences summed into this model over ALL
                              * ranks; sizes the unit of the integer count accumulator (2^-40
                              * up to 4M sequences, coarser beyond: the int64 sums never
                              * overflow).  0 = n_seqs_global, else this handle's own count.
                              * Ranks that all-reduce together must agree on it.  A shard also
                              * plans its kernels from it and from nothing else about its size
                              * (as the whole set would: the rows a window is multiplied through
                              * decide the last bit of r), so that the model does not depend on
                              * the number of ranks or on how lengths are spread over them.     */
} bamm_em_params;

void bamm_em_default_params(bamm_em_params* p);

/* seq_mask: NULL, or n_seqs bytes (1 = sequence takes part).  vbg holds orders 0..bg_order.
 * Mirrors EM::EM (EM.cpp:7-43); v_init is Motif::getV() flattened.
 * q, v_init, A and vbg are taken as they are, like the reference takes them.  Where they make a sequence's
 * statistics non-finite (q = 1 with every window of a sequence on a zero of v: Z = 0; NaN or infinite odds), the
 * pass still runs: the log-likelihood of that pass (bamm_em_get_llh, the trace) is NaN -- the reference's float
 * sum would hold -inf or NaN there --, r of such a sequence is undefined and adds nothing to the counts, every other
 * sequence is computed as usual, and nothing outlives the handle.                                              */
int  bamm_em_create(bamm_ctx* ctx, bamm_seqs* seqs, const bamm_em_params* params,
                    const float* vbg, const float* A, const float* v_init,
                    const uint8_t* seq_mask, bamm_em** out);
int  bamm_em_destroy(bamm_em* em);

/* EM::EStep (EM.cpp:139-200): s from the current v, responsibilities, log-likelihood.        */
int  bamm_em_estep(bamm_em* em);
/* EM::MStep (EM.cpp:217-259): counts from the responsibilities of the last EStep, updateV.   */
int  bamm_em_mstep(bamm_em* em);
/* EM::optimize_q (EM.cpp:505-519) from the responsibilities of the last EStep.  May be called
 * before or after the MStep (the reference calls it after, EM.cpp:93-99): getR() and MStep() keep
 * seeing the q that EStep used.                                                                */
int  bamm_em_optimize_q(bamm_em* em);
/* n fused EStep+MStep(+optimize_q while iteration<=5) passes, no convergence test, no host
 * round trip in between (benchmark / fixed-budget mode).                          */
int  bamm_em_iterate(bamm_em* em, uint32_t n);
/* EM::optimize (EM.cpp:62-137) including the stopping rule; *iterations = passes executed.   */
int  bamm_em_optimize(bamm_em* em, uint32_t* iterations);
/* EM::mask (EM.cpp:261-503, the `--advanceEM` path; f = Global::f, Global.cpp:54): an order-0
 * pass over every window, the global cut-off at the f-quantile of the responsibilities, then EM
 * restricted to the windows at or above it until the stopping rule fires.  Like both reference
 * call sites (mainBaMM.cpp:131-137, FDR.cpp:67-70) it expects a handle that has not run an
 * E-step yet.  With optimize_q the reference re-estimates q after every sequence of the first
 * pass (EM.cpp:321); that chain is inherently serial and is not offered across ranks
 * (BAMM_ERR_UNSUPPORTED when an all-reduce is installed).  W = 1 is refused: the reference
 * reads one float past its allocation there (EM.cpp:416).  *cutoff / *listed are optional.     */
int  bamm_em_mask(bamm_em* em, float f, uint32_t* iterations, float* cutoff, uint64_t* listed);

/* multi-GPU: between the local accumulation and the model update the fused accumulator
 * [n_K (4^(K+1)*W, [y][j]) | llh | sum_r | n_seqs] is summed across ranks.  It holds SIGNED 64-BIT
 * INTEGERS (fixed point: counts in units of 2^-40, llh 2^-24, sum_r 2^-30, n_seqs 1), on the device,
 * written on the context's stream: sum it as int64 (ncclInt64 / torch.int64) -- integer sums are
 * exact and order-free, so the model does not depend on the number of ranks.  The blocks of the
 * sequence kernels add into it directly; bamm_em_update consumes it and leaves it zeroed.
 * Either drive the three phases by hand ...                                                    */
int  bamm_em_accumulate(bamm_em* em);
int  bamm_em_reduce_buffer(bamm_em* em, void** dev_ptr, uint64_t* n_words);
int  bamm_em_update(bamm_em* em);
/* let the accumulator live in memory the caller allocated (e.g. a torch.int64 tensor that is handed
 * to torch.distributed.all_reduce): n_words >= 4^(K+1)*W + 3; the caller keeps ownership.        */
int  bamm_em_set_reduce_buffer(bamm_em* em, void* dev_ptr, uint64_t n_words);
/* ... or install a callback that bamm_em_iterate/optimize/mstep invoke at that point (int64 sum
 * of n_words words at dev_ptr, enqueued on hip_stream; EM::mask's window histogram goes through
 * the same callback) ...                                                                        */
typedef int (*bamm_allreduce_fn)(void* user, void* dev_ptr, uint64_t n_words, void* hip_stream);
int  bamm_em_set_allreduce(bamm_em* em, bamm_allreduce_fn fn, void* user);

/* ... or hand the handle a communicator: every pass then ends its accumulation with one
 * ncclAllReduce(ncclInt64, ncclSum) of the accumulator over RCCL / xGMI on the context's stream (the
 * reduction the reference gets from its OpenMP reduction clause and float atomics, EM.cpp:148,240,
 * 509-513).  The communicator must belong to the handle's context; it outlives the handle.       */
int  bamm_em_set_comm(bamm_em* em, bamm_comm* comm);

/* ------------------------------------------------------------------ communicators (RCCL) -- */
/* librccl is opened at the first of these calls; BAMM_ERR_COMM carries RCCL's message.         */
#define BAMM_COMM_ID_BYTES 128
/* one process, n devices: a communicator per context (distinct devices), ncclCommInitAll.  Drive
 * each context from a host thread of its own (as FDR.cpp:37 does with its folds).              */
int  bamm_comm_init_all(bamm_ctx* const* ctxs, uint32_t n, bamm_comm** out /* [n] */);
/* one process per device: rank 0 makes an id (BAMM_COMM_ID_BYTES bytes), the launcher carries it
 * to the other ranks (MPI, a file, torch.distributed ...), every rank calls init_rank.        */
int  bamm_comm_unique_id(void* id_out, size_t cap);
int  bamm_comm_init_rank(bamm_ctx* ctx, const void* id, uint32_t rank, uint32_t world, bamm_comm** out);
/* one process, n contexts on ANY devices (the same one included): the sum is staged through pinned host memory
 * between the ranks' host threads, no RCCL.  max_words >= the largest buffer summed (4^(K+1)*W + 3; EM::mask: 2049).
 * For self-tests of the N > 1 logic on a 1-GPU box and for hosts without librccl; *rccl_version reports 0.       */
int  bamm_comm_init_local(bamm_ctx* const* ctxs, uint32_t n, uint64_t max_words, bamm_comm** out /* [n] */);
/* the same between PROCESSES of one host: the sum is staged through a POSIX shared-memory segment `name` ("/something";
 * created by whichever rank comes first, unlinked once all `world` ranks are attached).  Every rank calls it with the same
 * name, world and max_words.  Every wait is bounded (a rank that does not arrive within a minute aborts the group).  For
 * self-tests -- it lets the cross-process half of the in-kernel all-reduce (hipIpc-mapped inboxes) run between two processes
 * on a 1-GPU box, where RCCL refuses two ranks on one device -- and for hosts without librccl.                          */
int  bamm_comm_init_shm(bamm_ctx* ctx, const char* name, uint32_t rank, uint32_t world, uint64_t max_words, bamm_comm** out);
int  bamm_comm_info(const bamm_comm* c, uint32_t* rank, uint32_t* world, int* rccl_version);
/* a rank that fails calls this on its communicator (any thread): the collectives its peers are blocked in return
 * BAMM_ERR_COMM instead of waiting for it for ever (ncclCommAbort; the local kind wakes its waiters).  Safe to call
 * from several threads at once on the same handle (one of them aborts, the others return).  The handle stays valid
 * for bamm_comm_destroy only; every later collective on it, and every result read from an EM handle that was using it,
 * fails with BAMM_ERR_COMM.                                                                                       */
int  bamm_comm_abort(bamm_comm* c);
int  bamm_comm_destroy(bamm_comm* c);
/* a bare loop of `iters` all-reduces of `n_words` int64 words on the context's stream (20 untimed ones first), timed with
 * HIP events: microseconds per call.  Collective: every rank of the communicator calls it with the same arguments.  What
 * a sharded iteration pays for its one collective (bench.py reports it beside the kernel time for N > 1).           */
int  bamm_comm_time_allreduce(bamm_comm* c, uint64_t n_words, uint32_t iters, float* us_per_call);
/* `count` consecutive draws of glibc's rand() stream as srand(seed) leaves it, starting behind its first `skip` draws:
 * from the restated generator (csrc/glibc_rand.h) entered by jump-ahead (use_jump != 0) or stepped `skip` times, or --
 * use_jump < 0 -- from libc's own srand(seed) / rand() (which this then advances).  *matches_libc (may be NULL): whether the
 * process-wide check found libc's rand() to be this generator.  How the N draws of Sequence.cpp:38 and the negative
 * sampler (SeqGenerator.cpp:188-348) enter the one stream in the middle, on host threads and on the device.     */
int  bamm_rand_stream_draws(uint32_t seed, uint64_t skip, int use_jump, uint32_t count, int32_t* out, int* matches_libc);
/* How this handle's passes are summed over the ranks: 0 = not at all (no communicator, no callback), 1 = one collective
 * per pass (RCCL, the host-staged group, or the caller's callback), 2 = inside the sequence kernels over peer-mapped
 * inboxes (bamm_ctx_set_tuning "peer_allreduce" = 1 on EVERY rank's context before the handle is created; default off).
 * Mode 2: the last block of a pass's launch to finish stores the GPU's totals into every peer's inbox (fine-grained device
 * memory, mapped through the process or hipIpc*; 8-byte entries that carry the pass's sequence number, so no fence and
 * no separate flag), collects the peers' entries as they arrive and leaves the sum in the accumulator, in place: no
 * collective launch behind the pass.  Same integers, same model.  Every poll is bounded ("peer_timeout_ms", default
 * 2000): a block that waits in vain raises a device flag that turns the handle's later launches into no-ops, and the
 * next result read from the handle fails with BAMM_ERR_COMM.  Applies to handles whose pass is ONE launch of a
 * grouped-column kernel built with the tail -- the mixed-row kernel (K = 2, both strands, W = 13, 14, 16, 17 or 20: the shapes
 * of BASELINE configs 2, 3 and 5) and the uniform-row kernel at K <= 2 (single strand, k = 0 / 1, other widths) -- over one
 * length class of at most 1024 positions, on 2..8 ranks; the ranks vote, and one that cannot keeps all of them on mode 1 (`note` then says why).  Collective on first use: every rank calls it (or starts its first pass). */
int  bamm_em_comm_mode(bamm_em* em, int* mode, char* note, size_t note_cap);
/* HIP devices visible to the process (0 and BAMM_ERR_NO_DEVICE when there is none)                               */
int  bamm_device_count(int* n);
/* Where a device sits and whom it reaches -- what a first multi-GPU run wants on record beside its numbers: the PCI bus id
 * ("0000:c1:00.0") of a visible device, and whether `device` can address `peer`'s memory directly (hipDeviceCanAccessPeer:
 * xGMI or PCIe peer-to-peer; the in-kernel all-reduce of bamm_em_comm_mode 2 and RCCL's direct rings need it).  No context is
 * created and nothing is enabled.                                                                                   */
int  bamm_device_pci_bus_id(int device, char* buf, size_t cap);
int  bamm_device_can_access_peer(int device, int peer, int* can);

/* results (each synchronises the stream)                                                     */
int  bamm_em_get_v(bamm_em* em, float* v_flat);        /* Motif::getV()                       */
int  bamm_em_get_counts(bamm_em* em, float* n_flat);   /* EM::n_   (EM.h:54)                  */
int  bamm_em_get_s(bamm_em* em, float* s);             /* Motif::getS() after EStep           */
int  bamm_em_get_q(bamm_em* em, float* q);             /* EM::getQ()                          */
int  bamm_em_get_llh(bamm_em* em, float* llh);         /* EM::llikelihood_ (EM.h:61)          */
int  bamm_em_get_vdiff(bamm_em* em, float* v_diff);    /* EM.cpp:102-108, last pass           */
int  bamm_em_get_iteration(bamm_em* em, uint32_t* it);
/* EM::getR() for sequences [begin,end): recomputed on demand from the s of the last EStep,
 * written in the reference's layout; out_off[n] = offset of sequence begin+n in `out`.       */
int  bamm_em_get_r(bamm_em* em, uint64_t begin, uint64_t end, float* out, uint64_t out_cap);
/* The windows of sequences [begin,end) with r >= cutoff -- r as bamm_em_get_r would report it at this moment, same
 * preconditions, same errors -- and per sequence the best window.  What EM::write puts into .positions at 0.3
 * (EM.cpp:577-601) and what GibbsSampling.cpp:105-116 initialises z from.  The dense r is produced on the device as
 * for bamm_em_get_r (a range of a handle on the fused kernels: in chunks of whole sequences of at most
 * "sites_chunk_positions" positions, a longer sequence alone) and reduced there (csrc/sites.hip): a count per
 * sequence, a prefix sum, then every hit stored at its rank.  The order is ascending (sequence, window start) and
 * does not depend on scheduling.  What crosses to the host: three words per sequence and 12 bytes per site.  NaN
 * cutoff: BAMM_ERR_ARG.  cutoff <= 0 lists every window i <= L-W (never the zero slots behind).  begin == end: an
 * empty result.  Sequences a seq_mask excludes still report, as in getR.  Pass counters and event bookkeeping of the
 * handle stay as they were.  The result owns host arrays; bamm_sites_destroy releases it.                         */
typedef struct bamm_sites bamm_sites;
int  bamm_em_sites(bamm_em* em, uint64_t begin, uint64_t end, float cutoff, bamm_sites** out);
int  bamm_sites_info(const bamm_sites* s, uint64_t* n_sites, uint64_t* n_seqs);
/* per site, ascending (sequence, window start): sequence index in the handle's set, i (0-based), r; any pointer may
 * be NULL; cap = elements each array holds (>= n_sites)                                                          */
int  bamm_sites_get(const bamm_sites* s, uint64_t* seq, uint32_t* pos, float* r, uint64_t cap);
/* per sequence of the range: z (0 = no window with r > 0, else the first arg-max window + 1) and its r (0 with z = 0);
 * the number of its sites; any pointer may be NULL; cap >= n_seqs                                                */
int  bamm_sites_best(const bamm_sites* s, uint32_t* z, float* r_best, uint32_t* count, uint64_t cap);
int  bamm_sites_destroy(bamm_sites* s);
/* per-iteration trace of optimize()/iterate(): what the reference prints with --verbose
 * (EM.cpp:112-115).  Returns up to cap entries, *n = entries available.                      */
int  bamm_em_get_trace(bamm_em* em, float* llh, float* v_diff, float* q, uint32_t cap, uint32_t* n);
/* device time of the sequence kernel over the last iterate()/optimize() call (HIP events on
 * the context's stream): total milliseconds over the timed passes and their number.  Passes
 * 0, every, 2*every, ... of a call are timed (default every = 8; 1 = all, 0 = none): an event
 * pair takes 7-8 us of stream time, which a short iteration notices.  BAMM_TIMING_WHOLE_CALL:
 * one pair around ALL passes of the call (first event in front of the first pass's kernel, second
 * behind the last pass's): every pass covered at no cost per pass; the interval includes the
 * launch gaps and whatever runs between two passes (a collective), `launches` = the passes in it. */
#define BAMM_TIMING_WHOLE_CALL 0xffffffffu
int  bamm_em_kernel_time(bamm_em* em, float* total_ms, uint32_t* launches);
int  bamm_em_set_kernel_timing(bamm_em* em, uint32_t every);
/* how one pass is laid out: sequences that go through the grouped-column kernel (grouped.hip)
 * and through the one-column-at-a-time kernel (kernels.hip), and the kernel launches per pass. */
int  bamm_em_plan(bamm_em* em, uint64_t* grouped_seqs, uint64_t* percolumn_seqs, uint32_t* launches);
/* of the grouped ones: sequences that go through the mixed-row flavour (csrc/mixed_kernel.h: K = 2, the motif's
 * last W mod 3 groups of four columns on 6-mer rows)                                              */
int  bamm_em_plan_mixed(bamm_em* em, uint64_t* mixed_seqs);
/* launch `index` (0 .. launches-1 of bamm_em_plan) of a pass: out[4] = its sequences, the positions per lane of the length
 * class it RUNS in (0: beyond the classes), 1 for the mixed-row kernel, 1 for that kernel's start-anchored flavour (the
 * windows anchored at their start: the class run is then shorter than the class of the sequences' lengths; "mix_anchor"
 * = 0 in bamm_ctx_set_tuning plans none).  BAMM_ERR_ARG beyond the last launch.                                  */
int  bamm_em_plan_launch(bamm_em* em, uint32_t index, uint64_t* out);
/* which of the other paths the handle takes: *sliced = 1 when its tables exceed one CU's LDS and a pass runs column
 * slices (k >= 4 at usual widths); *e_fused = 1 when the E pass of such a handle still holds the whole odds table (r in the
 * reference's layout), 0 when it is sliced as well (r per position slot); *long_seqs = sequences outside the length
 * classes: beyond BAMM_MAX_SEQ_POSITIONS, or every sequence of a model whose tables stay in global memory (orders >= 7) --
 * tile by tile or window by window, bamm_em_tile_plan tells which.  Any pointer may be NULL.                   */
int  bamm_em_plan_paths(bamm_em* em, int* sliced, int* e_fused, uint64_t* long_seqs);
/* which form of the model update the handle's update launches run: *form = 0 one block with every order of n and v in
 * LDS (at most 2048 cells of the top order), 1 one block on global memory ("update_blocks" = 0 in bamm_ctx_set_tuning),
 * 2 spread over blocks in bands of orders; *fusable = 1 when iterate() / optimize() run the update of a pass in the
 * prologue of the next pass's first kernel instead ("fused_update" = 0 plans none; a caller-owned reduce buffer ends it).
 * No device work; either pointer may be NULL.                                                                    */
int  bamm_em_plan_update(const bamm_em* em, int* form, int* fusable);
/* The tiles an EM pass cuts a sequence longer than BAMM_MAX_SEQ_POSITIONS into, for motifs of width W: the scorer's
 * rule (bamm_score_tile_geometry) with the EM kernels' own positions per lane.  Pure host arithmetic, no device needed;
 * either pointer may be NULL.  BAMM_ERR_ARG for W = 0 and for a W that leaves no stride of at least 16.              */
int  bamm_em_tile_geometry(uint32_t W, uint32_t* tile_positions, uint32_t* stride);
/* Of the handle's long_seqs (bamm_em_plan_paths): *tiled_seqs go tile by tile (csrc/em_tiles.hip), in *tiles tiles
 * (counted without the sequence mask), *window_seqs window by window (long_seq.hip: sliced handles, tables in global
 * memory, a W that leaves no stride, "em_tiles" = 0).  Any pointer may be NULL.                                 */
int  bamm_em_tile_plan(bamm_em* em, uint64_t* tiled_seqs, uint64_t* tiles, uint64_t* window_seqs);
/* The launch geometry bamm_em_mask computes for a model of width W with Y = 4^(K+1) rows (cells = W * Y) on a set of
 * n_seqs sequences, the longest of max_len positions, on a device of num_cus CUs -- a pure function, exported for tests
 * (no device needed).  out[13]: direct, wave_global, wave_bytes, s_in_lds, e_table, m_cols, m_table, init_table, e_waves,
 * m_waves, cus, mblocks, wave_scratch_bytes (csrc/handles.h: MaskPlan).                                           */
int  bamm_mask_plan(uint32_t W, uint32_t Y, uint32_t max_len, uint64_t n_seqs, uint64_t cells, int num_cus, uint64_t* out);

/* The mixed-row kernel's layout at K = 2 for motif width W and M positions per lane, and one lane's fix-lane word of the lane
 * records its handles build (csrc/lane_records.h) -- pure functions, exported for tests (no device needed).
 * bamm_mix_layout: out[4] = T groups, of which the first B are narrow, A wide, n1c leading columns with resident bins in
 * the accumulating pass; BAMM_ERR_UNSUPPORTED where the mixed rows do not apply.
 * bamm_mix_fix_word: lane 0..63 of a sequence of L positions; xw = the first word of its group record (lo | B << 12);
 * xfields = the exact y, 7 bits each, of the four positions that end at the lane's junction row; sE = the 2-bit stream
 * window that ends at position L - W.  out[2] = the record's word y (four 7-bit column codes, 64 = none; bit 31 =
 * something is left to log), 1 if the lane is a fix lane of the sequence.                                          */
int  bamm_mix_layout(uint32_t W, int M, uint32_t* out);
int  bamm_mix_fix_word(uint32_t lane, uint32_t W, uint32_t T, uint32_t B, uint32_t n1c, uint32_t L, uint32_t xw, uint32_t xfields,
                       uint32_t sE, uint32_t* out);

/* ------------------------------------------------------------------ seeding ------------- */
/* The pass over the sequences of Motif::initFromPWM (Motif.cpp:228-311): 0th-order posterior of
 * every window, one motif start sampled per sequence, integer k-mer counts of the sampled sites
 * for the orders 0..K.  score = floored PWM / 0th-order background, [4][W] (Motif.cpp:205-226).
 * u[n]: the uniform variate the reference's std::discrete_distribution would draw for sequence n
 * (std::generate_canonical<double,53> on the default-seeded std::mt19937 of Motif.cpp:237, drawn
 * in sequence order for the sequences with L >= W only).  counts: v_size(K,W) ints, flat
 * [k][y][j].  z (may be NULL): the sampled index per sequence, 0 = no motif, i = window i-1.   */
int  bamm_seed_from_pwm(bamm_ctx* ctx, bamm_seqs* seqs, uint32_t K, uint32_t W, const float* score,
                        float q, const double* u, int32_t* counts, uint32_t* z);

/* ------------------------------------------------------------------ scorer -------------- */
/* ScoreSeqSet::calcLogOdds (ScoreSeqSet.cpp:25-67) with Motif::calculateLogS
 * (Motif.cpp:471-483).  mops (may be NULL): concatenated L-W+1 scores per sequence;
 * zoops[n_seqs], z[n_seqs] (first arg-max).                                                  */
int  bamm_logodds(bamm_ctx* ctx, bamm_seqs* seqs, uint32_t K, uint32_t W, uint32_t bg_order,
                  const float* v_flat, const float* vbg, float* mops, uint64_t mops_cap,
                  float* zoops, uint64_t* z);

/* same, restricted to the sequences with seq_mask[n] != 0 (the others report 0): the test /
 * negative subsets of one CV fold over a shared resident set (FDR.cpp:49-60,84-89).          */
int  bamm_logodds_subset(bamm_ctx* ctx, bamm_seqs* seqs, const uint8_t* seq_mask, uint32_t K, uint32_t W,
                         uint32_t bg_order, const float* v_flat, const float* vbg, float* mops,
                         uint64_t mops_cap, float* zoops, uint64_t* z);

/* The tiles the scorer cuts a sequence longer than BAMM_MAX_SEQ_POSITIONS into, for motifs of width W: a tile holds
 * tile_positions consecutive positions and starts on a multiple of stride (a multiple of 16, at most
 * tile_positions - (W - 1)); it scores the windows that start in its first `stride` positions, the sequence's last tile
 * up to window L - W.  Pure host arithmetic, no device needed; either pointer may be NULL.  BAMM_ERR_ARG for W = 0 and
 * for a W that leaves no stride of at least 16 (such motifs are scored window by window).                          */
int  bamm_score_tile_geometry(uint32_t W, uint32_t* tile_positions, uint32_t* stride);
/* The slices of motif columns the scorer cuts a log-odds table of order K and width W into under "score_slices" = 1:
 * cmax = floor(163840 / ((4^(K+1) + 1) * 4)) columns fit one CU's LDS, *slices = ceil(W / cmax), *columns_per_slice =
 * ceil(W / slices) (balanced; the last slice may be shorter).  slices == 1: the table fits whole.  Pure host arithmetic, no
 * device needed; either pointer may be NULL.  BAMM_ERR_ARG for W = 0, K > BAMM_MAX_ORDER and where not one column fits
 * (orders 7..10, which are scored window by window whatever the key says).                                          */
int  bamm_score_slice_geometry(uint32_t K, uint32_t W, uint32_t* columns_per_slice, uint32_t* slices);
/* Which kernel the scorer takes for the sequences of `seqs` with a model of order K and width W, under the context's
 * tuning as it stands: sequences held in one wavefront's registers, sequences cut into tiles (and the number of tiles,
 * without a sequence mask), sequences walked window by window with the table in global memory.  Any pointer may be NULL. */
int  bamm_score_plan(bamm_ctx* ctx, const bamm_seqs* seqs, uint32_t K, uint32_t W, uint64_t* wave_seqs,
                     uint64_t* tiled_seqs, uint64_t* tiles, uint64_t* window_seqs);

/* ------------------------------------------------------------------ occurrences --------- */
/* ScoreSeqSet::calcPvalues + the cut of ScoreSeqSet::write (ScoreSeqSet.cpp:70-126, :245-291): every window of the
 * positives whose p-value is below p_cutoff, in ascending (sequence, window start) order.  Both sets are scored on the
 * device, the negatives' scores are sorted there (ascending, as the reference sorts them) and every positive window is
 * ranked against them there; what crosses to the host are the lowest nTop + 1 negative scores, a counter and the
 * candidate windows -- those the device's own evaluation of the interpolation branch (:118-124) puts below the cut-off
 * or leaves undecided (FPl < 10 with the exponential tail, :114-116: glibc's expf; a p that is not finite).  The host
 * evaluates the reference's formula on the candidates with the code behind the CLI's --hostPvalues path, so p and e are
 * that path's bits.  nTop = min(100, (int)negN / 10), S_ntop and lambda come from the LOWEST scores, as in the reference.
 * One corner is undefined there and decided here: FPl = 0 with |lambda| <= 1e-5 reads one element past the sorted
 * negatives (:120); this call takes +infinity for it (p = 0), the host path keeps reading what lies there.
 * Errors: sets of another context, a sequence shorter than W, no negative window, more than 2^31 - 1 negative windows
 * (the reference's (int)negN).  The result owns host arrays; bamm_occ_destroy releases it.                          */
typedef struct bamm_occ bamm_occ;
int  bamm_occurrences(bamm_ctx* ctx, bamm_seqs* positives, bamm_seqs* negatives, uint32_t K, uint32_t W,
                      uint32_t bg_order, const float* v_flat, const float* vbg, float p_cutoff, bamm_occ** out);
/* hits, negative windows, nTop, S_ntop, lambda, candidates the device handed over (>= hits); any pointer may be NULL */
int  bamm_occ_info(const bamm_occ* occ, uint64_t* n_hits, uint64_t* n_neg_scores, uint32_t* n_top, float* s_ntop,
                   float* lambda, uint64_t* n_candidates);
/* per hit: sequence, window start i (0-based), log-odds score, FPl, p, e = p * (float)n_positives; any pointer may be
 * NULL; cap = elements each array holds (>= n_hits)                                                              */
int  bamm_occ_get(const bamm_occ* occ, uint64_t* seq, uint32_t* pos, float* score, uint64_t* fp, float* p, float* e,
                  uint64_t cap);
int  bamm_occ_destroy(bamm_occ* occ);

/* ------------------------------------------------------------------ FDR --mops statistics */
/* FDR::calculatePR's MOPS branch and FDR::calculatePvalues (FDR.cpp:156-196, :278-333) over window scores that stay on
 * the device (csrc/fdr.hip).  A handle collects two lists, positive and negative window scores, in device arrays from
 * the context's scratch pool; bamm_fdr_statistics sorts them there, walks the merged order in parallel (a merge-path
 * search per block and per thread) and finds E_TP and idx_max; rows and p-values are computed for the range a call
 * names and only those cross to the host.  Every number is the host path's (host/fdr.cpp), bit for bit: both evaluate
 * csrc/fdr_rows.h.  As there, an exhausted list loses every comparison where the reference reads past its end.
 *   add_set     scores `set` (the sequences with seq_mask[n] != 0; NULL = all) with the scorer's kernels and appends the
 *               windows' scores behind what earlier calls added: the folds of one motif, each with its own model
 *   add_scores  appends scores the caller holds
 *   statistics  posN / negN: the SEQUENCE counts of FDR.cpp:152,164 (mFold, idx_max's initial value); afterwards the
 *               handle accepts no more scores.  with_pvalues: bamm_fdr_pvalues may be called
 *   info        scores in each list, rows = min(idx_max, n_pos + n_neg), E_TP, occ_mult = E_TP / posN; any may be NULL
 *   rows        TP, FP, FDR, recall of rows begin <= i < end <= n_rows; any array may be NULL
 *   pvalues     the p-value of the ascending positive scores begin <= i < end <= n_pos
 *   geometry    steps of the walk one thread / one block owns in this build (tests straddle them)
 * Folds that ran on several contexts or devices collect on a handle each and are brought together before statistics:
 *   seal        sorts both lists where they lie, on the handle's own context, into one ascending RUN each (an empty list
 *               seals to an empty run) and returns when they are in place; afterwards the handle accepts no more scores
 *               and cannot absorb, but may be absorbed or run statistics.  A second call is a no-op
 *   absorb      moves everything `src` holds into `dst`; `src` is empty afterwards and can only be destroyed.  A sealed
 *               `src` arrives as one more run per list, an unsealed one behind `dst`'s open (unsorted) scores, keeping
 *               the runs it had absorbed itself.  The handles may belong to different contexts: a device-to-device copy
 *               on `dst`'s stream behind an event of `src`'s stream, a peer copy between devices, the two contexts'
 *               pinned staging areas where the devices cannot reach each other; a list that arrives at an empty one on
 *               its own context brings its block along and nothing is copied.  Blocks come from and go back to the
 *               respective context's scratch pool
 *   statistics  (again) sorts what is still open into a run and MERGES each list's runs (two by two, ceil(log2 runs)
 *               streaming passes) instead of sorting them again.  The sort writes canonical bits (-0 as +0), equal keys
 *               are equal bits: the merged list is, bit for bit, the sorted concatenation, and every output is what one
 *               handle given all the scores reports
 * Errors: a set of another context, a sequence shorter than W, more than 2^32 - 1 scores in a list (the sort's index
 * width), statistics without any score, scores after statistics or seal, a range outside the rows / the positives.
 * seal and absorb return BAMM_ERR_ARG and leave both handles as they were for: dst == src, a handle past statistics (or
 * already absorbed), a sealed dst, a list of dst that would exceed 2^32 - 1 scores.                                */
typedef struct bamm_fdr bamm_fdr;
int  bamm_fdr_create(bamm_ctx* ctx, bamm_fdr** out);
int  bamm_fdr_add_set(bamm_fdr* fdr, int negative, bamm_seqs* set, const uint8_t* seq_mask, uint32_t K, uint32_t W,
                      uint32_t bg_order, const float* v_flat, const float* vbg);
int  bamm_fdr_add_scores(bamm_fdr* fdr, int negative, const float* scores, uint64_t n);
int  bamm_fdr_seal(bamm_fdr* fdr);
int  bamm_fdr_absorb(bamm_fdr* dst, bamm_fdr* src);
int  bamm_fdr_statistics(bamm_fdr* fdr, uint64_t posN, uint64_t negN, int with_pvalues);
int  bamm_fdr_info(const bamm_fdr* fdr, uint64_t* n_pos, uint64_t* n_neg, uint64_t* n_rows, float* e_tp, float* occ_mult);
int  bamm_fdr_rows(bamm_fdr* fdr, uint64_t begin, uint64_t end, float* tp, float* fp, float* fdr_out, float* rec);
int  bamm_fdr_pvalues(bamm_fdr* fdr, uint64_t begin, uint64_t end, float* p);
int  bamm_fdr_geometry(uint32_t* steps_per_thread, uint32_t* steps_per_block);
int  bamm_fdr_destroy(bamm_fdr* fdr);

/* Sequence::Sequence where the data will live: bamm_pack_codes_seeded + bamm_seqs_upload with the packing done on the
 * device (csrc/prep.hip) -- reverse complement, 2-bit stream, kmer_[i] next to unknown bases term by term with the
 * reference's rand() draws, the exception list.  The draws themselves are taken on the host (libc's one stream, entered
 * by jump-ahead on all threads).  *packed_out receives the same packed set bamm_pack_codes_seeded returns, array for
 * array (bamm_packed_free releases it); *seqs_out (may be NULL) the resident set.                                 */
int  bamm_seqs_from_codes(bamm_ctx* ctx, const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int single_strand,
                          uint32_t seed, bamm_packed** packed_out, bamm_seqs** seqs_out);
/* bamm_bg_model over a resident set: the counting pass of BackgroundModel (BackgroundModel.cpp:26-42) on the device,
 * calculateV (:441-473) on the handful of counts it leaves.  Same vbg_out as bamm_bg_model on the packed set.      */
int  bamm_seqs_bg_model(bamm_ctx* ctx, bamm_seqs* seqs, uint32_t K, const float* alpha, float* vbg_out);

/* SeqGenerator::sample_bgseqset_by_fold (SeqGenerator.cpp:63-348) on the device (csrc/negs.hip): m_fold negatives per
 * resident positive, each as long as its positive, every base one draw of the rand() stream srand(42) starts -- the
 * reference's negatives, base for base.  keep_stride > 1: only the negatives 0, stride, 2 stride, ... (with idx + stride <=
 * total) are generated and returned, which is all --FDR scores (FDR.cpp:58-60); the others still own their draws.
 * generic != 0: --genericNeg (the set's own conditionals for every positive).  *packed_out: the negatives as a packed set
 * (single strand, no exceptions; bamm_packed_free), *seqs_out (may be NULL): resident.  Any length: a negative of a
 * positive beyond BAMM_MAX_SEQ_POSITIONS is cut into segments (bamm_neg_segment_geometry), a lane per segment: from its
 * third position on a base is a function of the two bases before it and of its own draw, so a segment is a map over 16
 * contexts, and the maps compose exactly.  BAMM_ERR_UNSUPPORTED (the caller samples on the host instead): s_order != 2,
 * an empty set, a libc whose rand() is not glibc's generator.                                                     */
int  bamm_sample_negatives(bamm_ctx* ctx, bamm_seqs* positives, uint32_t s_order, uint64_t m_fold, int generic,
                           uint64_t keep_stride, bamm_packed** packed_out, bamm_seqs** seqs_out);
/* Positions per segment of a long negative (a multiple of 16: a 2-bit word belongs to one segment), as
 * bamm_sample_negatives cuts it unless "neg_segment_positions" is set.  Pure, no device needed: tests use it to place
 * sequence lengths on the cuts.                                                                                   */
int  bamm_neg_segment_geometry(uint32_t* segment_positions);

/* ------------------------------------------------------------------ w-mer counts -------- */
/* The exact w-mer table of a resident set, w = 6..8 (anything else: BAMM_ERR_ARG) -- what the de novo seeder of the
 * BaMMmotif driver ranks (--seedKmers; the reference has no such stage).  In terms of the FASTA codes the set was built
 * from (0 = unknown, 1..4 = A,C,G,T): every window of w consecutive codes of a record with no 0 in it adds 1 to counts[y],
 * y = the window read as a base-4 number of the codes minus 1, oldest base most significant (the digit order of kmer_);
 * unless the set is single-stranded the window's reverse complement adds 1 as well, so a reverse-palindromic window adds
 * 2 to its own cell.  No window spans the strand separator, and the bases Sequence.cpp:38 draws for unknown positions are
 * not counted: the table does not depend on the rand() stream.  *n_windows (may be NULL) = the sum of the table.
 * Records of any length: one beyond BAMM_MAX_SEQ_POSITIONS ("kmer_segment_positions" in bamm_ctx_set_tuning: 16..2^20,
 * rounded down to a multiple of 16) goes through the same kernel in segments that overlap by w - 1 positions.  The table
 * is privatised in LDS per workgroup (32-bit cells; at w = 8 two workgroups share a block's records, each with the half of
 * the table its leading base selects) and flushed into 64-bit cells; a workgroup also flushes after
 * "kmer_flush_windows" windows (default 2^31), so no LDS cell wraps.  bamm_ctx_set_launch's blocks apply.
 * The set must know where its unknown bases were: bamm_seqs_upload of a set bamm_pack_codes* made -- the list is noted
 * beside the packed set, by its address, until bamm_packed_free releases it (release every packed set through that call: a
 * bamm_packed copied by value has no list, and one freed any other way would leave its note to whatever is allocated at
 * that address next).  Every other set cannot tell and is refused with BAMM_ERR_UNSUPPORTED: one packed from kmer_ arrays
 * (bamm_pack_kmers*, the sampled negatives) and, as yet, one bamm_seqs_from_codes packed on the device.  The strand mode
 * is the one the packed set was made with.                                                                         */
int  bamm_kmer_counts(bamm_ctx* ctx, const bamm_seqs* seqs, uint32_t w, uint64_t* counts /* [4^w] host */,
                      uint64_t* n_windows);
/* The same table from the codes themselves, on the host threads (bamm_set_host_threads): the same integers for codes
 * 0..4, which is all the FASTA reader produces.  A code above 4 counts as unknown here, while the packers encode it as
 * (code - 1) mod 4 and list only code 0: the two tables agree on codes 0..4 only.                                  */
int  bamm_kmer_counts_host(const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int single_strand, uint32_t w,
                           uint64_t* counts /* [4^w] */, uint64_t* n_windows);
/* Dyad tables: w-mers whose two halves lie apart (--seedGaps).  For even w in {6, 8}, half h = w / 2, gap g >= 0 and span
 * S = w + g <= 16 (g <= 10 at w = 6, g <= 8 at w = 8): every window of S consecutive codes of a record with no 0 ANYWHERE in
 * the span, the g gap positions included, adds 1 to counts[g - gap_lo][y], y = the window's first h codes followed by its
 * last h codes (minus 1 each) read as a base-4 number, oldest base most significant.  Unless the set is single-stranded the
 * window's reverse complement adds 1 as well: with equal halves that is an (h, g, h) window again, so the table of every gap
 * is its own reverse complement and a reverse-palindromic dyad adds 2 to its own cell.  No window spans the strand
 * separator, and the bases drawn for unknown positions are never counted.  g = 0 is bamm_kmer_counts' table exactly (w = 7
 * is accepted with gap_lo = gap_hi = 0 only).  The tables of gaps gap_lo..gap_hi come from ONE launch whose grid has the
 * gaps as its third axis; n_windows[g - gap_lo] (may be NULL) = the sum of that gap's table.  BAMM_ERR_ARG: gap_lo > gap_hi,
 * w + gap_hi > 16, odd w with gap_hi > 0 (unequal halves would not map onto themselves under reverse complement), w
 * outside 6..8, a set of another context; BAMM_ERR_UNSUPPORTED: a set without a list of unknown positions, as above.  An
 * empty set gives zeroed tables.  "kmer_segment_positions" (segments overlap by S - 1 <= 15 positions: still the one word a
 * lane reads before its own), "kmer_flush_windows" and bamm_ctx_set_launch's blocks apply as they do above.        */
int  bamm_kmer_counts_gapped(bamm_ctx* ctx, const bamm_seqs* seqs, uint32_t w, uint32_t gap_lo, uint32_t gap_hi,
                             uint64_t* counts /* [(gap_hi-gap_lo+1) * 4^w] host */,
                             uint64_t* n_windows /* [gap_hi-gap_lo+1] or NULL */);
/* The same tables from the codes, on the host threads: the same integers for codes 0..4.                           */
int  bamm_kmer_counts_gapped_host(const uint8_t* codes, const uint64_t* off, uint64_t n_seqs, int single_strand,
                                  uint32_t w, uint32_t gap_lo, uint32_t gap_hi, uint64_t* counts, uint64_t* n_windows);

/* ------------------------------------------------------------------ small host helpers -- */
/* BackgroundModel ctor + calculateV (BackgroundModel.cpp:3-46, :441-473): interpolated
 * order-K conditionals learned from a packed set; alpha[K+1]; vbg_out[bamm_bg_size(K)].     */
int  bamm_bg_model(const bamm_packed* p, uint32_t K, const float* alpha, float* vbg_out);
/* Motif::calculateP (Motif.cpp:430-469); host arithmetic on <= 41k elements.                 */
int  bamm_calculate_p(const float* v_flat, const float* vbg, uint32_t bg_order, uint32_t K,
                      uint32_t W, float* p_flat);
size_t bamm_v_size(uint32_t K, uint32_t W);
size_t bamm_v_offset(uint32_t k, uint32_t W);
size_t bamm_bg_size(uint32_t K);

#ifdef __cplusplus
}
#endif
#endif /* BAMM_EM_H_ */
