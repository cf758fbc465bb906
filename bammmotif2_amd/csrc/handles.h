// The handles behind the C ABI (include/bamm_em.h) and the helpers their host units share: ctx.cpp (contexts, staging,
// scratch pool), seqs.cpp (resident sequence sets), negs.cpp (the negative sampler), plan.cpp (launch plan of an EM handle), em_pass.cpp (one pass, one
// update, the all-reduce), em.cpp (the EM entry points), score.cpp (the scorer), occurrences.cpp (window p-values) and sites.cpp (windows with r >= cut-off).  Host units only -- no kernel includes it.
//
// Who owns what: every device block of a sequence set or an EM handle belongs to the handle's one DevBlocks member
// (`mem`) from the moment it exists -- the lazily allocated ones, the plan's index lists and lane records, a set's per-order
// tables alike -- and goes back through scratch_free when the handle is deleted; the d_* pointers only address the blocks.
// What one model update moves is bamm::EmBook, which bamm_em derives from: optimize()'s snapshot of it is an assignment.
//
// Reference seam these replace: class EM (/root/reference/src/refinement/EM.h:11-69,
// EM.cpp:7-259,505-527) and ScoreSeqSet::calcLogOdds (seq_scoring/ScoreSeqSet.cpp:25-67).
#pragma once

#include <algorithm>
#include <cmath>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "common.h"
#include "packed_set.h"
#include "prep.h"

// the longest length class (positions per lane) whose grouped kernels are built with the fused-update prologue and the
// all-reduce tail (grouped_kernel.h carries the same default)
#ifndef BAMM_FUSE_MAX_M
#define BAMM_FUSE_MAX_M 16
#endif

namespace bamm {

// a std::vector whose resize() leaves the new elements uninitialised: the set-sized host mirrors are filled by a parallel
// copy right after (a value-initialising resize is one more single-threaded pass over 100 MB)
template <class T>
struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    template <class U, class... A> void construct(U* p, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new ((void*)p) U; else ::new ((void*)p) U(std::forward<A>(a)...);
    }
};
template <class T> using RawVec = std::vector<T, NoInitAlloc<T>>;

struct Bucket {
    int mclass = 0;
    uint32_t count = 0;
    uint32_t* d_idx = nullptr;   // nullptr: all sequences in natural order
    std::vector<uint32_t> h_idx; // host copy of d_idx (empty with d_idx == nullptr)
    double work = 0;             // sum of M over the bucket (LDS instruction proxy)
};

struct ExcK {                    // exceptions relevant at one model order
    uint64_t* d_off = nullptr;
    uint2* d_exc = nullptr;
    uint64_t count = 0;
    RawVec<uint64_t> h_off;               // host copies (the grouped kernel's records are built from them)
    RawVec<uint2> h_ex;
    struct XRec {                         // grouped kernel (grouped.hip), one set per group size G
        uint4* d_xrec = nullptr;          // per-sequence record
        RawVec<uint8_t> h_B;              // group ends that need a virtual row (0 = no exception, 255 = too many)
        RawVec<uint32_t> h_lo;            // first of them
    };
    std::map<uint32_t, XRec> xrec;
};

struct EmBucket {                // one kernel launch of an EM pass
    int mclass = 0;
    uint32_t count = 0;
    const uint32_t* d_idx = nullptr;
    bool grouped = false;        // k_em_grp instead of k_em_seq
    uint32_t G = 0;              // its group size
    uint32_t layout = 0;         // table layout (grp_geometry); with kMixAnchorBit the launch is start-anchored and mclass is the
                                 // class it RUNS in, shorter than the class of its sequences' lengths
    const uint4* d_xrec = nullptr;
    const uint2* d_lane_rec = nullptr;   // mixed rows: the bucket's lane records (lane_records.h), owned by the handle
    uint32_t blocks = 0, logc = 0, sparse_cap = 0, sparse_bytes = 0;
    double work = 0;
    // a long bucket (mclass == kLongClass) that goes tile by tile (em_tiles.hip) instead of window by window (long_seq.hip):
    // built once per handle, without the fold mask (getR needs every sequence's tiles), in the handle's own DevBlocks
    bool tiled = false;
    uint32_t n_tiles = 0, tile_stride = 0;
    const uint32_t* d_tile_off = nullptr;   // [count + 1] prefix sums of the sequences' tile counts
    double* d_tile_z = nullptr;             // [n_tiles] written and read within one pass
    float* d_rec_invz = nullptr;            // [count] likewise
};

// The host-side state one model update moves -- the part of bamm_em (which derives from it) that optimize() copies after
// every update and copies back when the stop rule fired behind its look-ahead.  A field an update moves belongs HERE.
struct EmBook {
    // the odds table / q the most recent E pass used stay intact for getR() and MStep(): s is double
    // buffered (only the update writes it), q lives in three slots because EM::optimize_q() may write
    // it between any two of EStep / MStep / getR (EM.cpp:93-99,505-519) -- see q_write_slot()
    float *d_s = nullptr, *d_s_alt = nullptr, *d_q = nullptr;
    float *d_v = nullptr, *d_v_alt = nullptr;   // fused updates read the old v while the writer block stores the new one
    const float *s_last = nullptr, *q_last = nullptr;
    long long* d_acc = nullptr;                 // the accumulator slot the current / next pass adds into
    uint32_t acc_cur = 0;                       // ... its index in the ring (bamm_em::d_acc_ring)
    uint32_t llh_cur = 0;                       // slot of d_llh the last update wrote
    uint32_t host_iteration = 0;
    uint32_t events_used = 0, pass_no = 0;      // kernel-timing samples of the call (bamm_em_set_kernel_timing)
    bool estep_done = false;
    bool acc_dirty = false;                     // the accumulator holds sums nobody consumed (accumulate without update, getR replay)
    bool mask_done = false;                     // getR() serves d_mask_r
    bool ring_prev_dirty = false;               // the ring slot behind acc_cur was read by a fused update and awaits clearing
};

// The finest unit 2^-shift the counts of `n` sequences may travel in: a cell is a sum of r * 2^shift over them, each
// contributing less than 1, and the int64 total (summed over the ranks as well) stays below 2^62.
inline uint32_t fix_shift_for(uint64_t n) {
    uint32_t bits = 0;
    while ((uint64_t(1) << bits) < n && bits < 63u) bits++;
    return std::min(40u, 62u - std::min(bits, 38u));
}

// What one pass over the handle's launches is (run_accumulate); a call site names the fields it sets.
struct EmPass {
    enum Fuse { kNoFuse, kFuse, kFuseQWindow };
    bool accumulate = false;     // the kernels add counts (else responsibilities' statistics only: EStep, a read-out)
    bool last_model = false;     // with (s_last, q_last), what the last E pass used, instead of the current (d_s, d_q); such a
                                 // pass leaves s_last / q_last / mask_done as they are
    bool dense_r = false;        // sliced path: leaves dense r in d_state (getR, bamm_em_sites)
    bool masked = true;          // the fold mask applies (a read-out reports masked-out sequences too)
    bool timed = true;           // a pass of its iterate() / optimize() call: counted in pass_no, bracketed by events as the
                                 // timing mode says (record_event); an untimed pass records nothing and opens no region
    Fuse fuse = kNoFuse;         // the PREVIOUS pass's model update runs in the prologue of this pass's first launch instead of
                                 // a k_update launch (fusable handles, accumulating passes), with or without the q window
    static EmPass e_only() { return EmPass{}; }
    static EmPass counting() { EmPass p; p.accumulate = true; return p; }
    // the E pass the caller last ran, once more, for its r: every sequence, outside the call's timing
    static EmPass read_out() { EmPass p; p.last_model = true; p.dense_r = true; p.masked = false; p.timed = false; return p; }
    EmPass with_last_model() const { EmPass p = *this; p.last_model = true; return p; }
    EmPass with_fused_update(bool q_window) const { EmPass p = *this; p.fuse = q_window ? kFuseQWindow : kFuse; return p; }
};

// What one launch of a bucket does (launch_fused, launch_long_bucket and the kernels' own launchers).
struct EmLaunch {
    bool accum = false;          // adds counts
    bool write_r = false;        // stores r
    bool slot_layout = false;    // ... window start i at slot i+W-1 (long bucket of a sliced handle whose E pass is k_e_slice)
    static EmLaunch of_pass(const EmPass& p) { EmLaunch l; l.accum = p.accumulate; return l; }
    static EmLaunch r_only() { EmLaunch l; l.write_r = true; return l; }
};

// A read-out of sequences [begin,end) into r (r[0] = position `base` of the set) instead of a pass of the handle.
struct RRange { float* r; uint64_t base; uint32_t begin, end; };

}  // namespace bamm

struct bamm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint32_t blocks = 0, threads = 0;   // 0 = default
    // bamm_ctx_set_tuning: kernel-selection switches for benchmarks and the cross-kernel parity tests
    bool use_grouped = true, use_sparse = true, use_e_fused = true, use_e_list = true, use_fused_update = true, use_adaptive_lists = true, use_update_blocks = true;
    bool use_em_tiles = true;           // EM handles take sequences beyond the length classes tile by tile (em_tiles.hip); read at bamm_em_create
    bool use_score_tiles = true;        // the scorer takes sequences beyond the length classes tile by tile (scorer.hip); read at every scoring call
    bool use_score_slices = false;      // ... and a log-odds table beyond the LDS a slice of columns per launch (scorer.hip) instead of window by window; read at every scoring call
    bool use_mix_anchor = true;         // mixed rows: sequences that fit a shorter length class start-anchored run there (plan.cpp); read at bamm_em_create
    uint32_t list_threshold_pct = 45;   // sliced path: a pass takes lists when fewer than this share of the windows was non-zero in the pass before
    uint32_t group_size = 0;            // 0 = planner's choice
    int group_layout = -1;              // -1 = planner's choice
    bool use_peer_allreduce = false;    // the pass's all-reduce inside the sequence kernels over peer-mapped inboxes (default off)
    uint32_t peer_timeout_ms = 2000;    // how long a block waits for a peer's sums before it gives up (BAMM_ERR_COMM)
    int num_cus = 0;
    std::string name;
    // Scratch that is as large as the sequence set (dense r, the lists between the E pass and the M slices, the fix
    // lanes' log, getR's staging): 10 GB per handle at config 4, and 0.1-0.3 s per handle to allocate and free on
    // some boxes of the pool (hipFree synchronises the device as well).  A handle returns such blocks to its context
    // and the next handle on it -- the next motif, the next CV fold -- takes them over; everything on a context runs
    // on its one stream, so the old owner's last kernel is ordered before the new owner's first.  At most a quarter
    // of the device's memory stays idle here, and an allocation that fails releases every context's idle blocks first.
    std::mutex scratch_mu;
    std::unordered_map<void*, size_t> scratch_live;          // blocks handed out: bytes
    std::vector<std::pair<void*, size_t>> scratch_idle;      // blocks waiting for their next owner, oldest first
    size_t scratch_idle_bytes = 0, scratch_cap_bytes = 0;
    uint32_t sites_chunk_positions = 0;                      // bamm_em_sites: dense r kept on the device at a time (0 = default)
    uint32_t neg_segment_positions = 0;                      // bamm_sample_negatives: positions per segment of a long record, rounded down to 16s (0 = default)
    uint32_t kmer_segment_positions = 0;                     // bamm_kmer_counts: positions per segment of a record longer than that, rounded down to 16s (0 = default)
    uint32_t kmer_flush_windows = 0;                         // bamm_kmer_counts: a workgroup flushes its LDS table once it has added this many windows (0 = default)
    bool scratch_poison = false;                             // tests: every block is filled with 0xFF when it is handed out
    uint64_t scratch_hits = 0, scratch_misses = 0;
    // Every transfer of 64 KiB or more between the CALLER's memory and the device goes through this pinned area (two chunks,
    // filled and drained in turn), never through a hipMemcpy on the caller's pages.  The HIP runtime pins pageable memory in
    // place for such a copy and keeps the registration; when the owner later unmaps those pages (a numpy array freed, a
    // std::vector going out of scope) the driver evicts the process's queues until it has dropped the registration:
    // the next launch or copy of the process then waits 17-39 ms (profiles/r05_first_call.txt -- the "29 ms second pass" of
    // profiles/r04_pass_times.txt was getR()'s result being freed; bamm_em_create's first upload paid the same for the
    // vectors of bamm_seqs_upload).  Memory this library pinned itself is never unmapped under a registration.
    std::mutex stage_mu;
    unsigned char* stage_buf[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};                     // an enqueued copy still reads (H2D) the chunk: wait for stage_ev first
};

namespace bamm {

// ---- ctx.cpp ----
// hipMalloc; when the device is out of memory the contexts' idle scratch blocks are released and it is tried again
int dev_alloc_bytes(void** p, size_t bytes);
template <class T>
int dev_alloc(T** p, size_t count) { return dev_alloc_bytes((void**)p, count * sizeof(T)); }
void par_memcpy(void* dst, const void* src, size_t bytes);
int ctx_upload(bamm_ctx* c, void* dst_dev, const void* src, size_t bytes);
int ctx_download(bamm_ctx* c, void* dst, const void* src_dev, size_t bytes);
template <class T>
int dev_upload(bamm_ctx* c, T** p, const T* host, size_t count) {
    int rc = dev_alloc(p, count);
    if (rc) return rc;
    return ctx_upload(c, *p, host, count * sizeof(T));
}
// a block of the context's scratch pool (ctx.cpp), or a plain allocation below 4 MB
int scratch_alloc_bytes(bamm_ctx* c, void** p, size_t bytes);
template <class T>
int scratch_alloc(bamm_ctx* c, T** p, size_t count) { return scratch_alloc_bytes(c, (void**)p, count * sizeof(T)); }
void scratch_free(bamm_ctx* c, void* p);
int use_device(const bamm_ctx* c);

// The owner of device blocks: of a handle's for its life (bamm_seqs::mem, bamm_em::mem), of a call's temporaries for the
// call.  A block is held from the moment it exists (an upload that fails behind its allocation included) and freed through
// scratch_free (pooled blocks go back to the context, the rest is freed) when the owner goes out of scope, or earlier by
// free_all() / release().  keep() hands a pointer over to whoever takes it, and the owner forgets it; adopt() is the same
// between two owners.
struct DevBlocks {
    bamm_ctx* c;
    std::vector<void*> held;
    explicit DevBlocks(bamm_ctx* ctx) : c(ctx) {}
    DevBlocks(const DevBlocks&) = delete;
    DevBlocks& operator=(const DevBlocks&) = delete;
    ~DevBlocks() { free_all(); }
    template <class T> int alloc(T** p, size_t count) { return hold(p, dev_alloc(p, count ? count : 1)); }
    template <class T> int upload(T** p, const T* host, size_t count) { return hold(p, dev_upload(c, p, host, count)); }
    template <class T> int scratch(T** p, size_t count) { return hold(p, scratch_alloc(c, p, count)); }
    void keep(const void* p) { held.erase(std::remove(held.begin(), held.end(), p), held.end()); }
    void adopt(DevBlocks& from, void* p) { if (p) held.push_back(p); from.keep(p); }   // (held here before `from` lets go)
    template <class T> void release(T*& p) { keep(p); scratch_free(c, p); p = nullptr; }   // this one now (nullptr: nothing)
    void free_all() { for (void* p : held) scratch_free(c, p); held.clear(); }
  private:
    template <class T> int hold(T** p, int rc) { if (*p) held.push_back((void*)*p); return rc; }
};

}  // namespace bamm

struct bamm_seqs {
    bamm_ctx* ctx = nullptr;
    bamm::DevBlocks mem;                        // every d_* below, the buckets' index lists and the per-order tables
    explicit bamm_seqs(bamm_ctx* c) : ctx(c), mem(c) {}      // (its destructor also runs on every error path of bamm_seqs_upload)
    int refs = 1;
    std::mutex mu;                              // guards refs and the lazily built per-order tables (handles may be
                                                // created on one set from several host threads, FDR.cpp:37)
    uint64_t n = 0, total_len = 0;
    uint32_t max_len = 0, min_len = 0;
    uint64_t hbm_bytes = 0;
    uint32_t* d_words = nullptr;
    uint64_t* d_word_off = nullptr;
    uint32_t* d_len = nullptr;
    uint64_t* d_pos_off = nullptr;
    std::vector<uint32_t> h_len;
    bamm::RawVec<uint32_t> h_words;             // host copy of the 2-bit stream (grouped kernel's exception records)
    std::vector<uint64_t> h_word_off;
    std::vector<uint64_t> h_pos_off;
    std::vector<uint64_t> h_exc_off;            // full (11-mer level) exception list
    bamm::RawVec<uint32_t> h_exc_pos, h_exc_kmer, h_exc_clean;
    std::vector<bamm::Bucket> buckets;
    std::map<uint32_t, bamm::ExcK> exc_by_order;   // node-based: pointers into it stay valid
    // the unknown forward positions of a set built from codes (packed_set.h; null: built from kmer_ arrays), record 0 of the
    // set being record unk_begin of the list; on the device from the first bamm_kmer_counts on (under `mu`)
    std::shared_ptr<const bamm::UnknownList> unk;
    uint64_t unk_begin = 0;
    uint64_t* d_unk_off = nullptr;              // [n + 1], rebased to the set's first record
    uint32_t* d_unk_pos = nullptr;
};

struct bamm_em : bamm::EmBook {                 // (the fields an update moves: d_s, d_q, d_v, d_acc, ... -- see EmBook)
    bamm_ctx* ctx = nullptr;
    bamm_seqs* seqs = nullptr;
    bamm::DevBlocks mem;                        // every device block of the handle, from bamm_em_create's to the lazily allocated ones
    bamm_em(bamm_ctx* c, bamm_seqs* s) : ctx(c), seqs(s), mem(c) {}
    bamm::EmBook& book() { return *this; }
    bamm_em_params prm{};
    uint32_t Y = 0, Kbg = 0;
    size_t vsz = 0, cells = 0;
    float *d_vbg = nullptr, *d_A = nullptr, *d_n = nullptr;
    float *d_status = nullptr, *d_trace = nullptr;
    float *d_qbuf[3] = {nullptr, nullptr, nullptr};  // the three slots d_q / q_last point into
    uint32_t* d_iteration = nullptr;
    uint8_t* d_mask = nullptr;
    // the pass's fused accumulator [cells | llh | sum_r | n_seqs] (d_acc): 64-bit integers the blocks add into,
    // summed across ranks as int64 (exact, order-free), consumed and zeroed by the update
    // ... a ring of three slots when the handle can fuse the model update into the next pass's kernel
    // (update_kernel.h): pass p adds into slot p mod 3, the next kernel's blocks read it, its writer block clears
    // the slot after next.  Outside a fused sequence only slot `acc_cur` is ever non-zero.
    long long* d_acc_ring = nullptr;
    size_t acc_stride = 0;                      // words per slot
    bool fusable = false;                       // K <= 2-sized tables, first launch of a pass is a grouped kernel with room for the update
    uint32_t fuse_upd_off = 0;                  // LDS offset of the update's scratch in that kernel
    float* d_s_block = nullptr;                 // [blocks of the first launch][W * (Y + 1)]
    float* d_llh[2] = {nullptr, nullptr};       // log-likelihood of the last two updates (the stop rule compares them)
    double* d_upd_partial = nullptr;            // the update spread over blocks (tables beyond its LDS form): v_diff partials
    uint32_t* d_upd_ticket = nullptr;           // ... and the word its blocks draw tickets from
    bool acc_external = false;                 // caller-owned (bamm_em_set_reduce_buffer)
    uint32_t fix_shift = 40;                   // counts travel in units of 2^-fix_shift (40 unless the set is huge)
    float fix_scale() const { return ldexpf(1.0f, (int)fix_shift - 40); }   // ... what the kernels multiply their 2^40-based addends by
    size_t acc_words() const { return cells + 3; }                          // one accumulator slot: [cells | llh | sum_r | n_seqs]
    float* h_status = nullptr;                  // pinned, 8 floats (+ 2 x 8 for optimize()'s look-ahead where the mirror below is missing)
    unsigned long long* h_tagged = nullptr;     // ... + 2 x 8 tagged words behind them: what the updates of optimize() report (UpdateArgs::status_mirror)
    unsigned long long* d_status_mirror = nullptr;   // h_tagged as the device addresses it
    uint32_t* d_stop = nullptr;                 // optimize(): set by k_update when the stop rule fires
    const uint32_t* stop_arg = nullptr;         // what the kernels are handed: d_stop inside optimize(), else null
    hipEvent_t opt_events[2] = {nullptr, nullptr};
    // this optimize() call's stop rule for k_update (run_update fills UpdateArgs from it)
    uint32_t opt_iteration = 0;
    float opt_llh_prev = 0.0f;
    uint32_t total_blocks = 0;
    std::vector<bamm::EmBucket> ebuckets;       // launches of one pass (length class x kernel flavour)
    uint32_t threads = 0;
    // column-sliced path (tables beyond the fused kernel's LDS budget)
    bool sliced = false;
    std::vector<std::pair<uint32_t, uint32_t>> e_slices, m_slices;
    uint32_t m_slice_logc = 0;
    bool e_fused = false;                       // the E pass of the sliced path is k_em_seq (whole odds table in LDS)
    uint32_t m_slice_cap = 0;                   // sparse list capacity per wave in the M-slices (0 = dense)
    float* d_state = nullptr;                   // one float per position slot: E-chain state, then r (allocated on first use)
    // e_fused: the E pass hands the M slices compacted lists of the non-zero windows instead of dense r
    float* d_list_r = nullptr;
    uint16_t* d_list_p = nullptr;
    uint32_t* d_list_n = nullptr;
    // ... or dense r, chosen per pass on the device: [2] counts of windows with a non-zero addend (the pass before, this pass)
    unsigned long long* d_nnz = nullptr;
    uint32_t nnz_prev_slot = 0;
    unsigned long long nnz_limit = 0;           // above it a pass takes the dense flavour
    bool adaptive_lists = true;                 // bamm_ctx_set_tuning("adaptive_lists") when the handle was created
    // K = 3 through the grouped kernel: per-wave log of the virtual rows' counts (grouped_kernel.h), grown on demand
    unsigned long long* d_fix_log = nullptr;
    size_t fix_log_words = 0;
    bamm::ExcK* exc = nullptr;
    float llh_prev = 0.0f;                      // EM.h:61
    bamm_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    bamm_comm* comm = nullptr;                  // native RCCL all-reduce (bamm_em_set_comm)
    bool comm_verified = false;                 // verify_comm() ran with the peers
    // in-kernel all-reduce (PeerArgs): the last block of every accumulating pass exchanges the GPU's totals with the peers
    // and leaves the sum in the accumulator, in place -- no collective launch behind the pass
    bool peer_on = false;                       // agreed with every rank in verify_comm()
    bool pass_summed_in_kernel = false;         // the pass just enqueued carried the tail (launch_fused): run_allreduce has nothing to add
    uint32_t* d_peer_words = nullptr;           // [0] ticket, [1] err
    long long* d_comm_words = nullptr;          // four words for verify_comm()'s own sums, kept for the handle's life (never released
                                                // early): a hipFree there would synchronise the DEVICE, and with several ranks on one
                                                // device (the rehearsal forms) a peer that has already launched its first pass spins in that
                                                // kernel's tail for THIS rank's sums, which this rank cannot launch from inside hipFree
    std::string peer_note;                      // why peer_on is false although asked for
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    uint32_t timing_every = 8;                  // bamm_em_set_kernel_timing
    bool timing_now = false;
    // timing_every == BAMM_TIMING_WHOLE_CALL: ONE pair of events around all the passes of a call
    bool region_open = false;
    uint32_t region_passes = 0;
    std::vector<uint32_t> event_passes;          // passes between the two events of pair i (1 in the per-pass modes)
    // EM::mask state (allocated on first use)
    uint64_t n_active = 0;                      // sequences the handle trains on (mask applied)
    float* d_mask_r = nullptr;                  // responsibilities in the reference layout
    uint32_t* d_mask_bits = nullptr;
    long long* d_mask_hist = nullptr;
    bamm::MaskSelect* d_mask_sel = nullptr;
    float* d_mask_qseq = nullptr;
    unsigned long long* d_mask_partial_n = nullptr;
    double* d_mask_partial_stat = nullptr;
    uint32_t mask_blocks = 0;
    bamm::EmBook books[4] = {};                 // book() right after update i at [i & 3]
};

// --FDR --mops statistics (fdr_stats.cpp): the window scores of every fold, positives and negatives, in two device arrays
// from the context's scratch pool that grow geometrically (a fold's count is not known before it is scored); sorted in
// place by bamm_fdr_statistics, which also leaves the walk's partition and the peak.  A list is a sequence of pieces, each
// either an ascending RUN (sorted by bamm_fdr_seal, here or on the handle bamm_fdr_absorb took it from) or OPEN (as the
// scores arrived); statistics and seal sort the open pieces and merge the runs (k_fdr_merge) instead of sorting them again.
struct bamm_fdr {
    struct Piece { uint64_t len; bool run; };
    bamm_ctx* ctx = nullptr;
    float* d[2] = {nullptr, nullptr};           // [0] positives, [1] negatives
    uint64_t n[2] = {0, 0}, cap[2] = {0, 0};
    std::vector<Piece> pieces[2];               // in the order they lie in d[]; no empty piece, no two open ones in a row; lengths sum to n[]
    bool sealed = false;                        // each list is one run (or empty): no more scores, may still be absorbed or run statistics
    bool moved = false;                         // bamm_fdr_absorb emptied it: only destroy is left
    bool done = false, with_pvalues = false;    // statistics ran: no more scores
    uint64_t posN = 0, negN = 0, n_rows = 0;
    float e_tp = 0.0f;
    bamm::FdrWalkArgs walk{};                   // part / block_max / peak: owned, freed with the handle
};

namespace bamm {

// ---- seqs.cpp ----
// fn(begin, end) over contiguous ranges of [0, n) on the host threads the process was granted (bamm_set_host_threads):
// the per-sequence set-up loops walk a million records and several million exceptions
template <class F>
void host_ranges(uint64_t n, F&& fn) {
    const uint32_t T = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(host_threads_hint(), n / 16384 + 1));
    if (T <= 1) { fn(uint64_t(0), n); return; }
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < T; t++) th.emplace_back([&fn, n, t, T] { fn(n * t / T, n * (t + 1) / T); });
    for (auto& x : th) x.join();
}
int exceptions_for_order(bamm_seqs* s, uint32_t K, ExcK** out);
int xrec_for_group(bamm_seqs* s, uint32_t K, uint32_t G, ExcK* k, const ExcK::XRec** out);

// the kernels' view of `count` sequences of a resident set (idx: their ids, nullptr = all in natural order)
inline SeqView make_view(const bamm_seqs* s, const ExcK* exc, const uint32_t* idx, uint32_t count, const uint8_t* mask) {
    return SeqView{s->d_words, s->d_word_off, s->d_len, s->d_pos_off, exc->d_off, exc->d_exc, mask, idx, count};
}

// ---- score.cpp ----
// ScoreSeqSet::calcLogOdds over a resident set, results left on the device in memory `tmp` owns: the log-odds table, the
// per-bucket launches with their long-sequence / large-table fall-backs.  Arguments are the caller's to check.
struct DeviceScores {
    float* mops = nullptr;              // concatenated L-W+1 scores per sequence (want_mops), else null
    float* zoops = nullptr;             // [n]
    uint32_t* z = nullptr;              // [n]
    std::vector<uint64_t> moff;         // [n+1] prefix sums of L-W+1
};
int score_on_device(bamm_ctx* c, bamm_seqs* s, const uint8_t* seq_mask, uint32_t K, uint32_t W, uint32_t bg_order, const float* v,
                    const float* vbg, bool want_mops, bool pooled_mops, DevBlocks& tmp, DeviceScores* out);
constexpr bool kWantMops = true, kPooledMops = true;         // what the callers that keep every window's score on the device pass

// ---- plan.cpp ----
uint32_t default_threads(const bamm_ctx* c, int mclass);
uint32_t bucket_threads(const bamm_ctx* c, const EmBucket& b);
uint32_t default_blocks(const bamm_ctx* c, uint32_t threads);
// threads that load the code objects of a new handle's kernels beside bamm_em_create's host work; joined on every way out
struct Primers {
    std::vector<std::thread> t;
    ~Primers() { for (auto& x : t) if (x.joinable()) x.join(); }
};
// the column slices of a handle whose tables exceed the fused kernel's LDS (em->sliced); true when not even one column
// fits and the tables stay in global memory (long_seq.hip)
bool plan_slices(bamm_em* em);
// the launches of one pass, their blocks, the fused update and the sliced path's lists; primes each kernel it names
int plan_launches(bamm_em* em, bool global_tables, const uint8_t* seq_mask, Primers& primers);
// The launch geometry of bamm_em_mask, a pure function of the model's shape (W, Y = 4^(K+1), cells = W * Y), the set's
// longest sequence and size, and the device's CUs.  M-step: as many columns per launch as fit next to one wave's arrays.
// Sequences whose arrays (10 bytes per position) do not fit beside one column's counts keep them in a global scratch
// region per wave instead (~16 000 positions at k = 2; the window lists are 32 bits wide there, so any length goes):
// slower, same arithmetic in the same order.  Orders whose count column alone exceeds the LDS (k >= 7) add the listed
// windows straight into the pass's accumulator.  The reference has neither limit (EM.cpp:261-503).
struct MaskPlan {
    bool direct, wave_global;                   // counts straight into the accumulator; per-wave arrays in global scratch
    size_t wave_bytes;                          // mask_wave_bytes(max_len, wave_global)
    bool s_in_lds;
    size_t e_table;                             // LDS table of the E launch (the odds when s_in_lds)
    uint32_t m_cols;                            // columns per M launch
    size_t m_table;                             // ... and their count table
    uint32_t init_table;                        // LDS table of the order-0 pass
    uint32_t e_waves, m_waves;                  // waves per block
    uint32_t cus, mblocks;                      // CUs the launches are sized for; blocks of the E / M launches
    size_t wave_scratch_bytes;                  // the global region of the per-wave arrays (0 unless wave_global)
    uint32_t waves_for(size_t table) const;     // waves per block beside an LDS table of that size
};
MaskPlan mask_plan(uint32_t W, uint32_t Y, uint32_t max_len, uint64_t n_seqs, size_t cells, int num_cus);

// ---- em.cpp ----
struct DenseR {
    const float* r;              // sequence n of the set starts at r[pos_off[n] - base]
    uint64_t base;
    bool slot_layout;            // window start i at slot i+W-1 (the e_slice kernels) instead of the reference's L-W-i
};
int dense_r_on_device(bamm_em* em, uint64_t begin, uint64_t end, DevBlocks& tmp, DenseR* out);

// ---- em_pass.cpp ----
int record_event(bamm_em* em, bool start);
int close_timed_region(bamm_em* em);
// the kernel-timing samples of one iterate() / optimize() / mask() call: they start afresh with it, and a whole-call
// interval still open is closed on every way out
struct TimedRegion {
    bamm_em* em;
    explicit TimedRegion(bamm_em* e) : em(e) { em->events_used = 0; em->pass_no = 0; em->region_open = false; }
    ~TimedRegion() { (void)close_timed_region(em); }
};
// the shape fields every EmKernelArgs starts from (a handle's launches; the priming threads, which have no handle)
inline EmKernelArgs shape_args(const bamm_em_params& prm, uint32_t Y) { EmKernelArgs a{}; a.K = prm.K; a.W = prm.W; a.Y = Y; return a; }
// the arguments of bucket `bk` in pass `p`, or (range) in a read-out of r over a range: the one place they are filled
EmKernelArgs pass_args(const bamm_em* em, const EmBucket& bk, const EmPass& p, const RRange* range = nullptr);
int launch_fused(bamm_em* em, const EmBucket& eb, EmLaunch what, EmKernelArgs& a, uint32_t threads, hipStream_t st,
                 const UpdateArgs* fuse = nullptr);
int clean_accumulator(bamm_em* em);
int run_accumulate(bamm_em* em, const EmPass& p);
// The one way a bucket of mclass kLongClass is launched, by a pass and by getR / bamm_em_sites alike: tile by tile when the
// plan says so (EmBucket::tiled), else window by window.  prime_long_bucket loads the same kernel's code object and launches nothing.
int launch_long_bucket(const bamm_ctx* c, const EmBucket& bk, const EmKernelArgs& a, EmLaunch what, hipStream_t st);
int prime_long_bucket(const EmBucket& bk, const EmKernelArgs& a, hipStream_t st);
int allreduce_words(bamm_em* em, void* dev_ptr, size_t n_words);
int run_allreduce(bamm_em* em);
float* q_write_slot(bamm_em* em);
int run_update(bamm_em* em, bool q_window);
int comm_still_sound(const bamm_em* em);
int fetch_status(bamm_em* em);
// optimize(): waits until update `done` of the call (enqueued with unit `unit`) has reported, and leaves its status in out[8]
int wait_update_status(bamm_em* em, uint32_t done, uint32_t unit, float* out);
int verify_comm(bamm_em* em);

}  // namespace bamm
