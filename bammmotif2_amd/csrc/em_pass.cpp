// One EM pass, one model update and the all-reduce between them: kernel-timing events, the launches of a pass, the
// update's arguments and the host's bookkeeping of it, the sums over the ranks and the communicator check.  Host code only.

#include <atomic>
#include <cmath>

#include "handles.h"

namespace bamm {

// An event pair costs 7-8 us of stream time per pass on gfx950 (0.9 % of a 1M-sequence iteration, 6.5 % of a 125k-sequence
// one: profiles/r04_timing_every_cost.txt).  Three ways: every `timing_every`-th pass of a call bracketed; none; or
// (BAMM_TIMING_WHOLE_CALL) one pair around ALL passes of a call -- every pass covered, nothing between two passes, the
// launch gaps inside the interval.
static int event_pair(bamm_em* em) {
    if (em->events_used == em->events.size()) {
        hipEvent_t a, b;
        BAMM_HIP(hipEventCreate(&a));
        BAMM_HIP(hipEventCreate(&b));
        em->events.emplace_back(a, b);
        em->event_passes.push_back(1u);
    }
    return BAMM_OK;
}
int record_event(bamm_em* em, bool start) {
    if (em->timing_every == BAMM_TIMING_WHOLE_CALL) {
        if (!start) return BAMM_OK;
        em->pass_no++;
        if (!em->region_open) {
            if (int rc = event_pair(em)) return rc;
            BAMM_HIP(hipEventRecord(em->events[em->events_used].first, em->ctx->stream));
            em->region_open = true;
            em->region_passes = 0;
        }
        em->region_passes++;
        return BAMM_OK;
    }
    if (start) {
        em->timing_now = em->timing_every != 0 && em->pass_no % em->timing_every == 0;
        em->pass_no++;
    }
    if (!em->timing_now) return BAMM_OK;
    if (start) {
        if (int rc = event_pair(em)) return rc;
        BAMM_HIP(hipEventRecord(em->events[em->events_used].first, em->ctx->stream));
    } else {
        BAMM_HIP(hipEventRecord(em->events[em->events_used].second, em->ctx->stream));
        em->event_passes[em->events_used] = 1u;
        em->events_used++;
    }
    return BAMM_OK;
}
// the second event of a whole-call interval: behind the last pass's kernels
int close_timed_region(bamm_em* em) {
    if (!em->region_open) return BAMM_OK;
    em->region_open = false;
    BAMM_HIP(hipEventRecord(em->events[em->events_used].second, em->ctx->stream));
    em->event_passes[em->events_used] = em->region_passes;
    em->events_used++;
    return BAMM_OK;
}

// one bucket through the fused kernel of its flavour (grouped columns or one column at a time)
int launch_fused(bamm_em* em, const EmBucket& eb, EmLaunch what, EmKernelArgs& a, uint32_t threads, hipStream_t st,
                 const UpdateArgs* fuse) {
    const bool accum = what.accum, write_r = what.write_r;
    if (!eb.grouped) {
        a.logC = eb.logc;
        a.sparse_cap = accum ? eb.sparse_cap : 0u;
        a.sparse_wave_bytes = accum ? eb.sparse_bytes : 0u;
        return launch_em_seq(eb.mclass, accum, write_r, a, eb.blocks, threads, st);
    }
    GrpKernelArgs ga{};
    a.logC = eb.logc;
    a.sparse_cap = 0; a.sparse_wave_bytes = 0;
    ga.e = a;
    ga.xrec = eb.d_xrec;
    ga.lane_rec = eb.d_lane_rec;
    if (!grp_geometry(em->prm.K, em->prm.W, eb.G, kMClasses[eb.mclass], threads / 64u, accum, accum ? eb.logc : 0u, eb.layout, &ga.g)) {
        set_error("grouped kernel geometry does not fit (K=%u W=%u)", em->prm.K, em->prm.W);
        return BAMM_ERR_UNSUPPORTED;
    }
    if ((em->prm.K == 3u || (eb.layout & 8u)) && accum) {      // kernels whose fix lanes log their sums
        const size_t waves = (size_t)eb.blocks * (threads / 64u);
        const size_t cap = ((eb.count + waves - 1) / waves) * std::min<size_t>(64, (size_t)ga.g.Bv * ga.g.T);   // entries per wave
        const size_t need = waves * cap;                      // 8-byte entries
        if (need > em->fix_log_words) {
            em->mem.release(em->d_fix_log); em->fix_log_words = 0;
            if (int rc = em->mem.scratch(&em->d_fix_log, need)) return rc;
            em->fix_log_words = need;
        }
        ga.fix_log = em->d_fix_log;
        ga.fix_log_cap = (uint32_t)cap;
    }
    if (fuse) {                                              // the previous pass's update runs in this launch's prologue
        ga.fused = 1u; ga.upd = *fuse; ga.upd_off = em->fuse_upd_off; ga.s_block = em->d_s_block;
    }
    if (em->peer_on && accum && !write_r) {                  // in-kernel all-reduce in the launch's tail (the pass's only launch)
        em->pass_summed_in_kernel = true;
        comm_peer_args(em->comm, &ga.peer);
        ga.peer.words = (uint32_t)em->acc_words();
        ga.peer.ticket = em->d_peer_words; ga.peer.err = em->d_peer_words + 1;
        ga.peer.timeout_ticks = (unsigned long long)em->ctx->peer_timeout_ms * 100000ull;      // 100 MHz wall clock
        ga.peer.seq = comm_peer_next_seq(em->comm);          // the ranks count their passes in step
        ga.peer.slot = (uint32_t)(ga.peer.seq % 3ull);
    }
    return launch_em_grp(eb.mclass, accum, write_r, ga, eb.blocks, threads, st);
}

// `blocks` of the long bucket's kernel (kPrimeOnly: its code object is loaded, nothing runs)
static int long_bucket_kernel(const EmBucket& bk, const EmKernelArgs& a, EmLaunch what, uint32_t blocks, hipStream_t st) {
    if (!bk.tiled) return launch_long_em(a, what.accum, what.write_r, what.slot_layout, blocks, st);
    EmTileArgs ta{};
    ta.e = a;
    ta.tile_off = bk.d_tile_off; ta.n_tiles = bk.n_tiles; ta.stride = bk.tile_stride;
    ta.tile_z = bk.d_tile_z; ta.rec_invz = bk.d_rec_invz;
    return launch_em_tiles(ta, what.accum, what.write_r, blocks, st);
}

int launch_long_bucket(const bamm_ctx* c, const EmBucket& bk, const EmKernelArgs& a, EmLaunch what, hipStream_t st) {
    if (!bk.tiled) return long_bucket_kernel(bk, a, what, bk.blocks, st);
    // a block per CU (its count table takes most of the CU's LDS), a wave per tile; nothing in the result depends on it
    const uint32_t waves = em_tile_threads() / 64u;
    const uint32_t blocks = std::min(c->blocks ? c->blocks : (uint32_t)std::max(1, c->num_cus), (bk.n_tiles + waves - 1u) / waves);
    return long_bucket_kernel(bk, a, what, blocks, st);
}

int prime_long_bucket(const EmBucket& bk, const EmKernelArgs& a, hipStream_t st) {
    return long_bucket_kernel(bk, a, EmLaunch::of_pass(EmPass::counting()), kPrimeOnly, st);
}

// clear whatever a pass left unconsumed (accumulate without update, getR replay, a fused sequence cut short)
int clean_accumulator(bamm_em* em) {
    if (!em->acc_dirty) return BAMM_OK;
    hipStream_t st = em->ctx->stream;
    if (em->d_acc_ring) {
        BAMM_HIP(hipMemsetAsync(em->d_acc_ring, 0, 3 * em->acc_stride * sizeof(long long), st));
        em->acc_cur = 0; em->d_acc = em->d_acc_ring; em->ring_prev_dirty = false;
    } else {
        BAMM_HIP(hipMemsetAsync(em->d_acc, 0, em->acc_words() * sizeof(long long), st));
    }
    em->acc_dirty = false;
    return BAMM_OK;
}

// The slot a new q may be written to: never the one the last E pass read (q_last: getR() and the
// MStep() replay recompute r from it, the reference's r_ keeps the EStep's q, EM.cpp:139-200), the
// current slot when that is free, else the third one.
float* q_write_slot(bamm_em* em) {
    if (em->d_q != em->q_last) return em->d_q;
    for (float* p : em->d_qbuf)
        if (p != em->q_last) return p;
    return em->d_q;
}

// Fill the arguments of one model update and move the host's bookkeeping past it (the launch that carries it --
// k_update, or the next pass's first sequence kernel when `fused` -- follows on the stream).
// q_window: this pass is one of the first five of its optimize() / iterate() call, where the reference
// re-estimates q (`iteration` is local to EM::optimize, EM.cpp:75-99)
static void prepare_update(bamm_em* em, bool q_window, bool fused, UpdateArgs& u) {
    u = UpdateArgs{};
    u.K = em->prm.K; u.W = em->prm.W; u.Kbg = em->Kbg;
    u.acc = em->d_acc; u.count_unit = ldexp(1.0, -(int)em->fix_shift); u.vbg = em->d_vbg; u.A = em->d_A; u.n = em->d_n; u.s = em->d_s_alt;
    float* q_out = q_write_slot(em);
    if (fused)                                               // every block reads d_q while the writer block stores q_out: never the same slot
        for (float* p : em->d_qbuf)
            if (p != em->q_last && p != em->d_q) { q_out = p; break; }
    u.q = em->d_q; u.q_out = q_out; u.status = em->d_status; u.trace = em->d_trace; u.trace_cap = em->prm.max_iterations;
    u.iteration = em->d_iteration; u.optimize_q = (em->prm.optimize_q && q_window) ? 1 : 0;
    u.n_seqs_override = (double)em->prm.n_seqs_global;
    u.llh_in = em->d_llh[em->llh_cur]; u.llh_out = em->d_llh[em->llh_cur ^ 1u];
    u.partial = em->d_upd_partial; u.ticket = em->d_upd_ticket;
    if (em->stop_arg) {
        u.stop = em->d_stop; u.epsilon = em->prm.epsilon; u.opt_iteration = em->opt_iteration;
        u.llh_prev = em->opt_llh_prev; u.llh_prev_from_status = em->opt_iteration > 1u ? 1 : 0;
        u.status_mirror = em->d_status_mirror ? em->d_status_mirror + 8 * (em->opt_iteration & 1u) : nullptr;
    }
    if (fused) {
        // every block of the carrying launch reads slot `acc_cur` and the old v; its writer block stores the new v
        // elsewhere and clears the slot after next; the launch's own pass adds into the next slot
        u.v_old = em->d_v; u.v = em->d_v_alt;
        u.acc_zero = em->d_acc_ring + (size_t)((em->acc_cur + 2u) % 3u) * em->acc_stride;
        std::swap(em->d_v, em->d_v_alt);
        em->acc_cur = (em->acc_cur + 1u) % 3u;
        em->d_acc = em->d_acc_ring + (size_t)em->acc_cur * em->acc_stride;
        em->ring_prev_dirty = true;                          // the slot just read stays as it is until the next update clears it
    } else {
        u.v = em->d_v; u.v_old = nullptr;
        u.acc_zero = em->ring_prev_dirty ? em->d_acc_ring + (size_t)((em->acc_cur + 2u) % 3u) * em->acc_stride : nullptr;
        em->ring_prev_dirty = false;
    }
    em->acc_dirty = false;                                    // consumed (k_update zeroes it; the ring moves on)
    std::swap(em->d_s, em->d_s_alt);
    em->d_q = q_out;
    em->llh_cur ^= 1u;
    em->host_iteration++;
    em->estep_done = false;
    em->books[em->host_iteration & 3u] = em->book();
}

EmKernelArgs pass_args(const bamm_em* em, const EmBucket& bk, const EmPass& p, const RRange* range) {
    EmKernelArgs a = shape_args(em->prm, em->Y);
    a.sv = make_view(em->seqs, em->exc, bk.d_idx, bk.count, p.masked ? em->d_mask : nullptr);
    a.logC = bk.logc;
    a.s = p.last_model ? em->s_last : em->d_s;
    a.q = p.last_model ? em->q_last : em->d_q;
    a.stop = em->stop_arg;                                   // non-null only inside optimize(): no read-out runs there
    if (range) {
        // responsibilities only: nothing is accumulated, so no accumulator and no unit (the kernels scale addends nobody
        // sums by 1); r of the range's sequences goes to a block of the caller's
        a.acc = nullptr; a.fix_scale = 1.0f;
        a.r_out = range->r; a.r_base = range->base; a.seq_begin = range->begin; a.seq_end = range->end;
    } else {
        // a pass of the handle, the sliced path's replay for getR included: its E-only kernels add their statistics too
        a.acc = em->d_acc; a.fix_scale = em->fix_scale();
    }
    return a;
}

// Sliced path, one bucket at `waves` waves per block beside the widest M slice's count table: whether a wave's copy of
// the decoded sequence fits there (the M slices can walk lists), and the longest list of the dense walk that does.
struct SlicedGeom { bool lists_fit; uint32_t sparse_cap, sparse_wave_bytes; };
static SlicedGeom sliced_geometry(const std::vector<std::pair<uint32_t, uint32_t>>& m_slices, uint32_t Y, uint32_t logc, uint32_t cap, int M,
                                  uint32_t waves) {
    constexpr size_t kLds = 160u * 1024u;
    uint32_t widest = 0;
    for (auto& sl : m_slices) widest = std::max(widest, sl.second - sl.first);
    const size_t table = m_slice_lds_bytes(widest, Y, logc);
    while (cap && table + waves * m_slice_wave_bytes(M, cap) > kLds) cap -= 64u;
    return SlicedGeom{m_list_lds_bytes(widest, Y, logc, M, waves) <= kLds, cap, (uint32_t)m_slice_wave_bytes(M, cap)};
}

enum class SlicedWalk { kDense, kLists };                    // what the E pass hands the M slices: dense r in d_state, or compacted lists
enum class RunWhen { kAlways, kFewWindows, kManyWindows };   // ... chosen on the device from the previous pass's count of non-zero windows

// one flavour of a sliced bucket's pass: the E pass (k_em_seq with the whole odds table in LDS, or the E slices), then -- in
// an accumulating pass -- the M slices over what it left
static int launch_sliced_walk(bamm_em* em, const EmBucket& bk, const EmKernelArgs& a, bool accum, SlicedWalk walk, RunWhen when,
                              const SlicedGeom& g, uint32_t threads, hipStream_t st) {
    EmKernelArgs f = a;
    int r = BAMM_OK;
    const bool use_lists = walk == SlicedWalk::kLists;
    f.r_out = em->d_state;
    if (when != RunWhen::kAlways) {
        f.nnz_prev = em->d_nnz + em->nnz_prev_slot; f.nnz_limit = em->nnz_limit; f.run_if_long = when == RunWhen::kManyWindows ? 1u : 0u;
    }
    if (em->d_nnz && accum) f.nnz_out = em->d_nnz + (em->nnz_prev_slot ^ 1u);
    if (em->e_fused) {
        // the whole odds table fits LDS (only the count table does not): the fused kernel's E
        // pass, leaving r in the reference's layout (k_em_seq WRITE_R) or the lists
        const EmLaunch e = EmLaunch::r_only();
        f.seq_end = (uint32_t)em->seqs->n;
        f.logC = 0; f.sparse_cap = 0; f.sparse_wave_bytes = 0;
        if (use_lists) { f.list_r = em->d_list_r; f.list_p = em->d_list_p; f.list_n = em->d_list_n; }
        r = launch_em_seq(bk.mclass, e.accum, e.write_r, f, bk.blocks, threads, st);
        if (use_lists) {
            f.logC = em->m_slice_logc;
            for (size_t i = 0; accum && i < em->m_slices.size() && !r; i++)
                r = launch_m_list(bk.mclass, f, em->m_slices[i].first, em->m_slices[i].second, bk.blocks, threads, st);
            return r;
        }
    } else {
        for (size_t i = 0; i < em->e_slices.size() && !r; i++)
            r = launch_e_slice(bk.mclass, f, em->e_slices[i].first, em->e_slices[i].second, i + 1 == em->e_slices.size(), bk.blocks, threads, st);
    }
    f.logC = em->m_slice_logc;
    f.sparse_cap = g.sparse_cap; f.sparse_wave_bytes = g.sparse_wave_bytes;   // this bucket's list capacity beside the widest slice
    for (size_t i = 0; accum && i < em->m_slices.size() && !r; i++)
        r = launch_m_slice(bk.mclass, f, em->m_slices[i].first, em->m_slices[i].second, em->e_fused, bk.blocks, threads, st);
    return r;
}

// one bucket of a sliced handle's pass
static int launch_sliced_bucket(bamm_em* em, const EmBucket& bk, const EmKernelArgs& a, const EmPass& p, uint32_t threads, hipStream_t st) {
    const SlicedGeom g = sliced_geometry(em->m_slices, em->Y, em->m_slice_logc, em->m_slice_cap, kMClasses[bk.mclass], threads / 64u);
    // compacted lists instead of dense r between the E pass and the M slices: when the whole odds table is
    // in LDS (the E pass is k_em_seq) and a wave's copy of the decoded sequence fits beside the count slice
    const bool lists = em->e_fused && em->d_list_r && !p.dense_r && g.lists_fit;
    // ... and per pass, decided on the device: while the model is uninformative every window has a non-zero
    // addend and the list walk costs far more than the dense one (config 4, pass 1: 26.5 against 15.4 ms,
    // profiles/r03_c4_cold_passes.txt).  Both flavours of the pass are enqueued; the count the previous pass's
    // E kernel took picks the one that runs (the other's launches return at entry).
    const bool adaptive = lists && p.accumulate && em->d_nnz && em->adaptive_lists;
    if ((!lists || adaptive) && !em->d_state)
        if (int rc = em->mem.scratch(&em->d_state, (size_t)em->seqs->total_len)) return rc;
    if (!adaptive) return launch_sliced_walk(em, bk, a, p.accumulate, lists ? SlicedWalk::kLists : SlicedWalk::kDense, RunWhen::kAlways, g, threads, st);
    if (int rc = launch_sliced_walk(em, bk, a, p.accumulate, SlicedWalk::kDense, RunWhen::kManyWindows, g, threads, st)) return rc;   // dense r while the lists would be long
    return launch_sliced_walk(em, bk, a, p.accumulate, SlicedWalk::kLists, RunWhen::kFewWindows, g, threads, st);
}

// One pass over every launch of the handle, as `p` describes it; every block adds its table into the pass's accumulator.
int run_accumulate(bamm_em* em, const EmPass& p) {
    hipStream_t st = em->ctx->stream;
    int rc = use_device(em->ctx);
    if (rc) return rc;
    UpdateArgs fuse{};
    em->pass_summed_in_kernel = false;
    const bool fusing = p.fuse != EmPass::kNoFuse;
    if (fusing) prepare_update(em, p.fuse == EmPass::kFuseQWindow, true, fuse);     // consumes the previous pass's sums on the stream
    else if ((rc = clean_accumulator(em))) return rc;
    if (em->d_nnz && p.accumulate)                            // sliced path: this pass's count of non-zero windows starts at 0
        BAMM_HIP(hipMemsetAsync(em->d_nnz + (em->nnz_prev_slot ^ 1u), 0, sizeof(unsigned long long), st));
    if (p.timed && (rc = record_event(em, true))) return rc;
    for (size_t b = 0; b < em->ebuckets.size(); b++) {
        const EmBucket& bk = em->ebuckets[b];
        EmKernelArgs a = pass_args(em, bk, p);
        if (bk.mclass == kLongClass) {
            // the sliced path's getR() reads dense r from d_state (slot layout unless the E pass is k_em_seq)
            EmLaunch what = EmLaunch::of_pass(p);
            what.write_r = em->sliced && p.dense_r;
            what.slot_layout = what.write_r && !em->e_fused;
            if (what.write_r && !em->d_state && (rc = em->mem.scratch(&em->d_state, (size_t)em->seqs->total_len))) return rc;
            a.r_out = em->d_state;
            rc = launch_long_bucket(em->ctx, bk, a, what, st);
        } else if (em->sliced) {
            rc = launch_sliced_bucket(em, bk, a, p, bucket_threads(em->ctx, bk), st);
        } else {
            rc = launch_fused(em, bk, EmLaunch::of_pass(p), a, bucket_threads(em->ctx, bk), st, (fusing && b == 0) ? &fuse : nullptr);
        }
        if (rc) return rc;
    }
    if (p.timed && (rc = record_event(em, false))) return rc;
    if (!p.last_model) { em->s_last = em->d_s; em->q_last = em->d_q; em->mask_done = false; }
    if (em->d_nnz && p.accumulate) em->nnz_prev_slot ^= 1u;   // the next pass chooses from what this one counted
    em->acc_dirty = true;                                     // until the update (or the E-only read-out) has consumed it
    return BAMM_OK;
}

// int64 sum of `n_words` words across the ranks, on the context's stream: RCCL or the caller's callback
int allreduce_words(bamm_em* em, void* dev_ptr, size_t n_words) {
    if (em->comm) return comm_allreduce_i64(em->comm, dev_ptr, n_words, em->ctx->stream);
    if (!em->allreduce) return BAMM_OK;
    if (int rc = em->allreduce(em->allreduce_user, dev_ptr, n_words, (void*)em->ctx->stream)) {
        set_error("all-reduce callback failed with %d", rc);
        return BAMM_ERR_COMM;
    }
    return BAMM_OK;
}

int run_allreduce(bamm_em* em) {
    // mode 2: a pass whose launch carried the tail left the all-reduced sums in the accumulator (launch_fused,
    // peer_allreduce_tail).  Every other pass of such a handle -- EStep() alone (an E-only launch has no tail), EM::mask's
    // kernels, a replay -- is summed by the communicator's collective like in mode 1: same integers either way.
    if (em->pass_summed_in_kernel) { em->pass_summed_in_kernel = false; return BAMM_OK; }
    return allreduce_words(em, em->d_acc, em->acc_words());
}

int run_update(bamm_em* em, bool q_window) {
    int rc = use_device(em->ctx);
    if (rc) return rc;
    UpdateArgs u;
    prepare_update(em, q_window, false, u);
    return launch_update(u, em->ctx->stream);
}

// A collective that was already enqueued when a peer aborted the communicator completes with whatever it had: what
// was computed from it is not a model.  Every read-out that follows a stream synchronisation says so.
int comm_still_sound(const bamm_em* em) {
    if (em->comm && comm_aborted(em->comm)) {
        set_error("the communicator was aborted while passes were in flight: the handle's model is not valid");
        return BAMM_ERR_COMM;
    }
    if (em->peer_on && em->d_peer_words) {                   // the stream is idle: did a block give up waiting for a peer?
        uint32_t w[2] = {0, 0};
        BAMM_HIP(hipMemcpy(w, em->d_peer_words, sizeof w, hipMemcpyDeviceToHost));
        if (w[1] != 0u) {
            set_error("in-kernel all-reduce: the sums of rank %u did not arrive within the deadline (peer_timeout_ms); the handle's model is not valid", w[1] - 1u);
            return BAMM_ERR_COMM;
        }
    }
    return BAMM_OK;
}

int fetch_status(bamm_em* em) {
    BAMM_HIP(hipSetDevice(em->ctx->device));
    BAMM_HIP(hipMemcpyAsync(em->h_status, em->d_status, 8 * sizeof(float), hipMemcpyDeviceToHost, em->ctx->stream));
    BAMM_HIP(hipStreamSynchronize(em->ctx->stream));
    return comm_still_sound(em);
}

// optimize(): the status of the call's update `done` (llh, v_diff, ...) into out[8], once it is there.  Where the update's
// writer stores it into the pinned mirror (UpdateArgs::status_mirror) as six self-validating words tagged with `done`, the
// host POLLS them; else it waits for the event recorded behind unit `unit`, whose copy of d_status sits in h_status.
int wait_update_status(bamm_em* em, uint32_t done, uint32_t unit, float* out) {
    std::fill(out, out + 8, 0.0f);
    if (!em->d_status_mirror) {
        if (hipEventSynchronize(em->opt_events[unit & 1u]) != hipSuccess) {
            set_error("hipEventSynchronize failed in optimize()");
            return BAMM_ERR_HIP;
        }
        memcpy(out, em->h_status + 8 + 8 * (done & 1u), 8 * sizeof(float));
        return BAMM_OK;
    }
    const volatile unsigned long long* slot = em->h_tagged + 8 * (done & 1u);
    auto arrived = [&] {
        for (int i = 0; i < 6; i++) {
            const unsigned long long w = slot[i];
            if ((uint32_t)(w >> 32) != done) return false;
            const uint32_t bits = (uint32_t)w;
            memcpy(&out[i], &bits, sizeof(float));
        }
        return true;
    };
    for (uint32_t spins = 1;; spins++) {
        if (arrived()) break;
        if ((spins & 2047u) == 0u) {                                    // now and then: is anything still running?
            const hipError_t qs = hipStreamQuery(em->ctx->stream);
            if (qs == hipSuccess) {                                     // the stream is idle: the tag is there, or never will be
                if (arrived()) break;
                if (int cs = comm_still_sound(em)) return cs;           // (a block gave up waiting for a peer: every later launch did nothing)
                set_error("optimize(): pass %u ended without reporting its status (a kernel of the pass failed?)", done);
                return BAMM_ERR_HIP;
            }
            if (qs != hipErrorNotReady) { (void)hipGetLastError(); set_error("optimize(): %s", hipGetErrorString(qs)); return BAMM_ERR_HIP; }
            if (em->comm && comm_aborted(em->comm)) { set_error("the communicator was aborted while optimize() was waiting for pass %u", done); return BAMM_ERR_COMM; }
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return BAMM_OK;
}

// int64 sums of host[0..n) (n <= 4) over the ranks of the handle's communicator, in place: through the handle's own four
// device words, on the context's stream, synchronised
static int sum_over_ranks(bamm_em* em, long long* host, size_t n) {
    int rc = use_device(em->ctx);
    if (!rc && !em->d_comm_words) rc = em->mem.alloc(&em->d_comm_words, 4);
    if (rc) return rc;
    hipStream_t st = em->ctx->stream;
    hipError_t e = hipMemcpyAsync(em->d_comm_words, host, n * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = comm_allreduce_i64(em->comm, em->d_comm_words, n, st);
    if (e == hipSuccess && !rc) e = hipMemcpyAsync(host, em->d_comm_words, n * sizeof(long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("sum over the ranks (verify_comm): %s", hipGetErrorString(e)); return BAMM_ERR_HIP; }
    return BAMM_OK;
}

// In front of the first pass that all-reduces over a communicator (every rank is in that call, on a thread or a
// process of its own): the ranks sum their sequence counts and compare their accumulator units.  A unit too fine for
// the SUM (8 ranks of 2 M sequences at 2^-40: a cell could reach 2^64) or units that differ would wrap or mis-scale
// silently; here they are an error on every rank at once.
int verify_comm(bamm_em* em) {
    if (!em->comm || em->comm_verified) return BAMM_OK;
    uint32_t world = 1;
    (void)bamm_comm_info(em->comm, nullptr, &world, nullptr);
    long long want_peer = 0;                                 // ranks whose context asks for the in-kernel all-reduce
    if (world > 1) {
        long long h[4] = {(long long)em->seqs->n, (long long)em->fix_shift, (long long)em->fix_shift * (long long)em->fix_shift,
                          em->ctx->use_peer_allreduce ? 1 : 0};
        if (int rc = sum_over_ranks(em, h, 4)) return rc;
        want_peer = h[3];
        if ((long long)world * h[2] != h[1] * h[1]) {
            set_error("the ranks' accumulator units differ (bamm_em_params.n_seqs_bound must be the same on every rank)");
            return BAMM_ERR_ARG;
        }
        if (em->fix_shift > fix_shift_for((uint64_t)h[0])) {
            set_error("%lld sequences over %u ranks need a coarser accumulator unit than 2^-%u: pass their number as "
                      "bamm_em_params.n_seqs_bound on every rank", h[0], world, em->fix_shift);
            return BAMM_ERR_ARG;
        }
    }
    // in-kernel all-reduce, when the context asks for it: every rank must be able to (a pass of ONE launch of the mixed-row
    // kernel, which is built with the tail) and must have mapped every peer's inbox -- the ranks vote, a single refusal keeps
    // all of them on RCCL
    em->peer_on = false;
    if (world > 1 && want_peer == (long long)world) {        // (asked for on every rank: the set-up below is a collective)
        constexpr uint32_t kStride = 2056;                   // entries per (slot, source): 2048 top-order cells + 3 statistics, padded
        // (the tail is built into k_em_mix -- K = 2, both strands, the widths the planner gives mixed rows: the bench / config
        // 2 / 3 / 5 shapes -- and into k_em_grp's classes up to BAMM_FUSE_MAX_M positions per lane at K <= 2: single strand, k = 0 / 1,
        // other widths)
        const EmBucket* eb0 = em->ebuckets.size() == 1u ? &em->ebuckets[0] : nullptr;   // (a shard may plan no launch at all)
        const bool can = eb0 && eb0->grouped && eb0->mclass != kLongClass &&
                         ((eb0->layout & 8u) != 0u || (em->prm.K <= 2u && kMClasses[eb0->mclass] <= BAMM_FUSE_MAX_M)) &&
                         world <= kPeerMaxWorld && em->acc_words() <= kStride && !em->allreduce;
        int ready = 0;
        // (every rank goes through the set-up, able or not: it is a collective; the vote inside it counts mapped inboxes)
        int rc = comm_peer_setup(em->comm, kStride, &ready);
        if (rc) return rc;
        long long vote[1] = {(ready && can) ? 1 : 0};
        if ((rc = sum_over_ranks(em, vote, 1))) return rc;
        if (vote[0] == (long long)world) {
            if (!em->d_peer_words) {
                if ((rc = em->mem.alloc(&em->d_peer_words, 2))) return rc;
                BAMM_HIP(hipMemsetAsync(em->d_peer_words, 0, 2 * sizeof(uint32_t), em->ctx->stream));
            }
            em->peer_on = true;
            em->peer_note.clear();
        } else {
            em->peer_note = !ready ? std::string("inboxes: ") + comm_peer_why(em->comm)
                          : !can ? "this handle's pass is not one launch of a grouped-column kernel built with the tail (K <= 2, one length class of at most 1024 positions, no N-rich sequences beside it)"
                                 : "another rank could not";
        }
    } else if (em->ctx->use_peer_allreduce) {
        em->peer_note = world > 1 ? "not every rank's context asked for it" : "one rank: nothing to reduce";
    }
    em->comm_verified = true;
    return BAMM_OK;
}

}  // namespace bamm
