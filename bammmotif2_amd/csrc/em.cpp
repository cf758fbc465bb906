// The EM handles of the C ABI: create / destroy, E / M / iterate / optimize / mask, the read-outs and the plan,
// communicator and timing queries.  Host code only -- the plan is plan.cpp's, one pass and one update em_pass.cpp's.

#include <cmath>

#include "handles.h"

using namespace bamm;

// The dense r of sequences [begin,end) (a non-empty range), as the E pass the caller last ran gives it, on the device:
// EM::mask's materialised r_, the sliced path's d_state after a replay of that pass (both span the whole set), or a
// scratch block `tmp` owns that the fused / per-column / long-sequence kernels fill for the range.  The handle's pass
// counters and event bookkeeping stay as they were.
int bamm::dense_r_on_device(bamm_em* em, uint64_t begin, uint64_t end, DevBlocks& tmp, DenseR* out) {
    bamm_seqs* s = em->seqs;
    hipStream_t st = em->ctx->stream;
    const uint64_t base = s->h_pos_off[begin], total = s->h_pos_off[end] - base;
    if (em->mask_done) {                                    // EM::mask keeps r_ materialised (EM.cpp:409-430)
        *out = DenseR{em->d_mask_r, 0, false};
        return BAMM_OK;
    }
    // the E pass the caller last ran (EM.cpp:521), without the fold mask: masked-out sequences still have an r in the reference
    const EmPass replay = EmPass::read_out();
    if (em->sliced) {
        // the sliced E pass leaves r per position slot p (window start i = p-W+1) in d_state unless it is k_em_seq
        if (int rc2 = run_accumulate(em, replay)) return rc2;
        *out = DenseR{em->d_state, 0, !em->e_fused};
        return BAMM_OK;
    }
    float* d_r = nullptr;
    int rc = tmp.scratch(&d_r, total);
    if (rc) return rc;
    if (hipMemsetAsync(d_r, 0, total * sizeof(float), st) != hipSuccess) { set_error("hipMemsetAsync failed"); return BAMM_ERR_HIP; }
    const RRange range{d_r, base, (uint32_t)begin, (uint32_t)end};
    for (size_t b = 0; b < em->ebuckets.size() && !rc; b++) {
        const EmBucket& bk = em->ebuckets[b];
        EmKernelArgs a = pass_args(em, bk, replay, &range);
        if (bk.mclass == kLongClass) rc = launch_long_bucket(em->ctx, bk, a, EmLaunch::r_only(), st);
        else rc = launch_fused(em, bk, EmLaunch::r_only(), a, bucket_threads(em->ctx, bk), st);
    }
    *out = DenseR{d_r, base, false};
    return rc;
}

extern "C" {

// ------------------------------------------------------------------------------ EM ---------
int bamm_em_destroy(bamm_em* em) {
    if (!em) return BAMM_OK;
    (void)hipSetDevice(em->ctx->device);
    (void)hipStreamSynchronize(em->ctx->stream);
    for (hipEvent_t e : em->opt_events) if (e) (void)hipEventDestroy(e);
    for (auto& ev : em->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (em->h_status) (void)hipHostFree(em->h_status);
    bamm_seqs_destroy(em->seqs);
    delete em;                                               // its device blocks: set-sized ones go back to the context, the rest is freed
    return BAMM_OK;
}

int bamm_em_create(bamm_ctx* c, bamm_seqs* seqs, const bamm_em_params* prm, const float* vbg, const float* A,
                   const float* v_init, const uint8_t* seq_mask, bamm_em** out) {
    if (!c || !seqs || !prm || !vbg || !A || !v_init || !out) { set_error("bamm_em_create: null argument"); return BAMM_ERR_ARG; }
    *out = nullptr;
    if (seqs->ctx != c) { set_error("sequence set belongs to another context"); return BAMM_ERR_ARG; }
    if (prm->K > BAMM_MAX_ORDER) { set_error("order %u > %d (kmer_ spans 11 bases)", prm->K, BAMM_MAX_ORDER); return BAMM_ERR_ARG; }
    if (prm->W == 0) { set_error("motif width 0"); return BAMM_ERR_ARG; }
    if (seqs->n && seqs->min_len < prm->W) {
        set_error("a sequence of length %u is shorter than the motif (W=%u); the reference drops those before EM (mainBaMM.cpp:75-83)",
                  seqs->min_len, prm->W);
        return BAMM_ERR_ARG;
    }
    const uint32_t Y = (uint32_t)ipow4(prm->K + 1);
    BAMM_HIP(hipSetDevice(c->device));
    bamm_em* em = new bamm_em(c, seqs);
    { std::lock_guard<std::mutex> lock(seqs->mu); seqs->refs++; }
    em->prm = *prm;
    if (em->prm.max_iterations == 0) em->prm.max_iterations = 1000;
    em->Y = Y;
    em->Kbg = std::min(prm->bg_order, prm->K);           // EM.cpp:23
    em->vsz = v_size(prm->K, prm->W);
    em->cells = (size_t)Y * prm->W;
    const bool global_tables = plan_slices(em);
    hipStream_t st = c->stream;
    int rc = BAMM_OK;
    Primers primers;                                         // plan_launches starts them; joined on every way out
    auto fail = [&](int code) { bamm_em_destroy(em); return code; };
    if ((rc = exceptions_for_order(seqs, prm->K, &em->exc))) return fail(rc);
    if ((rc = em->mem.upload(&em->d_vbg, vbg, bg_size(prm->bg_order)))) return fail(rc);
    if ((rc = em->mem.upload(&em->d_A, A, (size_t)(prm->K + 1) * prm->W))) return fail(rc);
    if ((rc = em->mem.upload(&em->d_v, v_init, em->vsz))) return fail(rc);
    if ((rc = em->mem.alloc(&em->d_n, em->vsz))) return fail(rc);
    if ((rc = em->mem.alloc(&em->d_s, (size_t)prm->W * (Y + 1)))) return fail(rc);
    if ((rc = em->mem.alloc(&em->d_s_alt, (size_t)prm->W * (Y + 1)))) return fail(rc);
    for (auto& slot : em->d_qbuf)
        if ((rc = em->mem.upload(&slot, &prm->q, 1))) return fail(rc);
    em->d_q = em->d_qbuf[0];
    if ((rc = em->mem.alloc(&em->d_status, 8))) return fail(rc);
    if ((rc = em->mem.alloc(&em->d_trace, (size_t)em->prm.max_iterations * 3))) return fail(rc);
    if ((rc = em->mem.alloc(&em->d_iteration, 1))) return fail(rc);
    em->acc_stride = (em->acc_words() + 1) & ~(size_t)1;     // slots start on 16-byte boundaries
    if ((rc = em->mem.alloc(&em->d_acc_ring, 3 * em->acc_stride))) return fail(rc);
    em->d_acc = em->d_acc_ring;
    if ((rc = em->mem.alloc(&em->d_v_alt, em->vsz))) return fail(rc);
    if ((rc = em->mem.alloc(&em->d_llh[0], 2))) return fail(rc);
    em->d_llh[1] = em->d_llh[0] + 1;
    if (!update_fits_lds(prm->K, prm->W) && c->use_update_blocks) {
        if ((rc = em->mem.alloc(&em->d_upd_partial, kUpdateMaxBlocks)) || (rc = em->mem.alloc(&em->d_upd_ticket, 1))) return fail(rc);
        if (hipMemsetAsync(em->d_upd_ticket, 0, sizeof(uint32_t), st) != hipSuccess) { set_error("hipMemsetAsync failed"); return fail(BAMM_ERR_HIP); }
    }
    // the counts' unit: for the sequences the caller bounds the sum over the ranks by, else this handle's own
    em->fix_shift = fix_shift_for(std::max<uint64_t>(prm->n_seqs_bound ? prm->n_seqs_bound : (prm->n_seqs_global ? prm->n_seqs_global : seqs->n), 1));
    if (hipMemsetAsync(em->d_n, 0, em->vsz * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(em->d_status, 0, 8 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(em->d_iteration, 0, sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(em->d_llh[0], 0, 2 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(em->d_acc_ring, 0, 3 * em->acc_stride * sizeof(long long), st) != hipSuccess) {
        set_error("hipMemsetAsync failed");
        return fail(BAMM_ERR_HIP);
    }
    if (seq_mask && seqs->n)
        if ((rc = em->mem.upload(&em->d_mask, seq_mask, seqs->n))) return fail(rc);
    em->n_active = seqs->n;
    if (seq_mask) em->n_active = (uint64_t)std::count_if(seq_mask, seq_mask + seqs->n, [](uint8_t m) { return m != 0; });
    if (hipHostMalloc((void**)&em->h_status, 24 * sizeof(float) + 16 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
        set_error("hipHostMalloc failed");
        return fail(BAMM_ERR_HIP);
    }
    memset(em->h_status, 0, 24 * sizeof(float) + 16 * sizeof(unsigned long long));
    em->h_tagged = reinterpret_cast<unsigned long long*>(em->h_status + 24);
    if (hipHostGetDevicePointer((void**)&em->d_status_mirror, em->h_tagged, 0) != hipSuccess) em->d_status_mirror = nullptr;   // then: copies + events
    if ((rc = plan_launches(em, global_tables, seq_mask, primers))) return fail(rc);
    if ((rc = launch_make_s(em->d_v, em->d_vbg, prm->K, prm->W, em->Kbg, em->d_s, st))) return fail(rc);
    em->s_last = em->d_s;
    em->q_last = em->d_q;
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("stream sync failed in bamm_em_create"); return fail(BAMM_ERR_HIP); }
    *out = em;
    return BAMM_OK;
}

int bamm_em_set_allreduce(bamm_em* em, bamm_allreduce_fn fn, void* user) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    // The int64 sums stay below 2^62 as long as (sequences summed over ALL ranks) x 2^fix_shift does; the unit was
    // chosen from this handle's own count unless the caller named a bound.  A callback says nothing about the world
    // behind it: up to 64 ranks of this size are assumed, beyond that the bound is required.
    if (fn && !em->prm.n_seqs_bound && !em->prm.n_seqs_global && em->seqs->n > (uint64_t(1) << 16)) {
        set_error("a shard of %llu sequences behind an all-reduce callback needs bamm_em_params.n_seqs_bound (all ranks together; "
                  "the unit of the integer accumulator must be the same on every rank and sized for their sum)", (unsigned long long)em->seqs->n);
        return BAMM_ERR_ARG;
    }
    em->allreduce = fn;
    em->allreduce_user = user;
    return BAMM_OK;
}

int bamm_em_set_comm(bamm_em* em, bamm_comm* comm) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    if (comm && comm_ctx(comm) != em->ctx) { set_error("the communicator belongs to another context"); return BAMM_ERR_ARG; }
    em->comm_verified = false;                                // checked with the peers in front of the first pass (verify_comm)
    em->comm = comm;
    return BAMM_OK;
}

int bamm_em_estep(bamm_em* em) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    if (int vrc = verify_comm(em)) return vrc;
    // s already reflects the current v (made at create / by the last update): E only
    int rc = run_accumulate(em, EmPass::e_only());
    if (rc) return rc;
    if ((rc = run_allreduce(em))) return rc;
    if ((rc = launch_stat_only(em->d_acc, (uint32_t)em->cells, em->d_status, em->ctx->stream))) return rc;
    em->acc_dirty = false;
    em->estep_done = true;
    return BAMM_OK;
}

int bamm_em_mstep(bamm_em* em) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    if (int vrc = verify_comm(em)) return vrc;
    if (!em->estep_done) { set_error("MStep needs the responsibilities of a preceding EStep"); return BAMM_ERR_STATE; }
    // the responsibilities are a pure function of (s, q), both unchanged since the EStep:
    // recompute them on the fly while accumulating counts instead of storing N*L floats
    int rc = run_accumulate(em, EmPass::counting().with_last_model());   // with the (s, q) the EStep saw, even if q moved since
    if (!rc) rc = run_allreduce(em);
    if (!rc) rc = run_update(em, false);              // outside the q window: EM::MStep never touches q
    return rc;
}

int bamm_em_optimize_q(bamm_em* em) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    int rc = fetch_status(em);
    if (rc) return rc;
    const double nseq = em->prm.n_seqs_global ? (double)em->prm.n_seqs_global : (double)em->h_status[5];
    const float q = (float)((nseq - (double)em->h_status[4] + 1.0) / (nseq + 2.0));   // EM.cpp:515
    // the slot the last EStep read stays intact for MStep()/getR(), in whatever order the caller
    // runs MStep() and optimize_q() (EM.cpp:93-99 has MStep first)
    float* slot = q_write_slot(em);
    BAMM_HIP(hipSetDevice(em->ctx->device));
    BAMM_HIP(hipMemcpyAsync(slot, &q, sizeof(float), hipMemcpyHostToDevice, em->ctx->stream));
    BAMM_HIP(hipStreamSynchronize(em->ctx->stream));
    em->d_q = slot;
    return BAMM_OK;
}

int bamm_em_accumulate(bamm_em* em) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    return run_accumulate(em, EmPass::counting());
}

int bamm_em_reduce_buffer(bamm_em* em, void** dev_ptr, uint64_t* n_words) {
    if (!em || !dev_ptr || !n_words) { set_error("bad argument"); return BAMM_ERR_ARG; }
    *dev_ptr = em->d_acc;
    *n_words = em->acc_words();
    return BAMM_OK;
}

int bamm_em_set_reduce_buffer(bamm_em* em, void* dev_ptr, uint64_t n_words) {
    if (!em || !dev_ptr) { set_error("bad argument"); return BAMM_ERR_ARG; }
    if (n_words < em->acc_words()) {
        set_error("reduce buffer holds %llu 64-bit words, %llu needed", (unsigned long long)n_words, (unsigned long long)em->acc_words());
        return BAMM_ERR_ARG;
    }
    BAMM_HIP(hipSetDevice(em->ctx->device));
    BAMM_HIP(hipStreamSynchronize(em->ctx->stream));
    em->mem.release(em->d_acc_ring);                         // a caller-owned accumulator is one slot: no fused updates
    em->acc_cur = 0; em->ring_prev_dirty = false; em->fusable = false;
    em->d_acc = static_cast<long long*>(dev_ptr);
    em->acc_external = true;
    em->acc_dirty = false;
    BAMM_HIP(hipMemsetAsync(em->d_acc, 0, em->acc_words() * sizeof(long long), em->ctx->stream));
    return BAMM_OK;
}

int bamm_em_update(bamm_em* em) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    // hand-driven passes have no optimize() call to be local to: the handle's first five updates
    return run_update(em, em->host_iteration < 5u);
}

int bamm_em_iterate(bamm_em* em, uint32_t n) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    if (int vrc = verify_comm(em)) return vrc;
    TimedRegion region(em);                                  // (closes on an error return as well)
    // fusable handles: the update of pass i runs in the prologue of pass i+1's first kernel (one launch and one
    // collective per iteration); the last pass's update is a k_update launch, so the handle is in the same state
    // at every API boundary whichever way its updates ran
    for (uint32_t i = 0; i < n; i++) {
        const EmPass pass = (em->fusable && i > 0u) ? EmPass::counting().with_fused_update(i - 1u < 5u) : EmPass::counting();
        int rc = run_accumulate(em, pass);
        if (!rc && i + 1u == n) rc = close_timed_region(em); // a whole-call interval ends behind the last pass's sequence kernel
        if (!rc) rc = run_allreduce(em);
        if (!rc && (!em->fusable || i + 1u == n)) rc = run_update(em, i < 5u);
        if (rc) { em->acc_dirty = true; return rc; }
    }
    return BAMM_OK;
}

int bamm_em_optimize(bamm_em* em, uint32_t* iterations) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    if (int vrc = verify_comm(em)) return vrc;
    TimedRegion region(em);
    if (iterations) *iterations = 0;
    const uint32_t max_it = em->prm.max_iterations;
    if (max_it == 0) return BAMM_OK;
    int rc = use_device(em->ctx);
    if (rc) return rc;
    hipStream_t st = em->ctx->stream;
    // The stop rule (EM.cpp:117-118) needs (llh, v_diff) of a pass on the host: a read-back and a stream
    // synchronisation per pass, 13 us during which the GPU idles (half of a pass at 300 sequences, a sixth at 50k).
    // So the loop runs AHEAD of the numbers it waits for.  The update evaluates the same rule on the device and
    // raises a flag; whatever was enqueued behind a raised flag does nothing (every kernel returns at entry), so the
    // model is exactly what the stopping pass left, and the host takes back the bookkeeping of the work that did
    // not happen (prepare_update keeps a snapshot per update).
    //
    // The stream carries UNITS.  Plain handles: unit u = pass u + all-reduce + k_update(u); status(u) is there when
    // unit u is.  Fusable handles (update_kernel.h): unit u = [update(u-1) in the prologue of] pass u + all-reduce,
    // and one last unit max_it + 1 = k_update(max_it); status(u) is there when unit u + 1 is (lag 1).  A fused
    // update that fires the rule ends every block of its kernel before the pass: same model, same trace.
    if (!em->d_stop && (rc = em->mem.alloc(&em->d_stop, 1))) return rc;
    for (hipEvent_t& e : em->opt_events)
        if (!e) BAMM_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    BAMM_HIP(hipMemsetAsync(em->d_stop, 0, sizeof(uint32_t), st));
    const uint32_t lag = em->fusable ? 1u : 0u;
    const uint32_t units = max_it + lag;
    // The status of update i reaches the host through pinned memory the update's writer stores into (UpdateArgs::
    // status_mirror) as six self-validating words tagged with i: the host POLLS them (wait_update_status).  An event per unit, which
    // this loop used to record and wait for, costs the stream 4 us per pass (optimize() against iterate(): +4.5 us at every size up to
    // 50k sequences, profiles/r05_optimize_vs_iterate.txt); events remain the fallback where the mirror could not be mapped.
    const bool poll = em->d_status_mirror != nullptr;
    if (poll) memset(em->h_tagged, 0, 16 * sizeof(unsigned long long));         // no tag of an earlier call (tags start at 1)
    const uint32_t first_update = em->host_iteration;       // update(i) of this call is the handle's update first_update + i
    em->stop_arg = em->d_stop;
    em->opt_llh_prev = em->llh_prev;
    auto enqueue_unit = [&](uint32_t u) -> int {            // 1-based
        int r = BAMM_OK;
        if (u <= max_it) {
            if (lag && u >= 2u) {
                em->opt_iteration = u - 1u;
                r = run_accumulate(em, EmPass::counting().with_fused_update(u - 1u <= 5u));     // EM.cpp:99 for update(u-1)
            } else {
                r = run_accumulate(em, EmPass::counting());
            }
            if (!r) r = run_allreduce(em);
            if (!r && !lag) { em->opt_iteration = u; r = run_update(em, u <= 5u); }    // EM.cpp:99
        } else {
            em->opt_iteration = max_it;
            r = run_update(em, max_it <= 5u);
        }
        if (r) return r;
        const uint32_t upd = u - lag;                        // the update this unit carried (0: none)
        if (!poll) {
            if (upd >= 1u) BAMM_HIP(hipMemcpyAsync(em->h_status + 8 + 8 * (upd & 1u), em->d_status, 8 * sizeof(float), hipMemcpyDeviceToHost, st));
            BAMM_HIP(hipEventRecord(em->opt_events[u & 1u], st));
        }
        return BAMM_OK;
    };
    // every exit: the kernels stop looking at the flag; sums nobody consumed are cleared before the next pass
    auto leave = [&](int r) { em->stop_arg = nullptr; if (r) em->acc_dirty = true; return r; };
    uint32_t enqueued = 0, done = 0;
    float llh = em->llh_prev;
    for (;;) {                                                              // EM.cpp:81
        done++;
        while (enqueued < std::min(units, done + lag + 1u)) {               // the unit with status(done) and one beyond it
            if ((rc = enqueue_unit(enqueued + 1u))) return leave(rc);
            enqueued++;
        }
        float hs[8];
        if ((rc = wait_update_status(em, done, done + lag, hs))) return leave(rc);
        const float llh_prev = llh;
        llh = hs[0];
        const float v_diff = hs[1];
        bool iterate = true;
        if (v_diff < em->prm.epsilon) iterate = false;                      // EM.cpp:117
        if (llh - llh_prev < 0 && done > 10) iterate = false;               // EM.cpp:118
        if (!iterate || done == max_it) {
            memcpy(em->h_status, hs, 8 * sizeof(float));
            if (!iterate) {
                // whatever was enqueued behind update(done) found the flag raised and did nothing: back to the snapshot
                // prepare_update took right after update(done) (buffers, iteration count, kernel-timing samples)
                em->book() = em->books[(first_update + done) & 3u];
                if (lag) em->acc_dirty = true;                              // the ring slot the fused update read was never cleared
            }
            break;
        }
    }
    em->stop_arg = nullptr;
    em->llh_prev = llh;
    if (iterations) *iterations = done;
    return BAMM_OK;
}

// ---- EM::mask (EM.cpp:261-503) in stages: checks, plan (plan.cpp: mask_plan), buffers, selection, EM over the listed windows ----
static int mask_checks(const bamm_em* em, float f) {
    if (!(f > 0.0f && f < 1.0f)) { set_error("bamm_em_mask: fraction %g outside (0,1)", (double)f); return BAMM_ERR_ARG; }
    if (em->n_active == 0) { set_error("bamm_em_mask: no sequences (the reference indexes an empty array, EM.cpp:343)"); return BAMM_ERR_ARG; }
    if (em->prm.W < 2) { set_error("bamm_em_mask: W=1 reads past pos_[n] in the reference (EM.cpp:416)"); return BAMM_ERR_UNSUPPORTED; }
    if (em->prm.optimize_q && (em->allreduce || em->comm)) {
        set_error("bamm_em_mask: optimize_q re-estimates q after every sequence (EM.cpp:321), a serial chain that cannot be sharded");
        return BAMM_ERR_UNSUPPORTED;
    }
    if (em->host_iteration != 0 || em->estep_done) {
        set_error("bamm_em_mask: the handle has already run E/M passes; the reference calls mask() on a fresh EM only");
        return BAMM_ERR_STATE;
    }
    return BAMM_OK;
}

// the handle's EM::mask state (allocated on first use) zeroed, and the kernels' arguments over it
static int mask_buffers(bamm_em* em, const MaskPlan& p, MaskKernelArgs* out) {
    bamm_seqs* s = em->seqs;
    hipStream_t st = em->ctx->stream;
    int rc;
    if (!em->d_mask_r) {
        em->mask_blocks = p.mblocks;
        if ((!p.direct && (rc = em->mem.alloc(&em->d_mask_partial_n, (size_t)p.mblocks * em->cells))) ||
            (rc = em->mem.alloc(&em->d_mask_partial_stat, (size_t)p.mblocks * 4)) ||
            (rc = em->mem.scratch(&em->d_mask_r, (size_t)s->total_len)) ||
            (rc = em->mem.alloc(&em->d_mask_bits, (size_t)s->total_len / 32 + 2)) ||
            (rc = em->mem.alloc(&em->d_mask_hist, 2049)) || (rc = em->mem.alloc(&em->d_mask_sel, 1)) ||
            (em->prm.optimize_q && (rc = em->mem.alloc(&em->d_mask_qseq, (size_t)s->n))))
            return rc;
    }
    BAMM_HIP(hipMemsetAsync(em->d_mask_r, 0, (size_t)s->total_len * sizeof(float), st));
    BAMM_HIP(hipMemsetAsync(em->d_mask_bits, 0, ((size_t)s->total_len / 32 + 2) * sizeof(uint32_t), st));
    BAMM_HIP(hipMemsetAsync(em->d_mask_hist, 0, 2049 * sizeof(long long), st));
    BAMM_HIP(hipMemsetAsync(em->d_mask_sel, 0, sizeof(MaskSelect), st));
    MaskKernelArgs a{};
    a.sv = make_view(s, em->exc, nullptr, (uint32_t)s->n, em->d_mask);   // every sequence in natural order
    a.K = em->prm.K; a.W = em->prm.W; a.Y = em->Y;
    a.max_len = s->max_len;
    a.wave_bytes = (uint32_t)p.wave_bytes;
    a.v0 = em->d_v; a.vbg0 = em->d_vbg;
    a.q = em->d_q;
    a.q_seq = em->prm.optimize_q ? em->d_mask_qseq : nullptr;
    a.n_total = (float)em->n_active;
    a.fix_scale = em->fix_scale();
    a.r = em->d_mask_r; a.bits = em->d_mask_bits; a.hist = em->d_mask_hist; a.sel = em->d_mask_sel;
    a.partial_n = em->d_mask_partial_n; a.partial_stat = em->d_mask_partial_stat;
    *out = a;
    return BAMM_OK;
}

// the windows EM::mask trains on: the order-0 pass (EM.cpp:266-323), the cut-off at fraction f in three histogram
// passes (EM.cpp:329-343), a bit per listed window (EM.cpp:345-356)
static int mask_select(bamm_em* em, const MaskPlan& p, MaskKernelArgs& a, float f) {
    hipStream_t st = em->ctx->stream;
    auto blocks_for = [&](uint32_t waves) {                  // every launch here has at most cus * 8 blocks
        const uint32_t need = ((uint32_t)em->seqs->n + waves - 1) / waves;
        return std::max(1u, std::min(need, p.cus * 8));
    };
    int rc;
    a.table_bytes = p.init_table;
    const uint32_t waves = p.waves_for(p.init_table);
    if ((rc = launch_mask_init(a, em->prm.optimize_q != 0, blocks_for(waves), waves * 64, st))) return rc;
    for (int pass = 0; pass < 3; pass++) {
        if ((rc = launch_mask_hist(a, pass, blocks_for(4), st))) return rc;
        if ((rc = allreduce_words(em, em->d_mask_hist, 2049))) return rc;
        if ((rc = launch_mask_pick(a, pass, f, st))) return rc;
    }
    return launch_mask_bits(a, blocks_for(4), st);
}

// EM over the listed windows (EM.cpp:373-494); *iteration = passes run, *llh = the last one's
static int mask_em_loop(bamm_em* em, const MaskPlan& p, MaskKernelArgs& a, uint32_t* iteration, float* llh) {
    hipStream_t st = em->ctx->stream;
    const uint32_t W = em->prm.W;
    int rc = BAMM_OK;
    bool iterate = true;
    while (iterate && *iteration < em->prm.max_iterations && !rc) {
        (*iteration)++;
        const float llh_prev = *llh;
        a.s = em->d_s;
        a.q = em->d_q;
        if ((rc = record_event(em, true))) break;
        a.table_bytes = (uint32_t)p.e_table;
        rc = launch_mask_e(a, p.s_in_lds, p.mblocks, p.e_waves * 64, st);
        a.table_bytes = (uint32_t)p.m_table;
        for (uint32_t j0 = 0; j0 < W && !rc; j0 += p.m_cols) {
            a.j0 = j0; a.j1 = std::min(W, j0 + p.m_cols);
            a.acc_direct = p.direct ? em->d_acc : nullptr;
            rc = launch_mask_m(a, p.mblocks, p.m_waves * 64, st);
        }
        if (!rc) rc = record_event(em, false);
        if (!rc) rc = launch_reduce_partials(p.direct ? nullptr : em->d_mask_partial_n, em->d_mask_partial_stat, p.mblocks, W, em->Y, em->d_acc, st);
        if (!rc) rc = run_allreduce(em);
        if (!rc) rc = run_update(em, false);
        if (!rc) rc = fetch_status(em);
        if (rc) break;
        *llh = em->h_status[0];
        if (em->h_status[1] < em->prm.epsilon) iterate = false;            // EM.cpp:488
        if (*llh - llh_prev < 0 && *iteration > 10) iterate = false;       // EM.cpp:489
    }
    return rc;
}

int bamm_em_mask(bamm_em* em, float f, uint32_t* iterations, float* cutoff, uint64_t* listed) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    if (int vrc = verify_comm(em)) return vrc;
    em->pass_summed_in_kernel = false;                       // EM::mask's kernels carry no tail: every one of its sums goes through the communicator
    int rc = mask_checks(em, f);
    if (rc || (rc = use_device(em->ctx))) return rc;
    if ((rc = clean_accumulator(em))) return rc;              // sums nobody consumed (bamm_em_accumulate without an update, a getR replay)
    const MaskPlan p = mask_plan(em->prm.W, em->Y, em->seqs->max_len, em->seqs->n, em->cells, em->ctx->num_cus);
    if (p.wave_bytes > 0xffffffffull) { set_error("bamm_em_mask: sequences beyond 2^28 positions"); return BAMM_ERR_UNSUPPORTED; }
    hipStream_t st = em->ctx->stream;
    MaskKernelArgs a;
    if ((rc = mask_buffers(em, p, &a))) return rc;
    DevBlocks wave_guard(em->ctx);
    if (p.wave_global && (rc = wave_guard.scratch(&a.wave_scratch, p.wave_scratch_bytes))) return rc;
    if ((rc = mask_select(em, p, a, f))) return rc;

    TimedRegion region(em);
    uint32_t iteration = 0;
    float llh = em->llh_prev;
    if ((rc = mask_em_loop(em, p, a, &iteration, &llh))) return rc;   // (its updates run outside the q window: q is not touched inside the loop)
    em->llh_prev = llh;
    em->mask_done = true;
    MaskSelect sel;
    BAMM_HIP(hipMemcpyAsync(&sel, em->d_mask_sel, sizeof(sel), hipMemcpyDeviceToHost, st));
    BAMM_HIP(hipStreamSynchronize(st));
    if (iterations) *iterations = iteration;
    if (cutoff) *cutoff = sel.cutoff;
    if (listed) *listed = sel.listed;
    return BAMM_OK;
}

static int copy_out(bamm_em* em, float* dst, const float* src, size_t count) {
    if (!em || !dst) { set_error("bad argument"); return BAMM_ERR_ARG; }
    BAMM_HIP(hipSetDevice(em->ctx->device));
    if (int rc = ctx_download(em->ctx, dst, src, count * sizeof(float))) return rc;
    BAMM_HIP(hipStreamSynchronize(em->ctx->stream));
    return comm_still_sound(em);
}

int bamm_em_get_v(bamm_em* em, float* v) { return copy_out(em, v, em ? em->d_v : nullptr, em ? em->vsz : 0); }
int bamm_em_get_counts(bamm_em* em, float* n) { return copy_out(em, n, em ? em->d_n : nullptr, em ? em->vsz : 0); }

int bamm_em_get_s(bamm_em* em, float* s) {
    if (!em || !s) { set_error("bad argument"); return BAMM_ERR_ARG; }
    const size_t Ys = em->Y + 1;
    std::vector<float> tmp((size_t)em->prm.W * Ys);
    int rc = copy_out(em, tmp.data(), em->d_s, tmp.size());
    if (rc) return rc;
    for (uint32_t y = 0; y < em->Y; y++)
        for (uint32_t j = 0; j < em->prm.W; j++) s[(size_t)y * em->prm.W + j] = tmp[(size_t)j * Ys + y];
    return BAMM_OK;
}

int bamm_em_get_q(bamm_em* em, float* q) { return copy_out(em, q, em ? em->d_q : nullptr, 1); }

static int status_word(bamm_em* em, int i, float* out) {     // [0] llh, [1] v_diff of the last update
    if (!em || !out) { set_error("bad argument"); return BAMM_ERR_ARG; }
    int rc = fetch_status(em);
    if (rc) return rc;
    *out = em->h_status[i];
    return BAMM_OK;
}

int bamm_em_get_llh(bamm_em* em, float* llh) { return status_word(em, 0, llh); }
int bamm_em_get_vdiff(bamm_em* em, float* vd) { return status_word(em, 1, vd); }

int bamm_em_get_iteration(bamm_em* em, uint32_t* it) {
    if (!em || !it) { set_error("bad argument"); return BAMM_ERR_ARG; }
    *it = em->host_iteration;
    return BAMM_OK;
}

int bamm_em_get_r(bamm_em* em, uint64_t begin, uint64_t end, float* out, uint64_t out_cap) {
    if (!em || !out || begin > end || end > em->seqs->n) { set_error("bamm_em_get_r: bad range"); return BAMM_ERR_ARG; }
    bamm_seqs* s = em->seqs;
    const uint64_t base = s->h_pos_off[begin], total = s->h_pos_off[end] - base;
    if (out_cap < total) { set_error("bamm_em_get_r: output holds %llu floats, %llu needed", (unsigned long long)out_cap, (unsigned long long)total); return BAMM_ERR_ARG; }
    if (total == 0) return BAMM_OK;
    BAMM_HIP(hipSetDevice(em->ctx->device));
    hipStream_t st = em->ctx->stream;
    DevBlocks tmp(em->ctx);
    DenseR dr;
    int rc = dense_r_on_device(em, begin, end, tmp, &dr);
    if (rc) return rc;
    rc = ctx_download(em->ctx, out, dr.r + (base - dr.base), total * sizeof(float));
    if (!rc && hipStreamSynchronize(st) != hipSuccess) { set_error("copy of r failed"); rc = BAMM_ERR_HIP; }
    if (!rc && dr.slot_layout)                               // window start i sits at slot i+W-1; the reference's index is L-W-i (EM.cpp:173)
        for (uint64_t n = begin; n < end; n++) {
            float* r = out + (s->h_pos_off[n] - base);
            std::reverse(r, r + s->h_len[n]);
        }
    return rc;
}

int bamm_em_get_trace(bamm_em* em, float* llh, float* v_diff, float* q, uint32_t cap, uint32_t* n) {
    if (!em || !n) { set_error("bad argument"); return BAMM_ERR_ARG; }
    const uint32_t avail = std::min(em->host_iteration, em->prm.max_iterations);
    *n = avail;
    const uint32_t m = std::min(avail, cap);
    if (m == 0) return BAMM_OK;
    std::vector<float> tmp((size_t)m * 3);
    int rc = copy_out(em, tmp.data(), em->d_trace, tmp.size());
    if (rc) return rc;
    for (uint32_t i = 0; i < m; i++) {
        if (llh) llh[i] = tmp[(size_t)i * 3 + 0];
        if (v_diff) v_diff[i] = tmp[(size_t)i * 3 + 1];
        if (q) q[i] = tmp[(size_t)i * 3 + 2];
    }
    return BAMM_OK;
}

int bamm_em_plan(bamm_em* em, uint64_t* grouped_seqs, uint64_t* percolumn_seqs, uint32_t* launches) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    uint64_t g = 0, o = 0;
    for (auto& b : em->ebuckets) (b.grouped ? g : o) += b.count;
    if (grouped_seqs) *grouped_seqs = g;
    if (percolumn_seqs) *percolumn_seqs = o;
    if (launches) *launches = (uint32_t)em->ebuckets.size();
    return BAMM_OK;
}

int bamm_em_plan_mixed(bamm_em* em, uint64_t* mixed_seqs) {
    if (!em || !mixed_seqs) { set_error("bad argument"); return BAMM_ERR_ARG; }
    uint64_t m = 0;
    for (auto& b : em->ebuckets) if (b.grouped && (b.layout & 8u)) m += b.count;
    *mixed_seqs = m;
    return BAMM_OK;
}

int bamm_em_plan_launch(bamm_em* em, uint32_t index, uint64_t* out) {
    if (!em || !out || index >= em->ebuckets.size()) { set_error("bamm_em_plan_launch: bad argument"); return BAMM_ERR_ARG; }
    const EmBucket& b = em->ebuckets[index];
    const bool mixed = b.grouped && (b.layout & 8u);
    out[0] = b.count;
    out[1] = b.mclass == kLongClass ? 0u : (uint64_t)kMClasses[b.mclass];
    out[2] = mixed ? 1u : 0u;
    out[3] = mixed && (b.layout & kMixAnchorBit) ? 1u : 0u;
    return BAMM_OK;
}

int bamm_em_plan_paths(bamm_em* em, int* sliced, int* e_fused, uint64_t* long_seqs) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    uint64_t l = 0;
    for (auto& b : em->ebuckets) if (b.mclass == kLongClass) l += b.count;
    if (sliced) *sliced = em->sliced ? 1 : 0;
    if (e_fused) *e_fused = em->sliced && em->e_fused ? 1 : 0;
    if (long_seqs) *long_seqs = l;
    return BAMM_OK;
}

int bamm_em_plan_update(const bamm_em* em, int* form, int* fusable) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    // prepare_update hands every update the handle's band scratch, allocated at creation or never
    if (form) *form = update_form(em->prm.K, em->prm.W, em->d_upd_partial != nullptr && em->d_upd_ticket != nullptr);
    if (fusable) *fusable = em->fusable ? 1 : 0;
    return BAMM_OK;
}

int bamm_em_tile_geometry(uint32_t W, uint32_t* tile_positions, uint32_t* stride) {
    if (!em_tile_geometry(W, tile_positions, stride)) {
        set_error("bamm_em_tile_geometry: W=%u leaves a tile no stride of at least 16 positions", W);
        return BAMM_ERR_ARG;
    }
    return BAMM_OK;
}

int bamm_em_tile_plan(bamm_em* em, uint64_t* tiled_seqs, uint64_t* tiles, uint64_t* window_seqs) {
    if (!em) { set_error("null em"); return BAMM_ERR_ARG; }
    uint64_t ts = 0, nt = 0, ws = 0;
    for (auto& b : em->ebuckets) {
        if (b.mclass != kLongClass) continue;
        if (b.tiled) { ts += b.count; nt += b.n_tiles; } else ws += b.count;
    }
    if (tiled_seqs) *tiled_seqs = ts;
    if (tiles) *tiles = nt;
    if (window_seqs) *window_seqs = ws;
    return BAMM_OK;
}

int bamm_em_comm_mode(bamm_em* em, int* mode, char* note, size_t note_cap) {
    if (!em || !mode) { set_error("bad argument"); return BAMM_ERR_ARG; }
    if (int vrc = verify_comm(em)) return vrc;                // collective on first use, like the first pass would be
    *mode = em->peer_on ? 2 : ((em->comm || em->allreduce) ? 1 : 0);
    if (note && note_cap) snprintf(note, note_cap, "%s", em->peer_note.c_str());
    return BAMM_OK;
}

int bamm_em_set_kernel_timing(bamm_em* em, uint32_t every) {
    if (!em) { set_error("null EM handle"); return BAMM_ERR_ARG; }
    em->timing_every = every;
    return BAMM_OK;
}

int bamm_em_kernel_time(bamm_em* em, float* total_ms, uint32_t* launches) {
    if (!em || !total_ms || !launches) { set_error("bad argument"); return BAMM_ERR_ARG; }
    if (int rc = close_timed_region(em)) return rc;           // hand-driven passes (bamm_em_accumulate) in whole-call mode
    BAMM_HIP(hipStreamSynchronize(em->ctx->stream));
    float acc = 0.0f;
    uint32_t passes = 0;
    for (uint32_t i = 0; i < em->events_used; i++) {
        float ms = 0.0f;
        BAMM_HIP(hipEventElapsedTime(&ms, em->events[i].first, em->events[i].second));
        acc += ms;
        passes += em->event_passes[i];
    }
    *total_ms = acc;
    *launches = passes;
    return BAMM_OK;
}

}  // extern "C"
