"""Host-side mirror of the reference's EM / ScoreSeqSet interface over the C ABI.

Method names follow the reference (`EStep`, `MStep`, `optimize`, `optimize_q`, `getR`, `getQ`;
/root/reference/src/refinement/EM.h:20-36, seq_scoring/ScoreSeqSet.h:26-36) so that the parity
tests read like calls into the reference.  Everything numeric happens in libbamm_em.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import numpy as np

from . import abi
from .abi import check


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def v_size(K: int, W: int) -> int:
    return W * ((4 ** (K + 2) - 4) // 3)


def v_offset(k: int, W: int) -> int:
    return W * ((4 ** (k + 1) - 4) // 3)


def bg_size(K: int) -> int:
    return (4 ** (K + 2) - 4) // 3


def bg_offset(k: int) -> int:
    return (4 ** (k + 1) - 4) // 3


def libc_srand(seed: int = 42) -> None:
    """mainBaMM.cpp:22 -- the reference seeds libc's rand() once before reading sequences."""
    C.CDLL(None).srand(C.c_uint(seed))


class PackedSeqs:
    """Host-resident 2-bit packed sequence set (+ N exceptions)."""

    def __init__(self, ptr):
        self._p = ptr
        self.lib = abi.load()

    @classmethod
    def from_kmers(cls, kmer, off) -> "PackedSeqs":
        lib = abi.load()
        off = _u64(off)
        out = C.POINTER(abi.Packed)()
        check(lib.bamm_pack_kmers(_u64(kmer), off, len(off) - 1, C.byref(out)))
        return cls(out)

    @classmethod
    def from_codes(cls, codes, off, single_strand: bool = False, seed: Optional[int] = 42) -> "PackedSeqs":
        lib = abi.load()
        off = _u64(off)
        out = C.POINTER(abi.Packed)()
        if seed is not None:      # the libc stream starts at srand(seed): the draws may be taken on all host threads
            check(lib.bamm_pack_codes_seeded(np.ascontiguousarray(codes, np.uint8), off, len(off) - 1,
                                             int(single_strand), seed, C.byref(out)))
        else:                     # wherever the caller's libc stream stands
            check(lib.bamm_pack_codes(np.ascontiguousarray(codes, np.uint8), off, len(off) - 1,
                                      int(single_strand), C.byref(out)))
        return cls(out)

    @property
    def c(self):
        return self._p.contents

    @property
    def n_seqs(self) -> int:
        return int(self.c.n_seqs)

    @property
    def total_len(self) -> int:
        return int(self.c.total_len)

    @property
    def lengths(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.c.len, (max(self.n_seqs, 1),))[: self.n_seqs].copy()

    @property
    def n_exceptions(self) -> int:
        return int(self.c.n_exc)

    @property
    def words(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.c.words, (max(int(self.c.n_words), 1),))[: int(self.c.n_words)].copy()

    def arrays(self) -> dict:
        """Every array of the packed set (copies): words, word_off, len, exc_off, exc_pos, exc_kmer, exc_clean."""
        c, n, ne = self.c, self.n_seqs, int(self.c.n_exc)
        view = lambda ptr, count: np.ctypeslib.as_array(ptr, (max(count, 1),))[:count].copy()
        return dict(words=view(c.words, int(c.n_words)), word_off=view(c.word_off, n + 1), len=view(c.len, n),
                    exc_off=view(c.exc_off, n + 1), exc_pos=view(c.exc_pos, ne), exc_kmer=view(c.exc_kmer, ne),
                    exc_clean=view(c.exc_clean, ne), total_len=int(c.total_len), max_len=int(c.max_len), min_len=int(c.min_len))

    def offsets(self) -> np.ndarray:
        return np.concatenate([[0], np.cumsum(self.lengths.astype(np.int64))]).astype(np.uint64)

    def unpack_y(self, K: int) -> np.ndarray:
        out = np.zeros(max(self.total_len, 1), np.uint32)
        check(self.lib.bamm_unpack_y(self._p, K, out))
        return out[: self.total_len]

    def bg_model(self, K: int, alpha) -> np.ndarray:
        """BackgroundModel (BackgroundModel.cpp:3-46,441-473) learned from this set."""
        out = np.zeros(bg_size(K), np.float32)
        alpha = _f32(alpha)
        assert len(alpha) >= K + 1
        check(self.lib.bamm_bg_model(self._p, K, alpha, out))
        return out

    def shard_range(self, W: int, rank: int, world: int):
        b, e = C.c_uint64(0), C.c_uint64(0)
        lens = np.ascontiguousarray(self.lengths, np.uint32)
        if len(lens) == 0:
            lens = np.zeros(1, np.uint32)
        check(self.lib.bamm_shard_range(lens, self.n_seqs, W, rank, world, C.byref(b), C.byref(e)))
        return int(b.value), int(e.value)

    def free(self):
        if self._p:
            self.lib.bamm_packed_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_count() -> int:
    """HIP devices visible to this process (raises without one: there is no CPU fallback)."""
    n = C.c_int()
    check(abi.load().bamm_device_count(C.byref(n)))
    return int(n.value)


def device_blocks_live() -> int:
    """Device blocks the library has handed out and not yet taken back, process-wide (bamm_device_blocks_live; for tests)."""
    return int(abi.load().bamm_device_blocks_live())


MASK_PLAN_FIELDS = ("direct", "wave_global", "wave_bytes", "s_in_lds", "e_table", "m_cols", "m_table", "init_table", "e_waves",
                    "m_waves", "cus", "mblocks", "wave_scratch_bytes")


def mask_plan(W: int, Y: int, max_len: int, n_seqs: int, cells: int, num_cus: int) -> dict:
    """The launch geometry of EM.mask() for these sizes (bamm_mask_plan: a pure function, no device needed)."""
    out = np.zeros(len(MASK_PLAN_FIELDS), np.uint64)
    check(abi.load().bamm_mask_plan(W, Y, max_len, n_seqs, cells, num_cus, out))
    return dict(zip(MASK_PLAN_FIELDS, (int(x) for x in out)))


def mix_layout(W: int, M: int) -> dict:
    """The mixed-row kernel's layout for motif width W at M positions per lane (bamm_mix_layout: a pure function, no device
    needed): T groups of which the first B are narrow and A wide, n1c leading columns with resident bins."""
    out = (C.c_uint32 * 4)()
    check(abi.load().bamm_mix_layout(W, M, out))
    return dict(zip(("T", "B", "A", "n1c"), (int(x) for x in out)))


def mix_fix_word(lane: int, W: int, T: int, B: int, n1c: int, L: int, xw: int, xfields: int, sE: int):
    """(word y of the lane's record, the lane is a fix lane) for one sequence (bamm_mix_fix_word: a pure function, no device needed)."""
    out = (C.c_uint32 * 2)()
    check(abi.load().bamm_mix_fix_word(lane, W, T, B, n1c, L, xw, xfields, sE, out))
    return int(out[0]), bool(out[1])


def device_pci_bus_id(device: int) -> str:
    buf = C.create_string_buffer(32)
    check(abi.load().bamm_device_pci_bus_id(int(device), buf, 32))
    return buf.value.decode()


def device_can_access_peer(device: int, peer: int) -> bool:
    can = C.c_int(0)
    check(abi.load().bamm_device_can_access_peer(int(device), int(peer), C.byref(can)))
    return bool(can.value)


def peer_access_matrix():
    """[d][p] = device d can address device p's memory (hipDeviceCanAccessPeer), over every visible device."""
    n = device_count()
    return [[device_can_access_peer(d, p) for p in range(n)] for d in range(n)]


class Context:
    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self.lib = abi.load()
        h = C.c_void_p()
        check(self.lib.bamm_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(h)))
        self.h = h
        self.device = device

    def sync(self):
        check(self.lib.bamm_ctx_sync(self.h))

    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        check(self.lib.bamm_ctx_device_name(self.h, buf, 256))
        return buf.value.decode()

    def set_launch(self, blocks: int = 0, threads: int = 0):
        check(self.lib.bamm_ctx_set_launch(self.h, blocks, threads))

    def set_tuning(self, **kv):
        """Kernel-selection switches for EM handles created afterwards (include/bamm_em.h:
        grouped, group_size, group_layout, sparse, e_fused)."""
        for k, v in kv.items():
            check(self.lib.bamm_ctx_set_tuning(self.h, k.encode(), int(v)))

    def close(self):
        if self.h:
            self.lib.bamm_ctx_destroy(self.h)
            self.h = None


COMM_ID_BYTES = 128


class Comm:
    """One rank of an RCCL communicator bound to a Context (include/bamm_em.h: bamm_comm_*)."""

    def __init__(self, ctx: Context, handle):
        self.ctx, self.lib, self.h = ctx, ctx.lib, handle

    @classmethod
    def init_all(cls, ctxs):
        """One process driving len(ctxs) distinct devices: ncclCommInitAll."""
        lib = ctxs[0].lib
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        out = (C.c_void_p * len(ctxs))()
        check(lib.bamm_comm_init_all(arr, len(ctxs), out))
        return [cls(c, C.c_void_p(h)) for c, h in zip(ctxs, out)]

    @classmethod
    def init_local(cls, ctxs, max_words: int):
        """One process, len(ctxs) contexts on any devices (even one): host-staged sum, no RCCL (self-tests)."""
        lib = ctxs[0].lib
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        out = (C.c_void_p * len(ctxs))()
        check(lib.bamm_comm_init_local(arr, len(ctxs), max_words, out))
        return [cls(c, C.c_void_p(h)) for c, h in zip(ctxs, out)]

    @classmethod
    def init_shm(cls, ctx: Context, name: str, rank: int, world: int, max_words: int):
        """One PROCESS per rank on one host, the sum staged through the POSIX shared-memory segment `name` ("/..."): no RCCL
        (self-tests of the cross-process paths on a 1-GPU box)."""
        h = C.c_void_p()
        check(ctx.lib.bamm_comm_init_shm(ctx.h, name.encode(), rank, world, max_words, C.byref(h)))
        return cls(ctx, h)

    def abort(self):
        """Wake the peers blocked in a collective with this rank (they get BAMM_ERR_COMM)."""
        if self.h:
            self.lib.bamm_comm_abort(self.h)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        check(abi.load().bamm_comm_unique_id(buf, COMM_ID_BYTES))
        return buf.raw

    @classmethod
    def init_rank(cls, ctx: Context, uid: bytes, rank: int, world: int):
        """One process per device: `uid` from rank 0's unique_id(), carried by the launcher."""
        assert len(uid) == COMM_ID_BYTES
        h = C.c_void_p()
        check(ctx.lib.bamm_comm_init_rank(ctx.h, C.c_char_p(uid), rank, world, C.byref(h)))
        return cls(ctx, h)

    def info(self):
        r, w, v = C.c_uint32(), C.c_uint32(), C.c_int()
        check(self.lib.bamm_comm_info(self.h, C.byref(r), C.byref(w), C.byref(v)))
        return dict(rank=r.value, world=w.value, rccl_version=v.value)

    def time_allreduce(self, n_words: int, iters: int = 200) -> float:
        """Microseconds per bare all-reduce of n_words int64 words (collective: every rank calls it)."""
        us = C.c_float()
        check(self.lib.bamm_comm_time_allreduce(self.h, n_words, iters, C.byref(us)))
        return float(us.value)

    def close(self):
        if self.h:
            self.lib.bamm_comm_destroy(self.h)
            self.h = None


class SeqSet:
    """Sequences resident in HBM (a shard [begin, end) of a PackedSeqs)."""

    def __init__(self, ctx: Context, packed: PackedSeqs, begin: int = 0, end: Optional[int] = None):
        self.ctx, self.lib = ctx, ctx.lib
        end = packed.n_seqs if end is None else end
        h = C.c_void_p()
        check(self.lib.bamm_seqs_upload(ctx.h, packed._p, begin, end, C.byref(h)))
        self.h = h
        self.n_seqs = end - begin
        self.lengths = packed.lengths[begin:end]
        self.off = np.concatenate([[0], np.cumsum(self.lengths.astype(np.int64))]).astype(np.uint64)

    @classmethod
    def from_codes(cls, ctx: "Context", codes, off, single_strand: bool = False, seed: int = 42, resident: bool = True):
        """Sequence::Sequence on the device (include/bamm_em.h: bamm_seqs_from_codes): returns (PackedSeqs, SeqSet) -- the
        packed set bamm_pack_codes_seeded would have built on the host, and the resident set (None with resident=False)."""
        off = _u64(off)
        pk, h = C.POINTER(abi.Packed)(), C.c_void_p()
        check(ctx.lib.bamm_seqs_from_codes(ctx.h, np.ascontiguousarray(codes, np.uint8), off, len(off) - 1, int(single_strand), seed,
                                           C.byref(pk), C.byref(h) if resident else None))
        packed = PackedSeqs(pk)
        if not resident:
            return packed, None
        self = cls.__new__(cls)
        self.ctx, self.lib, self.h = ctx, ctx.lib, h
        self.n_seqs = packed.n_seqs
        self.lengths = packed.lengths
        self.off = np.concatenate([[0], np.cumsum(self.lengths.astype(np.int64))]).astype(np.uint64)
        return packed, self

    def bg_model(self, K: int, alpha) -> np.ndarray:
        """BackgroundModel learned from the resident set, its counting pass on the device (bamm_seqs_bg_model)."""
        out = np.zeros(bg_size(K), np.float32)
        alpha = _f32(alpha)
        assert len(alpha) >= K + 1
        check(self.lib.bamm_seqs_bg_model(self.ctx.h, self.h, K, alpha, out))
        return out

    def info(self):
        n, t, m, b = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
        check(self.lib.bamm_seqs_info(self.h, C.byref(n), C.byref(t), C.byref(m), C.byref(b)))
        return dict(n_seqs=n.value, total_len=t.value, max_len=m.value, hbm_bytes=b.value)

    def close(self):
        if self.h:
            self.lib.bamm_seqs_destroy(self.h)
            self.h = None


class EM:
    """Drop-in for the reference's `EM` (EM.h:11-69) on one GPU shard."""

    def __init__(self, ctx: Context, seqs: SeqSet, K: int, W: int, vbg, A, v_init, q: float,
                 bg_order: int = 2, optimizeQ: bool = False, mask=None, epsilon: float = 0.01,
                 max_iterations: int = 1000, n_seqs_global: int = 0, n_seqs_bound: int = 0):
        self.ctx, self.lib, self.seqs = ctx, ctx.lib, seqs
        self.K, self.W = K, W
        prm = abi.EmParams()
        self.lib.bamm_em_default_params(C.byref(prm))
        prm.K, prm.W, prm.bg_order, prm.q = K, W, bg_order, q
        prm.optimize_q = int(optimizeQ)
        prm.epsilon, prm.max_iterations, prm.n_seqs_global = epsilon, max_iterations, n_seqs_global
        prm.n_seqs_bound = n_seqs_bound
        self.max_iterations = max_iterations
        vbg, A, v_init = _f32(vbg), _f32(A), _f32(v_init)
        assert len(vbg) >= bg_size(bg_order) and len(A) == (K + 1) * W and len(v_init) == v_size(K, W)
        mptr = None
        if mask is not None:
            self._mask = np.ascontiguousarray(mask, np.uint8)
            assert len(self._mask) == seqs.n_seqs
            mptr = self._mask.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        check(self.lib.bamm_em_create(ctx.h, seqs.h, C.byref(prm), vbg, A, v_init, mptr, C.byref(h)))
        self.h = h
        self._cb = None

    # -- the reference's public surface ---------------------------------------------------
    def EStep(self):
        check(self.lib.bamm_em_estep(self.h))

    def MStep(self):
        check(self.lib.bamm_em_mstep(self.h))

    def optimize_q(self):
        check(self.lib.bamm_em_optimize_q(self.h))

    def optimize(self) -> int:
        it = C.c_uint32()
        check(self.lib.bamm_em_optimize(self.h, C.byref(it)))
        return int(it.value)

    def mask(self, f: float = 0.05) -> int:
        """EM::mask (EM.cpp:261-503, --advanceEM); the cut-off and list size land in last_mask."""
        it, cut, listed = C.c_uint32(), C.c_float(), C.c_uint64()
        check(self.lib.bamm_em_mask(self.h, f, C.byref(it), C.byref(cut), C.byref(listed)))
        self.last_mask = dict(cutoff=float(cut.value), listed=int(listed.value))
        return int(it.value)

    def getQ(self) -> float:
        q = C.c_float()
        check(self.lib.bamm_em_get_q(self.h, C.byref(q)))
        return float(q.value)

    def getR(self, begin: int = 0, end: Optional[int] = None) -> np.ndarray:
        end = self.seqs.n_seqs if end is None else end
        total = int(self.seqs.off[end] - self.seqs.off[begin])
        out = np.zeros(max(total, 1), np.float32)
        check(self.lib.bamm_em_get_r(self.h, begin, end, out, total))
        return out[:total]

    def sites_and_best(self, cutoff: float = 0.3, begin: int = 0, end: Optional[int] = None):
        """One bamm_em_sites call over sequences [begin, end): ((seq, pos, r), (z, r_best, count)) -- what sites() and
        best_sites() return, for a caller who wants both."""
        end = self.seqs.n_seqs if end is None else end
        h = C.c_void_p()
        check(self.lib.bamm_em_sites(self.h, begin, end, cutoff, C.byref(h)))
        try:
            n_sites, n_seqs = C.c_uint64(), C.c_uint64()
            check(self.lib.bamm_sites_info(h, C.byref(n_sites), C.byref(n_seqs)))
            seq, pos, r = np.zeros(n_sites.value, np.uint64), np.zeros(n_sites.value, np.uint32), np.zeros(n_sites.value, np.float32)
            z, r_best, count = np.zeros(n_seqs.value, np.uint32), np.zeros(n_seqs.value, np.float32), np.zeros(n_seqs.value, np.uint32)
            check(self.lib.bamm_sites_get(h, *(a.ctypes.data_as(C.c_void_p) for a in (seq, pos, r)), n_sites.value))
            check(self.lib.bamm_sites_best(h, *(a.ctypes.data_as(C.c_void_p) for a in (z, r_best, count)), n_seqs.value))
        finally:
            self.lib.bamm_sites_destroy(h)
        return (seq, pos, r), (z, r_best, count)

    def sites(self, cutoff: float = 0.3, begin: int = 0, end: Optional[int] = None):
        """The windows of sequences [begin, end) with r >= cutoff -- r as getR() would report it now -- found on the device
        (bamm_em_sites): `seq` (uint64, index in the handle's set), `pos` (uint32, window start, 0-based), `r` (float32), in
        ascending (seq, pos) order.  cutoff = 0.3 gives the rows of EM::write's .positions (EM.cpp:577-601)."""
        return self.sites_and_best(cutoff, begin, end)[0]

    def best_sites(self, begin: int = 0, end: Optional[int] = None):
        """Per sequence of [begin, end): `z` (0 = no window with r > 0, else the first arg-max window + 1, as
        GibbsSampling.cpp:105-116 initialises it), `r_best` (its r) and `count` (windows with r >= 0.3)."""
        return self.sites_and_best(0.3, begin, end)[1]

    # -- extensions -------------------------------------------------------------------------
    def iterate(self, n: int = 1):
        check(self.lib.bamm_em_iterate(self.h, n))

    def accumulate(self):
        check(self.lib.bamm_em_accumulate(self.h))

    def update(self):
        check(self.lib.bamm_em_update(self.h))

    def reduce_buffer(self):
        p, n = C.c_void_p(), C.c_uint64()
        check(self.lib.bamm_em_reduce_buffer(self.h, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def set_reduce_buffer(self, dev_ptr: int, n_words: int):
        """Use caller-owned device memory (e.g. a torch int64 tensor) as the fused accumulator."""
        check(self.lib.bamm_em_set_reduce_buffer(self.h, C.c_void_p(dev_ptr), n_words))

    def set_allreduce(self, fn: Optional[Callable[[int, int, int], int]]):
        """fn(dev_ptr, n_words, hip_stream) -> 0 on success: sum n_words int64 words across ranks;
        called between the local accumulation and the model update of every pass."""
        if fn is None:
            self._cb = abi.ALLREDUCE_FN(0)
        else:
            def tramp(_user, ptr, n, stream):
                try:
                    return int(fn(int(ptr or 0), int(n), int(stream or 0)) or 0)
                except Exception:  # never unwind through C
                    import traceback
                    traceback.print_exc()
                    return 1
            self._cb = abi.ALLREDUCE_FN(tramp)
        check(self.lib.bamm_em_set_allreduce(self.h, self._cb, None))

    def set_comm(self, comm: Optional["Comm"]):
        """Native path: one ncclAllReduce(int64, sum) of the accumulator per pass, on the context's stream."""
        check(self.lib.bamm_em_set_comm(self.h, comm.h if comm is not None else None))
        self._comm = comm

    def comm_mode(self):
        """(mode, note): 0 = no reduction over ranks, 1 = one collective per pass, 2 = inside the sequence kernels over
        peer-mapped inboxes (Context.set_tuning(peer_allreduce=1) on every rank); collective on first use."""
        m = C.c_int()
        buf = C.create_string_buffer(512)
        check(self.lib.bamm_em_comm_mode(self.h, C.byref(m), buf, 512))
        return int(m.value), buf.value.decode()

    def getV(self) -> np.ndarray:
        out = np.zeros(v_size(self.K, self.W), np.float32)
        check(self.lib.bamm_em_get_v(self.h, out))
        return out

    def getCounts(self) -> np.ndarray:
        out = np.zeros(v_size(self.K, self.W), np.float32)
        check(self.lib.bamm_em_get_counts(self.h, out))
        return out

    def getS(self) -> np.ndarray:
        out = np.zeros(4 ** (self.K + 1) * self.W, np.float32)
        check(self.lib.bamm_em_get_s(self.h, out))
        return out

    def getLLH(self) -> float:
        x = C.c_float()
        check(self.lib.bamm_em_get_llh(self.h, C.byref(x)))
        return float(x.value)

    def getVdiff(self) -> float:
        x = C.c_float()
        check(self.lib.bamm_em_get_vdiff(self.h, C.byref(x)))
        return float(x.value)

    def iteration(self) -> int:
        x = C.c_uint32()
        check(self.lib.bamm_em_get_iteration(self.h, C.byref(x)))
        return int(x.value)

    def trace(self):
        cap = self.max_iterations
        llh, vd, q = (np.zeros(cap, np.float32) for _ in range(3))
        n = C.c_uint32()
        check(self.lib.bamm_em_get_trace(self.h, llh, vd, q, cap, C.byref(n)))
        m = min(int(n.value), cap)
        return llh[:m].copy(), vd[:m].copy(), q[:m].copy()

    TIMING_WHOLE_CALL = 0xFFFFFFFF                           # BAMM_TIMING_WHOLE_CALL

    def set_kernel_timing(self, every: int):
        """Time passes 0, every, 2*every, ... of each call with a pair of HIP events each (0 = none, 1 = all; a pair costs
        7-8 us of stream time); -1 / TIMING_WHOLE_CALL: one pair around all passes of a call (gaps included, no cost per pass)."""
        check(self.lib.bamm_em_set_kernel_timing(self.h, self.TIMING_WHOLE_CALL if every < 0 else every))

    def kernel_time(self):
        ms, n = C.c_float(), C.c_uint32()
        check(self.lib.bamm_em_kernel_time(self.h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def plan(self):
        """(sequences through the grouped-column kernel, through the per-column kernel, launches per pass)."""
        g, o, n = C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(self.lib.bamm_em_plan(self.h, C.byref(g), C.byref(o), C.byref(n)))
        return int(g.value), int(o.value), int(n.value)

    def plan_mixed(self) -> int:
        """Sequences (of the grouped ones) that go through the mixed-row kernel (csrc/mixed_kernel.h)."""
        m = C.c_uint64()
        check(self.lib.bamm_em_plan_mixed(self.h, C.byref(m)))
        return int(m.value)

    def plan_launches(self):
        """The launches of one pass, in order: dicts of `count` (sequences), `positions_per_lane` of the class the launch runs
        in (0: beyond the classes), `mixed` (the mixed-row kernel) and `anchored` (its start-anchored flavour)."""
        out = []
        for i in range(self.plan()[2]):
            v = (C.c_uint64 * 4)()
            check(self.lib.bamm_em_plan_launch(self.h, i, v))
            out.append(dict(count=int(v[0]), positions_per_lane=int(v[1]), mixed=bool(v[2]), anchored=bool(v[3])))
        return out

    def plan_paths(self):
        """(sliced, e_fused, long_seqs): the pass runs column slices; its E pass still holds the whole odds table; sequences
        that go window by window (include/bamm_em.h: bamm_em_plan_paths)."""
        sl, ef, ln = C.c_int(), C.c_int(), C.c_uint64()
        check(self.lib.bamm_em_plan_paths(self.h, C.byref(sl), C.byref(ef), C.byref(ln)))
        return bool(sl.value), bool(ef.value), int(ln.value)

    def plan_update(self):
        """(form, fusable): the form of the handle's update launches -- 0 one block with the tables in LDS, 1 one block on
        global memory, 2 spread over blocks -- and whether iterate() / optimize() run the update of a pass in the
        prologue of the next pass's first kernel (include/bamm_em.h: bamm_em_plan_update)."""
        form, fus = C.c_int(-1), C.c_int(-1)
        check(self.lib.bamm_em_plan_update(self.h, C.byref(form), C.byref(fus)))
        return int(form.value), bool(fus.value)

    def tile_plan(self) -> dict:
        """Of plan_paths()' long_seqs: `tiled_seqs` go tile by tile (csrc/em_tiles.hip) in `tiles` tiles, `window_seqs`
        window by window (bamm_em_tile_plan); decided at creation from the context's `em_tiles` tuning and the model's shape."""
        out = [C.c_uint64() for _ in range(3)]
        check(self.lib.bamm_em_tile_plan(self.h, *(C.byref(x) for x in out)))
        return dict(zip(("tiled_seqs", "tiles", "window_seqs"), (x.value for x in out)))

    def close(self):
        if self.h:
            self.lib.bamm_em_destroy(self.h)
            self.h = None


def sample_negatives(ctx: Context, positives: SeqSet, s_order: int = 2, m_fold: int = 1, generic: bool = False,
                     keep_stride: int = 0, resident: bool = True):
    """SeqGenerator's negative sampler on the device (include/bamm_em.h: bamm_sample_negatives): (PackedSeqs, SeqSet or
    None) -- m_fold negatives per resident positive, the reference's own, base for base."""
    pk, h = C.POINTER(abi.Packed)(), C.c_void_p()
    check(ctx.lib.bamm_sample_negatives(ctx.h, positives.h, s_order, m_fold, int(generic), keep_stride, C.byref(pk),
                                        C.byref(h) if resident else None))
    packed = PackedSeqs(pk)
    if not resident:
        return packed, None
    neg = SeqSet.__new__(SeqSet)
    neg.ctx, neg.lib, neg.h = ctx, ctx.lib, h
    neg.n_seqs = packed.n_seqs
    neg.lengths = packed.lengths
    neg.off = np.concatenate([[0], np.cumsum(neg.lengths.astype(np.int64))]).astype(np.uint64)
    return packed, neg


def kmer_counts(ctx: Context, seqs: SeqSet, w: int):
    """The exact w-mer table of a resident set built from codes, w = 6..8 (bamm_kmer_counts): (counts uint64 [4^w], their
    sum).  A w-mer's cell is its bases as a base-4 number, oldest base most significant."""
    counts = np.zeros(4 ** max(int(w), 0) if 0 <= int(w) <= 8 else 1, np.uint64)
    total = C.c_uint64(0)
    check(ctx.lib.bamm_kmer_counts(ctx.h, seqs.h, int(w), counts, C.byref(total)))
    return counts, int(total.value)


def kmer_counts_host(codes, off, w: int, single_strand: bool = False):
    """The same table from the FASTA codes, on the host threads (bamm_kmer_counts_host)."""
    off = _u64(off)
    counts = np.zeros(4 ** max(int(w), 0) if 0 <= int(w) <= 8 else 1, np.uint64)
    total = C.c_uint64(0)
    check(abi.load().bamm_kmer_counts_host(np.ascontiguousarray(codes, np.uint8), off, len(off) - 1, int(single_strand), int(w),
                                           counts, C.byref(total)))
    return counts, int(total.value)


_host_lib = None


def _host():
    """libbamm_host.so: the C++ host code behind the BaMMmotif driver (its seeder is what kmer_seeds calls)."""
    global _host_lib
    if _host_lib is None:
        from . import build
        build.build_host()                                    # (a no-op when the library is up to date)
        H = C.CDLL(build.HOST_LIB)
        H.bh_last_error.restype = C.c_char_p
        _host_lib = H
    return _host_lib


def kmer_seeds(counts, n_windows: int, vbg, Kbg: int, w: int, max_seeds: int = 4, single_strand: bool = False):
    """The seeds the BaMMmotif driver takes from a w-mer table under --seedKmers (host/seeder.cpp): (w-mers uint32 [n],
    z-scores float64 [n], PWMs float32 [n][4][w]) in rank order; vbg: the background model of order Kbg, flat [k][y]."""
    H = _host()
    counts, vbg = _u64(counts), _f32(vbg)
    assert len(counts) == 4 ** w and len(vbg) >= bg_size(Kbg)
    cap = max(int(max_seeds), 1)
    n = C.c_uint32(0)
    kmer, cnt, z = np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.float64)
    pwm = np.zeros((cap, 4, w), np.float32)
    if H.bh_kmer_seeds(counts.ctypes.data_as(C.c_void_p), C.c_uint64(int(n_windows)), C.c_uint32(w), C.c_uint32(Kbg),
                       vbg.ctypes.data_as(C.c_void_p), C.c_uint64(int(max_seeds)), C.c_int(int(single_strand)), C.byref(n),
                       kmer.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p),
                       pwm.ctypes.data_as(C.c_void_p)):
        raise RuntimeError(H.bh_last_error().decode(errors="replace"))
    return kmer[: n.value].copy(), z[: n.value].copy(), pwm[: n.value].copy()


def _gapped_tables(w: int, gap_lo: int, gap_hi: int):
    """Zeroed (counts [n_gaps, 4^w], n_windows [n_gaps]) for a range the library accepts; a 1 x 1 table for one it will refuse."""
    ok = 6 <= int(w) <= 8 and 0 <= int(gap_lo) <= int(gap_hi) <= 16 - int(w)
    n_gaps = int(gap_hi) - int(gap_lo) + 1 if ok else 1
    return np.zeros((n_gaps, 4 ** int(w) if ok else 1), np.uint64), np.zeros(n_gaps, np.uint64)


def kmer_counts_gapped(ctx: Context, seqs: SeqSet, w: int, gap_lo: int, gap_hi: int):
    """The dyad tables of a resident set built from codes (bamm_kmer_counts_gapped), w = 6 or 8, gaps gap_lo..gap_hi with
    w + gap_hi <= 16, in one launch: (counts uint64 [n_gaps, 4^w], n_windows uint64 [n_gaps]).  A cell is the window's first
    and last w / 2 bases as one base-4 number, oldest base most significant; gap 0 is kmer_counts' table."""
    counts, totals = _gapped_tables(w, gap_lo, gap_hi)
    check(ctx.lib.bamm_kmer_counts_gapped(ctx.h, seqs.h, int(w) & 0xffffffff, int(gap_lo) & 0xffffffff, int(gap_hi) & 0xffffffff, counts.reshape(-1), totals))
    return counts, totals


def kmer_counts_gapped_host(codes, off, w: int, gap_lo: int, gap_hi: int, single_strand: bool = False):
    """The same tables from the FASTA codes, on the host threads (bamm_kmer_counts_gapped_host)."""
    off = _u64(off)
    counts, totals = _gapped_tables(w, gap_lo, gap_hi)
    check(abi.load().bamm_kmer_counts_gapped_host(np.ascontiguousarray(codes, np.uint8), off, len(off) - 1, int(single_strand), int(w) & 0xffffffff,
                                                  int(gap_lo) & 0xffffffff, int(gap_hi) & 0xffffffff, counts.reshape(-1), totals))
    return counts, totals


def kmer_seeds_gapped(counts, n_windows, vbg, Kbg: int, w: int, gap_lo: int, gap_hi: int, max_seeds: int = 4, single_strand: bool = False):
    """The seeds the BaMMmotif driver takes from the dyad tables of gaps gap_lo..gap_hi under --seedKmers --seedGaps
    (host/seeder.cpp, kmer_seeds_gapped): (w-mers uint32 [n], gaps uint32 [n], z-scores float64 [n], a list of n PWMs
    float32 [4][w + gap]) in rank order."""
    H = _host()
    counts, totals, vbg = _u64(counts).reshape(-1), _u64(n_windows).reshape(-1), _f32(vbg)
    n_gaps = gap_hi - gap_lo + 1
    assert len(counts) == n_gaps * 4 ** w and len(totals) == n_gaps and len(vbg) >= bg_size(Kbg)
    cap = max(int(max_seeds), 1)
    n = C.c_uint32(0)
    kmer, gap, cnt, z = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64), np.zeros(cap, np.float64)
    pwm = np.zeros((cap, 4 * (w + gap_hi)), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if H.bh_kmer_seeds_gapped(vp(counts), vp(totals), C.c_uint32(w), C.c_uint32(gap_lo), C.c_uint32(gap_hi), C.c_uint32(Kbg), vp(vbg),
                              C.c_uint64(int(max_seeds)), C.c_int(int(single_strand)), C.byref(n), vp(kmer), vp(gap), vp(cnt), vp(z), vp(pwm)):
        raise RuntimeError(H.bh_last_error().decode(errors="replace"))
    k = n.value
    return (kmer[:k].copy(), gap[:k].copy(), z[:k].copy(),
            [pwm[i, : 4 * (w + int(gap[i]))].reshape(4, w + int(gap[i])).copy() for i in range(k)])


def seed_from_pwm(ctx: Context, seqs: SeqSet, K: int, W: int, score, q: float, u):
    """The pass over the sequences of Motif::initFromPWM (Motif.cpp:228-311) on the device: returns
    (counts[v_size(K,W)] int32, z[n_seqs] uint32).  score: [4][W] floored PWM / 0th-order background;
    u[n]: the uniform variate of sequence n's draw (see include/bamm_em.h)."""
    score = _f32(score)
    u = np.ascontiguousarray(u, np.float64)
    assert len(score) == 4 * W and len(u) == seqs.n_seqs
    counts = np.zeros(v_size(K, W), np.int32)
    z = np.zeros(seqs.n_seqs, np.uint32)
    check(ctx.lib.bamm_seed_from_pwm(ctx.h, seqs.h, K, W, score, q, u.ctypes.data_as(C.c_void_p),
                                     counts.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)))
    return counts, z


def logodds(ctx: Context, seqs: SeqSet, K: int, W: int, bg_order: int, v, vbg, want_mops: bool = True, mask=None):
    """ScoreSeqSet::calcLogOdds (ScoreSeqSet.cpp:25-67): returns (mops or None, zoops, z).

    mask: optional per-sequence bytes; sequences with 0 are skipped and report zeros."""
    lib = ctx.lib
    N = seqs.n_seqs
    total = int((seqs.lengths.astype(np.int64) - W + 1).sum()) if N else 0
    mops = np.zeros(max(total, 1), np.float32) if want_mops else None
    zoops = np.zeros(max(N, 1), np.float32)
    z = np.zeros(max(N, 1), np.uint64)
    mptr = mops.ctypes.data_as(C.c_void_p) if want_mops else None
    if mask is None:
        check(lib.bamm_logodds(ctx.h, seqs.h, K, W, bg_order, _f32(v), _f32(vbg), mptr, total, zoops, z))
    else:
        mk = np.ascontiguousarray(mask, np.uint8)
        assert len(mk) == N
        check(lib.bamm_logodds_subset(ctx.h, seqs.h, mk.ctypes.data_as(C.c_void_p), K, W, bg_order, _f32(v), _f32(vbg),
                                      mptr, total, zoops, z))
    return (mops[:total] if want_mops else None), zoops[:N], z[:N]


def score_tile_geometry(W: int):
    """(tile_positions, stride) of the tiles the scorer cuts a sequence beyond 8192 positions into for motifs of width W
    (bamm_score_tile_geometry: a pure function, no device needed); BammError for a W that leaves no stride."""
    tp, stride = C.c_uint32(), C.c_uint32()
    check(abi.load().bamm_score_tile_geometry(W, C.byref(tp), C.byref(stride)))
    return tp.value, stride.value


def score_slice_geometry(K: int, W: int):
    """(columns_per_slice, slices) of the slices of motif columns the scorer takes a log-odds table of order K and width W in
    under set_tuning(score_slices=1) (bamm_score_slice_geometry: a pure function, no device needed; slices == 1: the table
    fits one CU's LDS whole); BammError where not even one column fits."""
    cps, slices = C.c_uint32(), C.c_uint32()
    check(abi.load().bamm_score_slice_geometry(K, W, C.byref(cps), C.byref(slices)))
    return cps.value, slices.value


def em_tile_geometry(W: int):
    """(tile_positions, stride) of the tiles an EM pass cuts a sequence beyond 8192 positions into for motifs of width W
    (bamm_em_tile_geometry: a pure function, no device needed); BammError for a W that leaves no stride."""
    tp, stride = C.c_uint32(), C.c_uint32()
    check(abi.load().bamm_em_tile_geometry(W, C.byref(tp), C.byref(stride)))
    return tp.value, stride.value


def neg_segment_geometry() -> int:
    """Positions per segment of a negative beyond 8192 positions in sample_negatives (bamm_neg_segment_geometry: a pure
    function, no device needed); a multiple of 16."""
    s = C.c_uint32()
    check(abi.load().bamm_neg_segment_geometry(C.byref(s)))
    return s.value


def score_plan(ctx: Context, seqs: SeqSet, K: int, W: int) -> dict:
    """Which scorer the sequences of `seqs` take under the context's tuning (bamm_score_plan): `wave_seqs` in one wavefront's
    registers, `tiled_seqs` cut into `tiles` tiles, `window_seqs` window by window."""
    out = [C.c_uint64() for _ in range(4)]
    check(ctx.lib.bamm_score_plan(ctx.h, seqs.h, K, W, *(C.byref(x) for x in out)))
    return dict(zip(("wave_seqs", "tiled_seqs", "tiles", "window_seqs"), (x.value for x in out)))


class Occurrences:
    """What bamm_occurrences returns: per hit `seq`, `pos` (window start, 0-based), `score`, `fp`, `p`, `e`, and the scalars
    of ScoreSeqSet::calcPvalues (`n_neg_scores`, `n_top`, `s_ntop`, `lambda_`) with the number of windows the device handed
    to the host (`n_candidates`)."""

    def __init__(self, seq, pos, score, fp, p, e, n_neg_scores, n_top, s_ntop, lambda_, n_candidates):
        self.seq, self.pos, self.score, self.fp, self.p, self.e = seq, pos, score, fp, p, e
        self.n_neg_scores, self.n_top, self.s_ntop, self.lambda_, self.n_candidates = n_neg_scores, n_top, s_ntop, lambda_, n_candidates

    @property
    def n_hits(self) -> int:
        return len(self.p)


def occurrences(ctx: Context, positives: SeqSet, negatives: SeqSet, K: int, W: int, bg_order: int, v, vbg,
                p_cutoff: float) -> Occurrences:
    """ScoreSeqSet::calcPvalues + the cut of ScoreSeqSet::write (ScoreSeqSet.cpp:70-126, :245-291) on the device: the windows
    of `positives` with a p-value below `p_cutoff` against the scores of `negatives` (include/bamm_em.h: bamm_occurrences)."""
    lib = ctx.lib
    h = C.c_void_p()
    check(lib.bamm_occurrences(ctx.h, positives.h, negatives.h, K, W, bg_order, _f32(v), _f32(vbg), p_cutoff, C.byref(h)))
    try:
        n_hits, n_neg, n_cand, n_top = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        s_ntop, lam = C.c_float(), C.c_float()
        check(lib.bamm_occ_info(h, C.byref(n_hits), C.byref(n_neg), C.byref(n_top), C.byref(s_ntop), C.byref(lam), C.byref(n_cand)))
        n = n_hits.value
        seq, fp = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        pos = np.zeros(n, np.uint32)
        score, p, e = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        check(lib.bamm_occ_get(h, *(a.ctypes.data_as(C.c_void_p) for a in (seq, pos, score, fp, p, e)), n))
    finally:
        lib.bamm_occ_destroy(h)
    return Occurrences(seq, pos, score, fp, p, e, n_neg.value, n_top.value, np.float32(s_ntop.value), np.float32(lam.value), n_cand.value)


def fdr_geometry():
    """(steps per thread, steps per block) of the ranking walk's kernels in this build (csrc/fdr.hip)."""
    spt, spb = C.c_uint32(), C.c_uint32()
    check(abi.load().bamm_fdr_geometry(C.byref(spt), C.byref(spb)))
    return spt.value, spb.value


class FdrMops:
    """FDR::calculatePR's MOPS branch and FDR::calculatePvalues over window scores kept on the device
    (include/bamm_em.h: bamm_fdr).  Add the folds' scores, call statistics() once, then fetch rows / p-values by range.  Folds
    scored on several contexts: a handle each, seal() them there, absorb() them into the one that runs statistics()."""

    def __init__(self, ctx: Context):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        check(self.lib.bamm_fdr_create(ctx.h, C.byref(self.h)))

    def add_set(self, negative: bool, seqs: SeqSet, K: int, W: int, bg_order: int, v, vbg, mask=None):
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(mask, np.uint8)
            assert len(mk) == seqs.n_seqs
        check(self.lib.bamm_fdr_add_set(self.h, 1 if negative else 0, seqs.h, None if mk is None else mk.ctypes.data_as(C.c_void_p),
                                        K, W, bg_order, _f32(v), _f32(vbg)))

    def add_scores(self, negative: bool, scores):
        a = np.ascontiguousarray(scores, np.float32)
        check(self.lib.bamm_fdr_add_scores(self.h, 1 if negative else 0, a.ctypes.data_as(C.c_void_p), a.size))

    def seal(self):
        """Sorts both lists where they lie into one ascending run each; no more scores afterwards."""
        check(self.lib.bamm_fdr_seal(self.h))

    def absorb(self, other: "FdrMops"):
        """Moves everything `other` holds (of any context) into this handle; `other` can only be closed afterwards."""
        check(self.lib.bamm_fdr_absorb(self.h, other.h))

    def statistics(self, posN: int, negN: int, with_pvalues: bool = True):
        check(self.lib.bamm_fdr_statistics(self.h, posN, negN, 1 if with_pvalues else 0))

    def info(self) -> dict:
        n_pos, n_neg, n_rows, e_tp, occ = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float(), C.c_float()
        check(self.lib.bamm_fdr_info(self.h, C.byref(n_pos), C.byref(n_neg), C.byref(n_rows), C.byref(e_tp), C.byref(occ)))
        return dict(n_pos=n_pos.value, n_neg=n_neg.value, n_rows=n_rows.value, e_tp=np.float32(e_tp.value), occ_mult=np.float32(occ.value))

    def rows(self, begin: int = 0, end: Optional[int] = None, columns=("tp", "fp", "fdr", "rec")) -> dict:
        """The named columns of rows [begin, end) (end None: n_rows)."""
        if end is None:
            end = self.info()["n_rows"]
        out = {k: np.zeros(max(end - begin, 0), np.float32) for k in columns}
        ptrs = [out[k].ctypes.data_as(C.c_void_p) if k in out else None for k in ("tp", "fp", "fdr", "rec")]
        check(self.lib.bamm_fdr_rows(self.h, begin, end, *ptrs))
        return out

    def pvalues(self, begin: int = 0, end: Optional[int] = None) -> np.ndarray:
        if end is None:
            end = self.info()["n_pos"]
        p = np.zeros(max(end - begin, 0), np.float32)
        check(self.lib.bamm_fdr_pvalues(self.h, begin, end, p.ctypes.data_as(C.c_void_p)))
        return p

    def close(self):
        if self.h:
            self.lib.bamm_fdr_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def calculate_p(v, vbg, bg_order: int, K: int, W: int) -> np.ndarray:
    lib = abi.load()
    p = np.zeros(v_size(K, W), np.float32)
    check(lib.bamm_calculate_p(_f32(v), _f32(vbg), bg_order, K, W, p))
    return p
