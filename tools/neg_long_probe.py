#!/usr/bin/env python3
"""The negative set of a positive set with records beyond 8192 positions, m = 10, sequence-specific: the device route
(bamm_sample_negatives: the segment kernels of csrc/negs.hip, the packed words brought back, then the upload of the resident
set -- what the driver's NegativeSet::body does by default) against the route the driver took before the segment kernels, and
takes with --hostSampler (the host sampler through its hook bh_sample_negatives_strided, which includes bamm_unpack_y of the
positives, then bamm_pack_codes and the upload).  One process, per shape three alternating pairs device / host, host clock
around each part (every part ends in a stream synchronise or is host work); the hook's copy of the codes into the caller's
array is not counted.  The two routes' packed words are compared in the first pair.  Then the device route alone at other
segment lengths ("neg_segment_positions"), one warm-up call and three timed ones each.

  python tools/neg_long_probe.py [--shapes a,b] [--out profiles/neg_long_ab.txt] [--segments 1024,2048,...]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"a": (16, 4 * 1024 * 1024), "b": (20000, 10001), "t": (6, 70001)}     # (records, positions each); t: a quick check
M_FOLD, PAIRS = 10, 3


def main(shapes, out_path, segments):
    import numpy as np
    import bammmotif2_amd as bm
    from bammmotif2_amd import abi, build
    host = C.CDLL(build.HOST_LIB)
    host.bh_last_error.restype = C.c_char_p
    ctx = bm.Context(0)
    lib = ctx.lib
    S0 = bm.neg_segment_geometry()
    lines = [f"negative set, -s 2, m = {M_FOLD}, sequence-specific, single-strand records, one N in 5000 bases; {ctx.device_name()}; seconds, host clock.",
             f"device = bamm_sample_negatives (segments of {S0} positions; sample + download of the packed words) + upload of the resident set;",
             "host = bh_sample_negatives_strided (bamm_unpack_y + host/fdr.cpp::sample_negatives) + bamm_pack_codes + upload;",
             f"{PAIRS} alternating pairs per shape, device first", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for name in shapes:
        n, L = SHAPES[name]
        rs = np.random.RandomState(1)
        codes = rs.randint(1, 5, size=n * L).astype(np.uint8)
        codes[rs.randint(0, len(codes), size=len(codes) // 5000)] = 0
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
        del codes
        pos = bm.SeqSet(ctx, packed)
        emit(f"shape ({name}): {n} records x {L} positions, {n * M_FOLD} negatives, {n * L * M_FOLD / 1e6:.0f} M bases")

        def device_route():
            t0 = time.perf_counter()
            neg, _ = bm.sample_negatives(ctx, pos, 2, M_FOLD, False, 0, resident=False)
            t1 = time.perf_counter()
            res = bm.SeqSet(ctx, neg)
            ctx.sync()
            t2 = time.perf_counter()
            res.close()
            return neg, (t1 - t0, t2 - t1)

        def host_route():
            nn, nc = C.c_uint64(), C.c_uint64()
            t0 = time.perf_counter()
            assert host.bh_sample_negatives_strided(packed._p, 2, C.c_uint64(M_FOLD), 0, C.c_uint64(0), C.byref(nn), C.byref(nc), None, None) == 0, host.bh_last_error()
            t1 = time.perf_counter()
            ncodes, noff = np.empty(nc.value, np.uint8), np.empty(nn.value + 1, np.uint64)
            assert host.bh_sample_negatives_strided(packed._p, 2, C.c_uint64(M_FOLD), 0, C.c_uint64(0), C.byref(nn), C.byref(nc),
                                                    ncodes.ctypes.data_as(C.c_void_p), noff.ctypes.data_as(C.c_void_p)) == 0
            t2 = time.perf_counter()
            neg = bm.PackedSeqs.from_codes(ncodes, noff, True, seed=None)
            t3 = time.perf_counter()
            res = bm.SeqSet(ctx, neg)
            ctx.sync()
            t4 = time.perf_counter()
            res.close()
            return neg, (t1 - t0, t3 - t2, t4 - t3)

        dev_tot, host_tot = [], []
        for pair in range(PAIRS):
            dneg, d = device_route()
            dwords = dneg.words.copy() if pair == 0 else None
            del dneg
            hneg, h = host_route()
            if pair == 0:
                same = np.array_equal(dwords, hneg.words)
                del dwords
            del hneg
            dev_tot.append(sum(d)); host_tot.append(sum(h))
            emit(f"  pair {pair}: device {sum(d):8.3f} (sample + download {d[0]:.3f}, upload {d[1]:.3f})   "
                 f"host {sum(h):8.3f} (unpack + sample {h[0]:.3f}, pack {h[1]:.3f}, upload {h[2]:.3f})")
        med = lambda x: sorted(x)[len(x) // 2]
        spread = max(host_tot) - min(host_tot)
        faster = med(host_tot) - med(dev_tot) > spread
        emit(f"  device median {med(dev_tot):.3f} (min {min(dev_tot):.3f}, max {max(dev_tot):.3f}); host median {med(host_tot):.3f} "
             f"(min {min(host_tot):.3f}, max {max(host_tot):.3f}, spread {spread:.3f}): {med(host_tot) / med(dev_tot):.1f}x -> "
             + ("the device route is faster by more than the host route's spread" if faster else "NOT faster by more than the host route's spread"))
        emit("  packed words: " + ("the same in both routes" if same else "DIFFERENT"))
        try:
            for seg in segments:
                ctx.set_tuning(neg_segment_positions=seg)
                times = []
                for it in range(4):
                    t0 = time.perf_counter()
                    neg, _ = bm.sample_negatives(ctx, pos, 2, M_FOLD, False, 0, resident=False)
                    if it:
                        times.append(time.perf_counter() - t0)
                    del neg
                emit(f"  segments of {seg:6d} positions: sample + download {med(times):.3f} (min {min(times):.3f}, max {max(times):.3f})")
        finally:
            ctx.set_tuning(neg_segment_positions=0)
        emit("")
        pos.close()
        del packed
        if not same:
            break
    ctx.close()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neg_long_ab.txt"))
    ap.add_argument("--segments", default="1024,2048,4096,8192,16384")
    a = ap.parse_args()
    main(a.shapes.split(","), a.out, [int(s) for s in a.segments.split(",") if s])
