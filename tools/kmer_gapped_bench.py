"""Times bamm_kmer_counts and bamm_kmer_counts_gapped on the benchmark's own set (the method of profiles/kmer_counts.txt and
profiles/kmer_gapped.txt): whole calls through the Python binding -- memset of the tables, ONE kernel launch, download, the
call synchronises itself -- 3 warm-up calls, then 7 batches of 10 calls under one wall-clock interval each; median / min / max
of the batch means.  The host twin with bamm_set_host_threads(16), median of 3 calls.

    python tools/kmer_gapped_bench.py [--nseq 1000000] [--len 200] [--no-host]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bammmotif2_amd as bm                                  # noqa: E402
from bammmotif2_amd import abi, em, synth                    # noqa: E402


def timed(fn, warmup=3, batches=7, calls=10):
    for _ in range(warmup):
        fn()
    means = []
    for _ in range(batches):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        means.append((time.perf_counter() - t0) / calls * 1e3)
    return float(np.median(means)), min(means), max(means)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=200)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    codes, off = synth.make_sequences(a.nseq, a.len, synth.make_pwm(20, 1234), 1234, plant_frac=0.5)
    ctx = bm.Context(0)
    packed = bm.PackedSeqs.from_codes(codes, off, False)
    seqs = bm.SeqSet(ctx, packed)
    positions = int(seqs.lengths.astype(np.int64).sum())
    print(f"set: {a.nseq} x {a.len} bp, both strands, {positions} positions, device {ctx.device_name()}")
    print("call                          gaps  ms per call: median (min .. max)    per gap    windows counted (first gap .. last gap)")
    rows = [("contiguous", w, None, None) for w in (6, 7, 8)]
    rows += [("gapped", 6, 0, 10), ("gapped", 8, 0, 8), ("gapped", 6, 4, 4), ("gapped", 8, 4, 4), ("gapped", 6, 0, 0), ("gapped", 8, 0, 0)]
    tables = {}
    for kind, w, lo, hi in rows:
        if kind == "contiguous":
            fn = lambda: em.kmer_counts(ctx, seqs, w)
            n_gaps, label = 1, f"bamm_kmer_counts w={w}"
        else:
            fn = lambda: em.kmer_counts_gapped(ctx, seqs, w, lo, hi)
            n_gaps, label = hi - lo + 1, f"bamm_kmer_counts_gapped w={w} {lo}..{hi}"
        med, mn, mx = timed(fn)
        counts, totals = fn()
        totals = np.atleast_1d(np.asarray(totals, np.uint64))
        tables[(kind, w, lo, hi)] = np.asarray(counts).reshape(n_gaps, -1)
        print(f"{label:38s} {n_gaps:3d}  {med:8.3f} ({mn:.3f} .. {mx:.3f})   {med / n_gaps:8.3f}   {int(totals[0])} .. {int(totals[-1])}", flush=True)
    for w, G in ((6, 10), (8, 8)):
        whole = tables[("gapped", w, 0, G)]
        assert np.array_equal(whole[0], tables[("contiguous", w, None, None)][0])
        assert np.array_equal(whole[4], tables[("gapped", w, 4, 4)][0]) and np.array_equal(whole[0], tables[("gapped", w, 0, 0)][0])
    print("gap 0 == the contiguous table, the single-gap calls == their slices of the all-gaps call (array_equal)")
    if not a.no_host:
        lib = abi.load()
        lib.bamm_set_host_threads(16)
        for w, lo, hi in ((6, 0, 10), (8, 0, 8), (6, 4, 4), (8, 4, 4)):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                host, _ = em.kmer_counts_gapped_host(codes, off, w, lo, hi)
                ts.append((time.perf_counter() - t0) * 1e3)
            same = np.array_equal(host, tables[("gapped", w, lo, hi)])
            print(f"host twin, 16 threads, w={w} gaps {lo}..{hi}: {np.median(ts):.1f} ms (first {ts[0]:.1f}); device table == host table: {same}", flush=True)
        lib.bamm_set_host_threads(0)
    seqs.close(); packed.free(); ctx.close()


if __name__ == "__main__":
    main()
