#!/usr/bin/env python3
"""bamm_logodds with a log-odds table beyond one CU's LDS: the parent commit (every sequence window by window,
k_long_score) against this build with score_slices=1 (a slice of columns per launch through k_score / k_score_tile), per
call, zoops only and with mops -> profiles/score_slices_ab.txt.  The file decides where the BaMMmotif driver leaves the key
on: for a shape class only where the slices beat the parent by more than the parent's own spread.

  build --parent DIR   (where the compiler is) builds this tree and copies the parent commit's built package from the
                       worktree DIR to tools/.score_slices/parent/
  run [--out FILE] [--shapes a,b,...] [--variants parent,slices,off,parent]
                       (on the GPU) one fresh process per variant, the parent measured first and last with the others in
                       between; each process, per shape and per kind (zoops, mops): 2 warm-up calls and 7 timed ones (host
                       clock around the call, which ends in a stream synchronise and, with mops, includes their download)
                       and a SHA-1 of mops / zoops / z, which must be the same in every variant.  `off` = this build as
                       the library creates a context (score_slices=0)
  worker ...           one variant (what `run` starts)
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK = os.path.join(ROOT, "tools", ".score_slices")
BG = 2
# name: ([(records, bases per record), ...], both strands, K, W).  d, f, g: where a set becomes too small for several launches
# against one; h: the smallest set with one record beyond the length classes, which the parent gives to one workgroup
SHAPES = {"a": ([(200000, 200)], True, 5, 20), "b": ([(200000, 500)], True, 4, 40), "c": ([(50000, 200)], True, 6, 12),
          "d": ([(300, 205)], True, 5, 20), "f": ([(3000, 205)], True, 5, 20), "g": ([(30000, 205)], True, 5, 20),
          "h": ([(300, 205), (1, 20000)], True, 5, 20), "e": ([(16, 4 * 1024 * 1024)], False, 5, 20)}
KINDS = ("zoops", "mops")
WARMUP, REPEATS = 2, 7


def build(parent):
    sys.path.insert(0, ROOT)
    from bammmotif2_amd import build as b
    b.build_library()
    dst = os.path.join(WORK, "parent", "bammmotif2_amd")
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    src = os.path.join(parent, "bammmotif2_amd")
    for f in os.listdir(src):
        if f.endswith(".py") or f == "libbamm_em.so":
            shutil.copy2(os.path.join(src, f), dst)


def worker(variant, shapes):
    sys.path.insert(0, os.path.join(WORK, "parent") if variant == "parent" else ROOT)
    import numpy as np
    import ctypes as C
    import bammmotif2_amd as bm
    from bammmotif2_amd import abi, synth
    ctx = bm.Context(0)
    if variant == "slices":
        ctx.set_tuning(score_slices=1)
    out = {"variant": variant, "package": os.path.dirname(bm.__file__)}
    for name in shapes:
        groups, both, K, W = SHAPES[name]
        lens = np.concatenate([np.full(n, L, np.uint64) for n, L in groups])
        n = len(lens)
        v = synth.bamm_from_pwm((0.7 * synth.make_pwm(W, 3) + 0.075).astype(np.float32), K)
        rs = np.random.RandomState(1)
        codes = rs.randint(1, 5, size=int(lens.sum())).astype(np.uint8)
        codes[rs.randint(0, len(codes), size=len(codes) // 5000)] = 0          # one N in 5000 bases
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        packed = bm.PackedSeqs.from_codes(codes, off, not both, seed=42)
        vbg = packed.bg_model(BG, np.array([1, 10, 10], np.float32))
        seqs = bm.SeqSet(ctx, packed)
        del codes
        total = int((seqs.lengths.astype(np.int64) - W + 1).sum())
        if variant != "parent":
            out["plan_" + name] = bm.score_plan(ctx, seqs, K, W)
            out["geometry_" + name] = bm.score_slice_geometry(K, W)
        for kind in KINDS:
            mops = np.ones(total if kind == "mops" else 1, np.float32)          # touched: no page faults inside the timed calls
            zoops, z = np.ones(n, np.float32), np.ones(n, np.uint64)
            times = []
            for it in range(WARMUP + REPEATS):
                t0 = time.perf_counter()
                abi.check(ctx.lib.bamm_logodds(ctx.h, seqs.h, K, W, BG, v, vbg, mops.ctypes.data_as(C.c_void_p) if kind == "mops" else None,
                                               total if kind == "mops" else 0, zoops, z))
                if it >= WARMUP:
                    times.append((time.perf_counter() - t0) * 1e3)
            h = hashlib.sha1()
            for a in ((mops, zoops, z) if kind == "mops" else (zoops, z)):
                h.update(a.tobytes())
            out[f"{name}.{kind}"] = dict(ms=[round(t, 3) for t in times], sha1=h.hexdigest())
            print(f"{variant} {name}.{kind}: {out[f'{name}.{kind}']['ms']}", file=sys.stderr, flush=True)
            del mops
        seqs.close()
        del packed
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run(out_path, shapes, order):
    rows = []
    for vname in order:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", "--variant", vname, "--shapes", ",".join(shapes)],
                           stdout=subprocess.PIPE, text=True, timeout=120 + 60 * len(shapes))   # the worker's progress (stderr) passes through
        if r.returncode != 0:                                    # a fault or an abort: nothing more is started on the GPU
            print(r.stdout[-3000:])
            sys.exit(f"variant {vname} ended with status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    med = lambda x: sorted(x)[len(x) // 2]
    lines = [f"bamm_logodds, background order {BG}, one N in 5000 bases; {WARMUP} warm-up + {REPEATS} timed calls per process and case, host clock",
             "around the call (it ends in a stream synchronise and includes the download of mops where a case has them); ms.",
             "variants in the order they ran: parent = the parent commit's library (every sequence window by window), slices = this build",
             "with score_slices=1, off = this build as the library creates a context (score_slices=0)",
             "spread: the parent's, the larger of the gap between its two runs' medians and the min-max range of the timed calls of one run;",
             "the slices win a case when their median is below the parent's median (both runs) minus that spread", ""]
    verdicts = []
    for name in shapes:
        groups, both, K, W = SHAPES[name]
        for kind in KINDS:
            key = f"{name}.{kind}"
            lines.append(f"case ({key}): {' + '.join(f'{n} records x {L} bp' for n, L in groups)}, {'both strands' if both else 'single strand'}, K={K} W={W}, "
                         + ("zoops and z only" if kind == "zoops" else "with mops"))
            lines.append(f"  {'variant':8} {'median':>10} {'min':>10} {'max':>10}   slices (columns, slices) / plan")
            for r in rows:
                t = r[key]["ms"]
                lines.append(f"  {r['variant']:8} {med(t):10.3f} {min(t):10.3f} {max(t):10.3f}   {r.get('geometry_' + name, '')} {r.get('plan_' + name, '')}")
            runs = [r[key]["ms"] for r in rows if r["variant"] == "parent"]
            par = [x for t in runs for x in t]
            this = [r for r in rows if r["variant"] == "slices"][0][key]["ms"]
            spread = max([max(t) - min(t) for t in runs] + [abs(med(runs[0]) - med(runs[-1]))])
            wins = med(this) < med(par) - spread
            lines.append(f"  parent, both runs: median {med(par):.3f}, spread {spread:.3f}; slices: median {med(this):.3f}"
                         f" ({med(this) - med(par):+.3f} ms, {med(par) / med(this):.2f}x) -> {'the slices win' if wins else 'NO WIN BEYOND THE SPREAD'}")
            same = len({r[key]["sha1"] for r in rows}) == 1
            lines.append(f"  results: {'the same bytes in every variant' if same else 'DIFFERENT between variants: ' + str({r['variant']: r[key]['sha1'][:10] for r in rows})}")
            lines.append("")
            verdicts.append((key, wins, same))
    lines.append("summary: " + ("the slices win every case, the same bytes everywhere" if all(w and s for _, w, s in verdicts) else
                                "no win beyond the spread: " + ",".join(n for n, w, _ in verdicts if not w) + "; different bytes: " + ",".join(n for n, _, s in verdicts if not s)))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["build", "run", "worker"])
    ap.add_argument("--parent")
    ap.add_argument("--variant", default="slices")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--variants", default="parent,slices,off,parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_slices_ab.txt"))
    a = ap.parse_args()
    if a.mode == "build":
        build(a.parent)
    elif a.mode == "worker":
        worker(a.variant, a.shapes.split(","))
    else:
        run(a.out, a.shapes.split(","), a.variants.split(","))
