#!/usr/bin/env python3
"""EM passes over long records (K = 2, W = 20, single strand): the parent commit against this build, this build with the
other candidate tile geometry and with em_tiles=0 -> profiles/em_tiles_ab.txt.

  build --parent DIR   (where the compiler is) copies the parent commit's built package from the worktree DIR to
                       tools/.em_tiles/parent/ and links one library per candidate geometry into tools/.em_tiles/m<M>/
                       (em_tiles.hip recompiled with -DBAMM_EM_TILE_M / _THREADS, every other object as built)
  run [--out FILE] [--shapes a,b] [--variants parent,this,m64,off,parent]
                       (on the GPU) one fresh process per variant under its own time limit, the parent measured twice with
                       the others in between; nothing more is started after a variant that fails.  Each process, per shape
                       (a: 16 x 4 M positions, b: 20 000 x 10 001 positions): the first pass from the seed model (every
                       window has a non-zero addend: the dense case) on three fresh handles; then on one handle 2 warm-up
                       passes and 7 calls of iterate(10), host clock around call + stream synchronise; then 7 single passes
                       of the by then converged model.
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
WORK = os.path.join(ROOT, "tools", ".em_tiles")
CANDIDATES = [(32, 512), (64, 512)]
K, W, BG = 2, 20, 2
SHAPES = {"a": (16, 4 * 1024 * 1024), "b": (20000, 10001)}       # (records, positions each)
WARMUP, REPEATS, PASSES = 2, 7, 10


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
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for M, T in CANDIDATES:
        d = os.path.join(WORK, f"m{M}")
        os.makedirs(d, exist_ok=True)
        obj = os.path.join(d, "em_tiles.o")
        log = subprocess.run([hipcc] + b.FLAGS + b.TU_FLAGS["em_tiles.hip"] + [f"-DBAMM_EM_TILE_M={M}", f"-DBAMM_EM_TILE_THREADS={T}", "-c",
                              os.path.join(b.CSRC, "em_tiles.hip"), "-o", obj], capture_output=True, text=True, check=True).stderr
        res = {k: v for k, v in b.parse_resources(log).items() if "k_em_tile" in k}
        objs = [obj if s == "em_tiles.hip" else b._obj(s) for s in b.SOURCES]
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", os.path.join(d, "libbamm_em.so")])
        with open(os.path.join(d, "resources.json"), "w") as fh:
            json.dump(res, fh)
        print(f"m{M}:", res)


def worker(variant, shapes, repeats, passes):
    sys.path.insert(0, os.path.join(WORK, "parent") if variant == "parent" else ROOT)
    import numpy as np
    import bammmotif2_amd as bm
    from bammmotif2_amd import abi, synth
    if variant.startswith("m"):
        abi.LIB_PATH = os.path.join(WORK, variant, "libbamm_em.so")
    ctx = bm.Context(0)
    if variant == "off":
        ctx.set_tuning(em_tiles=0)
    pwm = synth.make_pwm(W, 3)
    v0 = synth.bamm_from_pwm((0.7 * pwm + 0.075).astype(np.float32), K)
    A = synth.alpha_matrix(synth.default_alpha(K), W)
    out = {"variant": variant, "package": os.path.dirname(bm.__file__), "lib": abi.LIB_PATH}
    if variant != "parent":
        out["geometry"] = bm.em_tile_geometry(W)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    for name in shapes:
        n, L = SHAPES[name]
        rs = np.random.RandomState(1)
        codes = rs.randint(1, 5, size=n * L).astype(np.uint8)
        codes[rs.randint(0, len(codes), size=len(codes) // 5000)] = 0          # one N in 5000 bases
        site = np.argmax(pwm, axis=0).astype(np.uint8) + 1       # pwm is [4][W]; codes are 1..4
        for p in rs.randint(0, len(codes) - W, size=max(n, len(codes) // 2000)):   # a planted site every 2000 bases: something to converge to
            codes[p:p + W] = site
        off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
        packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
        vbg = packed.bg_model(BG, np.array([1, 10, 10], np.float32))
        seqs = bm.SeqSet(ctx, packed)
        del codes
        res = {}
        seed_ms = []
        for _ in range(3):                                       # the dense pass: the first one from the seed model
            em = bm.EM(ctx, seqs, K, W, vbg, A, v0, 0.3)
            ctx.sync()
            seed_ms.append(timed(lambda: em.iterate(1)))
            em.close()
        em = bm.EM(ctx, seqs, K, W, vbg, A, v0, 0.3)
        if variant != "parent":
            res["plan"] = em.tile_plan()
        em.iterate(WARMUP)
        ctx.sync()
        res["seed_pass_ms"] = [round(t, 3) for t in seed_ms]
        res["ms"] = [round(timed(lambda: em.iterate(passes)), 3) for _ in range(repeats)]
        res["converged_pass_ms"] = [round(timed(lambda: em.iterate(1)), 3) for _ in range(repeats)]
        res["llh"] = em.getLLH()
        res["sha1_v"] = hashlib.sha1(em.getV().tobytes()).hexdigest()
        out[name] = res
        print(f"{variant} {name}: {res}", file=sys.stderr, flush=True)
        em.close()
        seqs.close()
        del packed
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run(out_path, shapes, order, repeats, passes, limit):
    rows = []
    for vname in order:
        if vname.startswith("m") and not os.path.exists(os.path.join(WORK, vname, "libbamm_em.so")):
            continue
        # each variant under its own time limit (timeout -k: a hung process is killed); a failure ends the run
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "worker", "--variant", vname,
                            "--shapes", ",".join(shapes), "--repeats", str(repeats), "--passes", str(passes)], stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:                                    # a fault, an abort or the time limit: nothing more is started on the GPU
            print(r.stdout[-3000:])
            sys.exit(f"variant {vname} ended with status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(rows[-1], flush=True)
    med = lambda x: sorted(x)[len(x) // 2]
    lines = [f"bamm_em_iterate, K={K} W={W}, single strand, one N in 5000 bases, a planted site every 2000; per process and shape: the first pass from",
             f"the seed model on 3 fresh handles (dense: every window adds), then {WARMUP} warm-up passes + {repeats} calls of iterate({passes}), then {repeats}",
             "single passes of the converged model; host clock around call + stream synchronise; ms.",
             "variants in the order they ran: parent = the parent commit's library, this = this build, mNN = this build with NN positions",
             "per lane, off = this build with em_tiles=0",
             "spread: the parent's, the larger of the gap between its two runs' medians and the min-max range of one run's timed calls", ""]
    for name in shapes:
        n, L = SHAPES[name]
        lines.append(f"shape ({name}): {n} sequences x {L} positions")
        for key, what in (("ms", f"iterate({passes})"), ("seed_pass_ms", "one dense pass from the seed"), ("converged_pass_ms", "one converged pass")):
            lines.append(f"  {what}")
            lines.append(f"    {'variant':8} {'median':>10} {'min':>10} {'max':>10}   geometry / plan")
            for r in rows:
                t = r[name][key]
                lines.append(f"    {r['variant']:8} {med(t):10.3f} {min(t):10.3f} {max(t):10.3f}   {r.get('geometry', '')} {r[name].get('plan', '')}")
            runs = [r[name][key] for r in rows if r["variant"] == "parent"]
            if not runs:
                continue
            par = [x for t in runs for x in t]
            spread = max([max(t) - min(t) for t in runs] + [abs(med(runs[0]) - med(runs[-1]))])
            for r in rows:
                if r["variant"] == "parent":
                    continue
                t = med(r[name][key])
                gain = med(par) - t
                lines.append(f"    {r['variant']:8} against the parent (median {med(par):.3f}, spread {spread:.3f}): {med(par) / t:.2f}x, {gain:+.3f} ms -> "
                             f"{'faster by more than the spread' if gain > spread else ('slower by more than the spread' if -gain > spread else 'within the spread')}")
        lines.append("  llh / sha1 of v after the passes: " + ", ".join(f"{r['variant']} {r[name]['llh']:.6g} {r[name]['sha1_v'][:10]}" for r in rows))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["build", "run", "worker"])
    ap.add_argument("--parent")
    ap.add_argument("--variant", default="this")
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--variants", default=",".join(["parent", "this"] + [f"m{M}" for M, _ in CANDIDATES[1:]] + ["off", "parent"]))
    ap.add_argument("--repeats", type=int, default=REPEATS)
    ap.add_argument("--passes", type=int, default=PASSES)
    ap.add_argument("--limit", type=int, default=420, help="seconds one variant's process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "em_tiles_ab.txt"))
    a = ap.parse_args()
    if a.mode == "build":
        build(a.parent)
    elif a.mode == "worker":
        worker(a.variant, a.shapes.split(","), a.repeats, a.passes)
    else:
        run(a.out, a.shapes.split(","), a.variants.split(","), a.repeats, a.passes, a.limit)
