#!/usr/bin/env python3
"""bamm_logodds (K = 2, W = 20): the parent commit against this build.  Long records with mops (shapes a, b), where this
build also runs with score_tiles=0 and with the other candidate tile geometries -> profiles/score_tiles_ab.txt; and one
shape of short records per length class of k_score (c1 .. c128: records of 64 * M positions, 2^27 positions, no mops, so that
the kernel and not the download is timed), parent / this / parent only, with the margin this build has to keep:
its median no more than the parent's median plus the parent's own spread on that shape.

  build --parent DIR   (where the compiler is) copies the parent commit's built package from the worktree DIR to
                       tools/.score_tiles/parent/ and links one library per candidate geometry into tools/.score_tiles/m<M>/
                       (scorer.hip recompiled with -DBAMM_SCORE_TILE_M / _THREADS, every other object as built)
  run [--out FILE] [--shapes a,b | classes | a,b,classes] [--variants parent,this,parent]
                       (on the GPU) one fresh process per variant, the parent measured twice with the others in between,
                       each process: shape (a) 16 x 4 M positions and (b) 20 000 x 10 001 positions, 2 warm-up calls and
                       7 timed ones (host clock around the call, which ends in a stream synchronise), and a SHA-1 of
                       mops / zoops / z, which must be the same for every variant; `seed`: bamm_seed_from_pwm at
                       1 M x 200 positions (k_seed_pwm shares device_utils.h's decode_to_lds with EM::mask's kernels)
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
WORK = os.path.join(ROOT, "tools", ".score_tiles")
CANDIDATES = [(32, 512), (64, 512), (128, 256)]            # classes of BAMM_FOR_EACH_MCLASS
K, W, BG = 2, 20, 2
M_CLASSES = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 128]
CLASS_POSITIONS = 1 << 27
SHAPES = {"a": (16, 4 * 1024 * 1024, "mops"), "b": (20000, 10001, "mops")}       # (records, positions each, what is timed)
SHAPES.update({f"c{M}": (CLASS_POSITIONS // (64 * M), 64 * M, "zoops") for M in M_CLASSES})
SHAPES["seed"] = (1000000, 200, "seed")                    # bamm_seed_from_pwm (k_seed_pwm), not the scorer
WARMUP, REPEATS = 2, 7


def shape_list(arg):
    names = [n for part in arg.split(",") for n in ([f"c{M}" for M in M_CLASSES] if part == "classes" else [part])]
    assert all(n in SHAPES for n in names), names
    return names


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
        obj = os.path.join(d, "scorer.o")
        log = subprocess.run([hipcc] + b.FLAGS + b.TU_FLAGS["scorer.hip"] + [f"-DBAMM_SCORE_TILE_M={M}", f"-DBAMM_SCORE_TILE_THREADS={T}", "-c",
                              os.path.join(b.CSRC, "scorer.hip"), "-o", obj], capture_output=True, text=True, check=True).stderr
        res = {k: v for k, v in b.parse_resources(log).items() if "k_score_tileI" in k}
        objs = [obj if s == "scorer.hip" else b._obj(s) for s in b.SOURCES]
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", os.path.join(d, "libbamm_em.so")])
        with open(os.path.join(d, "resources.json"), "w") as fh:
            json.dump(res, fh)
        print(f"m{M}:", res)


def worker(variant, shapes):
    if variant == "parent":
        sys.path.insert(0, os.path.join(WORK, "parent"))
    else:
        sys.path.insert(0, ROOT)
    import numpy as np
    import ctypes as C
    import bammmotif2_amd as bm
    from bammmotif2_amd import abi, synth
    if variant.startswith("m"):
        abi.LIB_PATH = os.path.join(WORK, variant, "libbamm_em.so")
    ctx = bm.Context(0)
    if variant == "off":
        ctx.set_tuning(score_tiles=0)
    v = synth.bamm_from_pwm((0.7 * synth.make_pwm(W, 3) + 0.075).astype(np.float32), K)
    out = {"variant": variant, "package": os.path.dirname(bm.__file__), "lib": abi.LIB_PATH}
    if variant != "parent":
        out["geometry"] = bm.score_tile_geometry(W)
    class_codes = None                                           # the class shapes: prefixes of one array of 2^27 codes
    for name in shapes:
        n, L, kind = SHAPES[name]
        want_mops, shared = kind == "mops", kind == "zoops"
        rs = np.random.RandomState(1)
        if not shared or class_codes is None:
            codes = rs.randint(1, 5, size=CLASS_POSITIONS if shared else n * L).astype(np.uint8)
            codes[rs.randint(0, len(codes), size=len(codes) // 5000)] = 0      # one N in 5000 bases
            if shared:
                class_codes = codes
        if shared:
            codes = class_codes[:n * L]
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
        packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
        vbg = packed.bg_model(BG, np.array([1, 10, 10], np.float32))
        seqs = bm.SeqSet(ctx, packed)
        del codes
        total = n * (L - W + 1) if want_mops else 0
        mops = np.ones(total, np.float32)                        # touched: no page faults inside the timed calls
        zoops, z = np.ones(n, np.float32), np.ones(n, np.uint64)
        if variant != "parent" and kind != "seed":
            out["plan_" + name] = bm.score_plan(ctx, seqs, K, W)
        times = []
        if kind == "seed":
            score = np.ascontiguousarray((0.7 * synth.make_pwm(W, 3) + 0.075) / 0.25, np.float32).ravel()   # [4][W] odds
            u = np.random.RandomState(2).random_sample(n)
        for it in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            if kind == "seed":
                hashed = bm.seed_from_pwm(ctx, seqs, K, W, score, 0.9, u)
            else:
                abi.check(ctx.lib.bamm_logodds(ctx.h, seqs.h, K, W, BG, v, vbg, mops.ctypes.data_as(C.c_void_p) if want_mops else None, total, zoops, z))
                hashed = (mops, zoops, z)
            if it >= WARMUP:
                times.append((time.perf_counter() - t0) * 1e3)
        h = hashlib.sha1()
        for a in hashed:
            h.update(a.tobytes())
        out[name] = dict(ms=[round(t, 3) for t in times], sha1=h.hexdigest())
        print(f"{variant} {name}: {out[name]['ms']}", file=sys.stderr, flush=True)
        seqs.close()
        del mops, packed
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run(out_path, shapes, order):
    rows = []
    for vname in order:
        if vname.startswith("m") and not os.path.exists(os.path.join(WORK, vname, "libbamm_em.so")):
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", "--variant", vname, "--shapes", ",".join(shapes)],
                           stdout=subprocess.PIPE, text=True, timeout=200 + 40 * len(shapes))   # the worker's progress (stderr) passes through
        if r.returncode != 0:                                    # a fault or an abort: nothing more is started on the GPU
            print(r.stdout[-3000:])
            sys.exit(f"variant {vname} ended with status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(rows[-1], flush=True)
    med = lambda x: sorted(x)[len(x) // 2]
    lines = [f"bamm_logodds (shape `seed`: bamm_seed_from_pwm), K={K} W={W}, single strand, one N in 5000 bases; {WARMUP} warm-up + {REPEATS} timed calls per process,",
             "host clock around the call (it ends in a stream synchronise and includes the download of mops where a shape has them); ms.",
             "variants in the order they ran: parent = the parent commit's library, this = this build, mNN = this build with NN positions",
             "per lane, off = this build with score_tiles=0",
             "margin: this build's median against the parent's median (both runs) + the parent's spread, the larger of the gap between",
             "its two runs' medians and the min-max range of the timed calls of one run", ""]
    verdicts = []
    for name in shapes:
        n, L, kind = SHAPES[name]
        lines.append(f"shape ({name}): {n} sequences x {L} positions, " + {"mops": "bamm_logodds with mops", "zoops": "bamm_logodds without mops", "seed": "bamm_seed_from_pwm (counts, z)"}[kind])
        lines.append(f"  {'variant':8} {'median':>10} {'min':>10} {'max':>10}   geometry / plan")
        for r in rows:
            t = r[name]["ms"]
            lines.append(f"  {r['variant']:8} {med(t):10.3f} {min(t):10.3f} {max(t):10.3f}   {r.get('geometry', '') if kind != 'seed' else ''} {r.get('plan_' + name, '')}")
        par = [x for r in rows if r["variant"] == "parent" for x in r[name]["ms"]]
        this = [r for r in rows if r["variant"] == "this"][0][name]["ms"]
        runs = [r[name]["ms"] for r in rows if r["variant"] == "parent"]
        spread = max([max(t) - min(t) for t in runs] + [abs(med(runs[0]) - med(runs[-1]))])
        within = med(this) <= med(par) + spread
        lines.append(f"  parent, both runs: median {med(par):.3f}, spread {spread:.3f}; this build: median {med(this):.3f}"
                     f" ({med(this) - med(par):+.3f} ms, {med(par) / med(this):.2f}x) -> {'within the margin' if within else 'OUTSIDE THE MARGIN'}")
        same = len({r[name]["sha1"] for r in rows}) == 1
        lines.append(f"  results: {'the same bytes in every variant' if same else 'DIFFERENT between variants: ' + str({r['variant']: r[name]['sha1'][:10] for r in rows})}")
        lines.append("")
        verdicts.append((name, within, same))
    lines.append("summary: " + ("every shape within the margin, the same bytes everywhere" if all(w and s for _, w, s in verdicts) else
                                "outside the margin: " + ",".join(n for n, w, _ in verdicts if not w) + "; different bytes: " + ",".join(n for n, _, s in verdicts if not s)))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["build", "run", "worker"])
    ap.add_argument("--parent")
    ap.add_argument("--variant", default="this")
    ap.add_argument("--shapes", default="a,b", help="comma-separated: a, b, c<M>, or `classes` for every c<M>")
    ap.add_argument("--variants", default=",".join(["parent", "this"] + [f"m{M}" for M, _ in CANDIDATES] + ["off", "parent"]))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_tiles_ab.txt"))
    a = ap.parse_args()
    if a.mode == "build":
        build(a.parent)
    elif a.mode == "worker":
        worker(a.variant, shape_list(a.shapes))
    else:
        run(a.out, shape_list(a.shapes), a.variants.split(","))
