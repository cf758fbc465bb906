#!/usr/bin/env python3
"""bamm_logodds (with mops, K = 2, W = 20) on long records: the parent commit against this build, this build with
score_tiles=0, and the other candidate tile geometries.  Result: profiles/score_tiles_ab.txt.

  build --parent DIR   (where the compiler is) copies the parent commit's built package from the worktree DIR to
                       tools/.score_tiles/parent/ and links one library per candidate geometry into tools/.score_tiles/m<M>/
                       (score_tile.hip recompiled with -DBAMM_SCORE_TILE_M / _THREADS, every other object as built)
  run [--out FILE]     (on the GPU) one fresh process per variant, the parent measured twice with the others in between,
                       each process: shape (a) 16 x 4 M positions and (b) 20 000 x 10 001 positions, 2 warm-up calls and
                       7 timed ones (host clock around the call, which ends in a stream synchronise), and a SHA-1 of
                       mops / zoops / z, which must be the same for every variant
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
SHAPES = {"a": (16, 4 * 1024 * 1024), "b": (20000, 10001)}
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
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    for M, T in CANDIDATES:
        d = os.path.join(WORK, f"m{M}")
        os.makedirs(d, exist_ok=True)
        obj = os.path.join(d, "score_tile.o")
        log = subprocess.run([hipcc] + b.FLAGS + [f"-DBAMM_SCORE_TILE_M={M}", f"-DBAMM_SCORE_TILE_THREADS={T}", "-c",
                              os.path.join(b.CSRC, "score_tile.hip"), "-o", obj], capture_output=True, text=True, check=True).stderr
        res = {k: v for k, v in b.parse_resources(log).items() if "k_score_tileI" in k}
        objs = [obj if s == "score_tile.hip" else b._obj(s) for s in b.SOURCES]
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
    for name in shapes:
        n, L = SHAPES[name]
        rs = np.random.RandomState(1)
        codes = rs.randint(1, 5, size=n * L).astype(np.uint8)
        codes[rs.randint(0, n * L, size=n * L // 5000)] = 0      # one N in 5000 bases
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
        packed = bm.PackedSeqs.from_codes(codes, off, True, seed=42)
        vbg = packed.bg_model(BG, np.array([1, 10, 10], np.float32))
        seqs = bm.SeqSet(ctx, packed)
        del codes
        total = n * (L - W + 1)
        mops = np.ones(total, np.float32)                        # touched: no page faults inside the timed calls
        zoops, z = np.ones(n, np.float32), np.ones(n, np.uint64)
        if variant != "parent":
            out["plan_" + name] = bm.score_plan(ctx, seqs, K, W)
        times = []
        for it in range(WARMUP + REPEATS):
            t0 = time.perf_counter()
            abi.check(ctx.lib.bamm_logodds(ctx.h, seqs.h, K, W, BG, v, vbg, mops.ctypes.data_as(C.c_void_p), total, zoops, z))
            if it >= WARMUP:
                times.append((time.perf_counter() - t0) * 1e3)
        h = hashlib.sha1()
        for a in (mops, zoops, z):
            h.update(a.tobytes())
        out[name] = dict(ms=[round(t, 3) for t in times], sha1=h.hexdigest())
        seqs.close()
        del mops, packed
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run(out_path, shapes):
    order = ["parent", "this"] + [f"m{M}" for M, _ in CANDIDATES] + ["off", "parent"]
    rows = []
    for vname in order:
        if vname.startswith("m") and not os.path.exists(os.path.join(WORK, vname, "libbamm_em.so")):
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", "--variant", vname, "--shapes", shapes],
                           capture_output=True, text=True, timeout=400)
        if r.returncode != 0:                                    # a fault or an abort: nothing more is started on the GPU
            print(r.stdout[-3000:], r.stderr[-3000:])
            sys.exit(f"variant {vname} ended with status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        print(rows[-1], flush=True)
    med = lambda x: sorted(x)[len(x) // 2]
    lines = [f"bamm_logodds with mops, K={K} W={W}, single strand, one N in 5000 bases; {WARMUP} warm-up + {REPEATS} timed calls per process,",
             "host clock around the call (it ends in a stream synchronise and includes the download of mops); ms.",
             "variants in the order they ran: parent = the parent commit's library, this = this build, mNN = this build with NN positions",
             "per lane, off = this build with score_tiles=0", ""]
    for name in shapes:
        n, L = SHAPES[name]
        lines.append(f"shape ({name}): {n} sequences x {L} positions")
        lines.append(f"  {'variant':8} {'median':>10} {'min':>10} {'max':>10}   geometry / plan")
        for r in rows:
            t = r[name]["ms"]
            lines.append(f"  {r['variant']:8} {med(t):10.2f} {min(t):10.2f} {max(t):10.2f}   {r.get('geometry', '')} {r.get('plan_' + name, '')}")
        par = [x for r in rows if r["variant"] == "parent" for x in r[name]["ms"]]
        this = [r for r in rows if r["variant"] == "this"][0][name]["ms"]
        lines.append(f"  parent, both runs: median {med(par):.2f}, spread (max - min) {max(par) - min(par):.2f}; this build: median {med(this):.2f}"
                     f" -> {med(par) / med(this):.2f}x, faster by {med(par) - med(this):.2f} ms")
        same = len({r[name]["sha1"] for r in rows}) == 1
        lines.append(f"  mops / zoops / z: {'the same bytes in every variant' if same else 'DIFFERENT between variants: ' + str({r['variant']: r[name]['sha1'][:10] for r in rows})}")
        lines.append("")
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
    ap.add_argument("--shapes", default="ab")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_tiles_ab.txt"))
    a = ap.parse_args()
    if a.mode == "build":
        build(a.parent)
    elif a.mode == "worker":
        worker(a.variant, a.shapes)
    else:
        run(a.out, a.shapes)
