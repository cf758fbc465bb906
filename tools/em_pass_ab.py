#!/usr/bin/env python3
"""The host code of an EM pass (csrc/em_pass.cpp, em.cpp, plan.cpp, handles.h): the parent commit against this build ->
profiles/em_pass_refactor_ab.txt.  The kernels are the same in both, so what could move is the enqueue cost per pass and
bamm_em_create; what must not move is any output byte or any planner report.

  build --parent DIR   (where the compiler is) builds this tree and copies the parent commit's built package from the worktree
                       DIR, with bench.py and tools/optimize_vs_iterate.py, to tools/.em_pass/parent/
  run NAMES REPS       (on the GPU) for each named command REPS times parent, this, parent, this, ...: one fresh process per
                       run under its own time limit; nothing more is started after a run that fails.  The first run of each
                       variant also dumps its outputs.  Figures accumulate in tools/.em_pass/out/ab.json.
  plans TREE DIR       one variant (what `run plans` starts): plan(), plan_mixed(), plan_paths(), tile_plan() at the default
                       shape, c2 and c4's (K = 4, W = 30, 500 bp; 200 000 sequences), and on the last the model after four
                       passes with the planner's choice, lists forced, dense r forced and the slot-indexed E slices
  table [FILE]         the text table from ab.json and the dumps
"""
import filecmp
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORK = os.path.join(ROOT, "tools", ".em_pass")
TREE = {"parent": os.path.join(WORK, "parent"), "this": ROOT}
OUT = os.path.join(WORK, "out")
STATE = os.path.join(OUT, "ab.json")
BENCH = ["bench.py", "--gpus", "1"]
# name: (script and arguments, seconds one run may take, name of its output dump)
CMDS = {
    "bench_default": (BENCH + ["--steps", "200", "--warmup", "20", "--full", "--no-cpu-baseline"], 300, "default"),
    "bench_125k": (BENCH + ["--nseq", "125000", "--steps", "200", "--warmup", "20"], 120, None),
    "bench_c4": (BENCH + ["--config", "c4"], 420, "c4"),
    "bench_c2": (BENCH + ["--config", "c2"], 120, "c2"),
    "opt_vs_it": (["tools/optimize_vs_iterate.py"], 300, None),
    "plans": (None, 300, "plans"),
}


def build(parent):
    sys.path.insert(0, ROOT)
    from bammmotif2_amd import build as b
    b.build_library()
    dst = TREE["parent"]
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(os.path.join(dst, "bammmotif2_amd"))
    os.makedirs(os.path.join(dst, "tools"))
    for f in os.listdir(os.path.join(parent, "bammmotif2_amd")):
        if f.endswith(".py") or f == "libbamm_em.so":
            shutil.copy2(os.path.join(parent, "bammmotif2_amd", f), os.path.join(dst, "bammmotif2_amd"))
    shutil.copy2(os.path.join(parent, "bench.py"), dst)
    shutil.copy2(os.path.join(parent, "tools", "optimize_vs_iterate.py"), os.path.join(dst, "tools"))


def plans(tree, out_dir):
    sys.path.insert(0, tree)
    import numpy as np
    import bammmotif2_amd as bm
    from bammmotif2_amd import synth
    os.makedirs(out_dir, exist_ok=True)
    ctx = bm.Context(0)
    report = {"package": os.path.dirname(bm.__file__)}
    for name, (N, L0, W, K) in {"default": (1_000_000, 200, 20, 2), "c2": (50_000, 200, 20, 2), "c4_200k": (200_000, 500, 30, 4)}.items():
        pwm = synth.make_pwm(W, 1234)
        codes, off = synth.make_sequences(N, L0, pwm, 1234, plant_frac=0.5)
        pk = bm.PackedSeqs.from_codes(codes, off, False, seed=42)
        ss = bm.SeqSet(ctx, pk)
        vbg = pk.bg_model(2, np.array([1.0, 10.0, 10.0], np.float32))
        A = synth.alpha_matrix(synth.default_alpha(K), W)
        v0 = synth.bamm_from_pwm((0.7 * pwm + 0.3 * 0.25).astype(np.float32), K)
        flavours = {"planner": {}} if K < 4 else {"planner": {}, "lists": {"adaptive_lists": 0}, "dense": {"e_list": 0}, "slots": {"e_fused": 0}}
        for fl, tune in flavours.items():
            ctx.set_tuning(**tune)
            em = bm.EM(ctx, ss, K, W, vbg, A, v0, 0.3, n_seqs_bound=N)
            ctx.set_tuning(**{k: 1 for k in tune})
            report[f"{name} {fl}"] = dict(plan=em.plan(), plan_mixed=em.plan_mixed(), plan_paths=em.plan_paths(), tile_plan=em.tile_plan())
            if K >= 4:
                em.iterate(4)
                llh, v_diff, _ = em.trace()
                for what, a in (("v", em.getV()), ("counts", em.getCounts()), ("llh", llh), ("v_diff", v_diff)):
                    np.save(os.path.join(out_dir, f"{name}_{fl}_{what}.npy"), np.ascontiguousarray(a, np.float32))
            em.close()
        ss.close()
    ctx.close()
    del report["package"]
    with open(os.path.join(out_dir, "planner_reports.json"), "w") as fh:
        json.dump(report, fh, indent=1, sort_keys=True)


def load():
    return json.load(open(STATE)) if os.path.exists(STATE) else {}


def run_one(name, variant, rep):
    argv, limit, dump = CMDS[name]
    tree = TREE[variant]
    if argv is None:
        cmd = [sys.executable, os.path.abspath(__file__), "plans", tree, os.path.join(OUT, "dumps", variant, dump)]
    else:
        cmd = [sys.executable, os.path.join(tree, argv[0])] + argv[1:]
        if dump and rep == 0:
            cmd += ["--dump-outputs", os.path.join(OUT, "dumps", variant, dump)]
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=tree)
    with open(os.path.join(OUT, f"{name}_{variant}_{rep}.log"), "w") as fh:
        fh.write(r.stdout)
    if r.returncode != 0:                                        # a fault, an abort or the time limit: nothing more is started on the GPU
        print(r.stdout[-3000:])
        sys.exit(f"{name} ({variant}, run {rep}) ended with status {r.returncode}")
    res = {}
    if name == "opt_vs_it":
        for m in re.finditer(r"N\s+(\d+): iterate\s+([\d.]+) us/pass, optimize\s+([\d.]+) us/pass", r.stdout):
            res[f"N={m.group(1)} iterate us/pass"] = float(m.group(2))
            res[f"N={m.group(1)} optimize us/pass"] = float(m.group(3))
    elif argv is not None:
        j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        fs = j.get("from_seed") or {}
        for src, keys in ((j, ("ms_per_step", "avg_kernel_ms")), (fs, ("first_create_ms", "first_call_ms", "ms_per_step_iterate", "ms_per_step_optimize"))):
            res.update({k: float(src[k]) for k in keys if isinstance(src.get(k), (int, float))})
    return res


def run(names, reps):
    os.makedirs(OUT, exist_ok=True)
    st = load()
    for name in names:
        for rep in range(1 if name == "plans" else reps):
            for variant in ("parent", "this"):
                res = run_one(name, variant, rep)
                st.setdefault(name, {}).setdefault(variant, []).append(res)
                with open(STATE, "w") as fh:
                    json.dump(st, fh, indent=1)
                print(name, variant, rep, res, flush=True)


def table(path):
    st = load()
    med = lambda x: sorted(x)[len(x) // 2]
    lines = ["parent = the parent commit's library (built in a worktree of its own), this = this build; the two alternate, parent first, one",
             "process per run.  A run reports one figure per quantity, so a run's median is that figure and the parent's spread is the range",
             "of its runs' figures.  Bar: this build's median <= the parent's median + the parent's spread.", ""]
    outside = []
    for name, by in st.items():
        if name == "plans" or not by.get("this"):
            continue
        lines.append(f"{name}: {' '.join(CMDS[name][0])}")
        for k in by["parent"][0]:
            p, t = [r[k] for r in by["parent"] if k in r], [r[k] for r in by["this"] if k in r]
            spread = max(p) - min(p)
            ok = med(t) <= med(p) + spread
            if not ok:
                outside.append(f"{name}: {k}")
            lines.append(f"  {k:30} parent {' '.join(f'{x:9.3f}' for x in p)} | this {' '.join(f'{x:9.3f}' for x in t)} | medians {med(p):.3f} / {med(t):.3f}, "
                         f"spread {spread:.3f}: {med(t) - med(p):+.3f} -> {'within the bar' if ok else 'OUTSIDE THE BAR'}")
        lines.append("")
    lines.append("outputs: bench.py --dump-outputs of each variant's first run (default, c2, c4), and `plans`: the four planner reports at the")
    lines.append("default shape, c2 and c4's shape with 200 000 sequences, and on the last v / counts / trace after iterate(4) per sliced flavour")
    base, differ = os.path.join(OUT, "dumps"), []
    for root, _, files in sorted(os.walk(os.path.join(base, "parent"))):
        for f in sorted(files):
            rel = os.path.relpath(os.path.join(root, f), os.path.join(base, "parent"))
            same = os.path.exists(os.path.join(base, "this", rel)) and filecmp.cmp(os.path.join(base, "parent", rel), os.path.join(base, "this", rel), shallow=False)
            differ += [] if same else [rel]
            lines.append(f"  {rel:42} {os.path.getsize(os.path.join(root, f)):9d} bytes  {'same bytes' if same else 'DIFFERENT'}")
    lines += ["", "outside the bar: " + (", ".join(outside) or "none"), "different outputs: " + (", ".join(differ) or "none")]
    text = "\n".join(lines)
    print(text)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "build":
        build(sys.argv[sys.argv.index("--parent") + 1])
    elif mode == "plans":
        plans(sys.argv[2], sys.argv[3])
    elif mode == "run":
        run(sys.argv[2].split(","), int(sys.argv[3]))
    else:
        table(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "em_pass_refactor_ab.txt"))
