"""Speed of the default path, a parent checkout against this tree (profiles/default_path_records_speed.txt,
profiles/fused_filter_records_speed.txt).

  python scripts/default_path_speed.py run PARENT TREE OUTDIR [session]   alternating processes parent, tree, tree, parent, ... five
                                                                          each, every process under its own time limit; stops at the
                                                                          first that fails; then the summary of the session
  python scripts/default_path_speed.py one ROOT LABEL OUT                 one such process: the checkout ROOT (built), one JSON line
  python scripts/default_path_speed.py summary OUTDIR [session ...]       the table from the processes' JSON lines

One process runs ROOT/bench.py (--gpus 1 --steps 20 --warmup 5) at c2, c1, c3, c4 and c2 --batch 8 and keeps ms_per_step, and at the
same sizes takes the device time per frame of the kernel classes PSM_K_PREP, PSM_K_GUIDE, PSM_K_WTA and PSM_K_CVF_F under
PSM_OPT_PROFILE 1 (20 frames after 3): the totals are dominated by the fused filter and would hide a change in the small kernels.
The forms of the fused filter that bench.py does not run - one volume per launch, the storing form - give their PSM_K_CVF_F per frame
at 450 x 375 x 64 and 1920 x 1080 x 64 (10 frames after 3).
The bar: every median of the tree inside the parent's own min .. max of that quantity in that session."""
import contextlib
import io
import json
import os
import runpy
import statistics
import subprocess
import sys

CONFIGS = (("c2", 1), ("c1", 1), ("c3", 1), ("c4", 1), ("c2", 8))
CLASSES = ("PSM_K_PREP", "PSM_K_GUIDE", "PSM_K_WTA", "PSM_K_CVF_F")
STEPS, WARMUP, FRAMES, N_EACH, LIMIT_S = 20, 5, 20, 5, 240
FORM_SHAPES, FORM_FRAMES = ((450, 375, 64), (1920, 1080, 64)), 10


def name(cfg, batch):
    return cfg if batch == 1 else f"{cfg} --batch {batch}"


def bench(root, cfg, batch):
    argv = [os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--config", cfg]
    if batch > 1:
        argv += ["--batch", str(batch)]
    old, buf = sys.argv, io.StringIO()
    sys.argv = argv
    try:
        with contextlib.redirect_stdout(buf):
            try:
                runpy.run_path(argv[0], run_name="__main__")
            except SystemExit as e:
                assert not e.code, e.code
    finally:
        sys.argv = old
    rec = json.loads(buf.getvalue().strip().split("\n")[-1])
    assert rec["config"]["batch"] == batch
    return rec["ms_per_step"]


def classes(P, shape, dtype, batch):
    from primestereomatch_amd import capi, synth
    from primestereomatch_amd.dispest import compute_batch
    W, H, D = shape
    des = [P.DispEst(*synth.make_pair(W, H, D, seed=b)[:2], D, dtype=dtype) for b in range(batch)]
    try:
        de = des[0]

        def frame():
            if batch > 1:
                compute_batch(des)
            else:
                de.CostConst_GPU(); de.CostFilter_GPU(); de.DispSelect_device()
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        for _ in range(3):
            frame()
        de.synchronize()
        de.reset_kernel_times()
        for _ in range(FRAMES):
            frame()
        de.synchronize()
        out = {}
        for k in CLASSES:
            ms, n = de.kernel_time_ms(getattr(capi, k))
            out[k] = {"ms_per_frame": round(ms / FRAMES, 5), "launches_per_frame": n / FRAMES}
        return out
    finally:
        for d in des:
            d.close()


def forms(P, shape):
    """PSM_K_CVF_F per frame of the fused filter's forms that bench.py does not run: one volume per launch (CostFilter_side 0, 1)
    and the storing form (the default path under PSM_FLAG_STORE_FILTERED)."""
    from primestereomatch_amd import capi, synth
    W, H, D = shape
    out = {}
    with P.DispEst(*synth.make_pair(W, H, D, seed=0)[:2], D) as de:
        def sides():
            de.CostConst_GPU(); de.CostFilter_side(0); de.CostFilter_side(1)

        def stored():
            de.CostConst_GPU(); de.CostFilter_GPU()
        de.set_option(capi.PSM_OPT_PROFILE, 1)
        for form, frame, flags in (("one volume per launch", sides, 0), ("storing form", stored, capi.PSM_FLAG_STORE_FILTERED)):
            de.set_option(capi.PSM_OPT_FLAGS, flags)
            for _ in range(3):
                frame()
            de.synchronize()
            de.reset_kernel_times()
            for _ in range(FORM_FRAMES):
                frame()
            de.synchronize()
            ms, n = de.kernel_time_ms(capi.PSM_K_CVF_F)
            out[form] = {"PSM_K_CVF_F": {"ms_per_frame": round(ms / FORM_FRAMES, 5), "launches_per_frame": n / FORM_FRAMES}}
    return out


def one(root, label, out):
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    import primestereomatch_amd as P
    assert os.path.abspath(P.__file__).startswith(root + os.sep), P.__file__
    shapes = runpy.run_path(os.path.join(root, "bench.py"), run_name="shapes")["CONFIGS"]
    res = {"label": label, "bench_ms_per_step": {}, "classes": {}}
    for cfg, batch in CONFIGS:
        res["bench_ms_per_step"][name(cfg, batch)] = bench(root, cfg, batch)
        res["classes"][name(cfg, batch)] = classes(P, shapes[cfg][:3], "u8" if cfg.startswith("c1") else "f32", batch)
    for shape in FORM_SHAPES:
        for form, v in forms(P, shape).items():
            res["classes"]["%d x %d x %d, %s" % (*shape, form)] = v
    line = json.dumps(res)
    print(line, flush=True)
    with open(out, "w") as f:
        f.write(line + "\n")


def run(parent, tree, outdir, session):
    os.makedirs(outdir, exist_ok=True)
    order = [("parent", parent) if i % 4 in (0, 3) else ("tree", tree) for i in range(2 * N_EACH)]
    count = {"parent": 0, "tree": 0}
    for label, root in order:
        count[label] += 1
        out = os.path.join(outdir, f"s{session}_{label}_{count[label]}.json")
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "one", root, label, out])
        if r.returncode != 0:         # a fault, a hang or a failure: nothing more is started
            print(f"{label} {count[label]}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
    summary(outdir, [session])
    return 0


def quantities(rec):
    """name -> (value in ms, launches per frame or None)"""
    out = {f"bench.py {k}: ms_per_step": (v, None) for k, v in rec["bench_ms_per_step"].items()}
    for k, cl in rec["classes"].items():
        for c, v in cl.items():
            out[f"{k}: {c} ms per frame"] = (v["ms_per_frame"], v["launches_per_frame"])
    return out


def summary(outdir, sessions):
    lines = []
    for s in sessions:
        recs = {"parent": [], "tree": []}
        for f in sorted(os.listdir(outdir)):
            if f.startswith(f"s{s}_") and f.endswith(".json"):
                rec = json.loads(open(os.path.join(outdir, f)).read())
                recs[rec["label"]].append(quantities(rec))
        lines.append(f"== session {s}: {len(recs['parent'])} parent and {len(recs['tree'])} tree processes, alternating ==")
        outside = 0
        for k in recs["parent"][0]:
            p, t = [r[k][0] for r in recs["parent"]], [r[k][0] for r in recs["tree"]]
            lo, hi, med = min(p), max(p), statistics.median(t)
            outside += not lo <= med <= hi
            n = (recs["parent"][0][k][1], recs["tree"][0][k][1])
            lines.append(k + ("" if n[0] is None else f"   (launches per frame: parent {n[0]:g}, tree {n[1]:g})"))
            lines.append("    parent  " + " ".join(f"{v:.5f}" for v in p) + f"   median {statistics.median(p):.5f}  min {lo:.5f}  max {hi:.5f}")
            lines.append("    tree    " + " ".join(f"{v:.5f}" for v in t) + f"   median {med:.5f}  " +
                         ("inside the parent's spread" if lo <= med <= hi else "BELOW the parent's spread" if med < lo else "ABOVE the parent's spread"))
        lines.append(f"medians outside the parent's min .. max: {outside} of {len(recs['parent'][0])}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(outdir, f"summary_s{'_'.join(sessions)}.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "one":
        one(*sys.argv[2:5])
    elif mode == "run":
        sys.exit(run(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] if len(sys.argv) > 5 else "1"))
    else:
        summary(sys.argv[2], sys.argv[3:] or ["1"])
