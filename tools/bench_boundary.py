"""Timings behind DESIGN.md 25 (boundary-aware scene evaluation), on one MI355X:

    python tools/make_fake_scenes.py <root> --scenes 1 --val 2 --size 2048 --learnable
    python tools/bench_boundary.py <root> [--radius 3] [--shape disk] [--runs 3] [--out profiles/boundary_bench.json]

Three arms over the validation scenes of <root>, ResNet-50, bf16, crop and stride 256, the same seeded weights:
  off      SceneEvaluator without `boundary`: what the parent commit runs (the launches are the same), evaluation 1 and evaluation 2
  on       SceneEvaluator(boundary=R): the same plus five launches of libemrt_hip_bnd.so per scene; then each of the five timed on scene 0 with
           HIP events, the median of 24 launches each, next to emrt_segmentation_areas on the same maps
  host     the evaluator of the off arm, then per scene a copy of the prediction to the host and tests/boundary_reference.py (numpy, the brute-force
           loop over offsets) on it and on the label map: the copy and the model are timed
The arms alternate, --runs times each, every run in a fresh process under its own time limit; the first run that fails ends the measurement.
The totals of evaluate() must be identical in all arms and the boundary counts of the on arm must equal the host model's (asserted).

Prints one JSON line and writes it to --out.  Needs the GPU: there is no CPU fallback.  (--arm off|on|host runs one arm in this process.)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_eval_scenes import ARM_TIMEOUT, _config, _model, _spread, _timed          # noqa: E402

SHAPES = ("disk", "square")


def _evaluator(root, **kw):
    from emrt_amd import val
    return val.scene_evaluator(_model(), _config(root), "cuda:0", **kw)


def _evaluations(ev, res):
    from emrt_amd import val
    for k in (1, 2):
        _, t = _timed(lambda: val.evaluate_scenes(ev))
        res["eval%d_s" % k] = t
    res["totals"] = ev.per_scene.sum(0).cpu().tolist()
    return res


def arm_off(root, radius, shape):
    ev = _evaluator(root)
    return _evaluations(ev, {"arm": "off", "scenes": len(ev.bank), "sizes": ev.bank.sizes})


def arm_on(root, radius, shape, launches=24):
    import torch
    from emrt_amd import _lib
    from emrt_amd import functional as Fn
    from emrt_amd.runtime import ctx
    ev = _evaluator(root, boundary=radius, boundary_shape=shape)
    res = _evaluations(ev, {"arm": "on", "scenes": len(ev.bank), "sizes": ev.bank.sizes})
    res["boundary_per_scene"] = ev.boundary_per_scene.cpu().tolist()
    # the launches of scene 0 one by one, on its prediction
    B, L, c = _lib.bnd_lib(), _lib.lib(), ctx()
    pred, (_, label), (H, W) = ev.predict(0), ev.bank.scene(0), ev.bank.sizes[0]
    run, bp, bl = ev._boundary_buffers(H, W)
    out3 = torch.zeros(3, ev.ncls, dtype=torch.int64, device="cuda")
    out6 = torch.zeros(2, 3, ev.ncls, dtype=torch.int64, device="cuda")
    P, r, s = Fn.P, ev.boundary, ev.boundary_shape
    calls = [("emrt_segmentation_areas", lambda: L.call("emrt_segmentation_areas", P(pred), P(label), 2, H * W, ev.ncls, 255, P(out3), c.stream)),
             ("emrt_bnd_runs(pred)", lambda: B.call("emrt_bnd_runs", P(pred), 0, H, W, r, P(run), c.stream)),
             ("emrt_bnd_band(pred)", lambda: B.call("emrt_bnd_band", P(pred), 0, P(run), H, W, r, s, P(bp), c.stream)),
             ("emrt_bnd_runs(label)", lambda: B.call("emrt_bnd_runs", P(label), 2, H, W, r, P(run), c.stream)),
             ("emrt_bnd_band(label)", lambda: B.call("emrt_bnd_band", P(label), 2, P(run), H, W, r, s, P(bl), c.stream)),
             ("emrt_bnd_areas", lambda: B.call("emrt_bnd_areas", P(pred), P(label), P(bp), P(bl), H * W, ev.ncls, 255, P(out6), c.stream))]
    res["kernels_ms"], res["kernel_scene"] = {}, [H, W]
    for name, call in calls:
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res["kernels_ms"][name] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    res["band_share"] = {"pred": round(float(bp.float().mean()), 4), "label": round(float(bl.float().mean()), 4)}
    return res


def arm_host(root, radius, shape):
    import torch
    from tests import boundary_reference as BR
    ev = _evaluator(root)
    res = _evaluations(ev, {"arm": "host", "scenes": len(ev.bank)})
    counts, copy_s, model_s = [], 0.0, 0.0
    for i in range(len(ev.bank)):
        pred_d = ev.predict(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred, label = pred_d.cpu().numpy()[0, 0], ev.bank.scene(i)[1].cpu().numpy()
        t1 = time.perf_counter()
        counts.append(BR.counts(pred, label, ev.ncls, 255, radius, shape).tolist())
        copy_s, model_s = copy_s + t1 - t0, model_s + time.perf_counter() - t1
    res.update({"copy_s": copy_s, "model_s": model_s, "boundary_per_scene": counts, "numpy_threads": os.environ.get("OMP_NUM_THREADS")})
    return res


ARMS = {"off": arm_off, "on": arm_on, "host": arm_host}


def _child(arm, a):
    cmd = [sys.executable, os.path.abspath(__file__), a.root, "--arm", arm, "--radius", str(a.radius), "--shape", a.shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=ARM_TIMEOUT, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("[bench_boundary] the %s arm ended with status %d; nothing more is started\n%s" % (arm, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("root")
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--shape", choices=SHAPES, default="disk")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_bench.json"))
    ap.add_argument("--arm", choices=list(ARMS), default=None)
    a = ap.parse_args(argv)
    if a.arm:
        print(json.dumps(ARMS[a.arm](a.root, a.radius, a.shape)), flush=True)
        return
    runs = {arm: [] for arm in ARMS}
    for _ in range(a.runs):
        for arm in ARMS:
            runs[arm].append(_child(arm, a))
    totals = [r["totals"] for arm in runs for r in runs[arm]]
    assert all(t == totals[0] for t in totals), "the arms returned different evaluation totals"
    counts = [r["boundary_per_scene"] for arm in ("on", "host") for r in runs[arm]]
    assert all(c == counts[0] for c in counts), "the device counts and the host model differ"
    n = runs["off"][0]["scenes"]
    off2, on2 = [r["eval2_s"] for r in runs["off"]], [r["eval2_s"] for r in runs["on"]]
    report = {"measurement": "boundary-aware evaluation of whole validation scenes", "scenes": n, "sizes": runs["off"][0]["sizes"], "backbone": "resnet50",
              "dtype": "bf16", "crop": 256, "radius": a.radius, "shape": a.shape, "runs_per_arm": a.runs, "totals_identical": True,
              "counts_equal_host_model": True,
              "off_eval1_s": _spread([r["eval1_s"] for r in runs["off"]]), "off_eval2_s": _spread(off2),
              "on_eval1_s": _spread([r["eval1_s"] for r in runs["on"]]), "on_eval2_s": _spread(on2),
              "added_ms_per_scene": round(1e3 * (statistics.median(on2) - statistics.median(off2)) / n, 3),
              "host_copy_s": _spread([r["copy_s"] for r in runs["host"]]), "host_model_s": _spread([r["model_s"] for r in runs["host"]]),
              "host_numpy_threads": runs["host"][0]["numpy_threads"],
              "kernel_scene": runs["on"][-1]["kernel_scene"], "kernels_ms": runs["on"][-1]["kernels_ms"], "band_share": runs["on"][-1]["band_share"]}
    line = json.dumps(report)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
