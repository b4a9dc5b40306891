"""Timings behind DESIGN.md 18 (native-resolution evaluation of whole validation scenes), on one MI355X:

    python tools/make_fake_scenes.py <root> --scenes 1 --val 4 --size 2048
    python tools/bench_eval_scenes.py <root> [--runs 3] [--out profiles/scene_eval.json]

Two arms over the validation scenes of <root>, ResNet-50, bf16, crop and stride 256, the same seeded weights:
  host     val.evaluate() over ValTiles(SceneVal(...)) with VAL.KEEP_ORI_SIZE true: every scene decoded and normalised on the host, kept there as
           fp32, copied host-to-device at every evaluation.  The first evaluation decodes, the second reads ValTiles' cache: timed separately.
  device   the validation SceneBank uploaded once (timed), then SceneEvaluator, evaluation 1 and evaluation 2.
The arms alternate, --runs times each, every run in a fresh process under its own time limit; the first run that fails ends the measurement.
Both arms must return identical integer totals (asserted); the report holds median and range per arm.  A last process times
emrt_segmentation_areas at n = 2048^2 for int64 labels (selector 1) and uint8 labels (selector 2): the median of 24 event-timed launches each.

Prints one JSON line and writes it to --out.  Needs the GPU: there is no CPU fallback.  (--arm host|device|kernel runs one arm in this process.)"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCLS, CROP = 6, 256
ARM_TIMEOUT = 420          # seconds per child process


def _config(root):
    from emrt_amd.config import get_config
    config = get_config()
    config.DATA.DATA_PATH, config.DATA.DATASET, config.DATA.NUM_CLASSES = root, "Potsdam", NCLS
    config.VAL.CROP_SIZE, config.VAL.STRIDE_SIZE = [CROP, CROP], [CROP, CROP]
    config.VAL.KEEP_ORI_SIZE, config.VAL.RESCALE_FROM_ORI = True, False
    config.TRAIN.IGNORE_INDEX = 255
    return config


def _model():
    import torch
    from emrt_amd.runtime import BF16
    from emrt_amd.src.models.emrt import EMRT
    torch.manual_seed(0)
    model = EMRT(num_classes=NCLS, backbone="resnet50")
    model.to_hip("cuda:0", BF16)
    model.eval()
    return model


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def arm_host(root):
    import torch
    from emrt_amd import val
    from emrt_amd.src.datasets import SceneVal
    from emrt_amd.src.transforms import get_val_transforms
    from emrt_amd.src.utils import metrics
    config, model = _config(root), _model()
    ds = SceneVal(get_val_transforms(config), root, NCLS)
    cache = {}
    images, labels = val.ValTiles(ds, 0, cache), val.ValTiles(ds, 1, cache)
    area, tot = metrics.calculate_area, torch.zeros(3, NCLS, dtype=torch.int64, device="cuda")

    def recording(*a, **k):          # evaluate() returns ratios: the integer totals behind them are summed here
        out = area(*a, **k)
        tot.add_(torch.stack(list(out)))
        return out

    metrics.calculate_area = recording
    res = {"arm": "host", "scenes": len(ds)}
    for k in (1, 2):
        tot.zero_()
        _, t = _timed(lambda: val.evaluate(model, images, labels, config))
        res["eval%d_s" % k] = t
        res["totals%d" % k] = tot.cpu().tolist()
    return res


def arm_device(root):
    from emrt_amd import val
    config, model = _config(root), _model()
    ev, t_up = _timed(lambda: val.scene_evaluator(model, config, "cuda:0"))
    res = {"arm": "device", "scenes": len(ev.bank), "upload_s": t_up, "bank_bytes": ev.bank.nbytes}

    def once():          # what the command lines run: the evaluation, the metric tuple (one small device-to-host copy), and the totals for the check
        val.evaluate_scenes(ev)
        return ev.per_scene.sum(0)

    for k in (1, 2):
        tot, t = _timed(once)
        res["eval%d_s" % k] = t
        res["totals%d" % k] = tot.cpu().tolist()
    return res


def arm_kernel(launches=24):
    import torch
    from emrt_amd import _lib
    from emrt_amd.runtime import F32, ctx
    ctx().init_device("cuda:0", F32)
    L, c = _lib.lib(), ctx()
    n = 2048 * 2048
    g = torch.Generator().manual_seed(0)
    pred = torch.randint(0, NCLS, (n,), generator=g).int().cuda()
    lab = torch.randint(0, NCLS, (n,), generator=g)
    lab[torch.rand(n, generator=g) < 0.015] = 255
    labels = {1: lab.cuda(), 2: lab.to(torch.uint8).cuda()}
    res = {"arm": "kernel", "n": n, "launches": launches}
    outs = {}
    for sel, lt in labels.items():
        out = torch.zeros(3, NCLS, dtype=torch.int64, device="cuda")
        call = lambda: L.call("emrt_segmentation_areas", ctypes.c_void_p(pred.data_ptr()), ctypes.c_void_p(lt.data_ptr()), sel, n, NCLS, 255,
                              ctypes.c_void_p(out.data_ptr()), c.stream)
        call()
        torch.cuda.synchronize()
        outs[sel] = out.cpu().clone()
        ms = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        res["selector%d_ms" % sel] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    assert torch.equal(outs[1], outs[2]), "int64 and uint8 labels count differently"
    return res


def _child(arm, root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), root, "--arm", arm], capture_output=True, text=True, timeout=ARM_TIMEOUT, cwd=ROOT)
    if r.returncode != 0:
        raise SystemExit("[bench_eval_scenes] the %s arm ended with status %d; nothing more is started\n%s" % (arm, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def _spread(values):
    return {"median": round(statistics.median(values), 3), "min": round(min(values), 3), "max": round(max(values), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("root")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_eval.json"))
    ap.add_argument("--arm", choices=["host", "device", "kernel"], default=None)
    a = ap.parse_args(argv)
    if a.arm:
        print(json.dumps({"host": lambda: arm_host(a.root), "device": lambda: arm_device(a.root), "kernel": arm_kernel}[a.arm]()), flush=True)
        return
    runs = {"host": [], "device": []}
    for _ in range(a.runs):
        for arm in ("host", "device"):
            runs[arm].append(_child(arm, a.root))
    totals = [r["totals%d" % k] for arm in runs for r in runs[arm] for k in (1, 2)]
    assert all(t == totals[0] for t in totals), "the arms (or two evaluations of one arm) returned different totals"
    report = {"measurement": "evaluation of whole validation scenes", "scenes": runs["host"][0]["scenes"], "backbone": "resnet50", "dtype": "bf16",
              "crop": CROP, "runs_per_arm": a.runs, "totals_identical": True, "totals": totals[0],
              "host_eval1_s": _spread([r["eval1_s"] for r in runs["host"]]), "host_eval2_s": _spread([r["eval2_s"] for r in runs["host"]]),
              "device_upload_s": _spread([r["upload_s"] for r in runs["device"]]), "bank_bytes": runs["device"][0]["bank_bytes"],
              "device_eval1_s": _spread([r["eval1_s"] for r in runs["device"]]), "device_eval2_s": _spread([r["eval2_s"] for r in runs["device"]]),
              "segmentation_areas": _child("kernel", a.root)}
    line = json.dumps(report)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
