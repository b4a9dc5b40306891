"""Timings behind DESIGN.md 16 (whole-scene prediction), on one MI355X:

    python tools/bench_predict.py [--sizes 2048 6000] [--runs 30] [--backbone resnet50] [--dtype bf16] [--no-wall]

(a) kernel time: emrt_scene_finish (index + colour + areas from sums and counts) against the pair it replaces, emrt_window_normalise +
    emrt_argmax_nchw, on the same buffers at 6 classes.  Each sample is a device-event pair around 10 back-to-back repetitions (a single
    launch of ~50 us would time the host's launch path), the two alternate, and the figure is the median of --runs samples after a warm-up.
    The indices of the two are compared first.  Effective bandwidth = the bytes the algorithm needs (32 B per pixel for the finish with
    colour, 80 B for the pair, both at 6 classes) over that time.
(b) host wall per square scene of the first size: ScenePredictor on the uint8 scene plus the device-to-host copy of index and colour bytes,
    against ss_inference + .cpu() + one boolean-mask numpy pass per class (the reference's colouring loop); and the same two without the
    model (the tails alone: what this work changes).  A host clock around work that ends in a synchronise; median of 8 (two alternating blocks of 4).

Prints one JSON line per measurement.  Needs the GPU: there is no CPU fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emrt_amd import _lib                                   # noqa: E402
from emrt_amd.functional import P                           # noqa: E402
from emrt_amd.runtime import ctx, BF16, F16, F32            # noqa: E402
from emrt_amd.src.utils import vis                          # noqa: E402

NCLS, REPS = 6, 10
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def _events(fn, runs, warmup=3):
    """[milliseconds per repetition] of `runs` samples, each REPS back-to-back calls of fn between two device events"""
    out = []
    for i in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1) / REPS)
    return out


def kernel_times(S, runs):
    L, c = _lib.lib(), ctx()
    g = torch.Generator(device="cuda").manual_seed(S)
    final = torch.randn(1, NCLS, S, S, generator=g, device="cuda")
    count = torch.randint(1, 5, (1, 1, S, S), generator=g, device="cuda").float()
    pal = vis.get_palette("Potsdam")
    parr = (ctypes.c_ubyte * pal.size)(*pal.reshape(-1).tolist())
    pp = ctypes.cast(parr, ctypes.c_void_p)
    logits = torch.empty_like(final)
    pred = torch.empty(1, 1, S, S, dtype=torch.int32, device="cuda")
    index = torch.empty(1, S, S, dtype=torch.uint8, device="cuda")
    color = torch.empty(1, S, S, 3, dtype=torch.uint8, device="cuda")
    areas = torch.zeros(NCLS, dtype=torch.int64, device="cuda")

    def pair():
        L.call("emrt_window_normalise", P(final), P(count), P(logits), NCLS, S, S, c.stream)
        L.call("emrt_argmax_nchw", P(logits), P(pred), 1, NCLS, S, S, c.stream)

    def finish():
        L.call("emrt_scene_finish", P(final), P(count), pp, None, 0.0, P(index), P(color), None, P(areas), 1, NCLS, S, S, c.stream)

    pair()
    finish()
    torch.cuda.synchronize()
    assert torch.equal(index.view(-1).int(), pred.view(-1)), "the finish and the pair disagree"
    t_pair, t_fin = [], []
    for _ in range(3):                                       # alternate the two in blocks of runs / 3 samples
        t_pair += _events(pair, max(1, runs // 3))
        t_fin += _events(finish, max(1, runs // 3))
    mp, mf = statistics.median(t_pair), statistics.median(t_fin)
    npix = S * S
    return {"measurement": "kernel", "shape": [NCLS, S, S], "samples": len(t_fin), "pair_ms": round(mp, 4), "finish_ms": round(mf, 4),
            "finish_over_pair": round(mf / mp, 3), "pair_min_max_ms": [round(min(t_pair), 4), round(max(t_pair), 4)],
            "finish_min_max_ms": [round(min(t_fin), 4), round(max(t_fin), 4)],
            "pair_GBps": round(80 * npix / mp / 1e6, 1), "finish_GBps": round(32 * npix / mf / 1e6, 1)}


def _paint(pred, pal):
    """the reference's colouring loop: one boolean mask per class"""
    out = np.zeros(pred.shape + (3,), dtype=np.uint8)
    for k in range(len(pal)):
        out[pred == k] = pal[k]
    return out


def _wall(fn, runs=7, warmup=2):
    out = []
    for i in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def wall_times(S, backbone, dtype):
    from emrt_amd.src.api import infer
    from emrt_amd.src.api.scene import ScenePredictor
    from emrt_amd.src.models.emrt import EMRT
    from emrt_amd.src.transforms import Normalize
    torch.manual_seed(0)
    model = EMRT(num_classes=NCLS, backbone=backbone)
    model.to_hip("cuda:0", {"fp32": F32, "bf16": BF16, "fp16": F16}[dtype])
    if dtype == "fp16":
        model.compute_aux_in_eval = False
    model.eval()
    pal = vis.get_palette("Potsdam")
    crop = stride = (256, 256)
    rng = np.random.RandomState(0)
    scene = rng.randint(0, 256, (S, S, 3), dtype=np.uint8)
    scene_d = torch.from_numpy(scene).cuda()
    img_d = torch.from_numpy(np.ascontiguousarray(np.transpose(Normalize(MEAN, STD)(scene.astype(np.float32))[0], (2, 0, 1)))).cuda()
    p = ScenePredictor(model, NCLS, crop, stride, pal, MEAN, STD)
    L, c = _lib.lib(), ctx()
    keep = {}

    def new():
        r = p(scene_d)
        keep["new"] = (r.index.cpu().numpy(), r.color.cpu().numpy())

    def old():
        pred = infer.ss_inference(model, [img_d], [(S, S)], True, None, stride, crop, NCLS)[0]
        pred = pred.cpu().numpy()[0, 0]
        keep["old"] = (pred, _paint(pred, pal))

    # the tails alone, on sums and counts that stay on the device
    final = torch.randn(1, NCLS, S, S, device="cuda")
    count = torch.ones(1, 1, S, S, device="cuda")
    out = p._outputs(1, S, S)

    def new_tail():
        p._finish(final, count, scene_d, out, 0, 1, S, S)
        keep["new_tail"] = (out.index[0].cpu().numpy(), out.color[0].cpu().numpy())

    def old_tail():
        logits = c.empty((1, NCLS, S, S), torch.float32)
        L.call("emrt_window_normalise", P(final), P(count), P(logits), NCLS, S, S, c.stream)
        pred = c.empty((1, 1, S, S), torch.int32)
        L.call("emrt_argmax_nchw", P(logits), P(pred), 1, NCLS, S, S, c.stream)
        pred = pred.cpu().numpy()[0, 0]
        keep["old_tail"] = (pred, _paint(pred, pal))

    t = {"new": [], "old": [], "new_tail": [], "old_tail": []}
    for _ in range(2):
        for name, fn in (("new", new), ("old", old), ("new_tail", new_tail), ("old_tail", old_tail)):
            t[name] += _wall(fn, runs=4, warmup=1)
    assert np.array_equal(keep["new"][0], keep["old"][0]) and np.array_equal(keep["new"][1], keep["old"][1]), "new and old maps differ"
    assert np.array_equal(keep["new_tail"][0], keep["old_tail"][0]) and np.array_equal(keep["new_tail"][1], keep["old_tail"][1]), "new and old tails differ"
    med = {k: round(statistics.median(v), 2) for k, v in t.items()}
    return {"measurement": "host wall per scene", "scene": [S, S], "backbone": backbone, "dtype": dtype, "crop": 256, "samples": len(t["new"]),
            "new_ms": med["new"], "old_ms": med["old"], "new_tail_ms": med["new_tail"], "old_tail_ms": med["old_tail"],
            "d2h_bytes_per_pixel": {"new": 4, "old": 4}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 6000])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--no-wall", action="store_true")
    a = ap.parse_args(argv)
    ctx().init_device("cuda:0", F32)
    for S in a.sizes:
        print(json.dumps(kernel_times(S, a.runs)), flush=True)
    if not a.no_wall:
        print(json.dumps(wall_times(a.sizes[0], a.backbone, a.dtype)), flush=True)


if __name__ == "__main__":
    main()
