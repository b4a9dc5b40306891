"""Timings behind DESIGN.md 22 (flip and rotation test-time augmentation of whole-scene inference), on one MI355X:

    python tools/bench_tta.py [--size 2048] [--crop 256] [--strides 256 128] [--runs 12] [--backbone resnet50] [--dtype bf16] [--no-predict]

(a) the glue around the model call, per mode and stride, on a synthetic uint8 scene at 6 classes.  One sample is a device-event pair around ONE
    pass over the scene -- every chunk of 64 // G windows -- with the model call left out (both sides read the same fixed logits):
      fused:    emrt_tta_crop_windows_u8 + emrt_tta_window_accumulate per chunk (libemrt_hip_tta.so);
      unfused:  what the library held before: emrt_scene_crop_windows_u8, torch flip / transpose copies into the variant batch, then per
                variant the inverse copy, a torch softmax and emrt_window_accumulate.
    The two alternate; the figure is the median of --runs samples after a warm-up.  Their sums and counts are compared first.  Bytes are what
    each side's launches move, computed from the shapes (the fused accumulation touches the windows' bounding box, the unfused one the whole
    scene per launch: that is emrt_window_accumulate's grid).
(b) host wall of ScenePredictor per scene and mode with a real model (a host clock around work that ends in a synchronise; median).

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
from emrt_amd.src.api import infer                          # noqa: E402
from emrt_amd.src.api import scene as S                     # noqa: E402
from emrt_amd.src.utils import vis                          # noqa: E402

NCLS = 6
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def _variant(x, code):
    dims = [d for d, on in ((-2, code & 2), (-1, code & 1)) if on]
    x = torch.flip(x, dims) if dims else x
    return x.transpose(-1, -2) if code & 4 else x


def _inverse(x, code):
    x = x.transpose(-1, -2) if code & 4 else x
    dims = [d for d, on in ((-2, code & 2), (-1, code & 1)) if on]
    return torch.flip(x, dims) if dims else x


def _ints(values):
    arr = (ctypes.c_int * len(values))(*values)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def glue_times(size, crop, stride, mode, runs):
    L, T, c = _lib.lib(), _lib.tta_lib(), ctx()
    codes = S.TTA_MODES[mode]
    G, per = len(codes), 64 // len(codes)
    H = W = size
    g = torch.Generator(device="cuda").manual_seed(size + stride)
    scene = torch.randint(0, 256, (H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    logits = torch.randn(per * G, NCLS, crop, crop, generator=g, device="cuda") * 4
    mean, stdinv = S.check_normalise(MEAN, STD)
    org = [(a, b) for (a, b, _, _) in infer.window_grid(H, W, (crop, crop), (stride, stride))]
    chunks = [org[i:i + per] for i in range(0, len(org), per)]
    hosts = [(_ints([v for yx in ch for v in yx]), len(ch)) for ch in chunks]
    karr, kptr = _ints(list(codes))
    sums = {k: (torch.zeros(1, NCLS, H, W, device="cuda"), torch.zeros(1, 1, H, W, device="cuda")) for k in ("fused", "unfused")}
    batch = torch.empty(per * G, 3, crop, crop, device="cuda")
    keep = {}

    def fused():
        final, count = sums["fused"]
        for (_arr, ptr), n in hosts:
            T.call("emrt_tta_crop_windows_u8", P(scene), P(batch), ptr, n, kptr, G, H, W, crop, crop, *mean, *stdinv, c.stream)
            T.call("emrt_tta_window_accumulate", P(logits), P(final), P(count), ptr, n, kptr, G, NCLS, H, W, crop, crop, c.stream)

    def unfused():
        final, count = sums["unfused"]
        for ((_arr, ptr), n), ch in zip(hosts, chunks):
            plain, _, _keep = S.crop_windows(scene, H, W, ch, crop, crop, mean, stdinv)
            keep["batch"] = torch.stack([_variant(plain, k) for k in codes], dim=1).view(n * G, 3, crop, crop)      # what the model would be given
            lg = logits[:n * G].view(n, G, NCLS, crop, crop)
            for gi, k in enumerate(codes):
                prob = torch.softmax(_inverse(lg[:, gi], k).contiguous(), dim=1)
                L.call("emrt_window_accumulate", P(prob), P(final), P(count), ptr, n, NCLS, H, W, crop, crop, c.stream)

    fused()
    unfused()
    torch.cuda.synchronize()
    assert torch.equal(keep["batch"], batch[:keep["batch"].shape[0]]), "the variant batches of the last chunk differ"
    cover = sums["fused"][1].max().item() / G
    bound = cover * G * (NCLS + 8) * 2.0 ** -23
    diff = (sums["fused"][0] - sums["unfused"][0]).abs().max().item()
    assert torch.equal(sums["fused"][1], sums["unfused"][1]) and diff <= 2 * bound, "fused and unfused sums differ by %g" % diff
    t = {"fused": [], "unfused": []}
    for i in range(2 + runs):
        for name, fn in (("fused", fused), ("unfused", unfused)):
            ms = _sample(fn)
            if i >= 2:
                t[name].append(ms)
    nwin, px = len(org), crop * crop
    box = sum((max(y for y, _ in ch) - min(y for y, _ in ch) + crop) * (max(x for _, x in ch) - min(x for _, x in ch) + crop) for ch in chunks)
    rmw = 2 * 4 * (NCLS + 1)          # final and count: read and written
    fused_bytes = nwin * px * (3 + G * 3 * 4 + G * NCLS * 4) + box * rmw
    unfused_bytes = nwin * px * (3 + 3 * 4 + 2 * G * 3 * 4 + G * NCLS * 4 * (2 + 2 + 1)) + len(chunks) * G * H * W * rmw
    mf, mu = statistics.median(t["fused"]), statistics.median(t["unfused"])
    return {"measurement": "glue per scene", "scene": [H, W], "crop": crop, "stride": stride, "mode": mode, "windows": nwin, "launches_fused": 2 * len(chunks),
            "samples": len(t["fused"]), "fused_ms": round(mf, 4), "unfused_ms": round(mu, 4), "fused_over_unfused": round(mf / mu, 3),
            "fused_min_max_ms": [round(min(t["fused"]), 4), round(max(t["fused"]), 4)],
            "unfused_min_max_ms": [round(min(t["unfused"]), 4), round(max(t["unfused"]), 4)],
            "fused_MB": round(fused_bytes / 1e6, 1), "unfused_MB": round(unfused_bytes / 1e6, 1), "max_abs_sum_diff": diff}


def launch_times(size, crop, mode, runs):
    """the two launches of ONE chunk of 64 // G windows (a row of windows at stride = crop), each alone: [crop ms, accumulate ms]"""
    T, c = _lib.tta_lib(), ctx()
    codes = S.TTA_MODES[mode]
    G, per = len(codes), min(64 // len(codes), size // crop)
    g = torch.Generator(device="cuda").manual_seed(7)
    scene = torch.randint(0, 256, (size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
    logits = torch.randn(per * G, NCLS, crop, crop, generator=g, device="cuda") * 4
    batch = torch.empty(per * G, 3, crop, crop, device="cuda")
    final, count = torch.zeros(1, NCLS, size, size, device="cuda"), torch.zeros(1, 1, size, size, device="cuda")
    mean, stdinv = S.check_normalise(MEAN, STD)
    _o, op = _ints([v for j in range(per) for v in (0, j * crop)])
    _k, kp = _ints(list(codes))
    crop_fn = lambda: [T.call("emrt_tta_crop_windows_u8", P(scene), P(batch), op, per, kp, G, size, size, crop, crop, *mean, *stdinv, c.stream) for _ in range(10)]
    acc_fn = lambda: [T.call("emrt_tta_window_accumulate", P(logits), P(final), P(count), op, per, kp, G, NCLS, size, size, crop, crop, c.stream) for _ in range(10)]
    out = []
    for fn in (crop_fn, acc_fn):
        out.append(statistics.median([_sample(fn) / 10 for _ in range(2 + runs)][2:]))
    px = per * crop * crop
    return {"measurement": "one chunk", "mode": mode, "windows": per, "crop": crop, "crop_us": round(out[0] * 1e3, 2), "accumulate_us": round(out[1] * 1e3, 2),
            "crop_GBps": round(px * (3 + G * 12) / out[0] / 1e6, 1), "accumulate_GBps": round(px * (G * NCLS * 4 + 56) / out[1] / 1e6, 1)}


def predict_times(size, crop, stride, backbone, dtype, runs):
    from emrt_amd.src.models.emrt import EMRT
    torch.manual_seed(0)
    model = EMRT(num_classes=NCLS, backbone=backbone)
    model.to_hip("cuda:0", {"fp32": F32, "bf16": BF16, "fp16": F16}[dtype])
    if dtype == "fp16":
        model.compute_aux_in_eval = False
    model.eval()
    scene = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (size, size, 3), dtype=np.uint8)).cuda()
    out = {"measurement": "host wall per scene", "scene": [size, size], "crop": crop, "stride": stride, "backbone": backbone, "dtype": dtype, "samples": runs}
    for mode in S.TTA_MODES:
        p = S.ScenePredictor(model, NCLS, (crop, crop), (stride, stride), vis.get_palette("Potsdam"), MEAN, STD, max_batch=64, tta=mode)
        ms = []
        for i in range(1 + runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p(scene)
            torch.cuda.synchronize()
            if i >= 1:
                ms.append((time.perf_counter() - t0) * 1e3)
        out[mode + "_ms"] = round(statistics.median(ms), 2)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--strides", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16", "fp16"])
    ap.add_argument("--no-predict", action="store_true")
    a = ap.parse_args(argv)
    ctx().init_device("cuda:0", F32)
    for mode in ("hflip", "flips", "d4"):
        print(json.dumps(launch_times(a.size, a.crop, mode, a.runs)), flush=True)
        for stride in a.strides:
            print(json.dumps(glue_times(a.size, a.crop, stride, mode, a.runs)), flush=True)
    if not a.no_predict:
        print(json.dumps(predict_times(a.size, a.crop, a.strides[0], a.backbone, a.dtype, max(3, a.runs // 4))), flush=True)


if __name__ == "__main__":
    main()
