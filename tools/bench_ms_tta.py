"""Timings behind DESIGN.md 23 (multi-scale test-time augmentation of whole-scene inference), on one MI355X:

    python tools/bench_ms_tta.py [--size 2048] [--crop 256] [--strides 256 128] [--scales 0.75 1.0 1.25] [--modes none hflip d4] [--runs 12]

The glue around the model call, per mode and stride, on a synthetic uint8 scene at 6 classes with max_batch 64.  One sample is a device-event
pair around ONE pass over the scene -- every scale, every chunk of 64 // G footprints -- with the model call left out (both sides read the same
fixed logits):
  fused:    emrt_mst_crop_windows_u8 + emrt_mst_window_accumulate per chunk (libemrt_hip_mstta.so);
  unfused:  the composition of what the libraries already hold.  Per scale and chunk: emrt_scene_crop_windows_u8 of the footprints, the resize
            kernel (infer._resize_nchw_f32) to the crop, torch flip / transpose copies into the variant batch; then per variant the inverse
            copy, a resize back to the footprint, a torch softmax and emrt_window_accumulate with the footprint's dimensions.
The two alternate; the figures are the median, minimum and maximum of --runs samples after a warm-up.  Their sums and counts are compared
first: equal counts, and sums within twice the per-pixel bound of tests/ms_tta_reference.py (the sum over a pixel's terms of
(C + 8) * 2^-23 + m * 2^-20, m the largest |logit| among the term's four taps).

Prints one JSON line per measurement.  Needs the GPU: there is no CPU fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from emrt_amd import _lib                                   # noqa: E402
from emrt_amd.functional import P                           # noqa: E402
from emrt_amd.runtime import ctx, F32                       # noqa: E402
from emrt_amd.src.api import infer                          # noqa: E402
from emrt_amd.src.api import scene as S                     # noqa: E402

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


def _taps(n_out, n_src):
    """the integer tap rule of include/emrt_hip_mstta.h -> (i0, i1) as int64 arrays"""
    i = np.arange(n_out, dtype=np.int64)
    num, den = (2 * i + 1) * n_src - n_out, 2 * n_out
    i0 = np.minimum(np.where(num <= 0, 0, num // den), n_src - 1)
    return i0, np.minimum(i0 + 1, n_src - 1)


def _bound_map(logits, grids, chunks_of, codes, H, W, crop):
    """the per-pixel bound of the sums, on the device: per scale, chunk slot and variant, (C + 8) * 2^-23 + 2^-20 * the largest |logit| at the
    four taps, added over the footprint"""
    G = len(codes)
    bound = torch.zeros(H, W, dtype=torch.float64, device="cuda")
    for (_s, fh, fw, _org), chunks in zip(grids, chunks_of):
        (y0, y1), (x0, x1) = _taps(fh, crop), _taps(fw, crop)
        y0, y1, x0, x1 = (torch.from_numpy(v).cuda() for v in (y0, y1, x0, x1))
        terms = []
        for j in range(logits.shape[0] // G):
            t = torch.zeros(fh, fw, dtype=torch.float64, device="cuda")
            for gi, k in enumerate(codes):
                a = _inverse(logits[j * G + gi], k).abs().amax(0).double()
                m = torch.maximum(torch.maximum(a[y0][:, x0], a[y0][:, x1]), torch.maximum(a[y1][:, x0], a[y1][:, x1]))
                t += (NCLS + 8) * 2.0 ** -23 + m * 2.0 ** -20
            terms.append(t)
        for ch in chunks:
            for j, (y, x) in enumerate(ch):
                bound[y:y + fh, x:x + fw] += terms[j]
    return bound


def glue_times(size, crop, stride, scales, mode, runs):
    L, T, c = _lib.lib(), _lib.mst_lib(), ctx()
    codes = S.TTA_MODES[mode]
    G, per = len(codes), 64 // len(codes)
    H = W = size
    g = torch.Generator(device="cuda").manual_seed(size + stride)
    scene = torch.randint(0, 256, (H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    logits = torch.randn(per * G, NCLS, crop, crop, generator=g, device="cuda") * 4
    mean, stdinv = S.check_normalise(MEAN, STD)
    grids = S.footprint_grids(H, W, (crop, crop), (stride, stride), scales)
    chunks_of = [[org[i:i + per] for i in range(0, len(org), per)] for _, _, _, org in grids]
    hosts_of = [[(_ints([v for yx in ch for v in yx]), len(ch)) for ch in chunks] for chunks in chunks_of]
    karr, kptr = _ints(list(codes))
    sums = {k: (torch.zeros(1, NCLS, H, W, device="cuda"), torch.zeros(1, 1, H, W, device="cuda")) for k in ("fused", "unfused")}
    batch = torch.empty(per * G, 3, crop, crop, device="cuda")
    keep = {}

    def fused():
        final, count = sums["fused"]
        for (_s, fh, fw, _org), hosts in zip(grids, hosts_of):
            for (_arr, ptr), n in hosts:
                T.call("emrt_mst_crop_windows_u8", P(scene), P(batch), ptr, n, kptr, G, H, W, fh, fw, crop, crop, *mean, *stdinv, c.stream)
                T.call("emrt_mst_window_accumulate", P(logits), P(final), P(count), ptr, n, kptr, G, NCLS, H, W, fh, fw, crop, crop, c.stream)

    def unfused():
        final, count = sums["unfused"]
        for (_s, fh, fw, _org), hosts, chunks in zip(grids, hosts_of, chunks_of):
            for ((_arr, ptr), n), ch in zip(hosts, chunks):
                plain, _, _keep = S.crop_windows(scene, H, W, ch, fh, fw, mean, stdinv)
                plain = infer._resize_nchw_f32(plain, crop, crop)
                keep["batch"] = torch.stack([_variant(plain, k) for k in codes], dim=1).view(n * G, 3, crop, crop)      # what the model would be given
                lg = logits[:n * G].view(n, G, NCLS, crop, crop)
                for gi, k in enumerate(codes):
                    back = infer._resize_nchw_f32(_inverse(lg[:, gi], k).contiguous(), fh, fw)
                    prob = torch.softmax(back, dim=1)
                    L.call("emrt_window_accumulate", P(prob), P(final), P(count), ptr, n, NCLS, H, W, fh, fw, c.stream)

    fused()
    unfused()
    torch.cuda.synchronize()
    bound = _bound_map(logits, grids, chunks_of, codes, H, W, crop)
    diff = (sums["fused"][0][0].double() - sums["unfused"][0][0].double()).abs().amax(0)
    ratio = (diff / bound.clamp_min(1e-30)).max().item()
    batch_diff = (keep["batch"] - batch[:keep["batch"].shape[0]]).abs().max().item()
    print(json.dumps({"measurement": "agreement", "mode": mode, "stride": stride, "max_abs_sum_diff": diff.max().item(),
                      "max_sum_diff_over_bound": ratio, "last_batch_max_abs_diff": batch_diff}), flush=True)
    assert torch.equal(sums["fused"][1], sums["unfused"][1]), "fused and unfused counts differ"
    assert ratio <= 2.0, "fused and unfused sums differ by %g times the per-pixel bound" % ratio
    t = {"fused": [], "unfused": []}
    for i in range(2 + runs):
        for name, fn in (("fused", fused), ("unfused", unfused)):
            ms = _sample(fn)
            if i >= 2:
                t[name].append(ms)
    mf, mu = statistics.median(t["fused"]), statistics.median(t["unfused"])
    return {"measurement": "glue per scene", "scene": [H, W], "crop": crop, "stride": stride, "scales": list(scales), "mode": mode,
            "footprints": [len(org) for _, _, _, org in grids], "launches_fused": 2 * sum(len(ch) for ch in chunks_of),
            "samples": len(t["fused"]), "fused_ms": round(mf, 4), "unfused_ms": round(mu, 4), "fused_over_unfused": round(mf / mu, 3),
            "fused_min_max_ms": [round(min(t["fused"]), 4), round(max(t["fused"]), 4)],
            "unfused_min_max_ms": [round(min(t["unfused"]), 4), round(max(t["unfused"]), 4)]}


def launch_times(size, crop, scale, mode, runs):
    """the two launches of ONE chunk of 64 // G footprints (a row of footprints side by side), each alone: [crop ms, accumulate ms]"""
    T, c = _lib.mst_lib(), ctx()
    codes = S.TTA_MODES[mode]
    (fw, fh), _ = S.footprint((crop, crop), (crop, crop), scale)
    G, per = len(codes), min(64 // len(codes), size // fw)
    g = torch.Generator(device="cuda").manual_seed(7)
    scene = torch.randint(0, 256, (size, size, 3), generator=g, device="cuda", dtype=torch.uint8)
    logits = torch.randn(per * G, NCLS, crop, crop, generator=g, device="cuda") * 4
    batch = torch.empty(per * G, 3, crop, crop, device="cuda")
    final, count = torch.zeros(1, NCLS, size, size, device="cuda"), torch.zeros(1, 1, size, size, device="cuda")
    mean, stdinv = S.check_normalise(MEAN, STD)
    _o, op = _ints([v for j in range(per) for v in (0, j * fw)])
    _k, kp = _ints(list(codes))
    crop_fn = lambda: [T.call("emrt_mst_crop_windows_u8", P(scene), P(batch), op, per, kp, G, size, size, fh, fw, crop, crop, *mean, *stdinv, c.stream)
                       for _ in range(10)]
    acc_fn = lambda: [T.call("emrt_mst_window_accumulate", P(logits), P(final), P(count), op, per, kp, G, NCLS, size, size, fh, fw, crop, crop, c.stream)
                      for _ in range(10)]
    out = [statistics.median([_sample(fn) / 10 for _ in range(2 + runs)][2:]) for fn in (crop_fn, acc_fn)]
    return {"measurement": "one chunk", "mode": mode, "scale": scale, "footprints": per, "footprint": fh, "crop": crop,
            "crop_us": round(out[0] * 1e3, 2), "accumulate_us": round(out[1] * 1e3, 2)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--crop", type=int, default=256)
    ap.add_argument("--strides", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--scales", type=float, nargs="+", default=[0.75, 1.0, 1.25])
    ap.add_argument("--modes", nargs="+", default=["none", "hflip", "d4"], choices=list(S.TTA_MODES))
    ap.add_argument("--runs", type=int, default=12)
    a = ap.parse_args(argv)
    scales = S.check_tta_scales(a.scales, None)
    ctx().init_device("cuda:0", F32)
    for mode in a.modes:
        for s in scales:
            print(json.dumps(launch_times(a.size, a.crop, s, mode, a.runs)), flush=True)
        for stride in a.strides:
            print(json.dumps(glue_times(a.size, a.crop, stride, scales, mode, a.runs)), flush=True)


if __name__ == "__main__":
    main()
