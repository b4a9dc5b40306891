"""Optimizer-pass timing: emrt_sgd_momentum_step, emrt_sgd_momentum_step_sched and emrt_adamw_step alternated in ONE process on the real flat
buffers of the flagship model (ResNet-50 EMRT, bf16 mirror, ~54 M trained parameters), a device-event pair around every launch.

    python tools/bench_optim.py [--reps 30] [--warmup 5] [--json profiles/optim_bench.json]

Bytes are counted from the shapes: SGD reads p, g, v and writes p, v (fp32) + the 2-byte mirror = 22 B / parameter; AdamW adds the second
moment read and written = 30 B / parameter.  The bytes-moved expectation for AdamW is therefore 30 / 22 = 1.36 x the SGD pass; the reported
ratio is measured against emrt_sgd_momentum_step in the same call.  Needs a GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--backbone", default="resnet50")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs a GPU")
    from emrt_amd import _lib
    from emrt_amd import functional as Fn
    from emrt_amd.config import get_config, update_config
    from emrt_amd.runtime import ctx, BF16
    from emrt_amd.src.models import get_model
    from emrt_amd.src.models.solver import PolynomialDecay, WarmupPolyLR
    cfg = update_config(get_config(), argparse.Namespace(cfg=os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml")))
    cfg.MODEL.ENCODER.TYPE = a.backbone
    torch.manual_seed(0)
    model = get_model(cfg)
    model.to_hip("cuda:0", BF16)
    st, c, L = model.store, ctx(), _lib.lib()
    n = st.n_train
    st.grad[:n].copy_(torch.randn(n, device="cuda") * 1e-3)
    moment2 = torch.zeros_like(st.velocity)
    clip_state = torch.tensor([1.0, 0.0], dtype=torch.float32, device="cuda")
    lr_dev = torch.zeros(1, dtype=torch.float32, device="cuda")
    ranges = (ctypes.c_longlong * (2 * len(st.lr_ranges)))(*[v for r in st.lr_ranges for v in r])
    rp, nr = ctypes.cast(ranges, ctypes.c_void_p), len(st.lr_ranges)
    poly = PolynomialDecay(0.01, 160000, 0.0, 0.9)
    d_poly = poly.descriptor()
    d_warm = WarmupPolyLR(6e-5, warmup_lr_init=1e-6, max_iters=160000, power=1.0, warmup_steps=1500).descriptor()
    sp = lambda d: ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    P = Fn.P
    launches = {
        "sgd": lambda: L.call("emrt_sgd_momentum_step", P(st.master), P(st.grad), P(st.velocity), n, P(clip_state), P(c.step_counter), poly.base_lr, poly.end_lr,
                              poly.power, poly.decay_steps, 0.9, 1e-4, rp, nr, st.lr_mult, P(lr_dev), P(st.mirror), st.dtype, c.stream),
        "sgd_sched": lambda: L.call("emrt_sgd_momentum_step_sched", P(st.master), P(st.grad), P(st.velocity), n, P(clip_state), P(c.step_counter), sp(d_poly),
                                    0.9, 1e-4, rp, nr, st.lr_mult, P(lr_dev), P(st.mirror), st.dtype, c.stream),
        "adamw": lambda: L.call("emrt_adamw_step", P(st.master), P(st.grad), P(st.velocity), P(moment2), n, P(clip_state), P(c.step_counter), sp(d_warm),
                                0.9, 0.999, 1e-8, 0.01, 1, rp, nr, st.lr_mult, P(lr_dev), P(st.mirror), st.dtype, c.stream),
        "adam": lambda: L.call("emrt_adamw_step", P(st.master), P(st.grad), P(st.velocity), P(moment2), n, None, P(c.step_counter), sp(d_warm),
                               0.9, 0.999, 1e-8, 1e-4, 0, rp, nr, st.lr_mult, P(lr_dev), P(st.mirror), st.dtype, c.stream),
    }
    for _ in range(a.warmup):
        for fn in launches.values():
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in launches}
    for _ in range(a.reps):          # alternated: every kind sees the same clocks, cache state and neighbours
        for k, fn in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(st.master[:n]).all())
    bytes_per = {"sgd": 22, "sgd_sched": 22, "adamw": 30, "adam": 30}
    res = {"device": torch.cuda.get_device_name(0), "backbone": a.backbone, "n_train": int(n), "reps": a.reps, "timer": "device events around each launch"}
    for k, pairs in evs.items():
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
        med = us[len(us) // 2]
        res[k] = {"median_us": round(med, 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2), "bytes_per_param": bytes_per[k],
                  "achieved_TBps": round(bytes_per[k] * n / med / 1e6, 3)}
    res["adamw_over_sgd"] = round(res["adamw"]["median_us"] / res["sgd"]["median_us"], 4)
    res["sgd_sched_over_sgd"] = round(res["sgd_sched"]["median_us"] / res["sgd"]["median_us"], 4)
    res["expected_from_bytes"] = round(30 / 22, 4)
    res["target"] = round(30 / 22 * 1.15, 4)
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
