"""Timing of the resnext50 backbone's grouped convolution and of the EMRT-resnext50 training step.

  (a) emrt_gconv2d forward and emrt_gconv2d_bwd (data gradient, weight gradient) at the four stage shapes of a batch-8 256 x 256 step, bf16 and
      fp32: microseconds per launch (device events around `--reps` launches after warm-up) and the fraction of 8 TB/s that the bytes of x + y + w
      (forward), dy + dx + w (data gradient) and x + dy (weight gradient, + the fp32 dW) would take at that rate.
  (b) the training step of EMRT-resnext50 at 8 x 256^2 through bench.py's engine path (TrainEngine, captured hipGraph, bf16), in tiles/s, and
      the fp32 step (eager).

    python tools/bench_resnext.py [--part a|b|ab] [--reps 50] [--steps 20] [--warmup 5] [--json out.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM = 8.0e12
# (name, N, H, W, C, stride): the 16 grouped layers of a step are 3 + 4 + 6 + 3 of these shapes, the first of stages 2-4 strided
SHAPES = [("s1", 8, 64, 64, 256, 1), ("s2", 8, 32, 32, 512, 1), ("s2-first", 8, 64, 64, 512, 2), ("s3", 8, 16, 16, 1024, 1),
          ("s3-first", 8, 32, 32, 1024, 2), ("s4", 8, 8, 8, 2048, 1), ("s4-first", 8, 16, 16, 2048, 2)]


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _time(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def part_a(reps):
    from emrt_amd import _lib
    from emrt_amd.runtime import ctx, F32, BF16
    c = ctx()
    c.init_device("cuda:0", BF16, 0)
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for dtype, td, esz in ((BF16, torch.bfloat16, 2), (F32, torch.float32, 4)):
        for name, N, H, W, C, s in SHAPES:
            groups, cg = 64, C // 64
            OH, OW = (H - 1) // s + 1, (W - 1) // s + 1
            x = torch.randn(N, H, W, C, device="cuda").to(td)
            w = (torch.randn(C, 3, 3, cg, device="cuda") * 0.1).to(td)
            y = torch.empty(N, OH, OW, C, device="cuda", dtype=td)
            dy = torch.randn(N, OH, OW, C, device="cuda").to(td)
            dx = torch.empty_like(x)
            dw = torch.zeros(C * 9 * cg, device="cuda")
            stats = torch.zeros(16 * C, dtype=torch.float64, device="cuda")
            fwd = lambda: L.call("emrt_gconv2d", _P(x), _P(w), _P(y), None, N, H, W, C, C, H * W * C, OH, OW, C, C, OH * OW * C, s, groups, 0, _P(stats),
                                 None, dtype, ctypes.c_void_p(st))
            dgrad = lambda: L.call("emrt_gconv2d_bwd", _P(x), _P(dy), _P(w), _P(dx), C, H * W * C, 0, None, None, N, H, W, C, C, H * W * C, OH, OW, C, C,
                                   OH * OW * C, s, groups, dtype, ctypes.c_void_p(st))
            wgrad = lambda: L.call("emrt_gconv2d_bwd", _P(x), _P(dy), _P(w), None, 0, 0, 0, _P(dw), None, N, H, W, C, C, H * W * C, OH, OW, C, C,
                                   OH * OW * C, s, groups, dtype, ctypes.c_void_p(st))
            t_f, t_d, t_w = _time(fwd, reps), _time(dgrad, reps), _time(wgrad, reps)
            xb, yb, wb = N * H * W * C * esz, N * OH * OW * C * esz, C * 9 * cg * esz
            row = dict(dtype="bf16" if dtype == BF16 else "fp32", shape=name, fwd_us=round(t_f, 2), dgrad_us=round(t_d, 2), wgrad_us=round(t_w, 2),
                       bwd_us=round(t_d + t_w, 2), fwd_hbm=round((xb + yb + wb) / HBM * 1e6 / t_f, 3), dgrad_hbm=round((xb + yb + wb) / HBM * 1e6 / t_d, 3),
                       wgrad_hbm=round((xb + yb + C * 9 * cg * 4) / HBM * 1e6 / t_w, 3), gflop=round(2.0 * N * OH * OW * C * 9 * cg / 1e9, 3))
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def part_b(steps, warmup):
    from emrt_amd.config import get_config, update_config
    from emrt_amd.engine import TrainEngine
    from emrt_amd.runtime import F32, BF16
    from emrt_amd.src.models import get_model
    from emrt_amd.src.models.losses import get_loss_function
    from emrt_amd.src.models.solver import get_optimizer, get_scheduler
    cfg = update_config(get_config(), argparse.Namespace(cfg=os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml")))
    cfg.MODEL.ENCODER.TYPE = "resnext50"
    B, S = 8, 256
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, 3, S, S, generator=g).cuda()
    lab = torch.randint(0, 6, (B, S, S), generator=g).cuda()
    out = []
    for dtype, graph in ((BF16, True), (F32, False)):
        torch.manual_seed(0)
        model = get_model(cfg)
        model.to_hip("cuda:0", dtype)
        model.eval()
        model(x)
        model.train()
        eng = TrainEngine(model, get_optimizer(model, get_scheduler(cfg), cfg), get_loss_function(cfg), 1, use_graph=graph)
        for _ in range(warmup):
            eng.step(x, lab)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = eng.step(x, lab)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        row = dict(step="bf16-captured" if dtype == BF16 else "fp32-eager", batch=B, size=S, ms_per_step=round(dt * 1e3, 3),
                   tiles_per_s=round(B / dt, 1), loss=round(float(loss.item()), 4))
        print(json.dumps(row), flush=True)
        out.append(row)
        del eng, model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {}
    if "a" in a.part:
        res["kernels"] = part_a(a.reps)
    if "b" in a.part:
        res["steps"] = part_b(a.steps, a.warmup)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
