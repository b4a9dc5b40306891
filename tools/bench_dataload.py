"""Training-loader throughput: the CPU TileLoader (transforms in the reader threads) against DeviceTileLoader (reader threads only decode;
the transforms run as one emrt_augment_tiles launch per batch), on seeded Potsdam-layout trees (tools/make_fake_potsdam.py) of 256^2 and
512^2 sources, the Potsdam training chain with a 256^2 crop, at 1, 2 and 4 reader threads.  Each figure is tiles per second over `--batches`
batches after `--warmup`, timed to a device synchronise.  Prints one JSON object (and writes it to --out).

    python tools/bench_dataload.py [--batch 8] [--batches 40] [--warmup 4] [--workers 1 2 4] [--sizes 256 512] [--out FILE]

Kernel time: run the same command under `rocprofv3 --kernel-trace --stats` (kernel emrt_augment_kernel)."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def rate(cls, ds, workers, batch, warmup, batches):
    import torch
    from emrt_amd.distributed import DistributedTileSampler
    gen = cls(ds, DistributedTileSampler(len(ds), batch, 0, 1, shuffle=True, seed=0), "cuda:0", workers=workers, prefetch=4).epochs()
    for _ in range(warmup):
        next(gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        x, y = next(gen)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    gen.close()
    return batches * batch / dt


def kernel_ms(ds, batch, reps=50):
    """Device-event time of one staged batch's emrt_augment_kernel launch (includes the launch; rocprofv3 gives the kernel alone)."""
    import torch
    from emrt_amd import functional as F
    from emrt_amd.src.datasets import DeviceTileLoader
    from emrt_amd.distributed import DistributedTileSampler
    ld = DeviceTileLoader(ds, DistributedTileSampler(len(ds), batch, 0, 1), "cuda:0", workers=1)
    buf, samples, size = ld._batch(ld._plan(list(range(batch))))
    src = buf.cuda()
    dp = ld.device_plan
    args = (src, samples, size, dp.mean, dp.stdinv, dp.img_pad, dp.label_pad, ld.lut)
    for _ in range(5):
        F.augment_tiles(*args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        F.augment_tiles(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from emrt_amd.config import get_config, update_config
    from emrt_amd.src.datasets import DeviceTileLoader, TileLoader, get_dataset
    from emrt_amd.src.transforms import get_transforms
    from tools.make_fake_potsdam import make
    torch.zeros(1, device="cuda:0")
    res = {"batch": a.batch, "batches": a.batches, "crop": [256, 256], "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "cpu_affinity": len(os.sched_getaffinity(0)), "tiles_per_s": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for size in a.sizes:
            root = make(os.path.join(tmp, "p%d" % size), n_train=a.tiles, n_val=1, size=size, seed=size)
            cfg = update_config(get_config(), argparse.Namespace(cfg=os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml")))
            cfg.DATA.DATA_PATH = root
            ds = get_dataset(cfg, get_transforms(cfg), "train")
            r = res["tiles_per_s"]["%d" % size] = {}
            for name, cls in (("cpu", TileLoader), ("device", DeviceTileLoader)):
                for w in a.workers:
                    # the CPU loader at 512^2 is ~30 tiles/s per thread: fewer batches keep it to seconds
                    nb = a.batches if name == "device" else max(4, a.batches // (4 if size > 256 else 2))
                    r["%s_w%d" % (name, w)] = round(rate(cls, ds, w, a.batch, a.warmup, nb), 1)
                    print("[bench_dataload] %d^2 %s workers=%d: %.1f tiles/s" % (size, name, w, r["%s_w%d" % (name, w)]), file=sys.stderr, flush=True)
            ms = kernel_ms(ds, a.batch)
            res.setdefault("augment_launch_event_ms", {})["%d" % size] = round(ms, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
