"""`train.py --data scenes` against the other data paths: the two kernels of the device-side tile sampler timed with device
events, and the 400-step synchronised training comparison of DESIGN.md 13 with a third arm.

    python tools/bench_scenes.py [--iters 400] [--runs 2] [--scene 2048] [--scenes 4] [--skip-train] [--baseline-tree DIR] [--out FILE]

(a) kernel time: emrt_scene_draw + emrt_scene_sample for batch 8 at a 256^2 crop out of `--scenes` noise scenes of `--scene`^2, `--reps`
    fills between two device events after a warm-up, and emrt_scene_draw alone.  Launched from Python, so a figure near the launch cost is host
    issue time; `rocprofv3 --kernel-trace --stats` over this command gives the kernels alone (emrt_scene_draw_kernel, emrt_scene_sample_kernel).
(b) training: ResNet-50, batch 8, bf16, captured step, the Potsdam 256^2 yaml with DATA.NUM_WORKERS 4, `--iters` steps with --no-eval, for
    --data synthetic, --data dataset --device_transforms (a 256-tile 256^2 tree, tools/make_fake_potsdam.py) and --data scenes, alternated,
    `--runs` runs each, every run a fresh process.  TrainEngine.step is wrapped to synchronise the device before step 51 and after the last
    step: wall ms/step and tiles/s over that window.  --baseline-tree DIR (a built checkout of another commit, with a copy of this file under
    its tools/) adds a fourth arm: --data dataset --device_transforms run by THAT tree's code, in the same alternation.

Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CFG = os.path.join(ROOT, "emrt_amd/configs/EMRT/EMRT_256x256_160k_potsdam.yaml")
FIRST = 51          # the timed window starts at this step


def kernel_ms(root, batch, reps):
    import torch
    from emrt_amd import functional as Fn
    from emrt_amd.config import get_config, update_config
    from emrt_amd.runtime import F32, ctx
    from emrt_amd.src.datasets import SceneBank, SceneSampler
    from emrt_amd.src.transforms import get_transforms
    import ctypes
    cfg = update_config(get_config(), argparse.Namespace(cfg=CFG))
    ctx().init_device("cuda:0", F32)
    bank = SceneBank(root, "cuda:0")
    s = SceneSampler(bank, get_transforms(cfg), batch, 1234, 0)
    B, OH, OW = s.batch_shape
    images = torch.empty((B, 3, OH, OW), dtype=torch.float32, device="cuda:0")
    labels = torch.empty((B, OH, OW), dtype=torch.int64, device="cuda:0")
    c = ctx()
    scenes_dev, cum_dev, scenes_host, cum_host = bank.tables(*s.tile)

    def draw_only():
        Fn._L().call("emrt_scene_draw", Fn.P(c.step_counter), Fn.P(scenes_dev), Fn.P(cum_dev), ctypes.cast(scenes_host, ctypes.c_void_p),
                     ctypes.cast(cum_host, ctypes.c_void_p), len(bank), bank.nbytes, s.key, s.rank, B, s.tile[0], s.tile[1], OH, OW, s.flip_prob,
                     ctypes.cast(s._scale_hw, ctypes.c_void_p), len(s.scales), Fn.P(s.draws), c.stream)

    out = {}
    for name, fn in (("draw_and_sample", lambda: s.fill(images, labels)), ("draw", draw_only)):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(reps):
            if i % 8 == 0:
                c.step_counter.add_(1)      # other windows: the run does not time one cached set of tiles
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name + "_launch_event_ms"] = round(e0.elapsed_time(e1) / reps, 4)
    out.update(bank_bytes=bank.nbytes, scenes=len(bank), tile_origins=s.total_origins, batch=B, crop=[OH, OW],
               bytes_written_per_batch=B * OH * OW * (3 * 4 + 8))
    return out


def one_run(mode, iters, data_path, save_dir):
    """This process trains once; prints `[wall] steps 51..N: X ms/step, Y tiles/s`."""
    import torch
    from emrt_amd import engine, train
    step = engine.TrainEngine.step
    t = {}

    def timed(self, *a, **k):
        if self.calls + 1 == FIRST:
            torch.cuda.synchronize()
            t["t0"] = time.perf_counter()
        out = step(self, *a, **k)
        if self.calls == iters:
            torch.cuda.synchronize()
            t["t1"] = time.perf_counter()
        return out

    engine.TrainEngine.step = timed
    cfg = os.path.join(save_dir, "bench.yaml")
    with open(cfg, "w") as f:
        f.write('BASE: ["%s"]\nDATA: {NUM_WORKERS: 4}\nSAVE_FREQ_CHECKPOINT: 1000000\n' % os.path.relpath(CFG, save_dir))
    argv = ["--config", cfg, "--iters", str(iters), "--no-eval", "--save_dir", save_dir]
    argv += {"synthetic": ["--data", "synthetic"], "device_transforms": ["--data", "dataset", "--device_transforms", "--data_path", data_path],
             "scenes": ["--data", "scenes", "--data_path", data_path]}[mode]
    train.main(argv)
    ms = (t["t1"] - t["t0"]) * 1e3 / (iters - FIRST + 1)
    print("[wall] steps %d..%d: %.3f ms/step, %.1f tiles/s" % (FIRST, iters, ms, 8 / ms * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scene", type=int, default=2048)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)       # (child process: mode, data path, save dir)
    ap.add_argument("--data_path", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--save_dir", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one_run(a.one, a.iters, a.data_path, a.save_dir)
    from tools.make_fake_potsdam import make
    from tools.make_fake_scenes import main as make_scenes
    res = {"iters": a.iters, "window": [FIRST, a.iters], "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "cpu_affinity": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        scenes = os.path.join(tmp, "scenes")
        make_scenes([scenes, "--scenes", str(a.scenes), "--size", str(a.scene)])
        res["kernels"] = kernel_ms(scenes, 8, a.reps)
        print("[bench_scenes] kernels: %s" % json.dumps(res["kernels"]), file=sys.stderr, flush=True)
        if not a.skip_train:
            tiles = make(os.path.join(tmp, "p256"), n_train=256, n_val=1, size=256, seed=256)
            paths = {"synthetic": tiles, "device_transforms": tiles, "scenes": scenes}
            if a.baseline_tree:
                paths["device_transforms@baseline"] = tiles
            res["train"] = {m: {"ms_per_step": [], "tiles_per_s": [], "last_log": []} for m in paths}
            for run in range(a.runs):
                for mode in paths:          # alternated: run 1 of every mode, then run 2
                    save = os.path.join(tmp, "out_%s_%d" % (mode.replace("@", "_"), run))
                    os.makedirs(save)
                    tree = os.path.abspath(a.baseline_tree) if mode.endswith("@baseline") else ROOT
                    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_scenes.py"), "--one", mode.split("@")[0], "--iters", str(a.iters),
                                        "--data_path", paths[mode], "--save_dir", save], cwd=tree, capture_output=True, text=True, timeout=900,
                                       env=dict(os.environ, PYTHONPATH=tree))
                    if r.returncode != 0:
                        raise SystemExit("[bench_scenes] %s run %d failed (%d):\n%s" % (mode, run, r.returncode, (r.stdout + r.stderr)[-4000:]))
                    m = re.search(r"\[wall\] steps \d+\.\.\d+: ([\d.]+) ms/step, ([\d.]+) tiles/s", r.stdout)
                    res["train"][mode]["ms_per_step"].append(float(m.group(1)))
                    res["train"][mode]["tiles_per_s"].append(float(m.group(2)))
                    res["train"][mode]["last_log"].append(re.findall(r"\[TRAIN\].*", r.stdout)[-1])
                    print("[bench_scenes] %s run %d: %s" % (mode, run, m.group(0)), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
