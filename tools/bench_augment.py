"""RandomVerticalFlip + RandomDistort on the device: what the augment yaml costs `--data scenes` against the plain Potsdam yaml.

    python tools/bench_augment.py [--iters 400] [--runs 2] [--scene 2048] [--scenes 4] [--reps 200] [--skip-train] [--skip-profile] [--out FILE]

(a) loader: SceneSampler.fill for batch 8 at a 256^2 crop with augmentation off (emrt_scene_draw + emrt_scene_sample) and on (emrt_aug_scene_draw
    + emrt_aug_scene_sample: draw, memset, statistics, apply), `--reps` fills between two device events after a warm-up, alternated off / on.
    Launched from Python, so a figure near the launch cost is host issue time, not kernel time; (c) has the kernels alone.
(b) training: ResNet-50, batch 8, bf16, captured step, `--data scenes`, `--iters` steps with --no-eval under the Potsdam yaml (off) and the
    augment yaml (on), alternated, `--runs` runs each, every run a fresh process.  TrainEngine.step is wrapped to synchronise the device before
    step 51 and after the last step: wall ms/step over that window.  The on arm's extra time per step is the difference of the medians.
(c) kernels: ONE `rocprofv3 --kernel-trace --stats` run of this file's --fills mode (both arms, `--reps` fills each): the average duration of
    every augmentation kernel, and for the new ones the fraction of the HBM rate (--hbm-gbs, 6300 by default) their compulsory traffic
    amounts to: written bytes (fp32 image + int64 label) plus the source bytes of the tile for apply, the source bytes alone for statistics.

Prints one JSON object (and writes it to --out)."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CFG_DIR = os.path.join(ROOT, "emrt_amd/configs/EMRT")
CFGS = {"off": os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam.yaml"), "on": os.path.join(CFG_DIR, "EMRT_256x256_160k_potsdam_augment.yaml")}
FIRST = 51          # the timed window starts at this step
KERNELS = ("emrt_scene_draw_kernel", "emrt_scene_sample_kernel", "aug_scene_draw_kernel", "aug_stats_kernel", "aug_apply_kernel")


def _samplers(root, batch):
    import torch
    from emrt_amd.config import get_config, update_config
    from emrt_amd.runtime import F32, ctx
    from emrt_amd.src.datasets import SceneBank, SceneSampler
    from emrt_amd.src.transforms import get_transforms
    ctx().init_device("cuda:0", F32)
    bank = SceneBank(root, "cuda:0")
    out = {}
    for arm, path in CFGS.items():
        cfg = update_config(get_config(), argparse.Namespace(cfg=path))
        out[arm] = SceneSampler(bank, get_transforms(cfg), batch, 1234, 0)
    B, OH, OW = out["off"].batch_shape
    images = torch.empty((B, 3, OH, OW), dtype=torch.float32, device="cuda:0")
    labels = torch.empty((B, OH, OW), dtype=torch.int64, device="cuda:0")
    return bank, out, images, labels


def fills(root, batch, reps, rounds=3):
    """-> event-timed ms per fill, per arm, `rounds` alternated measurements each (this is also what runs under rocprofv3)."""
    import torch
    from emrt_amd.runtime import ctx
    bank, samplers, images, labels = _samplers(root, batch)
    c = ctx()
    res = {arm: [] for arm in samplers}
    for _ in range(rounds):
        for arm, s in samplers.items():
            for _ in range(10):
                s.fill(images, labels)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(reps):
                if i % 8 == 0:
                    c.step_counter.add_(1)      # other windows: the run does not time one cached set of tiles
                s.fill(images, labels)
            e1.record()
            torch.cuda.synchronize()
            res[arm].append(round(e0.elapsed_time(e1) / reps, 4))
    B, OH, OW = samplers["off"].batch_shape
    return {"fill_launch_event_ms": res, "tiles_per_s": {a: round(B / statistics.median(v) * 1e3, 1) for a, v in res.items()}, "batch": B,
            "crop": [OH, OW], "bank_bytes": bank.nbytes, "bytes_written_per_batch": B * OH * OW * (3 * 4 + 8)}


def profile(root, batch, reps, hbm_gbs):
    """One rocprofv3 --kernel-trace --stats run of `--fills` -> {kernel: {calls, avg_us, hbm_fraction}}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--fills", root,
               "--reps", str(reps)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("[bench_augment] the rocprofv3 run failed (%d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-4000:]))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("[bench_augment] rocprofv3 wrote no kernel_stats.csv under %s" % d)
        rows = [row for f in files for row in csv.DictReader(open(f))]
    npix, B = 256 * 256, batch
    # compulsory bytes per launch: apply writes 3 fp32 + 1 int64 per pixel and reads at least the 4 source bytes of a tile pixel (scale 1);
    # statistics reads the 3 image bytes and writes 8 bytes per block
    traffic = {"aug_apply_kernel": B * npix * (12 + 8 + 4), "aug_stats_kernel": B * npix * 3, "emrt_scene_sample_kernel": B * npix * (12 + 8 + 4)}
    out = {}
    for row in rows:
        name = row.get("Name", "")
        key = next((k for k in KERNELS if k in name), None)
        if key is None:
            continue
        calls, avg_ns = int(row["Calls"]), float(row["AverageNs"])
        e = {"calls": calls, "avg_us": round(avg_ns / 1e3, 3)}
        if key in traffic:
            e["compulsory_bytes"] = traffic[key]
            e["hbm_fraction"] = round(traffic[key] / (avg_ns * 1e-9) / (hbm_gbs * 1e9), 4)
        out[key] = e
    return out


def one_run(arm, iters, data_path, save_dir):
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
        f.write('BASE: ["%s"]\nSAVE_FREQ_CHECKPOINT: 1000000\n' % os.path.relpath(CFGS[arm], save_dir))
    train.main(["--config", cfg, "--iters", str(iters), "--no-eval", "--save_dir", save_dir, "--data", "scenes", "--data_path", data_path])
    ms = (t["t1"] - t["t0"]) * 1e3 / (iters - FIRST + 1)
    print("[wall] steps %d..%d: %.3f ms/step, %.1f tiles/s" % (FIRST, iters, ms, 8 / ms * 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scene", type=int, default=2048)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-profile", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fills", default=None, help=argparse.SUPPRESS)      # (child process, alone or under rocprofv3: scene tree)
    ap.add_argument("--rounds", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)        # (child process: arm)
    ap.add_argument("--data_path", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--save_dir", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.fills:
        print(json.dumps(fills(a.fills, 8, a.reps, rounds=a.rounds)))
        return
    if a.one:
        return one_run(a.one, a.iters, a.data_path, a.save_dir)
    from tools.make_fake_scenes import main as make_scenes
    res = {"iters": a.iters, "window": [FIRST, a.iters], "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "cpu_affinity": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        scenes = os.path.join(tmp, "scenes")
        make_scenes([scenes, "--scenes", str(a.scenes), "--size", str(a.scene)])
        # (a) in a process of its own: this one never opens the GPU, so every arm below starts from the same state
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fills", scenes, "--reps", str(a.reps), "--rounds", "3"], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("[bench_augment] the loader run failed (%d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-4000:]))
        res["loader"] = json.loads(r.stdout.strip().splitlines()[-1])
        print("[bench_augment] loader: %s" % json.dumps(res["loader"]), file=sys.stderr, flush=True)
        if not a.skip_profile:
            res["kernels"] = profile(scenes, 8, a.reps, a.hbm_gbs)
            print("[bench_augment] kernels: %s" % json.dumps(res["kernels"]), file=sys.stderr, flush=True)
        if not a.skip_train:
            res["train"] = {arm: {"ms_per_step": [], "tiles_per_s": [], "last_log": []} for arm in CFGS}
            for run in range(a.runs):
                for arm in CFGS:            # alternated: run 1 of both arms, then run 2
                    save = os.path.join(tmp, "out_%s_%d" % (arm, run))
                    os.makedirs(save)
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", arm, "--iters", str(a.iters), "--data_path", scenes,
                                        "--save_dir", save], cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=ROOT))
                    if r.returncode != 0:
                        raise SystemExit("[bench_augment] %s run %d failed (%d):\n%s" % (arm, run, r.returncode, (r.stdout + r.stderr)[-4000:]))
                    m = re.search(r"\[wall\] steps \d+\.\.\d+: ([\d.]+) ms/step, ([\d.]+) tiles/s", r.stdout)
                    res["train"][arm]["ms_per_step"].append(float(m.group(1)))
                    res["train"][arm]["tiles_per_s"].append(float(m.group(2)))
                    res["train"][arm]["last_log"].append(re.findall(r"\[TRAIN\].*", r.stdout)[-1])
                    print("[bench_augment] %s run %d: %s" % (arm, run, m.group(0)), file=sys.stderr, flush=True)
            off, on = (statistics.median(res["train"][arm]["ms_per_step"]) for arm in ("off", "on"))
            res["train"]["on_minus_off_ms_per_step"] = round(on - off, 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
