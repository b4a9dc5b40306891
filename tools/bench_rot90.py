"""RandomRot90 on the device: what the d4 yaml costs `--data scenes` against the augment yaml, and what the post-pass kernel does.

    python tools/bench_rot90.py [--iters 400] [--runs 2] [--scene 2048] [--scenes 4] [--reps 200] [--baseline-tree DIR] [--skip-train]
                                [--skip-profile] [--out FILE]

(a) training: ResNet-50, batch 8, bf16, captured step, 256^2, `--data scenes` from `--scenes` noise scenes of `--scene`^2, `--iters` steps with
    --no-eval under the augment yaml (off) and the d4 yaml (on: the same chain plus ROT90_PROB 0.75), alternated, `--runs` runs each, every run a
    fresh process.  TrainEngine.step is wrapped to synchronise the device before step 51 and after the last step: wall ms/step over that window.
    The on arm's extra time per step is the difference of the medians.  With --baseline-tree (a built checkout of the parent commit) the off arm
    of THAT tree runs in the same alternation: the default key launches nothing new, so the two off arms differ by run-to-run scatter only.
(b) kernels: ONE `rocprofv3 --kernel-trace --stats` run of this file's --fills mode (`--reps` fills of the on arm's sampler, the step counter
    moved every 8 fills): the average duration of rot_turn_kernel with aug_apply_kernel of the same trace beside it as the yardstick.  The turn's
    compulsory traffic is 2 x 20 bytes (3 fp32 + 1 int64, read and written) per pixel of every TURNED sample; the number of turned samples per
    fill is read back from the sampler's turns, so the fraction of the HBM rate (--hbm-gbs, 6300 by default) is that of the fills measured.

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
FIRST = 51          # the timed window starts at this step
YAMLS = {"off": "EMRT_256x256_160k_potsdam_augment.yaml", "on": "EMRT_256x256_160k_potsdam_d4.yaml"}
KERNELS = ("rot_turn_kernel", "aug_apply_kernel", "aug_stats_kernel", "aug_scene_draw_kernel")


def _cfg(tree, arm):
    return os.path.join(tree, "emrt_amd/configs/EMRT", YAMLS[arm])


def fills(root, batch, reps):
    """`reps` fills of the on arm's sampler between two device events (this is what runs under rocprofv3) -> ms per fill and the turned samples."""
    import torch
    from emrt_amd.config import get_config, update_config
    from emrt_amd.runtime import F32, ctx
    from emrt_amd.src.datasets import SceneBank, SceneSampler
    from emrt_amd.src.transforms import get_transforms
    ctx().init_device("cuda:0", F32)
    c = ctx()
    s = SceneSampler(SceneBank(root, "cuda:0"), get_transforms(update_config(get_config(), argparse.Namespace(cfg=_cfg(ROOT, "on")))), batch, 1234, 0)
    B, OH, OW = s.batch_shape
    images = torch.empty((B, 3, OH, OW), dtype=torch.float32, device="cuda:0")
    labels = torch.empty((B, OH, OW), dtype=torch.int64, device="cuda:0")
    for _ in range(10):
        s.fill(images, labels)
    turned = torch.zeros((), dtype=torch.int64, device="cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        if i % 8 == 0:
            c.step_counter.add_(1)      # other windows and other turns: the run does not time one cached batch
        s.fill(images, labels)
        turned += (s.turns != 0).sum()
    e1.record()
    torch.cuda.synchronize()
    return {"fill_event_ms": round(e0.elapsed_time(e1) / reps, 4), "fills": reps + 10, "timed_fills": reps, "batch": B, "crop": [OH, OW],
            "turned_samples_in_timed_fills": int(turned.item())}


def profile(root, batch, reps, hbm_gbs):
    """One rocprofv3 --kernel-trace --stats run of `--fills` -> {kernel: {calls, avg_us, ...}}."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--fills", root,
               "--reps", str(reps)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit("[bench_rot90] the rocprofv3 run failed (%d):\n%s" % (r.returncode, (r.stdout + r.stderr)[-4000:]))
        run = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("[bench_rot90] rocprofv3 wrote no kernel_stats.csv under %s" % d)
        rows = [row for f in files for row in csv.DictReader(open(f))]
    npix, B = run["crop"][0] * run["crop"][1], run["batch"]
    # the warm-up fills sit at one step: their turned share is taken to be the timed fills' (the average over launches is what the trace gives)
    turned_per_fill = run["turned_samples_in_timed_fills"] / run["timed_fills"]
    traffic = {"rot_turn_kernel": turned_per_fill * npix * 2 * 20, "aug_apply_kernel": B * npix * (12 + 8 + 4)}
    out = {"fills": run}
    for row in rows:
        key = next((k for k in KERNELS if k in row.get("Name", "")), None)
        if key is None:
            continue
        avg_ns = float(row["AverageNs"])
        e = {"calls": int(row["Calls"]), "avg_us": round(avg_ns / 1e3, 3)}
        if key in traffic:
            e["compulsory_bytes"] = int(traffic[key])
            e["hbm_fraction"] = round(traffic[key] / (avg_ns * 1e-9) / (hbm_gbs * 1e9), 4)
        out[key] = e
    if "rot_turn_kernel" in out:
        out["rot_turn_kernel"]["turned_samples_per_fill"] = round(turned_per_fill, 3)
    return out


def one_run(tree, arm, iters, data_path, save_dir):
    """This process trains once from `tree`; prints `[wall] steps 51..N: X ms/step, Y tiles/s`."""
    import torch
    from emrt_amd import engine, train
    assert os.path.abspath(os.path.dirname(os.path.dirname(engine.__file__))) == os.path.abspath(tree), (engine.__file__, tree)
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
        f.write('BASE: ["%s"]\nSAVE_FREQ_CHECKPOINT: 1000000\n' % os.path.relpath(_cfg(tree, arm), save_dir))
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
    ap.add_argument("--baseline-tree", default=None, help="a built checkout of the parent commit: its off arm is timed in the same alternation")
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--skip-profile", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fills", default=None, help=argparse.SUPPRESS)      # (child process, under rocprofv3: scene tree)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)        # (child process: arm)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)       # (child process: the checkout it imports emrt_amd from)
    ap.add_argument("--data_path", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--save_dir", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    if a.fills:
        print(json.dumps(fills(a.fills, 8, a.reps)))
        return
    if a.one:
        return one_run(tree, a.one, a.iters, a.data_path, a.save_dir)
    from tools.make_fake_scenes import main as make_scenes
    res = {"iters": a.iters, "window": [FIRST, a.iters], "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "cpu_affinity": len(os.sched_getaffinity(0))}
    arms = [("off", ROOT, "off"), ("on", ROOT, "on")]
    if a.baseline_tree:
        arms.insert(0, ("parent_off", os.path.abspath(a.baseline_tree), "off"))
    with tempfile.TemporaryDirectory() as tmp:
        scenes = os.path.join(tmp, "scenes")
        make_scenes([scenes, "--scenes", str(a.scenes), "--size", str(a.scene)])
        if not a.skip_profile:
            res["kernels"] = profile(scenes, 8, a.reps, a.hbm_gbs)
            print("[bench_rot90] kernels: %s" % json.dumps(res["kernels"]), file=sys.stderr, flush=True)
        if not a.skip_train:
            res["train"] = {name: {"ms_per_step": [], "tiles_per_s": [], "last_log": []} for name, _, _ in arms}
            for run in range(a.runs):
                for name, src, arm in arms:            # alternated: run 1 of every arm, then run 2
                    save = os.path.join(tmp, "out_%s_%d" % (name, run))
                    os.makedirs(save)
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", arm, "--tree", src, "--iters", str(a.iters), "--data_path", scenes,
                                        "--save_dir", save], cwd=src, capture_output=True, text=True, timeout=900, env=dict(os.environ, PYTHONPATH=src))
                    if r.returncode != 0:
                        raise SystemExit("[bench_rot90] %s run %d failed (%d):\n%s" % (name, run, r.returncode, (r.stdout + r.stderr)[-4000:]))
                    m = re.search(r"\[wall\] steps \d+\.\.\d+: ([\d.]+) ms/step, ([\d.]+) tiles/s", r.stdout)
                    res["train"][name]["ms_per_step"].append(float(m.group(1)))
                    res["train"][name]["tiles_per_s"].append(float(m.group(2)))
                    res["train"][name]["last_log"].append(re.findall(r"\[TRAIN\].*", r.stdout)[-1])
                    print("[bench_rot90] %s run %d: %s" % (name, run, m.group(0)), file=sys.stderr, flush=True)
            med = {name: statistics.median(v["ms_per_step"]) for name, v in res["train"].items()}
            res["train"]["on_minus_off_ms_per_step"] = round(med["on"] - med["off"], 4)
            if "parent_off" in med:
                res["train"]["off_minus_parent_off_ms_per_step"] = round(med["off"] - med["parent_off"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
