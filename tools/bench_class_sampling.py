"""Class-aware tile sampling (DATA.SCENE_SAMPLING) against uniform origins: what the extra launch costs a training step, what the
index costs to build, and what it does to the share of a rare class in the batches.

    python tools/bench_class_sampling.py [--iters 400] [--runs 2] [--scene 2048] [--scenes 4] [--rare-share 0.01] [--baseline-tree DIR] [--out FILE]

(a) training: ResNet-50, batch 8, bf16, captured step, the Potsdam 256^2 yaml, `--iters` steps of --data scenes with --no-eval on `--scenes`
    noise scenes of `--scene`^2 in which class 5 covers `--rare-share` of the pixels (tools/make_fake_scenes.py).  Arms, alternated, `--runs` runs
    each, every run a fresh process: "uniform" (this tree, the default node), "class" (MODE class, PROB 0.5) and, with --baseline-tree DIR (a built
    checkout of another commit), "uniform@baseline": the same --data scenes run by THAT tree's tools/bench_scenes.py.  TrainEngine.step is wrapped
    to synchronise the device before step 51 and after the last step: wall ms/step over that window (the clock of tools/bench_scenes.py).
    Acceptance: |mean(uniform) - mean(uniform@baseline)| <= spread(uniform) + spread(uniform@baseline), spread = max - min of an arm's runs.
(b) index: SceneBank.class_index on that bank, the counting launch between two device events (read back and prefix sums excluded), first call
    and a repeat on a fresh bank.
(c) effect: `--iters` fills of the sampler alone per mode, same seed and step counters as the training runs, the labels counted on the device:
    the rare class's share of the non-ignored label pixels, over all batches and its smallest / largest per batch.

Prints one JSON object (and writes it to --out, default profiles/class_sampling_bench.json)."""
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
RARE = 5
CLASS_NODE = "{MODE: class, PROB: 0.5, TEMPERATURE: 0.1, CLASS_PROBS: None}"


def one_run(mode, iters, data_path, save_dir):
    """This process trains once; prints `[wall] steps 51..N: X ms/step, Y tiles/s` (the line of tools/bench_scenes.py)."""
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
        f.write('BASE: ["%s"]\nDATA: {NUM_WORKERS: 4%s}\nSAVE_FREQ_CHECKPOINT: 1000000\n' % (
            os.path.relpath(CFG, save_dir), ", SCENE_SAMPLING: " + CLASS_NODE if mode == "class" else ""))
    train.main(["--config", cfg, "--iters", str(iters), "--no-eval", "--save_dir", save_dir, "--data", "scenes", "--data_path", data_path])
    ms = (t["t1"] - t["t0"]) * 1e3 / (iters - FIRST + 1)
    print("[wall] steps %d..%d: %.3f ms/step, %.1f tiles/s" % (FIRST, iters, ms, 8 / ms * 1e3), flush=True)


def index_and_effect(root, iters, batch=8, seed=1234):          # (train.py's default --seed)
    """(b) and (c) of the module text, in this process."""
    import torch
    from emrt_amd.config import get_config, update_config
    from emrt_amd.runtime import F32, ctx
    from emrt_amd.src.datasets import SceneBank, SceneSampler
    from emrt_amd.src.transforms import get_transforms
    cfg = update_config(get_config(), argparse.Namespace(cfg=CFG))
    ctx().init_device("cuda:0", F32)
    out = {"index_build_event_ms": [SceneBank(root, "cuda:0").class_index(cfg.DATA.NUM_CLASSES).build_ms for _ in range(2)]}
    bank = SceneBank(root, "cuda:0")
    idx = bank.class_index(cfg.DATA.NUM_CLASSES)
    out.update(rows=int(idx.counts.shape[0]), index_bytes_on_device=int(idx.cum.nbytes + idx.row_start.nbytes),
               bank_share_of_rare_class=float(idx.totals[RARE]) / float(idx.totals.sum()))
    for mode in ("uniform", "class"):
        node = dict(cfg.DATA.SCENE_SAMPLING, MODE=mode)
        s = SceneSampler(bank, get_transforms(cfg), batch, seed, 0, sampling=node, num_classes=cfg.DATA.NUM_CLASSES)
        B, OH, OW = s.batch_shape
        images = torch.empty((B, 3, OH, OW), dtype=torch.float32, device="cuda:0")
        labels = torch.empty((B, OH, OW), dtype=torch.int64, device="cuda:0")
        per_batch = torch.zeros((iters, 2), dtype=torch.int64, device="cuda:0")
        ctx().step_counter.zero_()
        for i in range(iters):
            s.fill(images, labels)
            per_batch[i, 0] = (labels == RARE).sum()
            per_batch[i, 1] = (labels != 255).sum()
            ctx().step_counter.add_(1)
        pb = per_batch.cpu().double()
        share = pb[:, 0] / pb[:, 1].clamp(min=1)
        out["rare_share_" + mode] = {"over_all_batches": float(pb[:, 0].sum() / pb[:, 1].sum()), "smallest_batch": float(share.min()),
                                     "largest_batch": float(share.max()), "batches_without_a_rare_pixel": int((pb[:, 0] == 0).sum())}
        if s.class_mode:
            out["class_table"] = [[n, round(a, 6), round(b, 6)] for n, a, b in s.class_table]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--scene", type=int, default=2048)
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--rare-share", type=float, default=0.01)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_sampling_bench.json"))
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)       # (child process: mode, data path, save dir)
    ap.add_argument("--data_path", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--save_dir", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one_run(a.one, a.iters, a.data_path, a.save_dir)
    from tools.make_fake_scenes import main as make_scenes
    res = {"iters": a.iters, "window": [FIRST, a.iters], "bank": {"scenes": a.scenes, "side": a.scene, "rare_class": RARE, "rare_share": a.rare_share},
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "cpu_affinity": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as tmp:
        scenes = os.path.join(tmp, "scenes")
        make_scenes([scenes, "--scenes", str(a.scenes), "--size", str(a.scene), "--rare-share", str(a.rare_share), "--rare-class", str(RARE)])
        arms = (["uniform@baseline"] if a.baseline_tree else []) + ["uniform", "class"]
        if not a.skip_train:
            res["train"] = {m: {"ms_per_step": [], "last_log": []} for m in arms}
            for run in range(a.runs):
                for arm in arms:          # alternated: run 1 of every arm, then run 2
                    save = os.path.join(tmp, "out_%s_%d" % (arm.replace("@", "_"), run))
                    os.makedirs(save)
                    if arm.endswith("@baseline"):
                        tree = os.path.abspath(a.baseline_tree)
                        cmd = [sys.executable, os.path.join(tree, "tools", "bench_scenes.py"), "--one", "scenes"]
                    else:
                        tree = ROOT
                        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_class_sampling.py"), "--one", arm]
                    r = subprocess.run(cmd + ["--iters", str(a.iters), "--data_path", scenes, "--save_dir", save], cwd=tree, capture_output=True,
                                       text=True, timeout=900, env=dict(os.environ, PYTHONPATH=tree))
                    if r.returncode != 0:
                        raise SystemExit("[bench_class_sampling] %s run %d failed (%d):\n%s" % (arm, run, r.returncode, (r.stdout + r.stderr)[-4000:]))
                    m = re.search(r"\[wall\] steps \d+\.\.\d+: ([\d.]+) ms/step", r.stdout)
                    res["train"][arm]["ms_per_step"].append(float(m.group(1)))
                    res["train"][arm]["last_log"].append(re.findall(r"\[TRAIN\].*", r.stdout)[-1])
                    print("[bench_class_sampling] %s run %d: %s" % (arm, run, m.group(0)), file=sys.stderr, flush=True)
            for v in res["train"].values():
                v["mean"], v["spread"] = sum(v["ms_per_step"]) / len(v["ms_per_step"]), max(v["ms_per_step"]) - min(v["ms_per_step"])
            if a.baseline_tree:
                u, b = res["train"]["uniform"], res["train"]["uniform@baseline"]
                res["uniform_within_spread_of_baseline"] = abs(u["mean"] - b["mean"]) <= u["spread"] + b["spread"]
        res.update(index_and_effect(scenes, a.iters))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
