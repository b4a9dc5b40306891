"""Loss-pass timing: forward + backward of MixSoftmaxCrossEntropyLoss (emrt_softmax_ce_pair_*), its class-weighted form (emrt_wce_pair_*) and
OhemCrossEntropyLoss on two heads (emrt_ohem_ce_pair_fwd / _bwd) and DiceCrossEntropyLoss (emrt_lx_dice_ce_pair_*, the fourth library) at the
two training shapes, 8 x 6 x 256 x 256 and 4 x 7 x 512 x 512.

    python tools/bench_loss.py [--reps 30] [--inner 20] [--json profiles/loss_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_loss.py --reps 3 ; python tools/bench_loss.py --stats-csv OUT/.../*_kernel_stats.csv

Every variant is captured into a hipGraph holding `inner` forward + backward passes, as the training step runs it (one captured graph: no
host time between launches), and the graphs are replayed alternately with a device-event pair around each replay; the figure is the
median replay over `inner`.  The launch count is the number of GPU launches of one pass (kernels + the OHEM forward's memset node), counted
from the entry points' definitions.  --stats-csv reads a rocprofv3 kernel-stats file of a run of this tool and prints the share of the OHEM
kernels' time spent in the selection (digit histograms 2 and 3 and the three scans; the first digit's histogram is part of the pass that
computes p and is not separable).  Needs a GPU: there is no CPU path."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8, 6, 256, 256), (4, 7, 512, 512)]
# GPU launches of one forward + backward pass (csrc/loss.hip; dice: csrc/loss_ext/loss_ext.hip)
LAUNCHES = {"mix": 2 + 1, "weighted_mix": 2 + 1, "ohem": 9 + 1, "dice": 2 + 1}


def selection_share(path):
    sel = tot = 0.0
    rows = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            if "ohem_" not in name:
                continue
            rows[name] = ns
            tot += ns
            if "ohem_hist_kernel" in name or "ohem_scan_kernel" in name:
                sel += ns
    out = {"ohem_kernel_ns": rows, "selection_share_of_ohem_kernel_time": round(sel / tot, 4) if tot else None}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--stats-csv", default=None)
    a = ap.parse_args()
    if a.stats_csv is not None:
        selection_share(a.stats_csv)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss needs a GPU")
    from emrt_amd.runtime import ctx, F32, Tape
    from emrt_amd.src.models.losses import DiceCrossEntropyLoss, MixSoftmaxCrossEntropyLoss, OhemCrossEntropyLoss
    c = ctx()
    c.init_device("cuda:0", F32, 0)
    c.training = True

    class Out(tuple):
        tape = None

    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "inner": a.inner,
           "timer": "device events around one replay of a hipGraph of `inner` forward + backward passes, median / inner", "shapes": {}}
    for N, C, H, W in SHAPES:
        g = torch.Generator().manual_seed(N * W)
        labels = torch.randint(0, C, (N, H, W), generator=g)
        # confident logits, as a trained network's; 0 < min_kept < num_valid: all three digit passes of the selection run
        la = (torch.randn(N, C, H, W, generator=g) + 4 * torch.nn.functional.one_hot(labels, C).permute(0, 3, 1, 2).float()).cuda()
        lb = (torch.randn(N, C, H, W, generator=g) + 3 * torch.nn.functional.one_hot(labels, C).permute(0, 3, 1, 2).float()).cuda()
        labels[torch.rand(N, H, W, generator=g) < 0.05] = 255
        lab = labels.cuda()
        npix = N * H * W
        c.workspace(64 << 20)
        fns = {"mix": MixSoftmaxCrossEntropyLoss(ignore_index=255, aux=True, aux_weight=0.4),
               "weighted_mix": MixSoftmaxCrossEntropyLoss(ignore_index=255, aux=True, aux_weight=0.4, class_weights=[1.0 + 0.25 * i for i in range(C)]),
               "ohem": OhemCrossEntropyLoss(thresh=0.7, min_kept=npix // 8, ignore_index=255, aux=True, aux_weight=0.4),
               "dice": DiceCrossEntropyLoss(ce_weight=1.0, dice_weight=1.0, smooth=1.0, ignore_index=255, aux=True, aux_weight=0.4)}

        def one_pass(fn):
            out = Out((la, lb))
            out.tape = Tape()
            loss = fn(out, lab)
            loss.backward()
            return loss

        graphs, info = {}, {}
        for k, fn in fns.items():
            for _ in range(a.warmup):
                loss = one_pass(fn)
            torch.cuda.synchronize()
            info[k] = {"loss": round(loss.item(), 6)}
            if k == "dice":
                info[k]["ce"] = [round(p[1].item(), 6) for p in loss.parts]
                info[k]["dice"] = [round(p[2].item(), 6) for p in loss.parts]
            if k == "ohem":
                info[k]["kept"] = [int(p[1].item()) for p in loss.parts]
                info[k]["threshold"] = [round(p[2].item(), 6) for p in loss.parts]
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):          # (temporaries come from the graph's own pool and live as long as the graph)
                for _ in range(a.inner):
                    one_pass(fn)
            graphs[k] = gr
            gr.replay()
        torch.cuda.synchronize()
        evs = {k: [] for k in graphs}
        for _ in range(a.reps):          # alternated: every variant sees the same clocks and neighbours
            for k, gr in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                evs[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {}
        for k, pairs in evs.items():
            us = sorted(e0.elapsed_time(e1) * 1e3 / a.inner for e0, e1 in pairs)
            row[k] = dict(info[k], median_us=round(us[len(us) // 2], 2), min_us=round(us[0], 2), max_us=round(us[-1], 2), launches=LAUNCHES[k])
        row["weighted_over_mix"] = round(row["weighted_mix"]["median_us"] / row["mix"]["median_us"], 3)
        row["ohem_over_mix"] = round(row["ohem"]["median_us"] / row["mix"]["median_us"], 3)
        row["ohem_minus_mix_us"] = round(row["ohem"]["median_us"] - row["mix"]["median_us"], 2)
        row["dice_over_mix"] = round(row["dice"]["median_us"] / row["mix"]["median_us"], 3)
        row["dice_minus_mix_us"] = round(row["dice"]["median_us"] - row["mix"]["median_us"], 2)
        res["shapes"]["%dx%dx%dx%d" % (N, C, H, W)] = row
    print(json.dumps(res), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
