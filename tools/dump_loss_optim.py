"""Every output of the loss and optimizer entry points on a fixed list of cases, as one comparable file (developer tool, needs a GPU).

usage: PYTHONPATH=<checkout under test> python tools/dump_loss_optim.py --out FILE [--only loss|optim] [--raw]

The library of the checkout that PYTHONPATH names (this one without it) runs the 12 loss entry points (emrt_softmax_ce_*, emrt_wce_*,
emrt_ohem_ce_*), emrt_grad_clip_scale and the 3 optimizer entry points through emrt_amd._lib alone, so checkouts with the same C-ABI can be
compared: a refactor of the kernels leaves the file byte-identical (cmp).  Inputs come from seeded CPU generators.

FILE holds, case after case and output after output in a fixed order, the raw bytes of every output of at most RAW_LIMIT bytes and the
SHA-256 of the raw bytes of every larger one (the full cross product of the optimizer cases at the two-stride size alone is 33 GB of raw
output, and hashed files can be kept and copied); --raw writes every output as raw bytes, so that cmp -l on two such files says where a
mismatch lies (--only and a large disk go with it).  The last line printed is a JSON record: cases, outputs, the raw bytes the file
stands for, the bytes of the file.

Loss cases, (N, C, H, W): (1,3,1,5) less than a wave; (3,6,16,20) a partly filled last block, 10 % ignored; (4,7,24,40) 15 full blocks, odd
C, 15 % ignored; (3,6,16,20) with every label ignored; (3,6,16,20) with 5 % of the labels -1 or C + 3 (outside the range and not
ignore_index); (5,6,512,512), where the 1024-block forward, 4096-block backward and 128-block histogram grids all stride more than once.
For each: upstream NULL and a device scalar 0.37; plain, weighted with 0.5 + 1.5 rand, with ones, with NULL; OHEM at thresh 0.7 with
min_kept 0, npix // 8 and npix; each as the single form with weight 1.0 and with weight 0.4 and as the pair form with (1.0, 0.4).
Dumped: the documented result words, total, prob, dlogits.

Optimizer cases: n = 4099 (range (5, 11), multiplier 0.1) and n = 8192 * 1024 + 4099 (the 8192-block grid strides twice) x mirror none /
bf16 / fp16 x sgd_nt 1 / 0 x step 0 / 37 / 100 / 250 x clip_state NULL / [0.37] x {built-in SGD, _sched with kinds 0-3, Adam, AdamW};
emrt_grad_clip_scale at both sizes with clip 1.0 and 0.  Dumped: master, state streams, mirror, lr_out, the clip state."""
import argparse
import ctypes
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)            # (behind PYTHONPATH: the checkout under test wins)
import torch                     # noqa: E402

IGN = 255
RAW_LIMIT = 1 << 20
LOSS_SHAPES = [("sub_wave", (1, 3, 1, 5), 0.0, None), ("part_block", (3, 6, 16, 20), 0.10, None), ("odd_c", (4, 7, 24, 40), 0.15, None),
               ("all_ignored", (3, 6, 16, 20), 1.0, None), ("out_of_range", (3, 6, 16, 20), 0.0, 0.05), ("strided", (5, 6, 512, 512), 0.05, None)]
OPT_SIZES = [4099, 8192 * 1024 + 4099]
RANGE, MULT = (5, 11), 0.1


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Sink:
    """the file: outputs in the order they are given; large ones are hashed by a few threads while the GPU goes on"""

    def __init__(self, path, raw_limit):
        self.f, self.pool, self.pending, self.raw_limit = open(path, "wb"), ThreadPoolExecutor(8), [], raw_limit
        self.cases = self.outputs = self.raw_bytes = 0

    def case(self):
        self.cases += 1

    def put(self, t):
        t = t.detach().contiguous()
        if t.dtype in (torch.bfloat16, torch.float16):
            t = t.view(torch.int16)
        a = t.cpu().numpy()
        self.outputs += 1
        self.raw_bytes += a.nbytes
        self.pending.append(a.tobytes() if a.nbytes <= self.raw_limit else self.pool.submit(lambda a=a: hashlib.sha256(a).digest()))
        if len(self.pending) >= 16:
            self.flush()

    def flush(self):
        for b in self.pending:
            self.f.write(b if isinstance(b, bytes) else b.result())
        self.pending = []

    def close(self):
        self.flush()
        size = self.f.tell()
        self.f.close()
        self.pool.shutdown()
        return {"cases": self.cases, "outputs": self.outputs, "raw_bytes_compared": self.raw_bytes, "file_bytes": size, "raw_limit": self.raw_limit}


def loss_cases(L, stream, sink):
    for name, (N, C, H, W), ignored, stray in LOSS_SHAPES:
        g = torch.Generator().manual_seed(N * 1000 + W + len(name))
        npix = N * H * W
        la, lb = (torch.randn(N, C, H, W, generator=g) * 2).cuda(), (torch.randn(N, C, H, W, generator=g) * 3).cuda()
        labels = torch.randint(0, C, (N, H, W), generator=g)
        labels[torch.rand(N, H, W, generator=g) < ignored] = IGN
        if stray is not None:
            r = torch.rand(N, H, W, generator=g)
            labels[r < stray / 2] = -1
            labels[(r >= stray / 2) & (r < stray)] = C + 3
        lab = labels.cuda()
        up037 = torch.tensor([0.37], device="cuda")
        weights = {"plain": None, "rand": (0.5 + 1.5 * torch.rand(C, generator=g)).cuda(), "ones": torch.ones(C, device="cuda"), "null": None}
        ws = torch.empty(max(L.query("emrt_ce_workspace_bytes"), L.query("emrt_ohem_workspace_bytes", npix, 2)), dtype=torch.uint8, device="cuda")
        shape = (N, C, H, W, IGN)
        new = lambda *s: torch.zeros(*s, device="cuda")
        for up in (None, up037):
            for fam, cw in weights.items():
                ep, extra = ("emrt_softmax_ce", ()) if fam == "plain" else ("emrt_wce", (P(cw),))
                for lg, wgt in ((la, 1.0), (lb, 0.4)):
                    sink.case()
                    res, d = new(2), new(N, C, H, W)
                    L.call(ep + "_fwd", P(lg), P(lab), *extra, *shape, P(res), P(ws), stream)
                    L.call(ep + "_bwd", P(lg), P(lab), *extra, P(res), P(up), wgt, *shape, P(d), stream)
                    for t in (res, d):
                        sink.put(t)
                sink.case()
                ra, rb, total, da, db = new(2), new(2), new(1), new(N, C, H, W), new(N, C, H, W)
                L.call(ep + "_pair_fwd", P(la), P(lb), P(lab), *extra, *shape, 1.0, 0.4, P(ra), P(rb), P(total), P(ws), stream)
                L.call(ep + "_pair_bwd", P(la), P(lb), P(lab), *extra, P(ra), P(up), P(up), 1.0, 0.4, *shape, P(da), P(db), stream)
                for t in (ra, rb, total, da, db):
                    sink.put(t)
            for min_kept in (0, npix // 8, npix):
                for lg, wgt in ((la, 1.0), (lb, 0.4)):
                    sink.case()
                    prob, res, d = new(npix), new(8), new(N, C, H, W)
                    L.call("emrt_ohem_ce_fwd", P(lg), P(lab), *shape, 0.7, min_kept, P(prob), P(res), P(ws), stream)
                    L.call("emrt_ohem_ce_bwd", P(lg), P(lab), P(prob), P(res), P(up), wgt, *shape, P(d), stream)
                    for t in (res[:5], prob, d):
                        sink.put(t)
                sink.case()
                pa, pb, ra, rb, total, da, db = new(npix), new(npix), new(8), new(8), new(1), new(N, C, H, W), new(N, C, H, W)
                L.call("emrt_ohem_ce_pair_fwd", P(la), P(lb), P(lab), *shape, 0.7, min_kept, 1.0, 0.4, P(pa), P(pb), P(ra), P(rb), P(total), P(ws), stream)
                L.call("emrt_ohem_ce_pair_bwd", P(la), P(lb), P(lab), P(pa), P(pb), P(ra), P(rb), P(up), P(up), 1.0, 0.4, *shape, P(da), P(db), stream)
                for t in (ra[:5], rb[:5], total, pa, pb, da, db):
                    sink.put(t)


def schedules():
    from emrt_amd.src.models.solver import EmrtLrSchedule
    base = dict(base_lr=0.01, end_lr=1e-4, power=0.9, warmup_lr_init=1e-3, gamma=0.1, total_steps=100, warmup_steps=10, nmilestones=0)
    out = []
    for kind in range(4):
        d = EmrtLrSchedule(kind=kind, **base)
        if kind == 3:
            d.nmilestones = 2
            d.milestones[0], d.milestones[1] = 30, 60
        out.append(d)
    return out


def optim_cases(L, stream, sink):
    scheds = schedules()
    sp = lambda d: ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)
    rng = (ctypes.c_longlong * 2)(*RANGE)
    rp = ctypes.cast(rng, ctypes.c_void_p)
    gw = torch.empty(L.query("emrt_gradnorm_workspace_bytes"), dtype=torch.uint8, device="cuda")
    for n in OPT_SIZES:
        g_ = torch.Generator().manual_seed(n)
        p0, g0, m0 = torch.randn(n, generator=g_).cuda(), torch.randn(n, generator=g_).cuda(), (torch.randn(n, generator=g_) * 0.1).cuda()
        v0 = ((torch.randn(n, generator=g_) * 0.1) ** 2).cuda()
        for clip in (1.0, 0.0):
            sink.case()
            state = torch.zeros(2, device="cuda")
            L.call("emrt_grad_clip_scale", P(g0), n, clip, P(state), P(gw), stream)
            sink.put(state)
        for mdt, mtype in ((0, None), (1, torch.bfloat16), (2, torch.float16)):
            for nt in (1, 0):
                old = L.set_tuning("sgd_nt", nt)
                for step in (0, 37, 100, 250):
                    cnt = torch.tensor([step], dtype=torch.int64, device="cuda")
                    for clip_state in (None, torch.tensor([0.37, 0.0], device="cuda")):
                        def run(entry, two_moments, *mid):
                            sink.case()
                            p, m, v = p0.clone(), m0.clone(), v0.clone() if two_moments else None
                            mirror = None if mtype is None else torch.zeros(n, dtype=mtype, device="cuda")
                            lr = torch.zeros(1, device="cuda")
                            L.call(entry, P(p), P(g0), P(m), *((P(v),) if two_moments else ()), n, P(clip_state), P(cnt), *mid, rp, 1, MULT, P(lr),
                                   P(mirror), mdt, stream)
                            for t in (p, m, v, mirror, lr, clip_state):
                                if t is not None:
                                    sink.put(t)
                        run("emrt_sgd_momentum_step", False, 0.01, 1e-4, 0.9, 100, 0.9, 1e-4)
                        for d in scheds:
                            run("emrt_sgd_momentum_step_sched", False, sp(d), 0.9, 1e-4)
                        for decoupled in (0, 1):
                            run("emrt_adamw_step", True, sp(scheds[1]), 0.9, 0.999, 1e-8, 0.01, decoupled)
                L.set_tuning("sgd_nt", old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", choices=["loss", "optim"], default=None)
    ap.add_argument("--raw", action="store_true", help="raw bytes of every output, however large (no SHA-256 in place of outputs over 1 MiB)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dump_loss_optim needs a GPU")
    from emrt_amd import _lib
    from emrt_amd.runtime import ctx, F32
    c = ctx()
    c.init_device("cuda:0", F32, 0)
    L = _lib.lib()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sink = Sink(a.out, sys.maxsize if a.raw else RAW_LIMIT)
    if a.only != "optim":
        loss_cases(L, c.stream, sink)
    if a.only != "loss":
        optim_cases(L, c.stream, sink)
    torch.cuda.synchronize()
    rec = sink.close()
    rec["library"] = os.path.relpath(_lib.__file__, ROOT)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
