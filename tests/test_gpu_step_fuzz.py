"""-m gpu: the optimizer half of csrc/optim.hip -- emrt_grad_clip_scale, emrt_sgd_momentum_step, emrt_sgd_momentum_step_sched, emrt_adamw_step
through stream_update -- and emrt_segmentation_areas, swept by length, lr-mult range layout, mirror type, load arm and NULL arguments: the ops
"step" and "areas" of tests/fuzz_cases.py, every case through the C ABI.  Inputs, float64 references and bounds: tests/loss_step_reference.py.

What a case checks:
  * every buffer is n + PAD elements long and starts as a sentinel: from n on, the parameters, the state streams, the mirror, the clip state and
    the area counts must come back bit-unchanged;
  * clip: state[1] against the float64 norm.  All terms are positive, so the sum of squares is within (clip_depth(n) + 6 + 3 + 2) 2^-24 relative
    (the thread's additions from the restated grid, wave_sum's six, the block's three, the products and the final rounding; the blocks' partial
    sums are added in float64); half of that for the square root, plus one rounding.  state[0] is exactly 1.0f where the norm is below clip,
    clip <= 0 or the gradient is zero, and within the same count plus the division's rounding of clip / norm otherwise;
  * sgd / sgd_sched / adamw: the new parameters and state streams against float64 from the same fp32 inputs, with the fp32 learning rate the
    entry point reports for that step (sgd_reference / adam_reference state the roundings counted); mirror == p.to(dtype), tail included; the two
    sgd_nt arms agree bit for bit; lr_out holds the probed value, and NULL step / clip_state / lr_out mean step 0 / scale 1 / nothing written;
  * range membership EXACTLY: the case runs again with range_mult = 0, and p_new == p_old bit for bit must hold on the union of the ranges
    clipped to [0, n) and nowhere else (outside, every element moves by more than 4 ulp of itself: the input condition
    tests/test_fuzz_cases_cpu.py checks in float64), while the state streams carry the bits of the first run;
  * the refusals of fill_step_args return non-zero and leave every buffer as it was;
  * areas: counts exactly equal to a numpy restatement, added onto random contents, two runs equal.

-s prints the worst error / bound per case.  A run on an MI355X: DESIGN.md 2.4."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                    # noqa: E402
from emrt_amd.runtime import ctx, F32                        # noqa: E402
from emrt_amd.src.models import solver                       # noqa: E402
from emrt_amd.src.models.solver import EmrtLrSchedule        # noqa: E402
from tests import fuzz_cases as fc                           # noqa: E402
from tests import loss_step_reference as R                   # noqa: E402

U = R.U
PAD = 64
SENTINEL = -12345.0          # finite in every dtype (bf16 stores -12352)
MIRROR = {"none": (None, 0), "bf16": (torch.bfloat16, 1), "fp16": (torch.float16, 2)}
CLIP_CASES = [c for c in fc.CASES["step"] if c[1] == "clip"]
UPDATE_CASES = [c for c in fc.CASES["step"] if c[1] != "clip"]
LINES = []


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def sched_ptr(d):
    return ctypes.cast(ctypes.pointer(d), ctypes.c_void_p)


@pytest.fixture(scope="module")
def L():
    c = ctx()
    c.init_device("cuda:0", F32, 0)
    yield _lib.lib()
    if LINES:
        print("\n[step sweep] worst error / bound per case")
        for line in LINES:
            print(line)


def padded(host, dtype=torch.float32):
    """device buffer of len(host) + PAD elements: the data, then the sentinel"""
    t = torch.full((len(host) + PAD,), SENTINEL, dtype=dtype, device="cuda")
    t[:len(host)] = torch.from_numpy(np.ascontiguousarray(host)).to(device="cuda", dtype=dtype)
    return t


def tail_untouched(t, n):
    return bool((t[n:] == torch.tensor(SENTINEL, dtype=t.dtype)).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# clip
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_clip_sweep(L, case):
    _, _, n, _, _, _, kind, _, _, _ = case
    g = R.step_inputs(case)["g"]
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    clip = {"above": R.f32(0.25 * norm), "below": R.CLIP, "zero": 0.0, "negative": -1.0, "zerograd": R.CLIP}[kind]
    assert (kind != "above" or norm > clip > 0) and (kind != "below" or 0 < norm < clip) and (kind != "zerograd" or norm == 0.0)
    gd = padded(g)
    words = L.query("emrt_gradnorm_workspace_bytes") // 4
    runs = []
    for _ in range(2):
        state = torch.full((2 + PAD,), SENTINEL, device="cuda")
        ws = torch.full((words + PAD,), SENTINEL, device="cuda")
        L.call("emrt_grad_clip_scale", P(gd), n, clip, P(state), P(ws), ctx().stream)
        torch.cuda.synchronize()
        assert tail_untouched(state, 2) and tail_untouched(ws, words) and tail_untouched(gd, n)
        runs.append(state[:2].cpu())
    assert torch.equal(runs[0], runs[1]) and torch.equal(gd[:n].cpu(), torch.from_numpy(g))
    scale, got = runs[0][0].item(), runs[0][1].item()
    rel = (fc.clip_depth(n) + 6 + 3 + 2) * U / 2 + U
    e_norm = abs(got - norm) / (rel * norm) if norm > 0 else (0.0 if got == 0.0 else float("inf"))
    e_scale = 0.0
    if kind == "above":
        want = clip / norm
        e_scale = abs(scale - want) / ((rel + 2 * U) * want)
    else:
        assert scale == 1.0, (kind, scale)
    LINES.append("  %-8s clip %-9s n %-8d grid %-5d depth %-3d norm err/bound %.3f scale err/bound %.3f" % (case[0], kind, n, fc.clip_grid(n), fc.clip_depth(n), e_norm, e_scale))
    print(LINES[-1])
    assert e_norm <= 1.0 and e_scale <= 1.0, (got, norm, scale)


# ---------------------------------------------------------------------------------------------------------------------------------
# the three update entry points
# ---------------------------------------------------------------------------------------------------------------------------------
def _call(L, entry, p, g, s0, s1, n, state, cnt, ranges, mult, lr, mir, mdt, query=False):
    rng = (ctypes.c_longlong * max(2 * len(ranges), 2))(*[v for r in ranges for v in r])
    rp = ctypes.cast(rng, ctypes.c_void_p) if ranges else None
    run = L.query if query else L.call
    st = ctx().stream
    if entry == "sgd":
        return run("emrt_sgd_momentum_step", P(p), P(g), P(s0), n, P(state), P(cnt), R.SGD["base_lr"], R.SGD["end_lr"], R.SGD["power"], R.SGD["decay_steps"],
                   R.SGD["momentum"], R.SGD["weight_decay"], rp, len(ranges), mult, P(lr), P(mir), mdt, st)
    if entry == "sgd_sched":
        desc = solver.PolynomialDecay(R.SGD["base_lr"], R.SGD["decay_steps"], R.SGD["end_lr"], R.SGD["power"]).descriptor()
        return run("emrt_sgd_momentum_step_sched", P(p), P(g), P(s0), n, P(state), P(cnt), sched_ptr(desc), R.SGD["momentum"], R.SGD["weight_decay"],
                   rp, len(ranges), mult, P(lr), P(mir), mdt, st)
    sched = EmrtLrSchedule(**R.ADAM_SCHED)
    return run("emrt_adamw_step", P(p), P(g), P(s0), P(s1), n, P(state), P(cnt), sched_ptr(sched), R.ADAM["beta1"], R.ADAM["beta2"], R.ADAM["eps"],
               R.ADAM["weight_decay"], 1, rp, len(ranges), mult, P(lr), P(mir), mdt, st)


def probe_lr(L, entry, step):
    """the fp32 learning rate the entry point reports at `step`, from a call on eight zeros"""
    b = [torch.zeros(8, device="cuda") for _ in range(4)]
    cnt = torch.tensor([step], dtype=torch.int64, device="cuda")
    lr = torch.full((1,), -1.0, device="cuda")
    _call(L, entry, b[0], b[1], b[2], b[3], 8, None, cnt, [], 1.0, lr, None, 0)
    torch.cuda.synchronize()
    return lr.cpu()


def run_update(L, case, x, mult, nt):
    _, entry, n, layout, mirror, _, _, nulls, _, _ = case
    mtype, mdt = MIRROR[mirror]
    p, g, s0, s1 = (padded(x[k]) for k in ("p", "g", "s0", "s1"))
    mir = None if mtype is None else torch.full((n + PAD,), SENTINEL, dtype=mtype, device="cuda")
    state = None if "clip_state" in nulls else torch.tensor([R.SCALE, SENTINEL], device="cuda")
    cnt = None if "step" in nulls else torch.tensor([R.STEP_INDEX], dtype=torch.int64, device="cuda")
    lr = None if "lr_out" in nulls else torch.full((1 + PAD,), SENTINEL, device="cuda")
    old = L.set_tuning("sgd_nt", nt)
    try:
        _call(L, entry, p, g, s0, s1, n, state, cnt, fc.step_ranges(layout, n), mult, lr, mir, mdt)
        torch.cuda.synchronize()
    finally:
        L.set_tuning("sgd_nt", old)
    for t in (p, g, s0, s1) + (() if mir is None else (mir,)):
        assert tail_untouched(t, n), "%s: an element from n on was written" % case[0]
    assert torch.equal(g[:n].cpu(), torch.from_numpy(x["g"])) and (entry == "adamw" or torch.equal(s1[:n].cpu(), torch.from_numpy(x["s1"])))
    assert lr is None or tail_untouched(lr, 1)
    assert state is None or state[1].item() == SENTINEL
    return dict(p=p[:n].cpu(), s0=s0[:n].cpu(), s1=s1[:n].cpu(), mirror=None if mir is None else mir[:n].cpu(), lr=None if lr is None else lr[:1].cpu())


@pytest.mark.parametrize("case", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_update_sweep(L, case):
    _, entry, n, layout, mirror, nt, _, nulls, _, _ = case
    x = R.step_inputs(case)
    mask = R.step_mask(case)
    step = 0 if "step" in nulls else R.STEP_INDEX
    scale = 1.0 if "clip_state" in nulls else R.SCALE
    lr_t = probe_lr(L, entry, step)
    lr = float(lr_t.item())
    assert abs(lr - R.step_lr_host(entry, step)) < 1e-6 * 1e-2
    a = run_update(L, case, x, R.MULT, nt)
    assert a["lr"] is None or torch.equal(a["lr"], lr_t)
    gp, g0, g1 = (a[k].double().numpy() for k in ("p", "s0", "s1"))
    if entry == "adamw":
        p_ref, m_ref, v_ref, u_ref, m_mag, v_mag = R.adam_reference(x, scale, step, lr, R.MULT, mask)
        ratios = dict(p=np.abs(gp - p_ref) / np.maximum(U * (3 * np.abs(p_ref) + 8 * np.abs(u_ref)), 1e-300),
                      s0=np.abs(g0 - m_ref) / np.maximum(3 * U * m_mag, 1e-300), s1=np.abs(g1 - v_ref) / np.maximum(3 * U * v_mag, 1e-300))
    else:
        p_ref, v_ref, p_b, v_b, _ = R.sgd_reference(x, scale, lr, R.MULT, mask)
        ratios = dict(p=np.abs(gp - p_ref) / np.maximum(p_b, 1e-300), s0=np.abs(g0 - v_ref) / np.maximum(v_b, 1e-300))
    worst = {k: float(v.max()) for k, v in ratios.items()}
    LINES.append("  %-8s %-9s n %-8d %-8s mirror %-4s nt %d lr %.6g: worst error / bound %s" % (
        case[0], entry, n, layout, mirror, nt, lr, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    print(LINES[-1])
    assert all(w <= 1.0 for w in worst.values()), (worst, {k: int(v.argmax()) for k, v in ratios.items()})
    if a["mirror"] is not None:
        assert torch.equal(a["mirror"], a["p"].to(a["mirror"].dtype))
    b = run_update(L, case, x, R.MULT, 1 - nt)          # the other load / store arm
    for k in ("p", "s0", "s1", "mirror"):
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), "%s: the sgd_nt arms differ in %s" % (case[0], k)
    # range membership, exactly
    z = run_update(L, case, x, 0.0, nt)
    same = (z["p"] == torch.from_numpy(x["p"])).numpy()
    wrong = np.nonzero(same != mask)[0]
    assert wrong.size == 0, "%s: with range_mult = 0, p_new == p_old at %d elements that disagree with the ranges, first %s" % (case[0], wrong.size, wrong[:8])
    assert torch.equal(z["s0"], a["s0"]) and torch.equal(z["s1"], a["s1"]) and not torch.equal(z["s0"], torch.from_numpy(x["s0"]))
    if mask.any() and not mask.all():
        assert not torch.equal(z["p"], a["p"])
    assert z["mirror"] is None or torch.equal(z["mirror"], z["p"].to(z["mirror"].dtype))


def test_fill_step_args_refusals_leave_the_buffers_alone(L):
    """misaligned pointers, 33 ranges, a mirror of dtype 0, a misaligned mirror: a non-zero return with fill_step_args' reason, nothing written"""
    n = 64
    r = np.random.default_rng(5)
    host = {k: r.standard_normal(n + 4).astype(np.float32) for k in ("p", "g", "s0", "s1")}
    for entry in ("sgd", "sgd_sched", "adamw"):
        bufs = {k: padded(v) for k, v in host.items()}
        mir = torch.full((n + PAD,), SENTINEL, dtype=torch.bfloat16, device="cuda")
        state = torch.tensor([R.SCALE, 0.0], device="cuda")
        cnt = torch.tensor([R.STEP_INDEX], dtype=torch.int64, device="cuda")
        lr = torch.full((1,), SENTINEL, device="cuda")
        before = {k: v.clone() for k, v in bufs.items()}
        one, many = [(5, 11)], [(i, i + 1) for i in range(33)]
        off = lambda k: {q: (t[1:] if q == k else t) for q, t in bufs.items()}          # a view 4 bytes past the allocation's start
        tries = [(off(k), one, mir, 1, fc.fill_step_args_refuses(False, True, True, 1, 1, True)) for k in (("p", "g", "s0") + (("s1",) if entry == "adamw" else ()))]
        tries += [(bufs, many, mir, 1, fc.fill_step_args_refuses(True, True, True, 1, 33, True)),
                  (bufs, one, mir, 0, fc.fill_step_args_refuses(True, True, True, 0, 1, True)),
                  (bufs, one, mir[1:], 1, fc.fill_step_args_refuses(True, True, False, 1, 1, True))]
        for b, ranges, m, mdt, why in tries:
            assert why
            rc = _call(L, entry, b["p"], b["g"], b["s0"], b["s1"], n, state, cnt, ranges, R.MULT, lr, m, mdt, query=True)
            torch.cuda.synchronize()
            assert rc != 0 and why in L.last_error(), (entry, rc, why, L.last_error())
        for k in bufs:
            assert torch.equal(bufs[k], before[k]), (entry, k)
        assert bool((mir == torch.tensor(SENTINEL, dtype=torch.bfloat16)).all()) and lr.item() == SENTINEL and state[0].item() == np.float32(R.SCALE)
        assert _call(L, entry, bufs["p"], bufs["g"], bufs["s0"], bufs["s1"], n, state, cnt, many[:32], R.MULT, lr, mir, 1, query=True) == 0      # 32 ranges are taken
        torch.cuda.synchronize()
        assert not torch.equal(bufs["p"][:n], before["p"][:n]) and tail_untouched(bufs["p"], n + 4)


# ---------------------------------------------------------------------------------------------------------------------------------
# emrt_segmentation_areas
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.CASES["areas"], ids=[c[0] for c in fc.CASES["areas"]])
def test_areas_sweep(L, case):
    _, ncls, ltype, offset, n, ignore, _, seed = case
    pred, label = R.areas_inputs(case)
    want = R.areas_reference(pred, label, ncls, ignore)
    pd = torch.from_numpy(pred).cuda()
    raw = torch.zeros(label.nbytes + 16, dtype=torch.uint8, device="cuda")
    raw[offset:offset + label.nbytes] = torch.from_numpy(label.view(np.uint8)).cuda()
    lptr = ctypes.c_void_p(raw.data_ptr() + offset)
    assert (raw.data_ptr() + offset) % 2 == offset
    start = torch.from_numpy(np.random.default_rng(seed).integers(0, 1000, 3 * ncls)).to(torch.int64)
    runs = []
    for _ in range(2):
        out = torch.full((3 * ncls + PAD,), -7, dtype=torch.int64, device="cuda")
        out[:3 * ncls] = start.cuda()
        L.call("emrt_segmentation_areas", P(pd), lptr, ltype, n, ncls, ignore, P(out), ctx().stream)
        torch.cuda.synchronize()
        assert bool((out[3 * ncls:] == -7).all())
        runs.append(out[:3 * ncls].cpu())
    assert torch.equal(runs[0], runs[1])
    got = (runs[0] - start).numpy().reshape(3, ncls)
    print("  %-8s ncls %-3d type %d offset %d n %-8d grid %-4d ignore %-4d counted %d of %d labels" % (case[0], ncls, ltype, offset, n, fc.areas_grid(n), ignore, int(want[2].sum()), n))
    assert np.array_equal(got, want), (case[0], np.argwhere(got != want)[:8])
    assert want.sum() > 0 or n == 1
