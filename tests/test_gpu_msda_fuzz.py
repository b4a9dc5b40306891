"""-m gpu: seeded random pyramids through the deformable-attention kernels (LDS-staged, row-band and global-gather forward; LDS gradient,
band gradient, integer LDS scatter with and without query split, global-atomic backward -- whichever the dispatchers pick for the geometry)
against the oracle's torch expression of deformable_attention_core_func (EMRT_utils/utils.py:64-97) on the same rounded inputs.
Odd and non-square level sizes, levels that do not halve, few and many queries, offsets from sub-pixel to far outside the map.

Then the sweep by plan, build and layout (tests/fuzz_cases.py, op "msda"): every case names the kernel kinds it is there to reach, the planner
is asked on the device as well, and every tensor is held PER ROW against the float64 restatement of tests/msda_reference.py under its
calibrated bounds (MSDA_BOUND: 3 x the 16-bit contract floor, 16 x the fp32 torch floor; tests/test_msda_reference_cpu.py shows on the CPU
that these bounds separate a correct kernel from one that drops what a band has not staged, adds the last query twice, reads level 0's
reference point for every level, drops partly-outside samples whole or takes the fixed-point scale without the spike rows).  bf16 cases run
the value gradient three ways -- as planned, matrix product forced, integer scatter forced.  The strided layout calls the C entry points on a
channel slice of a wider value buffer and writes into pre-filled buffers: everything outside the slice, the pad columns and the guard rows
stays bit-identical, every dvalue element comes back finite, pixels no sample reaches as exact zeros.  -s prints worst error / bound per
tensor and case, and a table per dtype at the end.

Worst error / bound over the sweep, as printed by a run on an MI355X:
            out    doff   dlogit  dvalue: lds  mf     spike-lds  spike-mf   dref
    fp32   0.062  0.062  0.061      0.062      --      0.061       --      0.058
    bf16   0.333  0.333  0.333      0.333    0.332     0.333     0.332     0.074      (as planned, msda_scatter_mfma = 2 and = 0)
    fp16   0.332
Nothing above 0.5: the 16-bit kernels sit on their contract floor (bound / 3), the fp32 kernels on the fp32-torch floor (bound / 16).  The sweep
found no defect in csrc/msda.hip.

The sweep runs no sanitizer, reads no kernel assembly and contains no case that is meant to make a kernel misbehave; every case is inside the
entry points' domain (tests/test_fuzz_cases_cpu.py)."""
import contextlib
import ctypes
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import functional as Fn                    # noqa: E402
from emrt_amd import _lib                                 # noqa: E402
from emrt_amd.functional import P                         # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, F16, Tape     # noqa: E402
from tests import fuzz_cases as fc                        # noqa: E402
from tests import msda_reference as ms                    # noqa: E402
from tests.hip_utils import init, dev, host, rnd          # noqa: E402
from tests.test_gpu_kernels import _msda_ref, run_bwd     # noqa: E402
from tests.test_msda_reference_cpu import KNOB_DEFAULTS, plan_kinds      # noqa: E402


def _cases(seed, n):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        h0, w0 = rng.randint(6, 72), rng.randint(6, 72)
        if rng.random() < 0.5:      # a pyramid that halves (rounded up), as the backbone produces
            shapes = [(h0, w0), ((h0 + 1) // 2, (w0 + 1) // 2), ((h0 + 3) // 4, (w0 + 3) // 4)]
        else:                       # three unrelated maps
            shapes = [(h0, w0), (rng.randint(2, 40), rng.randint(2, 40)), (rng.randint(1, 20), rng.randint(1, 20))]
        out.append(dict(name="msda-fuzz%d-%d" % (seed, i), B=rng.randint(1, 6), shapes=shapes,
                        Lq=None if rng.random() < 0.6 else rng.randint(1, 400), sigma=rng.choice([0.3, 2.5, 2.5, 8.0, 40.0]),
                        dtype=rng.choice([BF16, BF16, F32]), seed=seed * 100 + i))
    return out


CASES = _cases(77, 16)


@pytest.mark.parametrize("cfg", CASES, ids=[c["name"] for c in CASES])
def test_msda_random_pyramid_vs_oracle(cfg):
    dt = cfg["dtype"]
    c = init(dt)
    g = torch.Generator().manual_seed(cfg["seed"])
    M, L, Pn = 8, 3, 6
    shapes, B = cfg["shapes"], cfg["B"]
    Lv = sum(h * w for h, w in shapes)
    Lq = cfg["Lq"] or Lv
    tp = M * L * Pn
    r = rnd if dt == BF16 else (lambda t: t)
    value = r(torch.randn(B, Lv, M * 32, generator=g))
    offw = torch.cat([torch.randn(B, Lq, 2 * tp, generator=g) * cfg["sigma"], torch.randn(B, Lq, tp, generator=g)], -1)
    if cfg["Lq"] is None:
        from emrt_amd.src.models.emrt import encoder_reference_points
        ref = encoder_reference_points(shapes)
    else:
        ref = torch.rand(1, Lq, 1, 2, generator=g)
    vr, orq = value.clone().requires_grad_(True), offw.clone().requires_grad_(True)
    out_r = _msda_ref(vr, orq, ref, shapes, M, L, Pn)
    dy = r(torch.randn(out_r.shape, generator=g))
    out_r.backward(dy)
    vd, od, rd = dev(value), dev(offw, torch.float32), dev(ref, torch.float32)
    tape = Tape()
    c.tape = tape
    y = Fn.msda(vd, od, rd, shapes, M, Pn)
    c.tape = None
    tape.watch(vd)
    tape.watch(od)
    den = out_r.detach().norm().item() or 1.0
    rel = ((host(y) - out_r.detach()).norm() / den).item()
    dv, do = run_bwd(tape, [(y, dev(dy))], [vd, od])
    gv, go = vr.grad, orq.grad
    rel_v = ((host(dv) - gv).norm() / (gv.norm().item() or 1.0)).item()
    if dt == BF16:      # the other value-gradient kernel too: matrix product forced wherever its plan exists / never (csrc/msda.hip: knob msda_scatter_mfma)
        from emrt_amd import _lib
        for knob in (2, 0):
            old = _lib.lib().set_tuning("msda_scatter_mfma", knob)
            try:
                tape2 = Tape()
                c.tape = tape2
                y2 = Fn.msda(vd, od, rd, shapes, M, Pn)
                c.tape = None
                tape2.watch(vd)
                dv2, = run_bwd(tape2, [(y2, dev(dy))], [vd])
            finally:
                _lib.lib().set_tuning("msda_scatter_mfma", old)
            rel_k = ((host(dv2) - gv).norm() / (gv.norm().item() or 1.0)).item()
            print("    msda_scatter_mfma = %d: dvalue rel %.2e" % (knob, rel_k))
            rel_v = max(rel_v, rel_k)
    rel_o = ((host(do) - go).norm() / (go.norm().item() or 1.0)).item()
    print("%s %s B=%d Lq=%d sigma=%.1f %s: fwd rel %.2e, dvalue rel %.2e, doffw rel %.2e" % (
        cfg["name"], shapes, B, Lq, cfg["sigma"], "bf16" if dt == BF16 else "fp32", rel, rel_v, rel_o))
    # bf16: one rounding of each stored result (2^-9) + the gather's weights rounded to bf16; fp32: summation order only
    # (the value gradient's integer scatter quantises to 2^-30 of Lq * max|g| per addend)
    tol, tol_v = (4e-3, 6e-3) if dt == BF16 else (2e-5, 2e-4)
    assert rel < tol and rel_v < tol_v and rel_o < (6e-3 if dt == BF16 else 2e-4), (rel, rel_v, rel_o)


# ---------------------------------------------------------------------------------------------------------------------------------
# the sweep by plan, build and layout
# ---------------------------------------------------------------------------------------------------------------------------------
F64 = torch.float64
SWEEP = fc.CASES["msda"]
DTYPE = {"f32": F32, "bf16": BF16, "f16": F16}
FILL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float16: (torch.int16, 0x7E01), torch.float32: (torch.int32, 0x7FC00001)}      # quiet NaNs with a payload
WORST = {}          # (dtype name, tensor key) -> (worst error / bound of this process, case id)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for d in ("f32", "bf16", "f16"):
        keys = sorted(k for k in WORST if k[0] == d)
        if keys:
            print("\n[msda sweep] worst error / bound  %-4s " % d + "  ".join("%s %.3f (%s)" % (k[1], WORST[k][0], WORST[k][1].rsplit("-", 1)[1]) for k in keys), end="")
    print()


@contextlib.contextmanager
def _knobs(kv):
    """set_tuning with the old values put back afterwards"""
    L_ = _lib.lib()
    old = []
    try:
        for k, v in kv.items():
            old.append((k, L_.set_tuning(k, v)))
        yield
    finally:
        for k, v in reversed(old):
            L_.set_tuning(k, v)


def _filled(shape, tdtype):
    it, pat = FILL[tdtype]
    return torch.full(shape, pat, dtype=it, device="cuda").view(tdtype)


def _is_fill(t):
    it, pat = FILL[t.dtype]
    return t.contiguous().view(it) == pat


def _shapes_arr(shapes):
    return (ctypes.c_int * (2 * len(shapes)))(*[int(v) for hw in shapes for v in hw])


def _run_dense(case, inp, dtype, backward):
    """through functional.msda -> dict of CPU float64 tensors shaped as msda_reference._chain's"""
    _, B, M, shapes, _, Pn, _, _, refmode, _, _, _ = case
    c = ctx()
    L = len(shapes)
    tp = M * L * Pn
    Lv = inp["value"].shape[1]
    Lq = inp["offw"].shape[1]
    vd, od, rd = dev(inp["value"].float()), dev(inp["offw"].float(), torch.float32), dev(inp["ref"].float(), torch.float32)
    want_dref = refmode.endswith("+dref")
    tape = Tape() if backward else None
    c.tape = tape
    try:
        y = Fn.msda(vd, od, rd, shapes, M, Pn, need_dref=want_dref)
    finally:
        c.tape = None
    res = {"out": y.to(F64).cpu().reshape(B, Lq, M, 32), "out_dev": y}
    if backward:
        watched = [vd, od] + ([rd] if want_dref else [])
        for w in watched:
            tape.watch(w)
        grads = run_bwd(tape, [(y, dev(inp["dout"].float()))], watched)
        do = grads[1].to(F64).cpu()
        res["dvalue"] = grads[0].to(F64).cpu().reshape(B, Lv, M, 32)
        res["doff"], res["dlogit"] = do[..., :2 * tp].reshape(B, Lq, M, L * Pn * 2), do[..., 2 * tp:].reshape(B, Lq, M, L * Pn)
        res["dref"] = grads[2].to(F64).cpu() if want_dref else None
    torch.cuda.synchronize()
    return res


def _run_strided(case, inp, dtype, backward):
    """the C entry points on a channel slice of a wider value buffer (ldv = 32 M + 64, v_bs padded by 8 ldv), offw rows of 3 M L P + 2, every
    output in a pre-filled buffer with two guard rows; asserts that nothing outside was written"""
    _, B, M, shapes, _, Pn, _, _, refmode, _, _, _ = case
    c = ctx()
    L_ = _lib.lib()
    L = len(shapes)
    tp = M * L * Pn
    Lv, Lq, E = inp["value"].shape[1], inp["offw"].shape[1], M * 32
    ldv, ldo = E + 64, 3 * tp + 2
    wide = _filled((B, Lv + 8, ldv), c.tdtype)
    wide[:, :Lv, 32:32 + E] = inp["value"].to(c.tdtype).cuda()
    value = wide[:, :, 32:]
    before = wide.clone()
    offw = _filled((B * Lq, ldo), torch.float32)
    offw[:, :3 * tp] = inp["offw"].reshape(B * Lq, 3 * tp).float().cuda()
    ref = inp["ref"].float().contiguous().cuda()
    ref_L = ref.shape[2]
    ref_bs = 0 if ref.shape[0] == 1 else Lq * ref_L * 2
    arr = _shapes_arr(shapes)
    sh = ctypes.cast(arr, ctypes.c_void_p)
    out = _filled((B * Lq + 2, E), c.tdtype)
    L_.call("emrt_msda_fwd", P(value), ldv, (Lv + 8) * ldv, P(offw), ldo, P(ref), ref_bs, ref_L, P(out), B, Lq, Lv, M, 32, L, Pn, sh, dtype, c.stream)
    torch.cuda.synchronize()
    assert bool(_is_fill(out[B * Lq:]).all()), "out: written beyond its rows"
    assert bool(torch.isfinite(out[:B * Lq].float()).all()), "out: an element was not written (or is not finite)"
    res = {"out": out[:B * Lq].to(F64).cpu().reshape(B, Lq, M, 32), "out_dev": out[:B * Lq].reshape(B, Lq, E)}
    if backward:
        want_dref = refmode.endswith("+dref")
        dout = inp["dout"].reshape(B * Lq, E).to(c.tdtype).cuda()
        dvalue = _filled((B * Lv + 2, E), c.tdtype)
        doffw = _filled((B * Lq + 2, ldo), c.tdtype if dtype != F32 else torch.float32)
        dref = torch.zeros(B, Lq, ref_L, 2, dtype=torch.float32, device="cuda") if want_dref else None
        nbytes = L_.query("emrt_msda_bwd_workspace_bytes", B, Lq, M, L, Pn, sh, dtype)
        assert nbytes > 0, L_.last_error()
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
        L_.call("emrt_msda_bwd", P(value), ldv, (Lv + 8) * ldv, P(offw), ldo, P(ref), ref_bs, ref_L, P(dout), P(dvalue), P(doffw), int(dtype != F32), P(dref),
                B, Lq, Lv, M, 32, L, Pn, sh, P(ws), nbytes, dtype, c.stream)
        torch.cuda.synchronize()
        assert bool(_is_fill(dvalue[B * Lv:]).all()), "dvalue: written beyond its rows"
        assert bool(_is_fill(doffw[B * Lq:]).all()) and bool(_is_fill(doffw[:, 3 * tp:]).all()), "doffw: pad columns or guard rows written"
        assert bool(torch.isfinite(doffw[:B * Lq, :3 * tp].float()).all()), "doffw: an element was not written (or is not finite)"
        do = doffw[:B * Lq, :3 * tp].to(F64).cpu().reshape(B, Lq, 3 * tp)
        res["dvalue"] = dvalue[:B * Lv].to(F64).cpu().reshape(B, Lv, M, 32)
        res["doff"], res["dlogit"] = do[..., :2 * tp].reshape(B, Lq, M, L * Pn * 2), do[..., 2 * tp:].reshape(B, Lq, M, L * Pn)
        res["dref"] = dref.to(F64).cpu() if want_dref else None
    it = FILL[c.tdtype][0]
    assert torch.equal(wide.view(it), before.view(it)), "the value buffer was written"
    assert bool(_is_fill(offw[:, 3 * tp:]).all()), "offw: pad columns written"
    return res


def _check_dvalue(cid, got, want):
    """every element finite; exact zeros on the pixels no sample reaches"""
    assert bool(torch.isfinite(got).all()), "%s: dvalue has non-finite elements (a pixel that was never written?)" % cid
    untouched = want["count"] == 0
    assert bool((got[untouched] == 0).all()), "%s: dvalue is not exactly zero on %d of the %d (pixel, head) rows no sample reaches" % (
        cid, int((got[untouched] != 0).any(-1).sum()), int(untouched.sum()))


def _hold(case, dname, errs, regime, kind, arm=""):
    """print error / bound per tensor, record the worst, assert"""
    ratios = {}
    for k, e in errs.items():
        key = k if k != "dvalue" else "dvalue:" + ms.dvalue_key(regime, kind)
        ratios[key] = e / ms.bound_of(dname, k, regime, kind)
        if ratios[key] > WORST.get((dname, key), (-1.0, None))[0]:
            WORST[(dname, key)] = (ratios[key], case[0])
    print("    %s %s%s error / bound: %s" % (case[0], dname, arm, "  ".join("%s %.3f" % kv for kv in ratios.items())))
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, "%s%s: above the bound (error / bound): %s" % (case[0], arm, over)


@pytest.mark.parametrize("case", SWEEP, ids=[c[0] for c in SWEEP])
def test_msda_sweep(case):
    cid, B, M, shapes, _, Pn, regime, layout, refmode, knobs, expect, _ = case
    dname, fwd_kinds, bwd_kinds = expect
    dtype = DTYPE[dname]
    c = init(dtype)
    backward = bwd_kinds is not None
    if not backward:
        c.training = False
    L_ = _lib.lib()
    inp = ms.make_inputs(case, dname)
    want, mag = ms.exact(inp, shapes, M, Pn), ms.magnitude(inp, shapes, M, Pn)
    shared = refmode.startswith("shared")
    run = _run_strided if layout == "strided" else _run_dense
    want_knobs = dict(KNOB_DEFAULTS)
    want_knobs.update(knobs)
    try:
        with _knobs(want_knobs):
            assert plan_kinds(L_, case, False)[0] == fwd_kinds and (not backward or plan_kinds(L_, case, True)[0] == bwd_kinds), (cid, "the planner's answer changed")
            got = run(case, inp, dtype, backward)
            kind = "mf" if backward and "SCATTER_MF" in bwd_kinds else "lds"
            if backward:
                _check_dvalue(cid, got["dvalue"], want)
            _hold(case, dname, ms.worst_errors(got, want, mag, inp, M, dname, kind, shared), regime, kind)
            if dname != "f32" and "FWD_LDS" in fwd_kinds:
                # msda_fwd_lds_kernel: "same arithmetic in the same order as msda_fwd_kernel: the two are bit-identical" (the band form is stated
                # to be so only when nothing misses: held to the bound alone)
                with _knobs({"msda_fwd_global": 1}):
                    assert plan_kinds(L_, case, False, {"msda_fwd_global": 1})[0] == ("FWD_GLOBAL",)
                    again = run(case, inp, dtype, False)
                assert torch.equal(got["out_dev"], again["out_dev"]), "%s: the LDS-staged and the global forward differ" % cid
            if dname == "bf16":          # the other value-gradient kernel too (knob msda_scatter_mfma: 2 = matrix product wherever a plan exists, 0 = never)
                for knob, k2 in ((2, "mf"), (0, "lds")):
                    with _knobs({"msda_scatter_mfma": knob}):
                        assert ("SCATTER_MF" if knob else "SCATTER_LDS") in plan_kinds(L_, case, True, {"msda_scatter_mfma": knob})[0]
                        g2 = run(case, inp, dtype, True)
                    _check_dvalue(cid, g2["dvalue"], want)
                    _hold(case, dname, ms.worst_errors({"dvalue": g2["dvalue"]}, want, mag, inp, M, dname, k2), regime, k2, " msda_scatter_mfma = %d" % knob)
    finally:
        c.training = True
