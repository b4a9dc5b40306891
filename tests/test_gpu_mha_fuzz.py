"""-m gpu: the attention kernels of csrc/attn.hip (emrt_mha_fwd / emrt_mha_bwd, fp32 and bf16) over every length of fuzz_cases.MHA_LS,
small batch and head counts, four input regimes, dropout on both sides of the VALU backward's LDS threshold, and three operand layouts,
each output held PER ROW against the float64 closed form of tests/mha_reference.py under its calibrated bounds (MHA_BOUND: 3 x the bf16
contract floor, 16 x the fp32 torch floor; tests/test_mha_reference_cpu.py shows on the CPU that these bounds separate a correct kernel from
one that loses the last key, lets a padding column into the denominator, or uses another mask in the backward).

Per case and dtype: forward and backward through the case's layout (fuzz_cases.MHA_LAYOUTS); the path emrt_mha_fwd reports equals
fuzz_cases.mha_path; bf16 runs three ways -- as dispatched, with mha_valu = 1, with mha_bwd_split = 0 -- each held to the same bound against
the exact values (each kernel is right, not: the kernels agree).  Dropout cases read the device's own dropped probabilities out of the forward
with one-hot values (ceil(L / 32) tiny launches), per kernel family; kept entries must equal P / (1 - p) to the output's rounding, the
dropped fraction must be p (floor(65536 p) / 65536 in the MFMA kernels) within 5 standard errors, and o, dq, dk, dv must equal the closed
form with THAT mask (and that mask must be the host model's, tests/dropout_reference.py, bit for bit at every position whose reference
probability is at least 1e-30: mha_drop4 at ((b M + m) L + i) 32 + (j >> 2) in the MFMA kernels, uniform01 at ((b M + m) L + i) L + j in the
VALU kernels) -- which ties the backward's re-derived masks (row pass, column pass, and the VALU kernel's second derivation past
L = 110) to the forward's.  The direct layouts write into wider buffers pre-filled with a NaN bit pattern, two guard rows behind: everything
outside rows < B L, columns < E stays bit-identical, everything inside is finite.

Worst error / bound over the sweep, as printed by a run on an MI355X (-s shows the table and one line per case and arm):
                                    o      dq     dk     dv
    fp32                          0.061  0.063  0.068  0.060
    bf16 as dispatched            0.327  0.332  0.333  0.331     (the MFMA kernels sit on the contract floor: bound / 3)
    bf16, mha_valu = 1            0.225  0.248  0.186  0.200
    bf16, mha_bwd_split = 0       0.327  0.332  0.333  0.331
Nothing above 0.5; kept probabilities came back within 0.98 of one bf16 rounding and 0.07 of the fp32 allowance.  The sweep found no defect
in csrc/attn.hip: the re-derived mask of L = 111 .. 128, odd tile counts, M = 1, 2, 3, 4, split strides and the 8-byte-aligned bf16 backward
all agree with the closed form.

The sweep runs no sanitizer, reads no kernel assembly and contains no case that is meant to make a kernel misbehave; every case is inside
the entry points' domain (tests/test_fuzz_cases_cpu.py), and the refusals are checked to return before any launch.
"""
import contextlib
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from emrt_amd import _lib                                                        # noqa: E402
from emrt_amd import functional as Fn                                            # noqa: E402
from emrt_amd.functional import P                                                # noqa: E402
from emrt_amd.runtime import ctx, F32, BF16, Tape                                # noqa: E402
from tests import dropout_reference as dr                                        # noqa: E402
from tests import fuzz_cases as fc                                               # noqa: E402
from tests import mha_reference as mr                                            # noqa: E402
from tests.hip_utils import init                                                 # noqa: E402
from tests.test_gpu_kernels import DTYPES, run_bwd                               # noqa: E402

F64 = torch.float64
NAME = {F32: "f32", BF16: "bf16"}
CASES = fc.CASES["mha"]
FILL = {torch.bfloat16: (torch.int16, 0x7FC1), torch.float32: (torch.int32, 0x7FC00001)}          # quiet NaNs with a payload
OUT_ROUNDING = {BF16: 2.0 ** -8, F32: 2.0 ** -24}          # one rounding to nearest of a stored output, relative: 8 and 24 significant bits
WORST = {}          # (dtype name, arm, tensor) -> worst error / bound of this process


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for d in ("f32", "bf16"):
        for arm in ("dispatched", "valu", "nosplit"):
            if (d, arm, "o") in WORST:
                print("\n[mha sweep] worst error / bound  %-4s %-10s " % (d, arm) + "  ".join("%s %.3f" % (n, WORST[(d, arm, n)]) for n in mr.TENSORS), end="")
    print()


def _rows(t, tdtype):
    """[B, M, L, 32] float64 -> device [B L, M 32] in the compute dtype (the values are already rounded through it)"""
    B, M, L, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * L, M * 32).to(tdtype).cuda()


def _heads(t, B, M, L):
    """device [B L, >= M 32] -> CPU [B, M, L, 32] float64"""
    return t[:, :M * 32].to(F64).cpu().reshape(B, L, M, 32).permute(0, 2, 1, 3).contiguous()


def _filled(rows, cols, tdtype):
    it, pat = FILL[tdtype]
    return torch.full((rows, cols), pat, dtype=it, device="cuda").view(tdtype)


def _untouched(name, buf, rows, cols):
    it, pat = FILL[buf.dtype]
    raw = buf.view(it)
    assert bool((raw[rows:] == pat).all()) and bool((raw[:, cols:] == pat).all()), "%s: written outside rows < %d, columns < %d" % (name, rows, cols)
    assert bool(torch.isfinite(buf[:rows, :cols].float()).all()), "%s: an element inside was not written (or is not finite)" % name


@contextlib.contextmanager
def _knobs(**kv):
    """set_tuning with the old values put back afterwards"""
    L_ = _lib.lib()
    old = [(k, L_.set_tuning(k, v)) for k, v in kv.items()]
    try:
        yield
    finally:
        for k, v in reversed(old):
            L_.set_tuning(k, v)


def _kept_tolerance(q, k, dtype):
    """Relative bound [B, M, L, 1] on a kept probability read back through o against the float64 P / (1 - p), worst case: the fp32 score is a
    32-term dot product (33 roundings of 2^-24 on sum |q_d k_d| scale), __expf rounds its argument (|s - max| 2^-23) and its result, the row
    sum is a weighted mean of the same relative errors and the divide and the keep scale add three roundings: twice the worst numerator error
    of the row plus 2^-21; then the one rounding of the stored output."""
    s = mr.scores(q, k)
    e = 33.0 * 2.0 ** -24 * mr.SCALE * (q.abs() @ k.abs().transpose(-1, -2)) + ((s - s.max(-1, keepdim=True).values).abs() + 1.0) * 2.0 ** -23
    return 2.0 * e.max(-1, keepdim=True).values + 2.0 ** -21 + OUT_ROUNDING[dtype] * (1.0 + 2.0 ** -7)


def _direct_operands(layout, dtype, q, k, v, B, M, L):
    """q, k, v views for the direct layouts: three buffers with row strides E, E + 8, 2 E + 16 (the columns beyond E hold the NaN pattern: a
    kernel that read them would show it); offset8 (bf16): q starts 4 elements = 8 bytes into its buffer"""
    c = ctx()
    E, R = M * 32, B * L
    if layout == "offset8" and dtype == BF16:
        flat = _filled(1, R * E + 8, c.tdtype).view(-1)
        qd = flat[4:4 + R * E].view(R, E)
        qd.copy_(q)
        assert qd.data_ptr() % 16 == 8
    else:
        qd = q.clone()
        assert qd.data_ptr() % 16 == 0
    kd = _filled(R, E + 8, c.tdtype)
    kd[:, :E] = k
    vd = _filled(R, 2 * E + 16, c.tdtype)
    vd[:, :E] = v
    return qd, kd, vd


def _run(layout, dtype, q, k, v, dy, B, M, L, p, salt, backward=True):
    """forward (+ backward) of device rows q, k, v, dy [B L, E] through `layout` -> {o, dq, dk, dv: CPU [B, M, L, 32] float64, path}"""
    c = ctx()
    L_ = _lib.lib()
    E, R = M * 32, B * L
    res = {}
    if layout == "fused":
        c.training = p > 0.0
        qk = torch.cat([q, k], 1).reshape(B, L, 2 * E).contiguous()
        vd = v.reshape(B, L, E).contiguous()
        tape = Tape() if backward else None
        c.tape = tape
        L_.start_record()
        try:
            y = Fn.mha(qk, vd, M, p, salt)
        finally:
            rec = L_.stop_record()
            c.tape = None
        (args,) = [a for n, a in rec if n == "emrt_mha_fwd"]
        res["path"] = args[17].contents.value          # path_out, as the call filled it
        res["o"] = _heads(y.reshape(R, E), B, M, L)
        if backward:
            tape.watch(qk)
            tape.watch(vd)
            dqk, dv = run_bwd(tape, [(y, dy.reshape(B, L, E).contiguous())], [qk, vd])
            dqk = dqk.reshape(R, 2 * E)
            res["dq"], res["dk"], res["dv"] = _heads(dqk[:, :E], B, M, L), _heads(dqk[:, E:], B, M, L), _heads(dv.reshape(R, E), B, M, L)
        c.training = True
        return res
    qd, kd, vd = _direct_operands(layout, dtype, q, k, v, B, M, L)
    o = _filled(R + 2, E + 8, c.tdtype)
    probs = torch.zeros(B, M, L, L, dtype=torch.float32, device="cuda")
    path = ctypes.c_int(-1)
    L_.call("emrt_mha_fwd", P(qd), qd.stride(0), P(kd), kd.stride(0), P(vd), vd.stride(0), P(o), o.stride(0), P(probs), B, M, L, 32, mr.SCALE, float(p),
            c.seed_ptr, salt, ctypes.pointer(path), dtype, c.stream)
    torch.cuda.synchronize()
    _untouched("o", o, R, E)
    res["path"], res["o"] = path.value, _heads(o[:R], B, M, L)
    if backward:
        dyd = _filled(R, E + 16, c.tdtype)
        dyd[:, :E] = dy
        dq, dk, dv = _filled(R + 2, E + 16, c.tdtype), _filled(R + 2, E + 24, c.tdtype), _filled(R + 2, E + 32, c.tdtype)
        L_.call("emrt_mha_bwd", P(qd), qd.stride(0), P(kd), kd.stride(0), P(vd), vd.stride(0), P(probs), P(dyd), dyd.stride(0),
                P(dq), dq.stride(0), P(dk), dk.stride(0), P(dv), dv.stride(0), B, M, L, 32, mr.SCALE, float(p), c.seed_ptr, salt, path.value, dtype, c.stream)
        torch.cuda.synchronize()
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            _untouched(n, t, R, E)
            res[n] = _heads(t[:R], B, M, L)
    return res


def _read_dropped_probs(layout, dtype, q, k, B, M, L, p, salt):
    """Pd [B, M, L(query), L(key)] as the forward itself applies it: with V_j = e_(j mod 32) for the keys of one block of 32 (zero elsewhere),
    o_i[d] is Pd[i][32 blk + d] -- one term, so the output's rounding is the only one"""
    cols = []
    for blk in range(fc.mha_fwd_chunks(L)):
        n = min(32, L - 32 * blk)
        vv = torch.zeros(B, M, L, 32, dtype=F64)
        for d in range(n):
            vv[:, :, 32 * blk + d, d] = 1.0
        r = _run(layout, dtype, q, k, _rows(vv, ctx().tdtype), None, B, M, L, p, salt, backward=False)
        cols.append(r["o"][..., :n])
    return torch.cat(cols, -1)


def _ids(cases):
    return [c[0] for c in cases]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_mha_random_shapes(dtype, case):
    cid, B, M, L, regime, p, layout, seed = case
    c = init(dtype, seed if p > 0.0 else 0)          # a dropout case has its own seed word on the device, both halves non-zero
    d = NAME[dtype]
    ins = mr.make_inputs(regime, B, M, L, seed, d)
    q, k, v, dy = (_rows(t, c.tdtype) for t in ins)
    salt = 1 + seed % 97
    aligned = not (layout == "offset8" and dtype == BF16)
    arms = [("dispatched", {})] + ([("valu", {"mha_valu": 1}), ("nosplit", {"mha_bwd_split": 0})] if dtype == BF16 else [])
    masks, refs = {}, {}
    if p == 0.0:
        refs[None] = (mr.exact(*ins), mr.magnitude(*ins))
    n = B * M * L * L
    for arm, kv in arms:
        with _knobs(**kv):
            want_path = fc.mha_path(dtype == BF16, L, kv.get("mha_valu", 0), aligned)
            key = None
            if p > 0.0:
                key = want_path          # one mask per kernel family: the VALU kernels hash per element, the MFMA kernels per quad of keys
                if key not in masks:
                    pd = _read_dropped_probs(layout, dtype, q, k, B, M, L, p, salt)
                    mask = (pd > 0).to(F64)
                    Pk = torch.softmax(mr.scores(ins[0], ins[1]), -1) / (1.0 - p)
                    # kept / dropped against the host model of csrc/drop_hash.hpp, bit for bit (the seed word of init(dtype, seed)); only a position whose
                    # reference probability is below 1e-30 is left out -- a zero read there is not a drop (the case list has none: the CPU suite checks)
                    model = torch.from_numpy((dr.mha_mfma_mask if key == 1 else dr.mha_valu_mask)(dr.context_seed(seed), salt, p, B, M, L))
                    live = Pk * (1.0 - p) >= 1e-30
                    differ = ((pd > 0) != model) & live
                    assert not bool(differ.any()), "%s %s path %d: the device keeps / drops %d of %d positions differently from the model; first at %s" % (
                        cid, arm, key, int(differ.sum()), int(live.sum()), torch.nonzero(differ)[0].tolist())
                    print("[mha sweep] %s %s path %d: mask equals the model's; %.4f of the positions left out (reference probability < 1e-30)" % (
                        cid, d, key, 1.0 - live.double().mean().item()))
                    off = ((pd - Pk * mask).abs() / (Pk * _kept_tolerance(ins[0], ins[1], dtype))).max().item()
                    p_eff = int(p * 65536.0) / 65536.0 if key == 1 else p
                    frac = 1.0 - mask.mean().item()
                    tol = 5.0 * (p * (1.0 - p) / n) ** 0.5
                    print("[mha sweep] %s %s path %d: kept weights off P / (1 - p) by %.3f of the allowed; dropped %.5f, expected %.5f +- %.5f" % (
                        cid, d, key, off, frac, p_eff, tol))
                    assert off <= 1.0, "%s %s: kept probabilities differ from P / (1 - p) by %.3g times the rounding allowed" % (cid, arm, off)
                    assert abs(frac - p_eff) <= tol, "%s %s: dropped fraction %.5f, expected %.5f +- %.5f" % (cid, arm, frac, p_eff, tol)
                    masks[key] = mask
                    refs[key] = (mr.exact(*ins, mask=mask, p=p), mr.magnitude(*ins, mask=mask, p=p))
            got = _run(layout, dtype, q, k, v, dy, B, M, L, p, salt)
            assert got["path"] == want_path, "%s %s: emrt_mha_fwd reports path %d, the mirrored rule says %d" % (cid, arm, got["path"], want_path)
            ex, mag = refs[key]
            errs = mr.worst_errors([got[t] for t in mr.TENSORS], ex, mag)
            ratios = {t: errs[t] / mr.MHA_BOUND[d][t] for t in mr.TENSORS}
            print("[mha sweep] %s %s %-10s path %d  error / bound  " % (cid, d, arm, got["path"]) + "  ".join("%s %.3f" % (t, ratios[t]) for t in mr.TENSORS))
            for t in mr.TENSORS:
                WORST[(d, arm, t)] = max(WORST.get((d, arm, t), 0.0), ratios[t])
            for t in mr.TENSORS:
                assert errs[t] <= mr.MHA_BOUND[d][t], "%s %s %s %s (B %d, M %d, L %d, %s, p %g, %s): worst per-row error %.4g, bound %.4g" % (
                    cid, d, arm, t, B, M, L, regime, p, layout, errs[t], mr.MHA_BOUND[d][t])


def _raw_bwd(dtype, bufs, B, M, L, D, path, lds):
    c = ctx()
    q, k, v, probs, dy, dq, dk, dv = bufs
    return _lib.lib().query("emrt_mha_bwd", P(q), lds[0], P(k), lds[1], P(v), lds[2], P(probs), P(dy), lds[3], P(dq), lds[4], P(dk), lds[5], P(dv), lds[6],
                            B, M, L, D, mr.SCALE, 0.0, c.seed_ptr, 3, path, dtype, c.stream)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mha_refusals_return_before_any_launch(dtype):
    """calls outside the domain return a nonzero status and leave every output as it was: L = 129, D = 16, a row stride of the VALU backward
    that is not a multiple of 8 (each of the seven), and -- bf16 -- path 1 with a dout that is only 8-byte aligned"""
    c = init(dtype)
    L_ = _lib.lib()
    B, M, L = 2, 2, 16
    E = M * 32
    R = B * 129          # every buffer holds the largest call below, refused or not
    W = E + 16

    def fresh():
        ins = [torch.zeros(R, W, dtype=c.tdtype, device="cuda") for _ in range(3)]
        probs = torch.zeros(B * M * 129 * 129, dtype=torch.float32, device="cuda")
        dy = torch.zeros(R * W + 8, dtype=c.tdtype, device="cuda")
        outs = [_filled(R, W, c.tdtype) for _ in range(4)]          # o, dq, dk, dv
        return ins, probs, dy, outs

    def untouched(outs, probs):
        torch.cuda.synchronize()
        for t in outs:
            it, pat = FILL[t.dtype]
            assert bool((t.view(it) == pat).all()), "a refused call wrote to an output"
        assert not bool(probs.any()), "a refused call wrote to `probs`"

    def fwd(ins, probs, o, L_arg, D_arg, ldo=W):
        path = ctypes.c_int(-1)
        rc = L_.query("emrt_mha_fwd", P(ins[0]), W, P(ins[1]), W, P(ins[2]), W, P(o), ldo, P(probs), B, M, L_arg, D_arg, mr.SCALE, 0.0, c.seed_ptr, 3,
                      ctypes.pointer(path), dtype, c.stream)
        return rc

    ins, probs, dy, outs = fresh()
    for L_arg, D_arg, msg in ((129, 32, "sequence length"), (L, 16, "head dim")):
        assert fwd(ins, probs, outs[0], L_arg, D_arg) != 0 and msg in L_.last_error(), L_.last_error()
        for path in ((0, 1) if dtype == BF16 else (0,)):
            assert _raw_bwd(dtype, ins + [probs, dy] + outs[1:], B, M, L_arg, D_arg, path, [W] * 7) != 0 and msg in L_.last_error(), L_.last_error()
    assert fwd(ins, probs, outs[0], L, 32, ldo=W + 4) != 0 and "multiples of 8" in L_.last_error(), L_.last_error()
    for bad in range(7):          # ldq, ldk, ldv, lddo, lddq, lddk, lddv
        lds = [W] * 7
        lds[bad] = W + 4
        assert _raw_bwd(dtype, ins + [probs, dy] + outs[1:], B, M, L, 32, 0, lds) != 0, "stride %d = %d was accepted" % (bad, W + 4)
        assert "multiples of 8" in L_.last_error(), L_.last_error()
    if dtype == BF16:
        dy8 = dy[4:4 + R * W].view(R, W)
        assert dy8.data_ptr() % 16 == 8
        assert _raw_bwd(dtype, ins + [probs, dy8] + outs[1:], B, M, L, 32, 1, [W] * 7) != 0 and "MFMA" in L_.last_error(), L_.last_error()
    untouched(outs, probs)
    # and the same operands in the domain are accepted (the refusals above are not an entry point that refuses everything)
    assert fwd(ins, probs, outs[0], L, 32) == 0, L_.last_error()
    assert _raw_bwd(dtype, ins + [probs, dy[:R * W].view(R, W)] + outs[1:], B, M, L, 32, 0 if dtype == F32 else 1, [W] * 7) == 0, L_.last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isfinite(t[:B * L, :E].float()).all())
