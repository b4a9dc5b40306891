"""CPU: the float16 ledger.  Every `extern "C"` function of emrt_amd/csrc/*.hip that reaches EMRT_REQUIRE_FWD_DTYPE -- directly or through a
file-local helper it calls -- accepts dtype 2 (float16) and must have a kernel-level float16 test: its name is a key of COVERED in
tests/test_gpu_fp16_kernels.py (value: a test function of that file) or of EXEMPT (value: the reason).  A new float16 entry point without a
test fails here, without a GPU.  Also: the helpers of tests/hip_utils.py those tests stand on, exercised on a simulated fp32 GEMM (a
round-to-nearest result passes, a truncated one fails both checks)."""
import ast
import glob
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_TESTS = os.path.join(ROOT, "tests", "test_gpu_fp16_kernels.py")
MARK = "EMRT_REQUIRE_FWD_DTYPE"


def _strip(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r'"(?:\\.|[^"\\\n])*"', lambda m: '"C"' if m.group(0) == '"C"' else '""', src)
    src = re.sub(r"'(?:\\.|[^'\\\n]){1,4}'", "' '", src)
    src = re.sub(r"^[ \t]*#(?:[^\n\\]|\\\n|\\.)*", " ", src, flags=re.M)          # preprocessor lines with their continuations
    return src


def _functions(src):
    """[(name, is_extern_c, body)] of the functions defined at file (or namespace) scope of one stripped translation unit"""
    out, depth, head_start, i, n = [], 0, 0, 0, len(src)
    transparent = []                                   # depths of `namespace x {` / `extern "C" {` blocks: their content counts as file scope
    while i < n:
        ch = src[i]
        if ch == "{":
            if depth == len(transparent):              # at file scope
                head = src[head_start:i].strip()
                if re.search(r'(namespace\s*\w*|extern\s+"C")$', head):
                    transparent.append(depth)
                    depth += 1
                    head_start = i + 1
                    i += 1
                    continue
                j, d = i + 1, 1
                while j < n and d:
                    d += {"{": 1, "}": -1}.get(src[j], 0)
                    j += 1
                body = src[i:j]
                if head.endswith(")"):
                    k, d = len(head) - 1, 0
                    while k >= 0:
                        d += {")": 1, "(": -1}.get(head[k], 0)
                        if d == 0:
                            break
                        k -= 1
                    m = re.search(r"(\w+)\s*$", head[:k])
                    if m:
                        out.append((m.group(1), 'extern "C"' in head, body))
                i = j
                head_start = i
                continue
            depth += 1
        elif ch == "}":
            depth -= 1
            if transparent and depth == transparent[-1]:
                transparent.pop()
                head_start = i + 1
        elif ch == ";" and depth == len(transparent):
            head_start = i + 1
        i += 1
    return out


def fp16_entry_points():
    """names of the extern "C" functions that reach the forward-dtype check"""
    names = set()
    for path in sorted(glob.glob(os.path.join(ROOT, "emrt_amd", "csrc", "*.hip"))):
        fns = _functions(_strip(open(path).read()))
        bodies = {}
        for name, _, body in fns:
            bodies[name] = bodies.get(name, "") + body          # (template specialisations / overloads share a name)
        reach = {name for name, body in bodies.items() if MARK in body}
        grew = True
        while grew:
            grew = False
            for name, body in bodies.items():
                if name not in reach and any(re.search(r"\b%s\s*(<[^;(){}]*>)?\s*\(" % re.escape(r), body) for r in reach):
                    reach.add(name)
                    grew = True
        names |= {name for name, ext, _ in fns if ext and name in reach}
    return names


def _ledger():
    tree = ast.parse(open(GPU_TESTS).read())
    vals, tests = {}, set()
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            tests.add(node.name)
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id in ("COVERED", "EXEMPT", "NO_DTYPE"):
            vals[node.targets[0].id] = ast.literal_eval(node.value)
    return vals["COVERED"], vals["EXEMPT"], vals["NO_DTYPE"], tests


def test_the_source_scan_sees_direct_and_indirect_entry_points():
    names = fp16_entry_points()
    assert len(names) >= 23, sorted(names)
    assert "emrt_mha_fwd" in names and "emrt_cast" in names                 # direct
    assert "emrt_conv2d" in names and "emrt_conv2d_drop" in names           # through the file-local conv2d_impl
    assert "emrt_mha_bwd" not in names and "emrt_conv2d_wgrad" not in names and "emrt_memcpy" not in names


def test_every_float16_entry_point_has_a_kernel_test_or_a_reason():
    covered, exempt, _, tests = _ledger()
    names = fp16_entry_points()
    missing = sorted(n for n in names if n not in covered and n not in exempt)
    assert not missing, "float16 entry points without a test in tests/test_gpu_fp16_kernels.py (add one and list it in COVERED): %s" % missing
    stale = sorted(n for n in list(covered) + list(exempt) if n not in names)
    assert not stale, "ledger entries that are no float16 entry point (any more): %s" % stale
    assert not set(covered) & set(exempt)
    for name, test in covered.items():
        assert test in tests, "COVERED[%r] names %r, which is not a test function of tests/test_gpu_fp16_kernels.py" % (name, test)
    for name, reason in exempt.items():
        assert isinstance(reason, str) and len(reason) > 20, name
    assert sorted(exempt) == ["emrt_conv2d_drop"], "a new exemption needs a reviewer: %s" % sorted(exempt)


def test_no_dtype_set_matches_the_header():
    from emrt_amd import _lib
    covered, exempt, no_dtype, _ = _ledger()
    protos = _lib.parse_header()
    for name in sorted(no_dtype):
        assert name in protos, "%s is not declared in include/emrt_hip.h" % name
        assert all(arg != "dtype" for _, arg in protos[name][1]), "%s takes a dtype: it belongs in COVERED or EXEMPT" % name
    for name in list(covered) + list(exempt):
        assert any(arg == "dtype" for _, arg in protos[name][1]), name


# ---- the helpers ------------------------------------------------------------------------------------------------------------------
def test_ulp16_and_round16_agree_with_torch_half():
    from tests.hip_utils import ulp16, round16
    x = torch.tensor([0.0, 2.0 ** -25, 2.0 ** -24, 6.0e-5, 2.0 ** -14, 1.0, 1.5, 2.0, 1023.9, 2048.0, 65504.0, 65519.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 0.5, 2.0, 32.0, 32.0], dtype=torch.float64)
    assert torch.equal(ulp16(x), want)
    g = torch.Generator().manual_seed(0)
    v = torch.cat([torch.randn(100000, generator=g), torch.randn(20000, generator=g) * 1e-5, torch.randn(20000, generator=g) * 4e4,
                   torch.tensor([65519.99, 65520.0, -65520.0, 2.0 ** -25, 3 * 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])]).float()
    assert torch.equal(round16(v.double()), v.half().double())            # fp32 -> half is one correctly rounded cast


def _truncate16(x):
    from tests.hip_utils import ulp16
    u = ulp16(x)
    return torch.trunc(x / u) * u


@pytest.mark.parametrize("K", [64, 2304])
def test_close_f16_and_rounding_is_nearest_tell_nearest_from_truncation(K):
    from tests.hip_utils import close_f16, rounding_is_nearest, gemm_slack, round16
    g = torch.Generator().manual_seed(K)
    a = torch.randn(512, K, generator=g).half()
    b = (torch.randn(K, 256, generator=g) / math.sqrt(K)).half()
    ref = a.double() @ b.double()
    acc32 = (a.float() @ b.float()).double()                                # an fp32 accumulation in some order
    slack = gemm_slack(K, (a.double() ** 2) @ (b.double() ** 2))
    use = close_f16("sim nearest K=%d" % K, round16(acc32), ref, slack)
    assert use < 0.5, use                                                    # (the issue's figure: at most 0.13 of the slack)
    assert abs(rounding_is_nearest("sim nearest", round16(acc32), ref)) < 0.01
    with pytest.raises(AssertionError):
        close_f16("sim truncated", _truncate16(acc32), ref, slack)
    with pytest.raises(AssertionError):
        rounding_is_nearest("sim truncated", _truncate16(acc32), ref)
    one_tap = acc32 + 0.01 * a[:, :1].double() @ b[:1].double()             # one of K products scaled by 1.01
    with pytest.raises(AssertionError):
        close_f16("sim one tap 1.01", round16(one_tap), ref, slack)


def test_close_f16_overflow_rule():
    from tests.hip_utils import close_f16
    ref = torch.tensor([65000.0, 65519.0, 65521.0, -70000.0, 1.0], dtype=torch.float64)
    ok = torch.tensor([64992.0, 65504.0, float("inf"), -float("inf"), 1.0], dtype=torch.float64)
    close_f16("overflow ok", ok, ref, 0.25)
    for i, bad in ((1, float("inf")), (2, 65504.0), (3, float("inf")), (0, float("inf"))):
        got = ok.clone()
        got[i] = bad
        with pytest.raises(AssertionError):
            close_f16("overflow bad %d" % i, got, ref, 0.25)
    close_f16("overflow band", torch.tensor([float("inf")], dtype=torch.float64), torch.tensor([65519.9], dtype=torch.float64), 0.25)
