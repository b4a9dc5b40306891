"""CPU: the C-ABI shared library loads and exports exactly what include/emrt_hip.h declares; the header's prototypes are
the definitions' prototypes and the generated descriptor classes have the compiled layout (no compute calls -- there is no GPU here)."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from emrt_amd import build_ext
    return build_ext.build(verbose=False)


def test_library_exports_every_declared_symbol(built):
    from emrt_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 50
    out = subprocess.run(["nm", "-D", "--defined-only", built], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [n for n in protos if n not in exported]
    assert not missing, missing
    undeclared = [n for n in exported if n.startswith("emrt_") and n not in protos]
    assert not undeclared, "exported but not declared in emrt_hip.h: %s" % undeclared


def test_header_matches_definitions():
    from emrt_amd import _lib
    protos = _lib.parse_header()
    defs = {}
    for f in glob.glob(os.path.join(ROOT, "emrt_amd/csrc/*.hip")):
        s = open(f).read()
        for m in re.finditer(r'extern "C" ([^{;]+?)\{', s, re.S):
            p = re.sub(r"/\*.*?\*/", "", " ".join(m.group(1).split()))
            name = re.search(r"(\w+)\s*\(", p).group(1)
            args = p[p.index("(") + 1:p.rindex(")")]
            types = [] if args.strip() in ("", "void") else [re.match(r"(.*?)(\w+)$", " ".join(a.split())).group(1).strip() for a in args.split(",")]
            defs[name] = types
    assert set(defs) == set(protos)
    for name, (ret, args) in protos.items():
        assert [t for t, _ in args] == defs[name], name


def _host_cxx():
    """the clang++ that sits beside the hipcc build_ext uses (host-only compiles: no offload arch, nothing GPU)"""
    from emrt_amd import build_ext
    hipcc = shutil.which(build_ext._hipcc())
    assert hipcc, "hipcc not found"
    d = os.path.dirname(os.path.realpath(hipcc))
    for cand in ("amdclang++", "../llvm/bin/clang++", "../lib/llvm/bin/clang++", "clang++"):
        if os.path.exists(os.path.join(d, cand)):
            return os.path.normpath(os.path.join(d, cand))
    raise AssertionError("no clang++ beside %s" % hipcc)


def test_generated_structs_have_the_compiled_layout(tmp_path):
    """sizeof and every offsetof, as the C++ compiler lays include/emrt_hip.h out, against the ctypes classes generated from the same header"""
    from emrt_amd import _lib
    structs = _lib.parse_structs()
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "emrt_hip.h"', "int main() {"]
    for name, members in structs.items():
        lines.append('  std::printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['  std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, m, name, m) for _, m, _ in members]
    (tmp_path / "layout.cpp").write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.run([_host_cxx(), "-std=c++17", "-I", os.path.dirname(_lib.HEADER), str(tmp_path / "layout.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    compiled = dict(line.split() for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    generated = {}
    for name, members in structs.items():
        S = _lib.struct(name)
        generated[name] = str(ctypes.sizeof(S))
        generated.update({"%s.%s" % (name, m): str(getattr(S, _lib.member_name(name, m)).offset) for _, m, _ in members})
    assert len(generated) == 8 + 151 and generated == compiled


def test_no_struct_of_the_header_escapes_the_parser():
    from emrt_amd import _lib
    structs = _lib.parse_structs()
    assert len(structs) == len(re.findall(r"typedef\s+struct", open(_lib.HEADER).read())) == 8
    # a prototype parameter is a scalar, a pointer to one (or to void / char), or a pointer to a parsed struct
    builtin = {"void", "char", "short", "int", "long", "unsigned", "signed", "float", "double", "size_t"}
    named = set()
    for name, (ret, args) in _lib.parse_header().items():
        for t, a in args:
            base = t.replace("const", "").replace("*", "").strip()
            if not set(base.split()) <= builtin:
                assert base in structs and t.endswith("*"), "%s.%s: %r" % (name, a, t)
                named.add(base)
    assert named == set(structs)
    assert len(_lib.parse_header()) == 109


@pytest.mark.parametrize("body, offender", [
    ("typedef struct A { int n; half x; } A;", r"A\.x.*half"),                        # an unknown member type
    ("typedef struct A { int n; float lambda; } A;", r"A\.lambda"),                   # a keyword member other than `in`
    ("typedef struct A { int n; } B;", r"'A'.*'B'"),                                  # tag and typedef name differ
    ("typedef struct A { float *a, *b; int n; } A;", r"A\.b"),                        # the `T *a, *b` form
    ("typedef struct A { int n; unsigned flags : 3; } A;", r"A: .*flags"),            # a bit-field
    ("typedef struct A { struct { int a; } inner; int n; } A;", r"A"),                # a nested struct
])
def test_struct_parser_refuses_what_it_does_not_understand(tmp_path, body, offender):
    from emrt_amd import _lib
    h = tmp_path / "snippet.h"
    h.write_text("/* a header */\ntypedef struct Ok { const void* in; long long m[4]; int a, b; } Ok;\n" + body + "\n")
    with pytest.raises(_lib.EmrtHipError, match=offender):
        _lib.parse_structs(str(h))
    h.write_text("typedef struct Ok { const void* in; long long m[4]; int a, b; } Ok;\n")
    assert _lib.parse_structs(str(h)) == {"Ok": [("const void*", "in", None), ("long long", "m", 4), ("int", "a", None), ("int", "b", None)]}
    assert _lib.member_name("Ok", "in") == "inp"


def test_one_class_per_struct_everywhere():
    from emrt_amd import _lib
    from emrt_amd import functional as Fn
    from emrt_amd.src import datasets
    from emrt_amd.src.models import solver
    for n in _lib.parse_structs():
        assert _lib.struct(n) is _lib.struct(n) and issubclass(_lib.struct(n), ctypes.Structure)
    assert (_lib.struct("EmrtConvDesc") * 3) is (Fn._ConvDesc * 3)
    users = {"EmrtConvDesc": Fn._ConvDesc, "EmrtConvBwdDesc": Fn._ConvBwdDesc, "EmrtConvDgradDesc": Fn._DgradDesc, "EmrtWgradDesc": Fn._WgradDesc,
             "EmrtBnGroupDesc": Fn._BnGroupDesc, "EmrtAugDesc": Fn._AugDesc, "EmrtSceneEntry": datasets._SceneEntry, "EmrtLrSchedule": solver.EmrtLrSchedule}
    # tools/bench_conv.py opens the GPU on import: the right-hand side of its `_WD = ...` line is evaluated instead
    tree = ast.parse(open(os.path.join(ROOT, "tools", "bench_conv.py")).read())
    (wd,) = [n.value for n in tree.body if isinstance(n, ast.Assign) and [t.id for t in n.targets if isinstance(t, ast.Name)] == ["_WD"]]
    assert eval(compile(ast.Expression(wd), "bench_conv.py", "eval"), {"_lib": _lib}) is _lib.struct("EmrtWgradDesc")
    for n, cls in users.items():
        assert cls is _lib.struct(n), n
    assert set(users) == set(_lib.parse_structs())
    with pytest.raises(_lib.EmrtHipError, match="EmrtNoSuchDesc"):
        _lib.struct("EmrtNoSuchDesc")


def test_loader_binds_all_entry_points(built):
    from emrt_amd import _lib
    _lib._LIB = None
    L = _lib.lib()
    assert L.query("emrt_abi_version") == 9
    assert L.query("emrt_colreduce_workspace_bytes", 1000, 256) > 0
    import ctypes
    small = (ctypes.c_int * 6)(2, 2, 2, 2, 1, 2)                   # Lv = 10
    base = lambda B, Lq, M: ((B * Lq * M * 18 + 512 + 2 * B * M + B * M * max((Lq + 63) // 64, 64) + 3) // 4 * 4) * 4     # probabilities + max |dout| partials (>= 64 per (batch, head): row bands)
    assert L.query("emrt_msda_bwd_workspace_bytes", 2, 10, 8, 3, 6, ctypes.cast(small, ctypes.c_void_p), 1) == base(2, 10, 8)
    # batch 8 at 256x256 (Lv = 1344): no range of the value-gradient scatter is split by queries -> no partial slabs
    cfg2 = (ctypes.c_int * 6)(32, 32, 16, 16, 8, 8)
    assert L.query("emrt_msda_bwd_workspace_bytes", 8, 1344, 8, 3, 6, ctypes.cast(cfg2, ctypes.c_void_p), 1) == base(8, 1344, 8)
    # batch 4 at 512x512 (Lv = 5376), bf16: level 1 (2 ranges x 3 query splits) and level 2 (5 splits) leave int32 partial slabs;
    # the fp32 path never splits
    cfg3 = (ctypes.c_int * 6)(64, 64, 32, 32, 16, 16)
    part = 4 * 8 * (2 * 3 * 512 * 32 + 5 * 256 * 32) * 4
    assert L.query("emrt_msda_bwd_workspace_bytes", 4, 5376, 8, 3, 6, ctypes.cast(cfg3, ctypes.c_void_p), 1) == base(4, 5376, 8) + part
    assert L.query("emrt_msda_bwd_workspace_bytes", 4, 5376, 8, 3, 6, ctypes.cast(cfg3, ctypes.c_void_p), 0) == base(4, 5376, 8)
    # without the level shapes the size would leave the partial slabs out -> an error, not a too-small answer
    assert L.query("emrt_msda_bwd_workspace_bytes", 4, 5376, 8, 3, 6, None, 1) == 0 and "level shapes" in L.last_error()
    assert L.query("emrt_msda_bwd_workspace_bytes", 4, 5376, 8, 5, 6, ctypes.cast(cfg3, ctypes.c_void_p), 1) == 0
    # adaptive pooling: no workspace for small maps / odd channel counts; 256x256 tiles (32x32 map, scales 1 2 3 6): 8 + 4*2 + 9 + 36 slots
    sc = (ctypes.c_int * 4)(1, 2, 3, 6)
    scp = ctypes.cast(sc, ctypes.c_void_p)
    assert L.query("emrt_adaptive_avgpool_workspace_bytes", 16, 16, 8, 256, scp, 4) == 0
    assert L.query("emrt_adaptive_avgpool_workspace_bytes", 32, 32, 8, 250, scp, 4) == 0
    assert L.query("emrt_adaptive_avgpool_workspace_bytes", 32, 32, 8, 256, scp, 4) == 8 * (9 + 4 * 3 + 9 * 2 + 36) * 256 * 4
    assert L.query("emrt_adaptive_avgpool_workspace_bytes", 32, 32, 8, 256, None, 4) == 0


def test_abi6_entry_points_refuse_bad_arguments_before_any_launch(built):
    """Argument checks of the round-4 entry points run on the host before anything touches a device: a bad call returns non-zero with a
    message (no GPU here; the pointers are never dereferenced)."""
    from emrt_amd import _lib
    _lib._LIB = None
    L = _lib.lib()
    p = ctypes.c_void_p(0x10000)          # "a device pointer": aligned, never read
    bn = (p, 64.0, 1e-5, 0.9, p, p, p, p, p, p, 1)      # sums, count, eps, momentum, mean, invstd, run_mean, run_var, gamma, beta, relu

    def refused(name, *args, match):
        with pytest.raises(_lib.EmrtHipError, match=match):
            L.call(name, *args)

    # classifier: C outside {64, 128, 256}; more than 8 outputs
    refused("emrt_bn_pointwise_fwd", p, 96, 96 * 64, p, None, p, 6, 6 * 64, 1, 64, 96, 6, *bn, 1, None, match="C in")
    refused("emrt_bn_pointwise_fwd", p, 256, 256 * 64, p, None, p, 9, 9 * 64, 1, 64, 256, 9, *bn, 1, None, match="OC <= 8")
    refused("emrt_bn_pointwise_bwd", p, 256, 256 * 64, p, 9, 9 * 64, p, p, 256, 256 * 64, p, None, None, 1, 64, 256, 9, p, p, p, p, 1, None, match="OC <= 8")
    # resize / max-pool with a BatchNorm operand: off the vector path, missing sums, non-positive count
    refused("emrt_bn_resize_bilinear_fwd", p, 6 * 16, 6, 4, 4, p, 6 * 64, 6, 8, 8, 1, 6, 0, *bn, 1, None, match="vector path")
    nosums = (None,) + bn[1:]
    refused("emrt_bn_resize_bilinear_fwd", p, 64 * 16, 64, 4, 4, p, 64 * 64, 64, 8, 8, 1, 64, 0, *nosums, 1, None, match="BatchNorm operand")
    zerocount = (p, 0.0) + bn[2:]
    refused("emrt_bn_maxpool_fwd", p, p, p, 1, 8, 8, 64, 3, 2, 1, *zerocount, 1, None, match="BatchNorm operand")
    refused("emrt_bn_maxpool_fwd", p, p, p, 1, 8, 8, 60, 3, 2, 1, *bn, 1, None, match="vector path")
    # the join: the shortcut's BatchNorm is not optional
    refused("emrt_bn_apply_join", p, 64, p, 64, p, 64, p, 64.0, 1e-5, 0.9, p, p, p, p, p, p, None, 64.0, 1e-5, 0.9, p, p, p, p, p, p, 64, 64, 1, 1, None,
            match="shortcut")
    # mask arguments come as a pair and replace y
    refused("emrt_bn_bwd_reduce", p, 64, p, 64, None, 0, p, p, 64, 64, p, p, None, 1, None, match="come together")
    refused("emrt_bn_bwd_reduce", p, 64, p, 64, p, 64, p, p, 64, 64, p, p, p, 1, None, match="replace y")
    refused("emrt_bn_bwd_dx", p, 64, p, 64, p, 64, p, 64, None, 64, p, p, p, p, None, 64.0, None, None, 64, 64, None, 0, p, 1, None, match="mask_beta")
    # pooling workspace smaller than the query's answer
    sc = (ctypes.c_int * 4)(1, 2, 3, 6)
    scp = ctypes.cast(sc, ctypes.c_void_p)
    need = L.query("emrt_adaptive_avgpool_workspace_bytes", 32, 32, 8, 256, scp, 4)
    refused("emrt_adaptive_avgpool_fwd", p, 32 * 32 * 256, 256, 32, 32, p, 50 * 256, 256, 8, 256, scp, 4, p, need - 4, 1, None, match="workspace smaller")


# the entry points whose FIRST check is the dtype check, by the macro they carry (csrc/common.hpp)
DTYPE_FIRST_FWD = [          # EMRT_REQUIRE_FWD_DTYPE: f32, bf16 and f16
    "emrt_acc3d", "emrt_adaptive_avgpool_fwd", "emrt_add", "emrt_add3d", "emrt_add_f32row", "emrt_add_f32row_levels", "emrt_bn_apply", "emrt_cast",
    "emrt_concat_tokens", "emrt_groupnorm_fwd", "emrt_groupnorm_levels_fwd", "emrt_layernorm_fwd", "emrt_maxpool_fwd", "emrt_mha_fwd", "emrt_msda_fwd",
    "emrt_nchw_to_nhwc", "emrt_pack_weights", "emrt_pyramid_resize_fwd", "emrt_resize_bilinear_fwd",
]
DTYPE_FIRST_TRAIN = [        # EMRT_REQUIRE_TRAIN_DTYPE: f32 and bf16, f16 is refused as inference-only
    "emrt_adaptive_avgpool_bwd", "emrt_bn_apply_join", "emrt_bn_bwd_dx", "emrt_bn_bwd_reduce", "emrt_bn_group_apply", "emrt_bn_group_bwd",
    "emrt_bn_maxpool_fwd", "emrt_bn_pointwise_bwd", "emrt_bn_pointwise_fwd", "emrt_bn_resize_bilinear_fwd", "emrt_bn_stats", "emrt_colsum_acc",
    "emrt_colsum_levels_multi", "emrt_conv2d_bna", "emrt_conv2d_drop", "emrt_dropout_fwd", "emrt_gconv2d_bwd", "emrt_groupnorm_bwd",
    "emrt_groupnorm_levels_bwd", "emrt_layernorm_bwd", "emrt_mask_bwd", "emrt_maxpool_bwd", "emrt_mha_bwd", "emrt_msda_bwd", "emrt_pyramid_resize_bwd",
    "emrt_resize_bilinear_bwd",
]


def _dtype_first_in_sources():
    """{name: "FWD" | "TRAIN"} of the extern "C" functions of csrc/*.hip whose first statement is an EMRT_REQUIRE_*_DTYPE line"""
    found = {}
    for f in glob.glob(os.path.join(ROOT, "emrt_amd/csrc/*.hip")):
        for m in re.finditer(r'extern "C" int (emrt_\w+)\([^{]*\)\s*\{\s*EMRT_REQUIRE_(FWD|TRAIN)_DTYPE\(dtype\);', open(f).read()):
            found[m.group(1)] = m.group(2)
    return found


def test_dtype_first_lists_match_the_sources():
    found = _dtype_first_in_sources()
    assert sorted(n for n, k in found.items() if k == "FWD") == sorted(DTYPE_FIRST_FWD)
    assert sorted(n for n, k in found.items() if k == "TRAIN") == sorted(DTYPE_FIRST_TRAIN)
    assert len(DTYPE_FIRST_FWD) + len(DTYPE_FIRST_TRAIN) == 45


@pytest.mark.parametrize("name", DTYPE_FIRST_FWD + DTYPE_FIRST_TRAIN)
def test_dtype_refusals_name_the_entry_point(built, name):
    """The dtype check is the first check of these entry points and returns before anything else is looked at: every pointer is null and every
    number 0 here (nothing is launched, nothing dereferenced; no GPU needed).  An unknown code (3) is refused under the entry point's own name;
    float16 (2) is refused as inference-only by the training entry points and passes the dtype check of the entry points of the float16 ledger
    (COVERED and EXEMPT of tests/test_gpu_fp16_kernels.py), which then stop at a later argument check.  emrt_conv2d_drop is in both groups: it
    is EXEMPT from a float16 kernel test BECAUSE its EMRT_REQUIRE_TRAIN_DTYPE line refuses float16, so the inference-only answer is the one
    asserted for it."""
    from emrt_amd import _lib
    from tests.test_fp16_ledger_cpu import _ledger
    L = _lib.lib()
    ret, args = _lib.parse_header()[name]
    assert ret == "int" and [a for _, a in args].count("dtype") == 1

    def refusal(dtype):
        vals = [dtype if a == "dtype" else (None if t.endswith("*") else (0.0 if t in ("float", "double") else 0)) for t, a in args]
        with pytest.raises(_lib.EmrtHipError) as e:
            L.call(name, *vals)
        text = str(e.value)
        assert text.startswith(name + " failed") and "launch failed" not in text, text
        return text

    text = refusal(3)
    assert ": %s: dtype must be" % name in text, text
    text = refusal(2)
    covered, exempt, _, _ = _ledger()
    if name in DTYPE_FIRST_TRAIN:
        assert ": %s: dtype must be" % name in text and "inference-only" in text, text
    else:
        assert name in covered or name in exempt, name
        assert "dtype must be" not in text and "inference-only" not in text, text


def test_the_one_table_of_libraries(built):
    """build_ext.LIBRARIES is the six libraries in build order, _lib.SIDE_LIBRARIES the five beside the first under the same names; every library
    and its stamp exist, every stamp is the one digest, and every public header is an input of every object."""
    from emrt_amd import _lib, build_ext
    assert [os.path.basename(row.lib) for row in build_ext.LIBRARIES] == [
        "libemrt_hip.so", "libemrt_hip_augment.so", "libemrt_hip_sampler.so", "libemrt_hip_loss.so", "libemrt_hip_tta.so", "libemrt_hip_mstta.so"]
    assert build_ext.LIBRARIES[0][1:] == (build_ext.LIB, build_ext.CSRC, build_ext.SOURCES, build_ext.HEADER) and _lib.HEADER == build_ext.HEADER
    assert [row.name for row in build_ext.LIBRARIES[1:]] == list(_lib.SIDE_LIBRARIES)
    digest = build_ext.source_digest()
    for row in build_ext.LIBRARIES:
        assert build_ext.library(row.name) is row and all(os.path.exists(os.path.join(row.dir, s)) for s in row.sources)
        with open(row.lib + ".inputs") as f:
            assert os.path.exists(row.lib) and f.read().strip() == digest, row.lib
        assert row.header in build_ext._headers()
    for name, side in _lib.SIDE_LIBRARIES.items():
        assert (side.header, side.path) == (build_ext.library(name).header, os.environ.get(side.env) or build_ext.library(name).lib)
        assert hasattr(_lib, side.slot) and [s.slot for s in _lib.SIDE_LIBRARIES.values()].count(side.slot) == 1
    with pytest.raises(KeyError):
        build_ext.library("nope")


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from emrt_amd import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_LIB", None)
    with pytest.raises(_lib.EmrtHipError):
        _lib.lib()


def test_product_never_imports_the_oracle():
    for f in glob.glob(os.path.join(ROOT, "emrt_amd/**/*.py"), recursive=True):
        src = open(f).read()
        assert "import oracle" not in src and "from oracle" not in src, f


def test_build_is_keyed_on_the_content_of_its_inputs(tmp_path):
    """build_ext decides what to rebuild from a sha256 of the sources, headers, compiler path and flags recorded beside every object and the
    library (not from modification times, which mean nothing once the built files have travelled to another machine): an untouched tree is
    "reused" whatever the timestamps say, and the recorded digest is the digest of the tree."""
    import os
    from emrt_amd import build_ext
    build_ext.build(verbose=False)
    assert build_ext.LAST_BUILD["mode"] in ("reused", "linked", "compiled")
    # timestamps shuffled: the sources now look newer than the objects -- still nothing to do
    for src in build_ext.SOURCES:
        os.utime(os.path.join(build_ext.CSRC, src), None)
    build_ext.build(verbose=False)
    assert build_ext.LAST_BUILD["mode"] == "reused" and build_ext.LAST_BUILD["compiled"] == []
    assert build_ext.LAST_BUILD["digest"] == build_ext.source_digest()
    with open(build_ext.LIB + ".inputs") as f:
        assert f.read().strip() == build_ext.source_digest()
    # a different flag set (or source byte) is a different digest
    assert build_ext._digest([os.path.join(build_ext.CSRC, build_ext.SOURCES[0])], ["x"]) != build_ext._digest([os.path.join(build_ext.CSRC, build_ext.SOURCES[0])], ["y"])
