"""ctypes binding of libemrt_hip.so, generated from include/emrt_hip.h (single source of truth): the prototypes (parse_header) and the
descriptor structs (parse_structs / struct) alike.

The product path has NO fallback: if the shared library is missing or a symbol is absent this module raises, and
every op in emrt_amd.functional raises with it.  (INTEGRATION.md shows this same stub as the reference-side binding.)
"""
import ctypes
import keyword
import os
import re
from collections import namedtuple

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "emrt_hip.h")
# EMRT_HIP_LIB: a differently built copy of the same library (developer experiments: tools/exp builds one with -DEMRT_8P_PROBES)
LIB_PATH = os.environ.get("EMRT_HIP_LIB") or os.path.join(_HERE, "csrc", "libemrt_hip.so")

# The libraries beside libemrt_hip.so.  The ABI of emrt_hip.h is frozen, and so is each side header once it has shipped, so every later feature got
# a library and a header of its own: bound from that header by side_lib(name), each loaded only when something asks for it.
# slot: the module attribute that holds the loaded library (below); env: overrides the path; prefix: of <prefix>_version / _last_error
SideLibrary = namedtuple("SideLibrary", "header path slot env prefix what")


def _side(stem, slot, env, prefix, what):
    return SideLibrary(os.path.join(os.path.dirname(_HERE), "include", "emrt_hip_%s.h" % stem),
                       os.environ.get(env) or os.path.join(_HERE, "csrc", "libemrt_hip_%s.so" % stem), slot, env, prefix, what)


SIDE_LIBRARIES = {
    "augment": _side("augment", "_AUG_LIB", "EMRT_HIP_AUGMENT_LIB", "emrt_aug", "the device augmentation"),      # vertical flip and colour distortion
    "sampler": _side("sampler", "_SMP_LIB", "EMRT_HIP_SAMPLER_LIB", "emrt_smp", "the class-aware scene sampler"),      # DATA.SCENE_SAMPLING.MODE "class"
    "loss": _side("loss", "_LOSS_LIB", "EMRT_HIP_LOSS_LIB", "emrt_lx", "the Dice + cross-entropy loss"),      # TRAIN.LOSS "DiceCrossEntropyLoss"
    "tta": _side("tta", "_TTA_LIB", "EMRT_HIP_TTA_LIB", "emrt_tta", "the test-time augmentation of whole-scene inference"),      # tta other than "none"
    "mstta": _side("mstta", "_MST_LIB", "EMRT_HIP_MSTTA_LIB", "emrt_mst", "the multi-scale test-time augmentation of whole-scene inference"),      # tta_scales
}
AUG_HEADER, SMP_HEADER, LOSS_HEADER, TTA_HEADER, MST_HEADER = (row.header for row in SIDE_LIBRARIES.values())      # (the stand-ins of the tests parse them)
# The side libraries that arrived after the suite pinned the table above to its five rows (tests/test_abi_cpu.py; build_ext.LATER_LIBRARIES is the
# build's half): the same row type, found by side_lib(name) like the others.  The two dicts become one in the first change that may edit that test.
LATER_SIDE_LIBRARIES = {
    "rot": _side("rot", "_ROT_LIB", "EMRT_HIP_ROT_LIB", "emrt_rot", "the quarter turn of the training augmentation"),      # DATA.AUGMENT.ROT90_PROB > 0
}
ROT_HEADER = LATER_SIDE_LIBRARIES["rot"].header
# That dict is pinned to its one row as well (tests/test_rot90_cpu.py).  This one is the open end (build_ext.OPEN_LIBRARIES is the build's half): its
# test asks that a row is in it and behaves like the others, never that the rows are its whole content, so the next library is one more row here.
OPEN_SIDE_LIBRARIES = {
    "bnd": _side("bnd", "_BND_LIB", "EMRT_HIP_BND_LIB", "emrt_bnd", "the boundary-aware scene evaluation"),      # SceneEvaluator(boundary=r)
}
BND_HEADER = OPEN_SIDE_LIBRARIES["bnd"].header

_TRACE = bool(int(os.environ.get("EMRT_TRACE", "0")))

_CTYPES = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
    "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
}


class EmrtHipError(RuntimeError):
    pass


def parse_header(path=HEADER):
    """-> {name: (restype_str, [(type_str, arg_name), ...])} for every prototype in the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = text.replace('extern "C" {', " ").replace("}", " ")
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(emrt_\w+)\s*\(([^)]*)\)\s*;", text):
        ret, name, args = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        arglist = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                mm = re.match(r"(.*?)(\w+)$", a)
                arglist.append((mm.group(1).strip(), mm.group(2)))
        protos[name] = (ret, arglist)
    return protos


def _ctype_of(t):
    t = t.replace("const ", "").strip()
    if t.endswith("*"):
        return ctypes.c_void_p
    if t in _CTYPES:
        return _CTYPES[t]
    raise EmrtHipError("emrt_hip.h: unknown C type %r" % t)


_MEMBER_RENAMES = {"in": "inp"}      # C member names that are Python keywords -> the attribute name the ctypes class gets
_POINTEES = ("void", "char", "unsigned char")      # what a pointer member may point to besides the scalars of _CTYPES


def member_name(struct_name, member):
    """The Python attribute of a struct member: its C name, unless that is a keyword (then the rename table must hold it)."""
    if member in _MEMBER_RENAMES:
        return _MEMBER_RENAMES[member]
    if keyword.iskeyword(member):
        raise EmrtHipError("emrt_hip.h: %s.%s: a Python keyword without an entry in the rename table" % (struct_name, member))
    return member


def parse_structs(path=HEADER):
    """-> {name: [(type_str, member, array_length or None), ...]} for every `typedef struct Name { ... } Name;` in the header, members in
    declaration order under their C names.  Anything that is not understood raises EmrtHipError naming struct and member."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    structs = {}
    found = list(re.finditer(r"\btypedef\s+struct\b\s*(\w*)\s*\{(.*?)\}\s*(\w*)\s*;", text, flags=re.S))
    if len(found) != len(re.findall(r"\btypedef\s+struct\b", text)):
        raise EmrtHipError("emrt_hip.h: a `typedef struct` that is not of the form `typedef struct Name { ... } Name;`")
    for m in found:
        tag, body, name = m.group(1), m.group(2), m.group(3)
        if tag != name or not name:
            raise EmrtHipError("emrt_hip.h: struct tag %r and typedef name %r differ" % (tag, name))
        members = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            first, *more = [d.strip() for d in decl.split(",")]
            mm = re.match(r"^([\w\s\*]+?)\s*\b(\w+)\s*(?:\[\s*(\d+)\s*\])?$", first)
            if mm is None:          # a nested struct / union body, a bit-field, a function pointer, ...
                raise EmrtHipError("emrt_hip.h: %s: cannot parse the member declaration %r" % (name, decl))
            ctype = re.sub(r"\s*\*\s*", "*", mm.group(1).strip())
            declared = [(mm.group(2), mm.group(3))]
            for d in more:
                md = re.match(r"^(\w+)\s*(?:\[\s*(\d+)\s*\])?$", d)
                if md is None or ctype.endswith("*"):      # `T *a, *b` (and `T* a, b`, whose b is no pointer)
                    raise EmrtHipError("emrt_hip.h: %s.%s: one pointer member per declaration, written `T* name`" % (name, d.lstrip("* ")))
                declared.append((md.group(1), md.group(2)))
            base = ctype.replace("const ", "").rstrip("*").strip()
            if base not in _CTYPES and not (ctype.endswith("*") and (base in _POINTEES or base in structs)):
                raise EmrtHipError("emrt_hip.h: %s.%s: unknown C type %r" % (name, declared[0][0], ctype))
            for member, count in declared:
                member_name(name, member)
                members.append((ctype, member, int(count) if count else None))
        structs[name] = members
    return structs


_STRUCTS = {}      # header path -> {name: the one ctypes.Structure subclass of that header struct}


def _struct_of(header, name):
    h = os.path.basename(header)
    if header not in _STRUCTS:
        _STRUCTS[header] = {
            sname: type(sname, (ctypes.Structure,), {"_fields_": [(member_name(sname, m), _ctype_of(t) * n if n else _ctype_of(t)) for t, m, n in members],
                                                     "__doc__": "%s of include/%s" % (sname, h)})
            for sname, members in parse_structs(header).items()}
    if name not in _STRUCTS[header]:
        raise EmrtHipError("%s declares no struct %s" % (h, name))
    return _STRUCTS[header][name]


def struct(name):
    """The ctypes.Structure subclass of a descriptor struct of the header, generated once: (struct(n) * k) is the same array type in every
    module.  Pointer members are c_void_p (None, an int address or data_ptr() all assign)."""
    return _struct_of(HEADER, name)


def augment_struct(name):
    """The same for a descriptor struct of include/emrt_hip_augment.h."""
    return _struct_of(AUG_HEADER, name)


def _bind(obj, dll, path, header):
    """Gives obj a `_raw_<name>` ctypes function for every prototype of the header; -> the prototypes.  A symbol the library lacks raises."""
    protos = parse_header(header)
    for name, (ret, args) in protos.items():
        try:
            fn = getattr(dll, name)
        except AttributeError:
            raise EmrtHipError("%s does not export %s declared in %s" % (os.path.basename(path), name, os.path.basename(header)))
        fn.argtypes = [_ctype_of(t) for t, _ in args]
        fn.restype = ctypes.c_char_p if ret == "const char*" else (ctypes.c_size_t if ret == "size_t" else ctypes.c_int)
        setattr(obj, "_raw_" + name, fn)
    return protos


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise EmrtHipError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU/PyTorch fallback for the EMRT hot path)" % LIB_PATH)
        # torch first: the library must bind to the HIP runtime torch has loaded (torch's streams and device memory are handed to it).
        # Loaded before torch it pulls in /opt/rocm's copy, torch then brings its bundled one, and launches fail with "no ROCm-capable
        # device is detected" (seen when build() and smoke() ran in one process).
        import torch  # noqa: F401
        self._dll = ctypes.CDLL(LIB_PATH)
        self._rec = None
        self.empty_pair_ms = 0.0
        self.replay_total_ms = 0.0
        self.protos = _bind(self, self._dll, LIB_PATH, HEADER)

    def last_error(self):
        return self._raw_emrt_last_error().decode("utf-8", "replace")

    # ---- launch recording / timed replay (bench.py) ------------------------------------------------------------
    # In eager mode the host needs ~20-30 us of Python per launch, so a HIP-event pair around a single small kernel
    # measures the HOST, not the GPU.  Instead the launches of one step are recorded (name + C arguments; the runtime
    # keeps every temporary alive meanwhile) and then replayed from a tight ctypes loop: once untimed as a backlog so the
    # host runs ahead of the GPU, then again with a HIP-event pair -- on the launch stream -- around every launch.
    def start_record(self):
        self._rec = []

    def stop_record(self):
        rec, self._rec = self._rec, None
        return rec

    def replay(self, rec, timed=False):
        """Re-issue recorded launches.  timed=True -> [(name, args, milliseconds)] from per-launch HIP events."""
        import torch
        raw = [(getattr(self, "_raw_" + n), a, n) for n, a in rec]
        if not timed:
            for fn, a, n in raw:
                rc = fn(*a)
                if rc != 0:
                    raise EmrtHipError("%s failed during replay (%d): %s" % (n, rc, self.last_error()))
            return None
        evs = []
        for fn, a, n in raw:
            e0 = self._event(a[-1])
            fn(*a)
            evs.append((e0, self._event(a[-1])))
        # calibration: the same event pair around NOTHING, 64 times behind the same backlog -- what the clock itself adds to every figure
        # (kept in self.empty_pair_ms, median; bench.py subtracts it per launch to put its roofline on the kernel-duration clock rocprofv3 reports)
        stream = raw[-1][1][-1] if raw else None
        empty = []
        if stream is not None:
            for _ in range(64):
                e0 = self._event(stream)
                empty.append((e0, self._event(stream)))
        torch.cuda.synchronize()
        out, ms = [], ctypes.c_float(0.0)
        for (n, a), (e0, e1) in zip(rec, evs):
            self._raw_emrt_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            out.append((n, a, ms.value))
            self._raw_emrt_event_destroy(e0)
            self._raw_emrt_event_destroy(e1)
        gaps = []
        for e0, e1 in empty:
            self._raw_emrt_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            gaps.append(ms.value)
            self._raw_emrt_event_destroy(e0)
            self._raw_emrt_event_destroy(e1)
        self.empty_pair_ms = sorted(gaps)[len(gaps) // 2] if gaps else 0.0
        # the SAME launch list once more with ONE event pair around all of it (behind a backlog pass, so the host is ahead of the GPU): the time the
        # step's kernels take back to back.  sum(per-launch readings) - this = what the per-launch pairs added in total (bench.py spreads it evenly)
        self.replay_total_ms = 0.0
        if stream is not None:
            for fn, a, n in raw:
                fn(*a)
            e0 = self._event(stream)
            for fn, a, n in raw:
                fn(*a)
            e1 = self._event(stream)
            torch.cuda.synchronize()
            self._raw_emrt_event_elapsed_ms(e0, e1, ctypes.byref(ms))
            self.replay_total_ms = ms.value
            self._raw_emrt_event_destroy(e0)
            self._raw_emrt_event_destroy(e1)
        return out

    def _event(self, stream):
        ev = ctypes.c_void_p()
        self._raw_emrt_event_create(ctypes.byref(ev))
        self._raw_emrt_event_record(ev, stream)
        return ev

    def call(self, name, *args):
        """Invoke an int-returning entry point; raise EmrtHipError on a non-zero return.
        EMRT_TRACE=1 prints every call before launching it and synchronises after it (locates GPU faults)."""
        if _TRACE:
            print("[emrt] %s%r" % (name, tuple(a.value if hasattr(a, "value") else a for a in args)), flush=True)
        if self._rec is not None:
            self._rec.append((name, args))
        rc = getattr(self, "_raw_" + name)(*args)
        if rc != 0:
            raise EmrtHipError("%s failed (%d): %s" % (name, rc, self.last_error()))
        if _TRACE:
            import torch
            torch.cuda.synchronize()

    def set_tuning(self, name, value):
        """Developer / test knob of the kernel dispatchers (include/emrt_hip.h: emrt_set_tuning); returns the old value."""
        old = ctypes.c_int(0)
        if self._raw_emrt_get_tuning(name.encode(), ctypes.byref(old)) != 0 or self._raw_emrt_set_tuning(name.encode(), int(value)) != 0:
            raise EmrtHipError(self.last_error())
        return old.value

    def query(self, name, *args):
        return getattr(self, "_raw_" + name)(*args)


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB


# ---- the side libraries ---------------------------------------------------------------------------------------------------------------------------

class _ExtLib:
    """A library beside libemrt_hip.so (a row of SIDE_LIBRARIES, LATER_SIDE_LIBRARIES or OPEN_SIDE_LIBRARIES), bound from its own header: call / query / last_error as _Lib, with the
    library's own `<prefix>_last_error` string and its `<prefix>_version` checked to be 1.  No fallback: a missing library or symbol raises."""

    def __init__(self, path, header, prefix, what):
        if not os.path.exists(path):
            raise EmrtHipError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU/PyTorch fallback for %s)" % (path, what))
        import torch  # noqa: F401      (torch first, for the reason given in _Lib.__init__)
        self._dll = ctypes.CDLL(path)
        self.protos = _bind(self, self._dll, path, header)
        self._last_error = getattr(self, "_raw_%s_last_error" % prefix)
        version = getattr(self, "_raw_%s_version" % prefix)()
        if version != 1:
            raise EmrtHipError("%s has version %d, this binding expects 1" % (os.path.basename(path), version))

    def last_error(self):
        return self._last_error().decode("utf-8", "replace")

    def call(self, name, *args):
        """Invoke an int-returning entry point; raise EmrtHipError on a non-zero return (EMRT_TRACE=1 as _Lib.call)."""
        if _TRACE:
            print("[emrt] %s%r" % (name, tuple(a.value if hasattr(a, "value") else a for a in args)), flush=True)
        rc = getattr(self, "_raw_" + name)(*args)
        if rc != 0:
            raise EmrtHipError("%s failed (%d): %s" % (name, rc, self.last_error()))
        if _TRACE:
            import torch
            torch.cuda.synchronize()

    def query(self, name, *args):
        return getattr(self, "_raw_" + name)(*args)


# The loaded side libraries, one module attribute per row (its `slot`): None until somebody asks for that library.  The tests put their stand-ins here.
_AUG_LIB = _SMP_LIB = _LOSS_LIB = _TTA_LIB = _MST_LIB = _ROT_LIB = _BND_LIB = None


def side_libraries():
    """SIDE_LIBRARIES, LATER_SIDE_LIBRARIES and OPEN_SIDE_LIBRARIES as one dict, in the order build_ext.all_libraries() builds them."""
    return {**SIDE_LIBRARIES, **LATER_SIDE_LIBRARIES, **OPEN_SIDE_LIBRARIES}


def side_lib(name):
    row, slots = side_libraries()[name], globals()
    if slots[row.slot] is None:
        slots[row.slot] = _ExtLib(row.path, row.header, row.prefix, row.what)
    return slots[row.slot]


def augment_lib():
    return side_lib("augment")


def sampler_lib():
    return side_lib("sampler")


def loss_lib():
    return side_lib("loss")


def tta_lib():
    return side_lib("tta")


def mst_lib():
    return side_lib("mstta")


def rot_lib():
    return side_lib("rot")


def bnd_lib():
    return side_lib("bnd")
