"""Recording stand-in for libemrt_hip.so used by the CPU tests of the HOST logic only (shapes, strides, tape order,
argument marshalling).  It computes nothing: every entry point validates its argument count/types against
include/emrt_hip.h and logs the call.  The product never uses it."""
import ctypes

import torch

from emrt_amd import _lib
from emrt_amd import runtime


class FakeLib:
    def __init__(self):
        self.protos = _lib.parse_header()
        self.structs = _lib.parse_structs()
        self.calls = []

    def _check(self, name, args):
        ret, spec = self.protos[name]
        assert len(args) == len(spec), "%s: %d args given, header declares %d" % (name, len(args), len(spec))
        for a, (t, an) in zip(args, spec):
            if t.replace("const ", "").rstrip("* ") in self.structs:
                # a descriptor table: a host array of exactly the generated class, or a plain address (a table in device memory, a cast host table)
                S = _lib.struct(t.replace("const ", "").rstrip("* "))
                assert a is None or isinstance(a, (ctypes.c_void_p, int)) or (isinstance(a, ctypes.Array) and a._type_ is S), \
                    "%s.%s: expected an array of %s, got %r" % (name, an, S.__name__, a)
            elif t.endswith("*"):
                assert a is None or isinstance(a, (ctypes.c_void_p, int)) or hasattr(a, "_type_"), "%s.%s: bad pointer %r" % (name, an, a)
            elif t in ("float", "double"):
                assert isinstance(a, (int, float)), "%s.%s: expected number, got %r" % (name, an, type(a))
            else:
                assert isinstance(a, int) and not isinstance(a, bool) or isinstance(a, bool), "%s.%s (%s): expected int, got %r" % (name, an, t, type(a))

    def call(self, name, *args):
        self._check(name, args)
        self.calls.append((name, args))

    def query(self, name, *args):
        self._check(name, args)
        return 1 << 16

    def last_error(self):
        return ""

    def canonical_log(self):
        return canonical_log(self.calls)


def _canon(v, ctype, structs, member_name):
    """one value of the canonical log: scalars by value, addresses as null / their residue modulo 16 (allocations move between runs, the offsets
    of views inside them do not), host arrays element by element and descriptors member by member (the header's struct members) under the same rule"""
    base = ctype.replace("const ", "").rstrip("* ")
    if isinstance(v, ctypes.Array) and base in structs:
        return "[%s]" % ", ".join("{%s}" % ", ".join("%s=%s" % (m, _canon(getattr(e, member_name(base, m)), t, structs, member_name)) for t, m, _n in structs[base]) for e in v)
    if isinstance(v, ctypes.Array):
        return "[%s]" % ", ".join(_canon(e, "void*" if v._type_ is ctypes.c_void_p else base, structs, member_name) for e in v)
    if ctype.endswith("*"):
        if isinstance(v, ctypes._Pointer):      # (ctypes.pointer(obj): an output argument)
            v = ctypes.cast(v, ctypes.c_void_p)
        v = getattr(v, "value", v)
        return "null" if not v else "ptr%%16=%d" % (v % 16)
    v = getattr(v, "value", v)
    return repr(int(v) if isinstance(v, bool) else v)


def canonical_log(calls, binding=_lib):
    """The recorded calls [(name, args)] as text that two checkouts can be compared by, one line per call: entry point, then every argument under
    its header name.  binding: the _lib module whose header describes the calls (tools/launch_log.py passes this tree's for another checkout's recording)."""
    protos, structs = binding.parse_header(), binding.parse_structs()
    lines = []
    for name, args in calls:
        lines.append("%s(%s)" % (name, ", ".join("%s=%s" % (an, _canon(a, t, structs, binding.member_name)) for a, (t, an) in zip(args, protos[name][1]))))
    return "\n".join(lines) + "\n"


def install():
    """Point the runtime at CPU tensors and the fake ABI.  Returns the FakeLib."""
    fake = FakeLib()
    _lib._LIB = fake
    c = runtime.ctx()
    c.device = torch.device("cpu")
    c.dtype = runtime.F32
    c._ws = torch.empty(1 << 20, dtype=torch.uint8)
    c._seed = torch.zeros(1, dtype=torch.int64)
    c.step_counter = torch.zeros(1, dtype=torch.int64)
    c.tape = None
    c.training = False
    c.world_size = 1
    type(c).stream = property(lambda self: ctypes.c_void_p(0))
    return fake


def uninstall():
    _lib._LIB = None
    c = runtime.ctx()
    type(c).stream = property(lambda self: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
