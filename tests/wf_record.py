"""The wavefront launch record (wcpt_wf_last_plan, Context.wf_last_plan()) held against the product's own rules: every
function here goes through tests/wf_plan_shim.cpp, i.e. wc-path-tracer_amd/csrc/wf_plan.h compiled with g++, so nothing
about the numbering of the instances or the plan is restated in Python. `shim` is test_wf_plan.py's fixture.

A GPU test calls these on the record of a real render, whose `cus`, `trace_bpc` and `persist_bpc` only the device knows;
tests/test_wf_plan.py calls them on made-up records, one wrong in each field."""
import ctypes
import os
import subprocess

from wcpt._lib import WF_MAX_PIPES, WF_NO_VARIANT, WfPipeInfo, WfPlanInfo

RENDER, COUNT, DIAG = 0, 1, 2
PLAN_FIELDS = ("ok", "empty", "persist", "K", "trace_grid", "shade_grid", "persist_grid")
PIPE_FIELDS = tuple(n for n, _ in WfPipeInfo._fields_)


_shim = None


def shim_library(mkdir):
    """tests/wf_plan_shim.cpp compiled with g++ into mkdir() and loaded, every signature declared; once per process."""
    global _shim
    if _shim is None:
        out = os.path.join(str(mkdir()), "libwf_plan_shim.so")
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wf_plan_shim.cpp")
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", src, "-o", out], check=True)
        lib = ctypes.CDLL(out)
        prototypes(lib)
        _shim = lib
    return _shim


def prototypes(lib):
    """ctypes signatures of the shim's functions"""
    u32, u64, i = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    ints, i64s, u32s = ctypes.POINTER(i), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(u32)
    lib.wfp_codes.restype = u32
    lib.wfp_max_pipes.restype = i
    lib.wfp_decode.argtypes = [u32, ints]
    lib.wfp_decode.restype = None
    lib.wfp_code.argtypes = [ints]
    lib.wfp_code.restype = u32
    lib.wfp_built.argtypes = [ints]
    lib.wfp_built.restype = i
    lib.wfp_select.argtypes = [i, u32, i, i, ints]
    lib.wfp_select.restype = None
    lib.wfp_persist_variant.argtypes = [ints]
    lib.wfp_persist_variant.restype = None
    lib.wfp_persist_eligible.argtypes = [ints, u32, i, i]
    lib.wfp_persist_eligible.restype = i
    lib.wfp_short_queue.argtypes = [u64, u32]
    lib.wfp_short_queue.restype = i
    lib.wfp_iterations.argtypes = [i, u32, u32]
    lib.wfp_iterations.restype = u32
    lib.wfp_share.argtypes = [u32, u32, u32, u32, u32s]
    lib.wfp_share.restype = None
    lib.wfp_plan.argtypes = [i64s, i64s]
    lib.wfp_plan.restype = None
    lib.wfp_continues.argtypes = [i64s, i, i, u32s]
    lib.wfp_continues.restype = i
    rec = ctypes.POINTER(WfPlanInfo)
    lib.wfp_record_layout.argtypes = [ctypes.POINTER(ctypes.c_uint32)]
    lib.wfp_record_layout.restype = None
    lib.wfp_record_expect.argtypes = [rec, rec]
    lib.wfp_record_expect.restype = ctypes.c_int
    lib.wfp_record_continues.argtypes = [rec, rec]
    lib.wfp_record_continues.restype = ctypes.c_int
    lib.wfp_persist_geo.restype = ctypes.c_int


def to_struct(rec):
    """Context.wf_last_plan()'s dict as the C record"""
    s = WfPlanInfo()
    for n, _ in WfPlanInfo._fields_:
        if n != "pipe":
            setattr(s, n, rec[n])
    for j in range(WF_MAX_PIPES):
        q = rec["pipe"][j] if j < len(rec["pipe"]) else dict(variant_code=WF_NO_VARIANT, dispatches=0, tiles=0, paths=0, iters=0)
        for n in PIPE_FIELDS:
            setattr(s.pipe[j], n, q[n])
    return s


def decode(shim, code):
    """(count, diag, geo, ldsn, persist) of an instance's code: wf_variant_decode"""
    assert 0 <= code < shim.wfp_codes(), code
    out = (ctypes.c_int * 5)()
    shim.wfp_decode(code, out)
    return tuple(out)


def code_of(shim, fields):
    return shim.wfp_code((ctypes.c_int * 5)(*[int(f) for f in fields]))


def built_codes(shim):
    """the codes of the instances a code object holds"""
    out = set()
    for c in range(shim.wfp_codes()):
        a = (ctypes.c_int * 5)()
        shim.wfp_decode(c, a)
        if shim.wfp_built(a) == 1:
            out.add(c)
    return out


def persist_code(shim):
    out = (ctypes.c_int * 5)()
    shim.wfp_persist_variant(out)
    return shim.wfp_code(out)


def unreachable_codes(shim):
    """built, yet no launch can select them: the persistent instances other than wf_persist_variant()"""
    return {c for c in built_codes(shim) if decode(shim, c)[4] == 1} - {persist_code(shim)}


def expect(shim, rec):
    """What wf_frame_plan and wf_pipe_variant make of the inputs `rec` reports, as a record dict."""
    out = WfPlanInfo()
    assert shim.wfp_record_expect(ctypes.byref(to_struct(rec)), ctypes.byref(out)) == 1, \
        f"the record's base instance {rec['base_code']} is not a built per-bounce instance"
    return out.as_dict()


def mismatches(shim, rec):
    """The names of the fields in which the record differs from the plan of the inputs it reports; [] when it holds."""
    try:
        want = expect(shim, rec)
    except AssertionError:
        return ["base_code"]
    bad = [f for f in PLAN_FIELDS if rec[f] != want[f]]
    if len(rec["pipe"]) != len(want["pipe"]):
        bad.append("pipe")
    for j, (q, r) in enumerate(zip(rec["pipe"], want["pipe"])):
        bad += [f"pipe[{j}].{f}" for f in PIPE_FIELDS if q[f] != r[f]]
    return bad


def continues(shim, rec, prev):
    """wf_frame_continues for the launch `rec` reports behind the launch `prev` reports (None: nothing pending)."""
    p = ctypes.byref(to_struct(prev)) if prev is not None else None
    return shim.wfp_record_continues(ctypes.byref(to_struct(rec)), p) == 1


def check(shim, rec, launches=None):
    """The assertions every record of a launched frame must pass; returns the decoded instance of each pipeline."""
    assert mismatches(shim, rec) == [], (mismatches(shim, rec), rec, expect(shim, rec))
    if launches is not None:
        assert rec["launches"] == launches, rec
    assert rec["ok"] == 1 and rec["empty"] == 0 and len(rec["pipe"]) == rec["K"] >= 1
    built = built_codes(shim)
    assert all(q["variant_code"] in built for q in rec["pipe"]), rec
    return [decode(shim, q["variant_code"]) for q in rec["pipe"]]
