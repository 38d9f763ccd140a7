"""ctypes binding of libmssvt_hip.so (include/mssvt_hip.h).

The product path has NO CPU fallback: if the HIP library is missing this module
raises at first use.  Arguments are raw device pointers (``tensor.data_ptr()``)
plus the current torch HIP stream -- torch is only the allocator / stream owner.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSSVT_LIB: another build of the same library (the schedule variants of mssvt_amd/build.py, for the hazard test)
LIB_PATH = os.environ.get("MSSVT_LIB") or os.path.join(_HERE, "lib", "libmssvt_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mssvt_hip.h")

_lib = None


class MssvtHipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MssvtHipError(
                "libmssvt_hip.so not built (%s). Run `python -m mssvt_amd.build`; there is no "
                "CPU fallback for the MsSVT hot path." % LIB_PATH)
        lib_ = ctypes.CDLL(LIB_PATH)
        _declare(lib_)
        _lib = lib_  # only a fully declared library is cached
    return _lib


def _declare(lib_):
    """argtypes / restype of every `mssvt_*` function from the declarations of include/mssvt_hip.h (int, float,
    long long, pointers).  With them ctypes converts plain Python ints, floats and addresses in C and refuses a float
    where C takes an int: callers pass plain values, never ctypes.c_int / c_void_p objects (the fused forward hands over
    ~600 scalars and pointers per frame).  A missing header or a parameter type unknown here is an error, so no entry
    point of the header stays undeclared."""
    if not os.path.exists(HEADER_PATH):
        raise MssvtHipError("%s not found: the argument types of libmssvt_hip.so are declared from it" % HEADER_PATH)
    with open(HEADER_PATH) as f:
        txt = f.read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    kinds = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    rets = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "const char *": ctypes.c_char_p}
    for ret, name, params in re.findall(r"\b(int|long long|const char \*)\s*(mssvt_\w+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S):
        fn = getattr(lib_, name, None)
        if fn is None:
            continue  # declared but not exported by this build (tests/test_abi_cpu.py holds the shipped library to the header)
        params = params.replace("\n", " ").strip()
        args = []
        for q in ([] if params in ("", "void") else params.split(",")):
            q = q.strip()
            args.append(ctypes.c_void_p if "*" in q else kinds.get(" ".join(q.split()[:-1])))
        if None in args:
            raise MssvtHipError("%s: cannot type parameter %d of %s (`%s`)" % (HEADER_PATH, args.index(None), name, params))
        fn.argtypes = args
        fn.restype = rets[ret]


def check(status, what):
    if status != 0:
        raise MssvtHipError("%s failed: %s (status %d)" % (
            what, lib().mssvt_hip_status_string(int(status)).decode(), status))


def ptr(t):
    """Address of a contiguous CUDA(HIP) tensor as a plain int (None -> NULL)."""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise MssvtHipError("mssvt_amd ops need contiguous tensors on the GPU (no CPU path)")
    return t.data_ptr()


def addr(t):
    """`ptr` without the device / contiguity checks: for buffers the fused path allocated itself and for module
    parameters (the frame's front is launch bound: ~200 pointer conversions per frame)."""
    return None if t is None else t.data_ptr()


def f3(xs):
    """Host array of three floats (voxel size, range minimum, window size in metres)."""
    return (ctypes.c_float * 3)(*[float(v) for v in xs])


def stream():
    """Raw handle of torch's current HIP stream as a plain int (the fast C accessor: torch.cuda.current_stream()
    builds a Python Stream object, ~8 us per call, 20+ calls per forward)."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


_fns = {}


def call(name, *args):
    fn = _fns.get(name)
    if fn is None:
        fn = getattr(lib(), name)
        if fn.argtypes is None:  # exported but not in the header: a plain-int address would be cut to 32 bits
            raise MssvtHipError("%s is not declared in include/mssvt_hip.h: set its argtypes and call it through lib()" % name)
        _fns[name] = fn
    status = fn(*args)
    if status != 0:
        check(status, name)
