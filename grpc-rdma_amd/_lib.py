"""ctypes binding of libgrdma_amd.so (the C ABI in include/grdma_amd.h).

The library is the product; this module only loads it.  There is no Python or
CPU fallback: if the shared object is missing the import of any symbol raises,
and on a machine without a HIP device `init()` raises `GrdmaError`.
"""
import ctypes as C
import os

from ._abi import SIGNATURES, UNDECLARED, Config, PairState, ReadSlice, Slice, u64  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GRDMA_LIB_PATH") or os.path.join(HERE, "libgrdma_amd.so")  # (override: A/B builds in tools/)

u64p = C.POINTER(u64)


class GrdmaError(RuntimeError):
    pass


_lib = None


def bind(lib):
    """Give every function of the ABI its prototype on the handle `lib`; raises if the library lost a symbol."""
    for table in (SIGNATURES, UNDECLARED):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
    return lib


def load():
    """Load the shared object; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GrdmaError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the HIP data plane has no fallback)" % LIB_PATH)
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def check(rc):
    if rc < 0:
        raise GrdmaError("grdma error %d: %s" % (-rc, load().grdma_last_error().decode()))
    return rc


def init(device=None):
    lib = load()
    if device is None:
        device = int(os.environ.get("GRPC_RDMA_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    check(lib.grdma_init(device))
    return device
