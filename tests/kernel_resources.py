"""What the compiler allocated to the kernels of a unit of csrc/ for gfx950 (-Rpass-analysis=kernel-resource-usage): one
compile per unit and process (`report`), one parser of the remarks (`parse`).  The tests that pin scratch, spills,
registers and LDS of their kernels call `report` and assert on its slice; nothing else in tests/ starts that compile."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

REMARKS = "-Rpass-analysis=kernel-resource-usage"
# unit -> (flags beside the product build's, name of the output)
UNITS = {"grdma_h2.hip": ([], "h2.o"),
         "grdma_rx_plan.hip": (["-I" + os.path.join(ROOT, "include"), "--cuda-device-only"], "rx_plan.co")}

# the remark block's label -> the key of the report; every block must carry all of them
FIELDS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
          "Occupancy [waves/SIMD]": "occupancy", "SGPRs Spill": "sspill", "VGPRs Spill": "vspill",
          "LDS Size [bytes/block]": "lds"}

_REMARK = re.compile(r"remark:\s+([^:]+): (\S+)")
_LENGTH = re.compile(r"\d+")


def short_name(mangled):
    """The function's own name out of an Itanium-mangled one: _Z<len><name>..., or the last <len><name> of the nested
    _ZN<len><scope>...<len><name>E...; a name that is not mangled (extern "C") is returned as it is."""
    m = re.match(r"_ZN?", mangled)
    if not m:
        return mangled
    pos, name = m.end(), None
    while True:
        d = _LENGTH.match(mangled, pos)
        if not d:
            break
        pos = d.end() + int(d.group())
        name = mangled[d.end():pos]
    if not name or pos > len(mangled):
        raise ValueError("no length-prefixed name in %r" % mangled)
    return name


def parse(remarks_text):
    """The remarks of one compile -> {kernel: {field: int}} with the keys of FIELDS for every function the compiler
    reported.  A block without one of those fields, or two blocks of one name, raise ValueError."""
    out, cur = {}, None
    for line in remarks_text.splitlines():
        m = _REMARK.search(line)
        if not m:
            continue
        label, value = m.groups()
        if label == "Function Name":
            cur = short_name(value)
            if cur in out:
                raise ValueError("two remark blocks for %s" % cur)
            out[cur] = {}
        elif label in FIELDS and cur is not None:
            out[cur][FIELDS[label]] = int(value)
    for k, v in out.items():
        missing = sorted(set(FIELDS.values()) - set(v))
        if missing:
            raise ValueError("the remark block of %s lacks %s" % (k, missing))
    return out


@functools.lru_cache(maxsize=None)
def report(unit):
    """csrc/<unit> compiled for gfx950 with the product build's flags (and the unit's own of UNITS) into a temporary
    directory -> parse() of its remarks.  Cached for the life of the process only: a stale report would be worse than
    a compile."""
    flags, out = UNITS[unit]
    src = os.path.join(ROOT, "grpc-rdma_amd", "csrc", unit)
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value"] + flags +
                           ["-c", src, "-o", os.path.join(td, out), REMARKS], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("hipcc %s: %s" % (unit, p.stderr[-2000:]))
    return parse(p.stderr)


def kernels_of(unit, *prefixes):
    """The slice of report(unit) whose kernels' names begin with one of the prefixes."""
    return {k: v for k, v in report(unit).items() if k.startswith(prefixes)}
