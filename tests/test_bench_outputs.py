"""bench.py --dump-outputs: what the last timed step delivered, written as .npy files so that two builds can be compared
output for output.  CPU: dump_outputs over a host arena (the device copy replaced by a memmove) -- slice lengths, every
slice's byte sum, the seeded sample of the byte stream, the size limit.  GPU: a plain run of the script at a small size,
its line and its dump against the messages as framed on the host."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["delivered_slice_lengths", "delivered_slice_byte_sums", "delivered_stream_sample_positions",
         "delivered_stream_sample_bytes"]


class _HostLib:
    def grdma_copy_to_host(self, dst, src, n):
        C.memmove(dst, src, n)
        return 0


class _HostG:
    """Stands in for grpc_rdma_amd: `dst` is host memory here."""
    class _lib:
        check = staticmethod(lambda rc: rc)

    def load(self):
        return _HostLib()


class _Buf:
    def __init__(self, arr):
        self.arr = arr
        self.ptr = arr.ctypes.data


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_outputs_host_arena(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(7)
    arena = rng.integers(0, 256, 3 << 20, dtype=np.uint8)
    # slices out of order in the arena, one of length 0, gaps between them
    slices, off = [], 0
    for n in [9, 16384, 0, 5, 16393] * 40 + [1]:
        slices.append((off, n))
        off += n + 24
    slices = slices[::-1]
    exp = [arena[o:o + n] for o, n in slices]
    stream = np.concatenate(exp)
    bench.dump_outputs(str(tmp_path / "a"), _HostG(), _Buf(arena), arena.size, slices)
    bench.dump_outputs(str(tmp_path / "b"), _HostG(), _Buf(arena), arena.size, slices)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in NAMES:
        assert a[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(a[n], b[n]), "%s differs between two dumps of the same output" % n
    assert a["delivered_slice_lengths"].tolist() == [n for _, n in slices]
    assert a["delivered_slice_byte_sums"].tolist() == [int(e.astype(np.int64).sum()) for e in exp]
    pos = a["delivered_stream_sample_positions"].astype(np.int64)
    assert pos.size == 1 << 21 and pos.min() >= 0 and pos.max() < stream.size and np.all(np.diff(pos) >= 0)
    assert np.array_equal(a["delivered_stream_sample_bytes"], stream[pos].astype(np.float32))
    # at the default size (1008 messages x 130 slices) the dump stays well under 64 MB
    many = [(0, 8)] * (1008 * 130)
    bench.dump_outputs(str(tmp_path / "c"), _HostG(), _Buf(arena), arena.size, many)
    total = sum(os.path.getsize(os.path.join(tmp_path, "c", n + ".npy")) for n in NAMES)
    assert total < 64 * 10 ** 6, total


def _framed_slices(n_msgs, payload):
    """The slices of one step as bench.Workload lays them out, and as they must come out of the endpoint."""
    sys.path.insert(0, ROOT)
    import bench
    from grpc_rdma_amd import h2
    msgs = [bench.proto_message(i, payload) for i in range(min(n_msgs, 8))]
    layout = h2.frame_message(len(msgs[0]), 1, 16384)
    out = []
    for i in range(n_msgs):
        m = msgs[i % len(msgs)]
        out += [it[1] if it[0] == "inl" else m[it[1][0]:it[1][0] + it[1][1]] for it in layout]
    return out


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_what_it_delivered(built, tmp_path):
    n_msgs = 8
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--msgs", str(n_msgs), "--leg-msgs", str(n_msgs), "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and d["value"] > 0
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["repetitions"]["n"] == 1 and len(d["repetitions"]["ms_per_step"]) == 1
    # a plain run carries the headline only
    assert d["roofline"] is None and d["cpu_baseline"] is None and "value_with_h2" not in d and "rtt_p50_us" not in d
    got = _load(tmp_path / "out")
    # the reader's slices cut the stream where the receiver does (not where the sender's slices end): together they are
    # the framed messages, byte for byte
    stream = np.frombuffer(b"".join(_framed_slices(n_msgs, 1 << 20)), dtype=np.uint8)
    lens = got["delivered_slice_lengths"].astype(np.int64)
    assert lens.min() >= 0 and int(lens.sum()) == stream.size
    ends = np.cumsum(lens)
    assert got["delivered_slice_byte_sums"].tolist() == [int(stream[e - n:e].astype(np.int64).sum()) for e, n in zip(ends, lens)]
    pos = got["delivered_stream_sample_positions"].astype(np.int64)
    assert np.array_equal(got["delivered_stream_sample_bytes"], stream[pos].astype(np.float32))
