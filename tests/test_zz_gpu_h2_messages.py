"""The message assembler (grdma_h2_asm): received gRPC messages contiguous in device memory, one descriptor each.
Every case compares the descriptors with the sequential model of tests/h2_asm_model.py over the oracle's events and
the message bytes in the arena with the payloads that were framed."""
import ctypes as C
import os
import random

import pytest

from oracle import pyorc
from tests.h2_asm_model import OK, TOO_LARGE, NO_SPACE, TRUNCATED
from tests.h2_device_lib import BATCHES, SENTINEL, Harness, _batch, _eight_streams, _pipe_setup, pack_slices
from tests.h2_helpers import frame, grpc_msg, grpcio_capture, messages_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lens,max_frame", BATCHES)
def test_batches_in_one_call(gpu, lens, max_frame):
    bodies, wire, slices = _batch(lens, max_frame, len(lens))
    h = Harness(gpu, 8 << 20, max_pending=8192, streams=[1], max_frame=max_frame)
    got = h.feed(slices)
    assert [m.length for m in got] == lens and all(m.status == OK for m in got)
    assert [h.asm.view(m) for m in got] == bodies
    h.close()


@pytest.mark.parametrize("lens,max_frame", [b for b in BATCHES if sum(b[0]) < 4 << 20])
def test_batches_cut_into_calls(gpu, lens, max_frame):
    bodies, wire, _ = _batch(lens, max_frame, len(lens) + 1)
    rng = random.Random(len(wire))
    for trial in range(2):
        k = rng.randrange(1, min(49, len(wire) - 1) + 1)
        cuts = sorted(rng.sample(range(1, len(wire)), k))
        bounds = [0] + cuts + [len(wire)]
        h = Harness(gpu, 8 << 20, max_pending=8192, streams=[1], max_frame=max_frame)
        got = []
        for a, b in zip(bounds, bounds[1:]):
            got += h.feed([wire[a:b]], rng=rng)
        assert [h.asm.view(m) for m in got] == bodies
        h.close()


def test_every_cut_of_a_small_wire(gpu):
    bodies = [b"x" * 40, b"", bytes(range(120))]
    wire = b"".join(frame(0, 0, 1, grpc_msg(m)) for m in bodies)
    assert 150 < len(wire) < 260
    for cut in range(1, len(wire)):
        h = Harness(gpu, 1 << 16, streams=[1])
        got = h.feed([wire[:cut]]) + h.feed([wire[cut:]])
        assert [h.asm.view(m) for m in got] == bodies
        h.close()


def test_eight_interleaved_streams(gpu):
    for seed in range(3):
        wire, parts = _eight_streams(seed)
        h = Harness(gpu, 4 << 20, prefix=True)
        got = []
        for p in parts:
            got += h.feed([p[i:i + 1000] for i in range(0, len(p), 1000)])
        _, ev = pyorc.H2Parser(expect_client_prefix=True).feed(wire, cap=len(wire) * 4)
        exp = messages_of([e[:5] for e in ev], wire)
        assert [(m.stream_id, h.asm.view(m)) for m in got] == exp
        h.close()


def test_truncation_and_reuse(gpu):
    body = bytes(range(256)) * 40
    m = grpc_msg(body)
    h = Harness(gpu, 1 << 15, streams=[1, 3, 5, 7])
    # RST_STREAM mid-message
    got = h.feed([frame(0, 0, 1, m[:5000]), frame(3, 0, 1, (8).to_bytes(4, "big"))])
    assert [x.status for x in got] == [TRUNCATED]
    # END_STREAM on a frame that ends mid-message
    got = h.feed([frame(0, 1, 3, m[:7000])])
    assert [x.status for x in got] == [TRUNCATED]
    h.release(2)
    assert h.asm.stats()["bytes_in_use"] == h.model.bytes_in_use() == 0
    # the space is reused: the next message starts where the ring's head is and completes
    got = h.feed([frame(0, 0, 5, m)])
    assert [x.status for x in got] == [OK] and h.asm.view(got[0]) == body
    # a connection error mid-message (a frame larger than SETTINGS_MAX_FRAME_SIZE)
    got = h.feed([frame(0, 0, 7, m[:3000]), (20000).to_bytes(3, "big") + bytes([0, 0]) + (7).to_bytes(4, "big")])
    assert [x.status for x in got] == [TRUNCATED]
    h.close()


def test_too_large_partial_at_a_connection_error(gpu):
    """a TOO_LARGE message and an OK one, both partial when the connection fails: reported in seq order, and every
    partial record is given back at once (bytes in use and the record count agree with the model)"""
    h = Harness(gpu, 1 << 15, max_msg=2000, max_pending=4, streams=[1, 3])
    big, ok = grpc_msg(b"B" * 5000), grpc_msg(b"o" * 1500)
    got = h.feed([frame(0, 0, 1, big[:3000]), frame(0, 0, 3, ok[:700]),
                  (20000).to_bytes(3, "big") + bytes([0, 0]) + (3).to_bytes(4, "big")])
    assert [x.status for x in got] == [TOO_LARGE, TRUNCATED]
    h.release(0)
    assert h.asm.stats()["bytes_in_use"] == h.model.bytes_in_use() == 0
    assert h.model.rec_head == h.model.rec_tail
    st = h.asm.stats()
    assert (st["too_large"], st["truncated"], st["reported"]) == (1, 1, 2)
    h.close()


def test_pieces_larger_than_a_frame_of_16k(gpu):
    """frames of up to 1 MiB and whole-frame slices: single pieces of many copy tiles, spread over the grid"""
    lens = [3 << 20, 5, 1 << 20, 70001]
    bodies, wire, slices = _batch(lens, 1 << 20, 11)
    h = Harness(gpu, 8 << 20, streams=[1], max_frame=1 << 20)
    got = h.feed(slices)
    assert [m.status for m in got] == [OK] * 4 and [h.asm.view(m) for m in got] == bodies
    h.close()


def test_limits(gpu):
    lim = 3000
    bodies = [b"a" * lim, b"b" * (lim + 1), b"c" * 10]
    h = Harness(gpu, 1 << 16, max_msg=lim, streams=[1])
    got = h.feed([frame(0, 0, 1, grpc_msg(b)) for b in bodies])
    assert [x.status for x in got] == [OK, TOO_LARGE, OK]
    raw = h.arena.read()
    used = sorted((x.offset, x.offset + ((x.length + 255) // 256) * 256) for x in got if x.status == OK)
    for i, v in enumerate(raw):
        if not any(a <= i < b for a, b in used):
            assert v == SENTINEL, "byte %d written" % i
    h.close()
    # a full ring: NO_SPACE for the rest of the call; a release lets the next call allocate; wrap-around
    h = Harness(gpu, 4096, streams=[1])
    msgs = [b"x" * 1000, b"y" * 1500, b"z" * 2000, b"w" * 10]
    got = h.feed([frame(0, 0, 1, grpc_msg(b)) for b in msgs])
    assert [x.status for x in got] == [OK, OK, NO_SPACE, NO_SPACE]
    h.release(1)
    got = h.feed([frame(0, 0, 1, grpc_msg(b)) for b in [b"p" * 900, b"q" * 900, b"s" * 1800]])
    # the second wraps to the start; the third finds no room in front of the tail
    assert [x.status for x in got] == [OK, OK, NO_SPACE] and (got[0].offset, got[1].offset) == (2560, 0)
    h.release()
    got = h.feed([frame(0, 0, 1, grpc_msg(b"r" * 3000))])
    assert [x.status for x in got] == [OK]
    h.close()
    # max_pending
    h = Harness(gpu, 1 << 16, max_pending=3, streams=[1])
    got = h.feed([frame(0, 0, 1, grpc_msg(b"m" * 5)) for _ in range(5)])
    assert [x.status for x in got] == [OK, OK, OK, NO_SPACE, NO_SPACE]
    h.release(4)
    got = h.feed([frame(0, 0, 1, grpc_msg(b"n" * 5)) for _ in range(4)])
    assert [x.status for x in got] == [OK, OK, OK, NO_SPACE]
    h.close()


def test_random_ring_pressure(gpu):
    rng = random.Random(5)
    h = Harness(gpu, 1 << 14, max_msg=9000, max_pending=7, streams=[1, 3])
    for call in range(30):
        parts = []
        for _ in range(rng.randrange(1, 6)):
            sid = rng.choice([1, 3])
            parts.append(frame(0, 0, sid, grpc_msg(bytes([call]) * rng.choice([0, 1, 255, 256, 257, 3000, 9001]))))
        h.feed(parts)
        h.release(rng.randrange(0, 4))
        assert h.asm.stats()["bytes_in_use"] == h.model.bytes_in_use()
    h.close()


def test_stock_client_capture(gpu):
    data, exp = grpcio_capture()
    for seed in range(3):
        rng = random.Random(seed)
        if seed == 0:
            cuts = []
        elif seed == 1:
            cuts = list(range(16384, len(data), 16384))
        else:
            cuts = sorted(rng.sample(range(1, len(data)), 50))
        bounds = [0] + cuts + [len(data)]
        h = Harness(gpu, 4 << 20, prefix=True)
        got = []
        for a, b in zip(bounds, bounds[1:]):
            got += h.feed([data[a:b]])
        assert [h.asm.view(m) for m in got] == list(exp)
        h.close()


def test_chunked_deframer_same_messages(gpu):
    lens = [70000] * 40 + [5, 0, 300]
    bodies, wire, slices = _batch(lens, 16384, 9)
    small = [s[i:i + 64] for s in slices for i in range(0, len(s), 64)][:]
    assert len(small) >= 2048
    res = []
    for chunks in (True, False):
        h = Harness(gpu, 4 << 20, streams=[1], chunks=chunks)
        got = h.feed(small)
        res.append([(tuple(m), h.asm.view(m)) for m in got])
        h.close()
    assert res[0] == res[1] and [b for _, b in res[0]] == bodies


def test_events_out_equal_deframe(gpu):
    from grpc_rdma_amd import h2dev
    bodies, wire, slices = _batch([3, 70000, 16379, 0, 5], 16384, 4)
    h = Harness(gpu, 1 << 20, streams=[1])
    got, ev, _ = h.feed(slices, want_events=True)
    p = h2dev.Parser(False)
    assert p.open_streams([1]) == 0
    data, table = pack_slices(slices)
    buf = gpu.DeviceBuffer(data=data)
    err, ev2 = p.deframe(buf.ptr, table)
    assert err == 0 and ev == ev2
    p.close()
    h.close()


_TENSOR_CHILD = r"""
import sys, torch
t = torch.full((1 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
sys.path.insert(0, sys.argv[1])
import grpc_rdma_amd as g
from grpc_rdma_amd import h2dev
from tests.h2_device_lib import _batch, pack_slices
g.init(0)
bodies, wire, slices = _batch([1000, 0, 70000], 16384, 2)
p = h2dev.Parser(False)
assert p.open_streams([1]) == 0
a = h2dev.Assembler(p, t, 4 << 20, 64)
data, table = pack_slices(slices)
buf = g.DeviceBuffer(data=data)
err, got = p.deframe_messages(buf.ptr, table, a)
torch.cuda.synchronize()
assert err == 0 and [m.status for m in got] == [0, 0, 0], got
for m, b in zip(got, bodies):
    v = a.view(m)
    assert isinstance(v, torch.Tensor), type(v)
    h = bytes(v.cpu().numpy().tobytes())
    assert h == b, m
end = max(m.offset + m.length for m in got)
assert end == 1024 + 70000 and int((t[end:] != 0xA5).sum()) == 0
a.close()
p.close()
print("tensor arena ok")
"""


def test_torch_tensor_arena(gpu):
    """The arena as a torch tensor, in a child process that brings torch's device up first (one HIP runtime then
    serves both); Assembler.view returns tensor slices."""
    if os.environ.get("GRDMA_TEST_ALLOW_EMU") == "1":
        pytest.skip("the emulator has no torch device memory")
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _TENSOR_CHILD, root], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tensor arena ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_bad_arguments(gpu):
    from grpc_rdma_amd import h2dev, _lib
    lib = _lib.load()
    h2dev.load()
    p = h2dev.Parser(False)
    other = h2dev.Parser(False)
    buf = gpu.DeviceBuffer(nbytes=4096)
    assert not lib.grdma_h2_asm_create(None, buf.ptr, 4096, 0, 16)
    assert not lib.grdma_h2_asm_create(p.h, None, 4096, 0, 16)
    assert not lib.grdma_h2_asm_create(p.h, buf.ptr, 4096, 0, 0)
    a = h2dev.Assembler(p, buf, 0, 16)
    out = (h2dev.H2RxMsg * 4)()
    err = C.c_int(0)
    sl = (_lib.ReadSlice * 1)()
    assert lib.grdma_h2_deframe_messages(other.h, a.h, buf.ptr, sl, 0, None, 64, out, 4, C.byref(err)) == -2
    assert lib.grdma_h2_deframe_messages(p.h, None, buf.ptr, sl, 0, None, 64, out, 4, C.byref(err)) == -2
    assert lib.grdma_h2_deframe_messages(p.h, a.h, None, sl, 0, None, 64, out, 4, C.byref(err)) == -2
    assert lib.grdma_h2_deframe_messages(p.h, a.h, buf.ptr, sl, 0, None, 0, out, 4, C.byref(err)) == -2
    assert lib.grdma_h2_deframe_messages(p.h, a.h, buf.ptr, sl, 0, None, 64, out, 4, C.byref(err)) == 0
    # descriptors beyond the cap
    wire = b"".join(frame(0, 0, 1, grpc_msg(b"k")) for _ in range(6))
    dev = gpu.DeviceBuffer(data=wire + bytes(64))
    assert p.open_streams([1]) == 0
    sl[0].off, sl[0].len = 0, len(wire)
    assert lib.grdma_h2_deframe_messages(p.h, a.h, dev.ptr, sl, 1, None, 256, out, 4, C.byref(err)) == -5
    assert lib.grdma_h2_asm_release(None, 1) == -2
    assert lib.grdma_h2_asm_stats(a.h, None) == -2
    assert lib.grdma_h2_pipe_attach_assembler(None, a.h) == -2
    assert lib.grdma_h2_pipe_messages(None, out, 4) == -2
    a.close()
    p.close()
    other.close()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_pipe_messages(gpu, fused):
    g = gpu
    from grpc_rdma_amd import h2dev, stream as gs
    old = os.environ.get("GRDMA_H2_PIPE_FUSED")
    os.environ["GRDMA_H2_PIPE_FUSED"] = fused
    try:
        sizes = [70000, 1, 16379, 0, 200000, 5000]
        bodies = [bytes((j * 7 + i) % 251 for j in range(n)) for i, n in enumerate(sizes)]
        parser = h2dev.Parser(False)
        assert parser.open_streams([1]) == 0
        pipes, jobs, keep = _pipe_setup(g, h2dev, gs, sizes, 2, parser)
    finally:
        if old is None:
            os.environ.pop("GRDMA_H2_PIPE_FUSED", None)
        else:
            os.environ["GRDMA_H2_PIPE_FUSED"] = old
    arena = g.DeviceBuffer(nbytes=512 << 10)
    a = h2dev.Assembler(parser, arena, 4 << 20, 4096)
    for p in pipes:
        p.attach_assembler(a)
    step_bytes = sum(((n + 255) // 256) * 256 for n in sizes)
    for step in range(5):
        p = pipes[step % 2]
        p.enqueue()
        r = p.sync()
        assert r["h2_error"] == 0
        got = p.messages()
        assert [(m.status, m.length, m.stream_id) for m in got] == [(OK, n, 1) for n in sizes]
        assert [m.seq for m in got] == list(range(step * len(sizes), (step + 1) * len(sizes)))
        assert [a.view(m) for m in got] == bodies
        st = a.stats()
        assert st["bytes_in_use"] <= step_bytes + max(sizes)  # (one step, and the end of the ring it skipped)
    # a release of its own, and a standalone call, on an attached assembler are refused
    with pytest.raises(Exception):
        a.release(1)
    with pytest.raises(Exception):
        parser.deframe_messages(arena.ptr, [(0, 0)], a)
    for p in pipes:
        p.close()
    for j in jobs:
        j.close()
    a.close()
    parser.close()
