"""The call table's sequential reference (tests/h2_calls_model.py) held to vectors written by hand from the rules of
include/grdma_amd.h ("Call table"): what the device tests compare against must itself be right."""
from tests.h2_calls_model import (BAD_INPUT, BAD_STATUS, COMPRESSED, COMPRESSED_IDENTITY, DEADLINE, ERR_METHOD, ERR_STREAM, EXPIRED_MSG, FIRST,
                                  LAST, LEFT, LOST, NO_CALL, NONE, READS_CLOSED, U64, WAS_READS_CLOSED, CallsModel, closed, dispatch_bytes,
                                  done_bytes, entry_bytes, message, request)

BIG = 1 << 40


def step(m, reqs=(), msgs=(), events=(), now=0, dispatch_cap=BIG, done_cap=BIG):
    return m.step([r[0] for r in reqs], [r[1] for r in reqs], list(msgs), list(events), now, dispatch_cap, done_cap)


def test_a_unary_call_in_one_step():
    m = CallsModel(16, 2)
    disp, segs, done, res, err = step(m, [request(1, 1, timeout=500)], [message(1, length=10, offset=256)], [closed(1, False), closed(1, True)],
                                      now=1000)
    assert err is None and res == (1, 1, 0, 2, 0, 0, 0, 0) and segs == [0, 0, 1, 1]
    assert disp == [(256, 10, 0, 1, 0, 1, FIRST | LAST, 0, 0)]
    assert done == [(0, 10, 1, 1, 1, READS_CLOSED), (0, 10, 1, 1, 1, LEFT | WAS_READS_CLOSED << 8)]
    assert m.dump() == [] and m.serial == 1
    assert m.stats == dict(steps=1, opened=1, messages=1, bytes=10, orphans=0, done=2, lost=0)


def test_a_unary_call_across_three_steps():
    m = CallsModel(16, 1)
    assert step(m, [request(5, 0, timeout=7)], now=100)[3] == (1, 0, 0, 0, 0, 1, 0, 0)
    assert m.dump() == [(0, 107, 0, 5, 0, 0, 0)]
    disp, segs, done, res, err = step(m, msgs=[message(5, length=3), message(5, length=4)], now=101)
    assert disp == [(0, 3, 0, 5, 0, 0, FIRST, 0, 0), (0, 4, 0, 5, 1, 0, 0, 1, 0)] and segs == [0, 2, 2] and done == []  # (no LAST: no close here)
    assert m.dump() == [(0, 107, 7, 5, 0, 2, 0)]
    disp, segs, done, res, err = step(m, events=[closed(5, False)], now=102)
    assert done == [(0, 7, 5, 0, 2, READS_CLOSED)] and m.dump() == [(0, 107, 7, 5, 0, 2, 1 << 8)]
    disp, segs, done, res, err = step(m, events=[closed(5, True)], now=103)
    assert done == [(0, 7, 5, 0, 2, LEFT | WAS_READS_CLOSED << 8)] and res[5] == 0


def test_a_refused_request_s_messages_are_orphans():
    m = CallsModel(16, 1)
    reqs = [request(1, 0, verdict=6), request(3, 0, status=2), request(5, 0, kind=2), request(7, 0, kind=3)]
    disp, segs, done, res, err = step(m, reqs, [message(1), message(3), message(5, compressed=True)])
    assert res == (0, 0, 3, 0, 0, 0, 0, 0) and segs == [0, 0, 3]
    assert [r[3:7] for r in disp] == [(1, 0, NONE, NO_CALL << 8), (3, 1, NONE, NO_CALL << 8), (5, 2, NONE, COMPRESSED | NO_CALL << 8)]


def test_timeout_zero_and_no_timeout():
    m = CallsModel(16, 1)
    disp, segs, done, res, err = step(m, [request(1, 0, timeout=0), request(3, 0), request(5, 0, timeout=U64)], [message(1), message(3)], now=9)
    assert done == [(0, 0, 1, 0, 0, DEADLINE)] and res[4] == 1 and res[5] == 3
    assert [(r[3], r[2], r[6]) for r in disp] == [(3, 1, FIRST), (1, 0, EXPIRED_MSG << 8)]
    assert m.dump() == [(0, 9, 0, 1, 0, 0, 2 << 8), (1, U64, 8, 3, 0, 1, 0), (2, U64, 0, 5, 0, 0, 0)]  # (saturated)


def test_a_deadline_passes_between_steps_then_a_late_message():
    m = CallsModel(16, 1)
    step(m, [request(1, 0, timeout=10, encoding=1)], [message(1, length=5)], now=100)
    assert step(m, now=109)[2] == []
    disp, segs, done, res, err = step(m, msgs=[message(1)], now=110)
    assert done == [(0, 5, 1, 0, 1, DEADLINE)] and disp == [(0, 8, 0, 1, 0, NONE, EXPIRED_MSG << 8 | 1 << 16, 0, 0)]
    assert step(m, now=111)[2] == []  # (one record per call)
    disp, segs, done, res, err = step(m, events=[closed(1, True)], now=112)
    assert done == [(0, 5, 1, 0, 1, LEFT)]


def test_a_compressed_message_on_identity_and_on_gzip():
    m = CallsModel(16, 2)
    disp, segs, done, res, err = step(m, [request(1, 0), request(3, 1, encoding=1)],
                                      [message(1, compressed=True), message(3, compressed=True), message(1), message(7, status=1, compressed=True)])
    assert [(r[3], r[5], r[6], r[7]) for r in disp] == [(1, 0, FIRST, 0), (3, 1, FIRST | COMPRESSED | 1 << 16, 0),
                                                      (1, NONE, COMPRESSED | COMPRESSED_IDENTITY << 8, 0), (7, NONE, COMPRESSED | BAD_STATUS << 8, 0)]
    assert segs == [0, 1, 2, 4] and m.dump()[0][5] == 1  # (the orphan does not count in its call)


def test_rst_and_end_stream_then_left():
    m = CallsModel(16, 1)
    step(m, [request(1, 0), request(3, 0)])
    disp, segs, done, res, err = step(m, msgs=[message(1), message(3), message(3)],
                                      events=[closed(1, True), closed(1, False), closed(3, False), (7, 2, 0, 3, 0, 0), (6, 1, 0, 3, 0, 0), closed(3, True)])
    assert done == [(0, 8, 1, 0, 1, LEFT), (1, 16, 3, 0, 2, READS_CLOSED), (1, 16, 3, 0, 2, LEFT | WAS_READS_CLOSED << 8)]
    assert [(r[3], r[6]) for r in disp] == [(1, FIRST | LAST), (3, FIRST), (3, LAST)]


def test_a_duplicate_request():
    m = CallsModel(16, 2)
    disp, segs, done, res, err = step(m, [request(1, 0), request(1, 1), request(3, 1)])
    assert res[0] == 2 and m.dump() == [(0, U64, 0, 1, 0, 0, 0), (1, U64, 0, 3, 1, 0, 0)]
    assert step(m, [request(1, 1)])[3][0] == 0 and m.serial == 2


def test_the_table_is_full_at_half_its_slots_and_one():
    m = CallsModel(16, 1)
    disp, segs, done, res, err = step(m, [request(2 * k + 1, 0) for k in range(9)] + [request(17, 0)], [message(17)])
    assert res == (8, 0, 1, 0, 0, 8, LOST, 0) and disp[0][6] == NO_CALL << 8 and m.serial == 8
    assert step(m)[3][6] == LOST  # (sticky)


def test_both_caps_and_their_repeat():
    for caps in (dict(dispatch_cap=1), dict(done_cap=0)):
        m = CallsModel(16, 1)
        args = ([request(1, 0, timeout=0)], [message(1), message(3)], [closed(1, True)])
        disp, segs, done, res, err = step(m, *args, **caps)
        assert err == "capacity" and res == (1, 0, 2, 2, 1, 0, 0, 1) and (disp, segs, done) == ([], None, [])
        assert m.dump() == [] and m.serial == 0 and m.stats["steps"] == 0
        again = step(m, *args)
        assert again == step(CallsModel(16, 1), *args) and again[3] == (1, 0, 2, 2, 1, 0, 0, 0)


def test_both_kinds_of_bad_input():
    m = CallsModel(16, 2)
    for reqs, word in (([request(1, 0), request(0, 0)], BAD_INPUT | ERR_STREAM << 8 | 1 << 32), ([request(1 << 31, 5)], BAD_INPUT | ERR_STREAM << 8),
                       ([request(1, 0), request(3, 1), request(5, 2), request(0, 0)], BAD_INPUT | ERR_METHOD << 8 | 2 << 32)):
        disp, segs, done, res, err = step(m, reqs, [message(1)])
        assert err == "invalid" and res == (0, 0, 0, 0, 0, 0, word, 0) and m.dump() == [] and m.stats["steps"] == 0
    assert step(m, [request(0, 9, verdict=2), request(1, 0)])[3][0] == 1  # (a record that cannot open a call is not looked at)


def test_the_records_bytes():
    assert len(dispatch_bytes((1, 2, 3, 4, 5, 6, 7, 8, 0))) == 48 and len(done_bytes((1, 2, 3, 4, 5, 6))) == 32
    assert entry_bytes((1, 2, 3, 4, 5, 6, 7)) == b"".join(x.to_bytes(8, "little") for x in (1, 2, 3)) + b"".join(
        x.to_bytes(4, "little") for x in (4, 5, 6, 7, 0, 0))
