"""Byte-level builders shared by the HTTP/2 deframing tests (CPU oracle and GPU parity)."""
import json
import os

from oracle.pyorc import EV_MSG_BEGIN, EV_MSG_BYTES, EV_MSG_END

PREFACE = b"PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n"


def frame(ftype, flags, sid, payload=b""):
    return len(payload).to_bytes(3, "big") + bytes([ftype, flags]) + sid.to_bytes(4, "big") + payload


def grpc_msg(body, compressed=0):
    return bytes([compressed]) + len(body).to_bytes(4, "big") + body


def unary_call(sid, body, hdr=b"\x82\x86"):
    """HEADERS(END_HEADERS) + DATA(END_STREAM) of one unary request on stream sid."""
    return frame(1, 4, sid, hdr) + frame(0, 1, sid, grpc_msg(body))


def messages_of(events, data):
    out, cur = [], {}
    for k, a, b, c, d in events:
        if k == EV_MSG_BEGIN:
            cur[c] = bytearray()
        elif k == EV_MSG_BYTES:
            cur[c] += data[a:a + b]
        elif k == EV_MSG_END:
            out.append((c, bytes(cur.pop(c))))
    return out


def grpcio_capture():
    """tests/golden/h2_grpcio_capture.json -> (the bytes a stock gRPC client put on the wire, the payloads that went in)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "h2_grpcio_capture.json")
    d = json.load(open(path))
    data = bytes.fromhex(d["client_bytes_hex"])
    from oracle import gen_h2_grpcio_capture
    unary, stream = gen_h2_grpcio_capture.payloads()   # the payloads that went into the capture
    assert [len(p) for p in unary + stream] == d["payload_lengths"]
    return data, unary + stream
