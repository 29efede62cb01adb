"""The sequential reference of the call-metadata reader (grdma_h2_meta, include/grdma_amd.h "Call metadata"): a decoder's
output -- a block table, a field table and a string arena -- read into one call record per block and a compact list of
rejection blocks over the reader's constant tables.  It defines the exact output of the device.  The known-key table and
the rejection strings below are the source of csrc/grdma_h2_meta_tables.h (tools/gen_h2_meta_tables.py)."""
from tests.h2_hpenc_model import hash_bytes

NONE = 0xffffffff
REQUEST, RESPONSE, TRAILERS = 1, 2, 3
(OK, MALFORMED, BAD_METHOD, BAD_CONTENT_TYPE, BAD_TE, BAD_TIMEOUT, UNIMPLEMENTED, BAD_ENCODING, HTTP_STATUS, NO_STATUS,
 BAD_GRPC_STATUS) = range(11)
HAS_TIMEOUT, END_STREAM, HAS_GRPC_STATUS, HAS_MESSAGE = 1, 2, 4, 8
BAD_INPUT = 1
ERR_FIELD_RANGE, ERR_STREAM, ERR_STRING = 1, 2, 3
STAT_KEYS = ("calls", "blocks", "requests", "responses", "trailers", "rejections", "malformed")
MAX_NS = (1 << 63) - 1

# key id = position + 1 (0: a custom name).  1..5 the pseudo-headers, 13..17 the connection-specific names.
KNOWN_KEYS = (b":method", b":scheme", b":path", b":authority", b":status", b"content-type", b"te", b"grpc-timeout",
              b"grpc-encoding", b"grpc-accept-encoding", b"grpc-status", b"grpc-message", b"connection", b"keep-alive",
              b"proxy-connection", b"transfer-encoding", b"upgrade")
(K_METHOD, K_SCHEME, K_PATH, K_AUTHORITY, K_STATUS, K_CONTENT_TYPE, K_TE, K_TIMEOUT, K_ENCODING, K_ACCEPT, K_GRPC_STATUS,
 K_MESSAGE, K_CONNECTION) = range(1, 14)
ENCODINGS = (b"identity", b"gzip", b"deflate")  # bit k of accept_encodings, value k of the record
UNITS = {b"H": 3600 * 10**9, b"M": 60 * 10**9, b"S": 10**9, b"m": 10**6, b"u": 10**3, b"n": 1}
CONTENT_TYPE = b"application/grpc"
# verdict -> (:status, grpc-status, grpc-message) of the Trailers-Only response; the fixed policy of rule 8
REJECTIONS = (
    (BAD_METHOD, b"405", b"13", b"the request's method is not POST"),
    (BAD_CONTENT_TYPE, b"415", b"13", b"the request's content-type is not application/grpc"),
    (BAD_TE, b"400", b"13", b"the request has no te: trailers"),
    (BAD_TIMEOUT, b"400", b"13", b"the request's grpc-timeout is malformed"),
    (UNIMPLEMENTED, b"200", b"12", b"the method is not implemented"),
    (BAD_ENCODING, b"200", b"12", b"the request's grpc-encoding is not supported"),
)


def accept_bits(names):
    bits = 0
    for n in names:
        bits |= 1 << ENCODINGS.index(n.encode() if isinstance(n, str) else n)
    return bits


def reject_tables(accept):
    """the reader's constant tables -> (fields [(name offset, value offset, name length | 1 << 24, value length)], the
    string arena, {verdict: (first field, fields)})"""
    fields, arena, lists = [], bytearray(), {}
    for verdict, status, grpc_status, message in REJECTIONS:
        hs = [(b":status", status), (b"content-type", CONTENT_TYPE), (b"grpc-status", grpc_status), (b"grpc-message", message)]
        if verdict == BAD_ENCODING:
            hs.append((b"grpc-accept-encoding", b",".join(e for k, e in enumerate(ENCODINGS) if accept >> k & 1)))
        lists[verdict] = (len(fields), len(hs))
        for name, value in hs:
            fields.append((len(arena), len(arena) + len(name), len(name) | 1 << 24, len(value)))
            arena += name + value
    return fields, bytes(arena), lists


def key_of(name):
    return KNOWN_KEYS.index(name) + 1 if name in KNOWN_KEYS else 0


def name_is_legal(name):
    if not name:
        return False
    legal = b"abcdefghijklmnopqrstuvwxyz0123456789-_."
    return all(b in legal or (k == 0 and b == 0x3a) for k, b in enumerate(name))


def field_is_bad(name, value):
    """rule 2"""
    key = key_of(name)
    if not name_is_legal(name) or (name[:1] == b":" and not 1 <= key <= 5):
        return True
    if not name.endswith(b"-bin") and any(b < 0x20 or b > 0x7e for b in value):
        return True
    return key >= K_CONNECTION or (key == K_TE and value != b"trailers")


def digits(value, lo, hi):
    return lo <= len(value) <= hi and all(0x30 <= b <= 0x39 for b in value)


def timeout_ns(value):
    """grpc-timeout -> nanoseconds saturated at 2^63 - 1, or None"""
    if not digits(value[:-1], 1, 8) or value[-1:] not in UNITS:
        return None
    n, unit = int(value[:-1]), UNITS[value[-1:]]
    return MAX_NS if n > MAX_NS // unit else n * unit


def content_type_is_good(value):
    return value == CONTENT_TYPE or (value.startswith(CONTENT_TYPE) and value[len(CONTENT_TYPE):len(CONTENT_TYPE) + 1] in (b"+", b";"))


class MethodTable:
    """the registered paths: open addressing over a power of two >= 2 n slots, FNV-1a, linear probing; bytes decide"""

    def __init__(self, methods):
        self.nslots = 2
        while self.nslots < 2 * len(methods):
            self.nslots *= 2
        self.slots = [None] * self.nslots
        for i, path in enumerate(methods):
            at = hash_bytes(path) & (self.nslots - 1)
            while self.slots[at] is not None:
                at = (at + 1) & (self.nslots - 1)
            self.slots[at] = (path, i)

    def find(self, path):
        at = hash_bytes(path) & (self.nslots - 1)
        while self.slots[at] is not None:
            if self.slots[at][0] == path:
                return self.slots[at][1]
            at = (at + 1) & (self.nslots - 1)
        return NONE


def check_methods(methods, accept):
    """why create refuses, or None"""
    if len(methods) > 4096:
        return "more than 4096 methods"
    if any(not 1 <= len(p) <= 1024 for p in methods):
        return "a path outside 1 .. 1024 bytes"
    if len(set(methods)) != len(methods):
        return "a path twice"
    if accept >> 3 or not accept & 1:
        return "accept_encodings"
    return None


def dump_methods(methods):
    return b"".join(len(p).to_bytes(4, "little") + p for p in methods)


def record_bytes(rec):
    """a call record (12 words) as the device writes it"""
    return b"".join(int(w).to_bytes(4, "little") for w in rec)


class MetaModel:
    def __init__(self, methods=(), accept=1):
        assert check_methods(list(methods), accept) is None
        self.methods, self.accept = MethodTable(list(methods)), accept
        self.reject_fields, self.reject_arena, self.reject_lists = reject_tables(accept)
        self.stats = dict.fromkeys(STAT_KEYS, 0)

    def block(self, stream, first, n, flags, fields, arena):
        """one block -> the 12 words of its call record"""
        seen, regular, bad_field, status_late = {}, False, NONE, NONE
        ncustom = 0

        def fault(i):
            nonlocal bad_field
            bad_field = min(bad_field, i)

        for i in range(first, first + n):
            no, vo, nl, vl = fields[i]
            name, value = bytes(arena[no:no + (nl & 0xffffff)]), bytes(arena[vo:vo + vl])
            key = key_of(name)
            ncustom += key == 0
            if field_is_bad(name, value):
                fault(i)
            if name[:1] == b":":
                if regular:
                    fault(i)  # behind a regular field
                if 1 <= key <= 5:
                    if key in seen:
                        fault(i)  # twice
                    if (key == K_STATUS and any(k in seen for k in (1, 2, 3, 4))) or (key != K_STATUS and K_STATUS in seen):
                        fault(i)  # :status beside a request pseudo-header
                    if (key == K_SCHEME and value not in (b"http", b"https")) or (key == K_PATH and not value):
                        fault(i)
                    if key == K_STATUS and K_STATUS not in seen and not digits(value, 3, 3):
                        status_late = i  # (a fault of a RESPONSE only: known at the block's end)
            else:
                regular = True
            if key and key not in seen:
                seen[key] = (i, value)  # the first occurrence wins
        kind = REQUEST if any(k in seen for k in (1, 2, 3, 4)) else RESPONSE if K_STATUS in seen else TRAILERS
        if kind == RESPONSE:
            fault(status_late)
        malformed = bad_field != NONE or (kind == REQUEST and not all(k in seen for k in (K_METHOD, K_SCHEME, K_PATH)))

        def val(key):
            return seen[key][1] if key in seen else None

        def idx(key):
            return seen[key][0] if key in seen else NONE

        timeout = timeout_ns(val(K_TIMEOUT)) if K_TIMEOUT in seen else None
        enc = 0
        if K_ENCODING in seen:
            enc = ENCODINGS.index(val(K_ENCODING)) if val(K_ENCODING) in ENCODINGS else 255
        method = self.methods.find(val(K_PATH)) if K_PATH in seen else NONE
        http_status = int(val(K_STATUS)) if K_STATUS in seen and digits(val(K_STATUS), 3, 3) else NONE
        grpc_ok = K_GRPC_STATUS in seen and digits(val(K_GRPC_STATUS), 1, 3)
        grpc_status = int(val(K_GRPC_STATUS)) if grpc_ok else NONE
        end = flags & 1
        if malformed:
            verdict = MALFORMED
        elif kind == REQUEST and val(K_METHOD) != b"POST":
            verdict = BAD_METHOD
        elif kind != TRAILERS and not (K_CONTENT_TYPE in seen and content_type_is_good(val(K_CONTENT_TYPE))):
            verdict = BAD_CONTENT_TYPE
        elif kind == REQUEST and K_TE not in seen:
            verdict = BAD_TE
        elif K_TIMEOUT in seen and timeout is None:
            verdict = BAD_TIMEOUT
        elif kind == REQUEST and method == NONE:
            verdict = UNIMPLEMENTED
        elif kind == REQUEST and (enc == 255 or not self.accept >> enc & 1):
            verdict = BAD_ENCODING
        elif kind == RESPONSE and http_status != 200:
            verdict = HTTP_STATUS
        elif end and kind != REQUEST and K_GRPC_STATUS not in seen:
            verdict = NO_STATUS
        elif K_GRPC_STATUS in seen and not grpc_ok:
            verdict = BAD_GRPC_STATUS
        else:
            verdict = OK
        fl = (HAS_TIMEOUT if timeout is not None else 0) | (END_STREAM if end else 0) | \
             (HAS_GRPC_STATUS if K_GRPC_STATUS in seen else 0) | (HAS_MESSAGE if K_MESSAGE in seen else 0)
        t = timeout or 0
        return (stream, kind | verdict << 8 | enc << 16 | fl << 24, method, http_status, grpc_status, t & 0xffffffff, t >> 32,
                idx(K_PATH), idx(K_AUTHORITY), idx(K_MESSAGE), ncustom, bad_field)

    def _check(self, k, blocks, fields, arena_len):
        stream, first, n, _ = blocks[k]
        if first + n > len(fields):
            return ERR_FIELD_RANGE
        if stream == 0 or stream > 0x7fffffff:
            return ERR_STREAM
        for no, vo, nl, vl in fields[first:first + n]:
            if no + (nl & 0xffffff) > arena_len or vo + vl > arena_len:
                return ERR_STRING
        return 0

    def read(self, blocks, fields, arena, meta_cap, reject_cap):
        """-> (call records [12 words], rejection blocks [(stream, first field, fields, 1)], result tuple, the error the
        call raises: None | "capacity" | "invalid")"""
        for k in range(len(blocks)):
            err = self._check(k, blocks, fields, len(arena))
            if err:
                return [], [], (0, 0, 0, 0, 0, 0, BAD_INPUT | err << 8 | k << 32, 0), "invalid"
        recs = [self.block(s, f, n, fl, fields, arena) for s, f, n, fl in blocks]
        kinds = [r[1] & 0xff for r in recs]
        verdicts = [r[1] >> 8 & 0xff for r in recs]
        rej = [(r[0],) + self.reject_lists[v] + (1,) for r, k, v in zip(recs, kinds, verdicts) if k == REQUEST and v not in (OK, MALFORMED)]
        res = (len(blocks), kinds.count(REQUEST), kinds.count(RESPONSE), kinds.count(TRAILERS), len(rej), verdicts.count(MALFORMED), 0)
        if len(blocks) > meta_cap or len(rej) > reject_cap:
            return [], [], res + (1,), "capacity"
        st = self.stats
        st["calls"] += 1
        for key, v in zip(STAT_KEYS[1:], res):
            st[key] += v
        return recs, rej, res + (0,), None
