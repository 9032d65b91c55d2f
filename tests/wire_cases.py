"""Wire batches whose records take no arena byte: an invalid request carries only its
connection's address, so one without an address (gm_wire_msg.raddr_len 0 -- include/gpumatch.h
allows it) and without a PROXY address has a zero-size slot.  Shared by the oracle's known answers
(tests/test_wire.py) and the GPU parity tests (tests/test_gpu_wire.py)."""

from __future__ import annotations

import numpy as np

from gpumatch import records, wire
from oracle_py import parse_requests

# invalid requests and the status nginx 1.17.3 answers (orc_parse_one)
BAD = [
    (b"G@T / HTTP/1.1\r\nHost: a\r\n\r\n", 400),                                  # a bad request line
    (b"GET /\r\n\r\n", 400),                                                       # no version
    (b"GET / HTTP/2.0\r\nHost: a\r\n\r\n", 505),                                  # unsupported version
    (b"POST /x HTTP/1.1\r\nHost: a\r\nTransfer-Encoding: gzip\r\n\r\n", 501),      # unknown transfer coding
    (b"GET /x HTTP/1.1\r\nHost: a\r\n", 400),                                      # no empty line
]
# an unknown method: nginx's request line takes any [A-Z_-]+ token (the 501 / 405 is the content
# handler's), so this one is valid -- with no address its slot is not empty
UNKNOWN_METHOD = b"BREW /pot HTTP/1.1\r\nHost: cafe.example.com\r\n\r\n"
COMPLEX = b"GET //tea/./x/%2e%2E/y?q=1 HTTP/1.1\r\nHost: cafe.example.com\r\n\r\n"     # a full-list request
NO_ADDR = {"https": False, "port": 80, "raddr": ""}


def _status(r):
    return int(r["pad0"][1]) | int(r["pad0"][2]) << 8 if r["flags"] & records.REQ_INVALID else 0


def zero_slot_batch(n=2000, seed=606):
    """(messages, conn).  The head (HEAD below) places zero-size requests first, three in a row,
    between two flat valid requests, either side of both kinds of full-list request (a complex-URI
    path; a chunked body of more than WIRE_PIECES = 8 chunks), and -- behind a request padded for it -- at a base that is a multiple of 1024; a seeded mix follows
    (valid requests without an address among it) and a zero-size request ends the batch."""
    rng = np.random.Generator(np.random.PCG64(seed))
    flat = wire.serialize({"uri": "/tea", "host": "cafe.example.com", "headers": [("Accept", "*/*")]})
    chunks = wire.serialize({"method": "POST", "uri": "/tea/x", "host": "cafe.example.com", "body": b"c" * 36,
                             "chunked": [3] * 12})
    Z = [m for m, _ in BAD]
    C = {"https": False, "port": 80}
    head = [(Z[0], NO_ADDR), (flat, C), (Z[2], NO_ADDR), (flat, C),
            (Z[3], NO_ADDR), (Z[1], NO_ADDR), (Z[4], NO_ADDR), (flat, C),
            (Z[2], NO_ADDR), (COMPLEX, C), (Z[3], NO_ADDR), (flat, NO_ADDR),
            (Z[0], NO_ADDR), (chunks, C), (Z[2], NO_ADDR), (UNKNOWN_METHOD, NO_ADDR)]
    # the pad request: its slot ends the arena so far on a multiple of 1024
    W, M = wire.build([m for m, _ in head], [c for _, c in head])
    reqs, arena = parse_requests(W, M)
    it = {"uri": "/coffee", "host": "cafe.example.com", "headers": [("X-Pad", "")]}
    P = dict(C, raddr="10.0.0.1")   # (wire.build's default address grows with the index)
    r0, _ = parse_requests(*wire.build([wire.serialize(it)], [P]))
    tot0 = sum(records.field_len(r0[0], f) for f in records.WIRE_FIELDS)
    k = (-(len(arena) + tot0)) % 1024
    it["headers"] = [("X-Pad", "p" * k)]
    head += [(wire.serialize(it), P), (Z[3], NO_ADDR), (flat, C)]
    msgs, conn = wire.synthetic(n - len(head) - 1, seed=seed)
    for i in range(len(msgs)):
        u = rng.random()
        if u < 0.2:
            msgs[i] = Z[int(rng.integers(0, len(Z)))]
            conn[i] = dict(conn[i], raddr="")
        elif u < 0.3:
            conn[i] = dict(conn[i], raddr="")        # (most of these are valid: a non-empty slot)
    msgs = [m for m, _ in head] + msgs + [Z[1]]
    conn = [c for _, c in head] + conn + [NO_ADDR]
    return msgs, conn


# where zero_slot_batch's head puts what (message indices)
HEAD = {"first": 0, "between": 2, "row": (4, 5, 6), "complex": 9, "chunked": 13, "valid_no_addr": (11, 15),
        "pad": 16, "k1024": 17}


def slot_sizes(reqs):
    """the bytes each record takes in the arena (before alignment)"""
    return np.array([sum(records.field_len(r, f) for f in records.WIRE_FIELDS) for r in reqs], dtype=np.int64)


def only_zero_slots(n=300):
    """A batch of zero-size requests alone: the arena's length is 0."""
    msgs = [BAD[i % len(BAD)][0] for i in range(n)]
    return msgs, [dict(NO_ADDR, https=bool(i % 2), port=443 if i % 2 else 80) for i in range(n)]
