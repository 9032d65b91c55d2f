"""gm_ws_messages (gm_ws.inc: a wave per segment, a uniform walk over the frame headers) against the
grammar restated in Python (ws_reference.py): views byte for byte and every result field, one batch
that holds every case; the capacity contract; and the point of it all: a masked `union select` the
scan cannot see as sent, and sees in the view."""

import numpy as np
import pytest

import ws_reference as ref
from gpumatch import engine, records, sigs, workloads
from ws_reference import frame

REPEATS = 9000   # segments in the batch: more than 8 workgroups of 4 waves on each of 256 CUs


def pay(n, salt=0):
    return bytes((7 * k + 31 * (k >> 8) + salt) & 0xFF for k in range(n))


GOOD = frame(1, b"good message", key=b"\x01\xfe\x7f\x80")
THREE = frame(1, b"GET /a", fin=False, key=b"\xa1\xb2\xc3\xd4") + frame(0, b"?id=1 union", fin=False, key=b"\x00\x01\x02\x03") + \
    frame(0, b" select 2", key=b"\xff\x00\xff\x01")
TRAIL = frame(2, pay(200), key=b"\x0f\x1e\x2d\x3c")   # an 8-byte header
FORMS = {0: 20, 2: 300, 8: 65536}                    # a payload length of each length form
ERRORS = {"RSV": frame(1, b"x", rsv=2), "OPCODE": frame(3, b"x"), "UNMASKED": frame(1, b"x", masked=False),
          "CTRL_FRAG": frame(9, b"x", fin=False), "CTRL_LEN": frame(9, b"x" * 126), "LENGTH": frame(1, b"x" * 10, length_form=2),
          "CONT": frame(0, b"x"), "NESTED": frame(1, b"a", fin=False) + frame(1, b"b")}


def cases():
    """(name, segment, the alignment its offset must have or None)"""
    c = [(f"len_{n}", frame(1, pay(n, n)) + frame(2, b"tail"), None) for n in (0, 1, 3, 4, 5, 15, 16, 17, 125, 126, 127, 65535, 65536)]
    c += [(f"align_{k}", THREE, k) for k in range(16)]
    c += [(f"phase_{j}", frame(9, b"p" * j) + frame(1, pay(40, j), key=b"\x10\x20\x40\x80"), 0) for j in range(4)]
    c += [("fragments_ping", frame(1, b"abc", fin=False) + frame(9, b"ping") + frame(0, b"def", fin=False) + frame(10, b"") +
           frame(0, b"ghi"), None),
          ("empty_message", frame(1, b""), None), ("text_binary", frame(1, b"text") + frame(2, b"\x00\xffbin"), None)]
    c += [(f"header_{d}_before_step_form_{f}", frame(2, pay(1024 - d - 8)) + frame(1, pay(n, d), key=b"\x55\xaa\x0f\xf0") + GOOD, 0)
          for d in (1, 2, 9, 13) for f, n in FORMS.items()]
    c += [("payload_3000", frame(1, pay(3000)), None), ("ends_at_step", frame(1, pay(1016)), 0),
          ("ping_over_step", frame(1, pay(1000)) + frame(9, b"p" * 100) + frame(1, b"after"), 0),
          ("empty_x300", frame(1, b"") * 300, None)]
    c += [(f"cut_{k}", GOOD + TRAIL[:k], None) for k in (1, 2, 3, 4, 5, 6, 7, 8, 58)]
    c += [("open_at_end", GOOD + frame(1, b"open ", fin=False) + frame(0, b"still", fin=False), None)]
    c += [(f"error_{name}", GOOD + bad + GOOD, None) for name, bad in ERRORS.items()]
    c += [("length_64_small", GOOD + frame(1, pay(200), length_form=8), None),
          ("length_64_top_bit", GOOD + b"\x81\xff\x80" + bytes(7) + b"abcd", None),
          ("length_64_huge", GOOD + b"\x81\xff\x00\x00\x01" + bytes(5) + b"abcd" + pay(100), None),
          ("rsv1_data", GOOD + frame(1, b"deflated", rsv=4) + GOOD, None),
          ("close_then_more", GOOD + frame(8, b"\x03\xe8bye") + GOOD, None), ("zero_length", b"", None)]
    return c


CASES = cases()
SMALL = [i for i, (_, s, _) in enumerate(CASES) if len(s) < 4096]


def batch():
    """the wire bytes and the segments: every case once, then the small ones again up to REPEATS"""
    order = list(range(len(CASES))) + [SMALL[k % len(SMALL)] for k in range(REPEATS - len(CASES))]
    wire, segs = bytearray(), []
    for i in order:
        _, s, align = CASES[i]
        if align is not None:
            wire += bytes((align - len(wire)) % 16)
        segs.append((len(wire), len(s)))
        wire += s
    return bytes(wire), segs, order


@pytest.fixture(scope="module")
def run():
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    wire, segs, order = batch()
    views, res = engine.Engine(0).ws_messages_host(wire, segs)
    return views, res, order


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_ws_matches_reference(run, i):
    views, res, order = run
    view, status, reason, consumed, stop, n_messages = ref.parse(CASES[i][1])
    for k in [k for k, j in enumerate(order) if j == i]:
        assert views[k] == view
        assert tuple(int(x) for x in res[k]) == (status | reason << 8, consumed, stop, n_messages)


def test_reference_on_spelled_out_cases():
    got = {name: ref.parse(s) for name, s, _ in CASES}
    assert got["align_0"] == (b"GET /a?id=1 union select 2\n", ref.OK, 0, len(THREE), len(THREE), 1)
    assert got["fragments_ping"][0] == b"abcdefghi\n" and got["text_binary"][0] == b"text\n\x00\xffbin\n"
    assert got["empty_x300"][0] == b"\n" * 300 and got["empty_x300"][5] == 300
    assert all(got[f"cut_{k}"] == (b"good message\n", ref.OK, 0, len(GOOD), len(GOOD), 1) for k in (1, 8, 58))
    assert got["open_at_end"] == (b"good message\n", ref.OK, 0, len(GOOD), len(CASES[[c[0] for c in CASES].index("open_at_end")][1]), 1)
    for name in ERRORS:
        view, status, reason = got[f"error_{name}"][:3]
        assert (view, status, ref.REASONS[reason]) == (b"good message\n", ref.PROTO, name)
    assert got["error_NESTED"][3:5] == (len(GOOD), len(GOOD) + 7)   # consumed before the open message, stop at the nested frame
    assert got["length_64_top_bit"][1:3] == (ref.PROTO, ref.LENGTH) and got["length_64_huge"][1] == ref.OK
    assert got["rsv1_data"][:5] == (b"good message\n", ref.DEFLATE, 0, len(GOOD), len(GOOD))
    assert got["close_then_more"][:5] == (b"good message\n", ref.CLOSED, 0, len(GOOD) + 11, len(GOOD))
    assert all(len(v[0]) <= len(s) for v, (_, s, _) in zip(got.values(), CASES))


@pytest.mark.gpu
def test_ws_capacity_overflow_is_reported_once():
    eng = engine.Engine(0)
    segs = [(0, len(THREE)), (len(THREE), len(GOOD))]
    with pytest.raises(engine.GmError) as err:
        eng.ws_messages_host(THREE + GOOD, segs, out_cap=len(THREE) + len(GOOD) - 1)
    assert err.value.code == engine.GM_E_OVERFLOW
    eng.sync(0)   # reported once
    views, res = eng.ws_messages_host(THREE + GOOD, segs)
    assert views == [b"GET /a?id=1 union select 2\n", b"good message\n"] and list(res["n_messages"]) == [1, 1]


@pytest.mark.gpu
def test_ws_view_shows_the_scan_what_the_wire_hides():
    eng = engine.Engine(0)
    (view,), _ = eng.ws_messages_host(THREE, [(0, len(THREE))])
    eng.load(workloads.c4_blob(sigs.SigSet([sigs.Rule("lit", True, "ab", b"union select")], ())), 1)
    hits = []
    for body in (THREE, view):
        reqs, arena = records.from_dicts([{"host": "cafe.example.com", "uri": "/tea/chat", "https": True, "body": body}])
        hits.append(int(eng.match_host(reqs, arena)[0]["n_hits"][0]))
    assert hits == [0, 1]
