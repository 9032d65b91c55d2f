"""The multipart request parser in the match path (gm_multipart.inc -> gm_decode.inc's shadow views):
a request with a multipart body hits what the oracle finds in the request as sent or in the request
whose body is the part view M (mp_reference.py) with Content-Type application/json if a part is JSON,
else text/plain (the oracle ignores the name `multipart`, so it runs every other declared parser);
with `wallarm_parser_disable multipart` only the former.  The CPU test: the compiler's bit."""

import base64
import ctypes

import numpy as np
import pytest

import mp_reference as ref
from gpumatch import blob, engine, records, sigs, workloads
from oracle_py import Oracle

# no '\n' and no end anchor in any rule: no match can depend on where a part of a view ends
RULES = [sigs.Rule("lit", True, "ab", b"union select"), sigs.Rule("lit", False, "b", b"/bin/sh"),
         sigs.Rule("lit", True, "ab", b"<script>"), sigs.Rule("re", False, "ab", r"etc/pass(wd|wd2)"),
         sigs.Rule("re", True, "ab", r"[0-9]{3}zq")]
EXAMPLES = [b"1 union select 2", b"run /bin/sh -c id", b"<script>alert(1)</script>", b"cat /etc/passwd now", b"a 123zq b"]
MID = [8, 7, 4, 10, 4]   # an offset inside what the rule matches in each example
DECODERS = ("multipart", "json_doc", "base64")
CT = b"multipart/form-data; boundary=----gm7MA4YWxk"
CD = b"Content-Disposition: form-data; "


def body(parts):
    return b"".join(b"------gm7MA4YWxk\r\n" + b"\r\n".join(h) + b"\r\n\r\n" + c + b"\r\n" for h, c in parts) + \
        b"------gm7MA4YWxk--\r\n"


def wrap76(t):
    return b"\r\n".join(t[i:i + 76] for i in range(0, len(t), 76))


def items():
    out = []
    for i in range(70):
        ex, pad = EXAMPLES[i % 5], b" lorem ipsum dolor" * (i % 7)
        it = {"host": "cafe.example.com", "uri": "/tea/" + "x" * (i % 5), "https": True, "headers": [("Content-Type", CT)]}
        text = ([CD + b'name="note"'], b"plain text" + pad)
        k = i % 7
        if k == 0:     # base64 part, the payload across a 76-column break
            raw = b"z" * (57 - MID[i % 5]) + ex + b" tail" + pad   # a line of 76 characters holds 57 bytes
            it["body"] = body([text, ([CD + b'name="f"; filename="a.bin"', b"Content-Transfer-Encoding: base64"],
                                      wrap76(base64.b64encode(raw)))])
        elif k == 1:   # quoted-printable part, with a soft break inside the payload
            qp = b"".join(b"=%02X" % c if c in b"<>/ =" else bytes([c]) for c in ex)
            it["body"] = body([([CD + b'name="q"', b"Content-Transfer-Encoding: quoted-printable"],
                                qp[:5] + b"=\r\n" + qp[5:] + pad), text])
        elif k == 2:   # \u-escaped in a JSON part beside a file part
            it["body"] = body([([CD + b'name="meta"', b"Content-Type: application/json"],
                                b'{"v": "' + b"".join(b"\\u%04x" % c for c in ex) + b'"}'), text])
        elif k == 3:   # percent-encoded in filename*=
            it["body"] = body([([CD + b"name=up; filename*=UTF-8''" + b"".join(b"%%%02x" % c for c in ex)], b"data" + pad)])
        elif k == 4:   # plain in a part
            it["body"] = body([text, ([CD + b'name="c"'], ex + pad)])
        elif k == 5:   # benign multipart
            it["body"] = body([text, ([CD + b'name="f"', b"Content-Transfer-Encoding: base64"], wrap76(base64.b64encode(pad * 4)))])
        else:          # benign raw body, no Content-Type
            it["headers"], it["body"] = [], b"q=nothing to see" + pad
        out.append(it)
    return out


def viewed(it):
    """the request whose body is M (a raw body: as it is)"""
    v = ref.view(it["body"], dict(it["headers"]).get("Content-Type"))
    if v is None:
        return it
    return dict(it, body=v[0], headers=[("Content-Type", "application/json" if v[1] & 1 else "text/plain")])


def per_request(v, h):
    return [set(int(x) for x in h[int(r["first_hit_off"]):int(r["first_hit_off"]) + int(r["n_hits"])]) for r in v]


@pytest.mark.gpu
@pytest.mark.parametrize("disable", ["", "multipart"])
def test_multipart_bodies_parity(disable):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    b = workloads.c4_blob(sigs.SigSet(RULES, DECODERS), "monitoring", parser_disable=disable)
    its = items()
    reqs, arena = records.from_dicts(its)
    ora = Oracle(b, 5)
    exp_v, exp_h = ora.match(reqs, arena, nthreads=4)
    exp = per_request(exp_v, exp_h)
    # as sent the oracle sees only the plain plants: it misses the base64, quoted-printable, JSON and filename* ones
    assert all(not exp[i] for i in range(70) if i % 7 < 4) and sum(map(len, exp)) == 10
    if not disable:
        exp = [a | c for a, c in zip(exp, per_request(*ora.match(*records.from_dicts([viewed(it) for it in its]), nthreads=4)))]
        assert sum(map(len, exp)) == 50
    eng = engine.Engine(0)
    eng.load(b, 5)
    got_v, got_h = eng.match_host(reqs, arena)
    assert per_request(got_v, got_h) == exp
    for f in got_v.dtype.names:
        if f not in ("n_hits", "first_hit_off"):
            assert np.array_equal(got_v[f], exp_v[f]), f
    assert eng.stats()["last_multipart"] == (0 if disable else 60)
    # a second run of the batch (the shadow is rebuilt from the inputs): the same hits
    again_v, again_h = eng.match_host(reqs, arena)
    assert np.array_equal(again_v, got_v) and np.array_equal(again_h, got_h)


CONF = """http {
    wallarm_mode block;
    upstream u { server 10.0.0.1:80; }
    server {
        listen 80;
        server_name a.example.com;
        location / { proxy_pass http://u; }
        location /nomp/ { wallarm_parser_disable multipart; proxy_pass http://u; }
    }
}
"""


def test_multipart_decoder_bit_and_parser_disable():
    e = engine.Engine(compile_only=True)
    e.load(blob.make_blob(CONF, {}, sigs.SigSet(RULES, ("multipart",)).to_text()), 1)
    assert e.stats()["decoders"] == 0x20
    f = engine.lib().gm_debug_loc_decoders
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    assert [f(e.h, 0), f(e.h, 1), f(e.h, 2)] == [0x20, 0, -1]
    e.load(blob.make_blob(CONF, {}, sigs.SigSet(RULES, ("gzip", "base64", "multipart")).to_text()), 2)
    assert e.stats()["decoders"] == 0x38 and [f(e.h, 0), f(e.h, 1)] == [0x38, 0x18]
