"""The xml request parser in the match path (gm_xml.inc -> gm_decode.inc's shadow views): a request
with an XML body hits what the oracle finds in the request as sent or in the request whose body is
the character-data view X (xml_reference.py) under text/plain (the oracle ignores the name `xml`, so
it runs every other declared parser); with `wallarm_parser_disable xml` only the former.  The CPU
test: the compiler's bit."""

import base64
import ctypes

import numpy as np
import pytest

import xml_reference as ref
from gpumatch import blob, engine, records, sigs, workloads
from oracle_py import Oracle

# no '\n' and no end anchor in any rule: no match can depend on where a piece of a view ends
RULES = [sigs.Rule("lit", True, "ab", b"union select"), sigs.Rule("lit", False, "b", b"/bin/sh"),
         sigs.Rule("lit", True, "ab", b"<script>"), sigs.Rule("re", False, "ab", r"etc/pass(wd|wd2)"),
         sigs.Rule("re", True, "ab", r"[0-9]{3}zq")]
EXAMPLES = [b"1 union select 2", b"run /bin/sh -c id", b"<script>alert(1)</script>", b"cat /etc/passwd now", b"a 123zq b"]
MID = [8, 7, 4, 10, 4]   # an offset inside what the rule matches in each example
DECODERS = ("xml", "base64")


def soap(inner, attr=b"1"):
    return b'<?xml version="1.0"?><!-- request --><e:Envelope xmlns:e="http://x/"><e:Body><op id="' + attr + \
        b'">' + inner + b"</op></e:Body></e:Envelope>"


def items():
    out = []
    for i in range(70):
        ex, pad = EXAMPLES[i % 5], b" lorem ipsum dolor" * (i % 7)
        it = {"host": "cafe.example.com", "uri": "/tea/" + "x" * (i % 5), "https": True, "headers": [("Content-Type", b"text/xml")]}
        k = i % 7
        if k == 0:     # numeric references with leading zeros
            it["body"] = soap(b"".join(b"&#x%07x;" % c if j % 2 else b"&#%05d;" % c for j, c in enumerate(ex)) + pad)
        elif k == 1:   # named references in an attribute value
            it["body"] = soap(pad, b"x &lt;script&gt;alert(&quot;1&quot;)&lt;/script&gt;")
        elif k == 2:   # a CDATA section, under a Content-Type that needs the prolog rule
            it["headers"] = [("Content-Type", b"application/octet-stream")]
            it["body"] = soap(b"<![CDATA[" + ex[:MID[i % 5]] + b"]]><![CDATA[" + ex[MID[i % 5]:] + b"]]>" + pad)
        elif k == 3:   # the keyword split by a comment
            a, z = (s.replace(b"<", b"&lt;").replace(b">", b"&gt;") for s in (ex[:MID[i % 5]], ex[MID[i % 5]:]))
            it["body"] = soap(a + b"<!-- -->" + z + pad)
        elif k == 4:   # a base64 run inside text, itself split by a comment
            t = base64.b64encode(b"zzzz" + ex + b" tail" + pad)
            it["body"] = soap(t[:9] + b"<!--x-->" + t[9:])
        elif k == 5:   # benign XML
            it["body"] = soap(b"<n>tea &amp; cake</n>" + pad)
        else:          # benign raw body, no Content-Type
            it["headers"], it["body"] = [], b"q=nothing to see" + pad
        out.append(it)
    return out


def viewed(it):
    """the request whose body is X (a body that is not taken: as it is)"""
    v = ref.view(it["body"], dict(it["headers"]).get("Content-Type"))
    return it if v is None else dict(it, body=v, headers=[("Content-Type", "text/plain")])


def per_request(v, h):
    return [set(int(x) for x in h[int(r["first_hit_off"]):int(r["first_hit_off"]) + int(r["n_hits"])]) for r in v]


@pytest.mark.gpu
@pytest.mark.parametrize("disable", ["", "xml"])
def test_xml_bodies_parity(disable):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    b = workloads.c4_blob(sigs.SigSet(RULES, DECODERS), "monitoring", parser_disable=disable)
    its = items()
    reqs, arena = records.from_dicts(its)
    ora = Oracle(b, 5)
    exp_v, exp_h = ora.match(reqs, arena, nthreads=4)
    exp = per_request(exp_v, exp_h)
    # as sent the oracle sees none of the plants: references, CDATA and comments hide every one
    assert sum(map(len, exp)) == 0
    if not disable:
        exp = [a | c for a, c in zip(exp, per_request(*ora.match(*records.from_dicts([viewed(it) for it in its]), nthreads=4)))]
        assert all(len(exp[i]) == (1 if i % 7 < 5 else 0) for i in range(70))
    eng = engine.Engine(0)
    eng.load(b, 5)
    got_v, got_h = eng.match_host(reqs, arena)
    assert per_request(got_v, got_h) == exp
    for f in got_v.dtype.names:
        if f not in ("n_hits", "first_hit_off"):
            assert np.array_equal(got_v[f], exp_v[f]), f
    assert eng.stats()["last_xml"] == (0 if disable else 60)
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
        location /noxml/ { wallarm_parser_disable xml; proxy_pass http://u; }
    }
}
"""


def test_xml_decoder_bit_and_parser_disable():
    e = engine.Engine(compile_only=True)
    e.load(blob.make_blob(CONF, {}, sigs.SigSet(RULES, ("xml",)).to_text()), 1)
    assert e.stats()["decoders"] == 0x40
    f = engine.lib().gm_debug_loc_decoders
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    assert [f(e.h, 0), f(e.h, 1), f(e.h, 2)] == [0x40, 0, -1]
    e.load(blob.make_blob(CONF, {}, sigs.SigSet(RULES, ("gzip", "multipart", "xml")).to_text()), 2)
    assert e.stats()["decoders"] == 0x70 and [f(e.h, 0), f(e.h, 1)] == [0x70, 0x30]
