"""The gzip request parser in the match path (gm_inflate.inc -> gm_decode.inc's shadow views): a
request with a gzipped body hits what the oracle finds in the request as sent or in the request
with its body inflated (the oracle ignores the name `gzip`, so it runs every other declared
parser); with `wallarm_parser_disable gzip` only the former.  The CPU test: the compiler's bit."""

import base64
import ctypes
import gzip

import numpy as np
import pytest

from gpumatch import blob, engine, records, sigs, workloads
from oracle_py import Oracle

# no '\n' and no end anchor in any rule: no match can depend on where a part of a view ends
RULES = [sigs.Rule("lit", True, "ab", b"union select"), sigs.Rule("lit", False, "b", b"/bin/sh"),
         sigs.Rule("lit", True, "ab", b"<script>"), sigs.Rule("re", False, "ab", r"etc/pass(wd|wd2)"),
         sigs.Rule("re", True, "ab", r"[0-9]{3}zq")]
EXAMPLES = [b"1 union select 2", b"run /bin/sh -c id", b"<script>alert(1)</script>", b"cat /etc/passwd now", b"a 123zq b"]
DECODERS = ("gzip", "json_doc", "base64")
JSON = ("Content-Type", "application/json")


def items():
    out = []
    for i in range(60):
        ex, pad = EXAMPLES[i % 5], b" lorem ipsum dolor" * (i % 7)
        it = {"host": "cafe.example.com", "uri": "/tea/" + "x" * (i % 5), "https": True}
        k = i % 6
        if k == 0:     # plain in a gzipped body
            it["body"] = gzip.compress(b"q=" + ex + pad)
        elif k == 1:   # JSON-escaped in a gzipped JSON body
            it["headers"] = [JSON]
            it["body"] = gzip.compress(b'{"v": "' + b"".join(b"\\u%04x" % c for c in ex) + b'", "p": "' + pad + b'"}')
        elif k == 2:   # base64 in a gzipped body
            it["body"] = gzip.compress(b"data=" + base64.b64encode(ex + b" padding-bytes") + pad)
        elif k == 3:   # raw body
            it["body"] = b"q=" + ex + pad
        elif k == 4:   # benign, gzipped
            it["body"] = gzip.compress(b"nothing to see here" + pad)
        else:          # benign, raw or no body
            it["body"] = pad
        out.append(it)
    return out


def is_gzip(b):
    return len(b) >= 18 and b[:3] == b"\x1f\x8b\x08"


def per_request(v, h):
    return [set(int(x) for x in h[int(r["first_hit_off"]):int(r["first_hit_off"]) + int(r["n_hits"])]) for r in v]


@pytest.mark.gpu
@pytest.mark.parametrize("disable", ["", "gzip"])
def test_gzip_bodies_parity(disable):
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    b = workloads.c4_blob(sigs.SigSet(RULES, DECODERS), "monitoring", parser_disable=disable)
    its = items()
    reqs, arena = records.from_dicts(its)
    ora = Oracle(b, 5)
    exp_v, exp_h = ora.match(reqs, arena, nthreads=4)
    exp = per_request(exp_v, exp_h)
    assert sum(map(len, exp)) == 10   # the oracle ignores `gzip`: only the raw bodies' plants
    if not disable:
        inflated = [dict(it, body=gzip.decompress(it["body"])) if is_gzip(it["body"]) else it for it in its]
        exp = [a | c for a, c in zip(exp, per_request(*ora.match(*records.from_dicts(inflated), nthreads=4)))]
        assert sum(map(len, exp)) == 40
    eng = engine.Engine(0)
    eng.load(b, 5)
    got_v, got_h = eng.match_host(reqs, arena)
    assert per_request(got_v, got_h) == exp
    for f in got_v.dtype.names:
        if f not in ("n_hits", "first_hit_off"):
            assert np.array_equal(got_v[f], exp_v[f]), f
    assert eng.stats()["last_inflated"] == (0 if disable else sum(is_gzip(it["body"]) for it in its))
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
        location /nogz/ { wallarm_parser_disable gzip; proxy_pass http://u; }
    }
}
"""


def test_gzip_decoder_bit_and_parser_disable():
    e = engine.Engine(compile_only=True)
    e.load(blob.make_blob(CONF, {}, sigs.SigSet(RULES, ("gzip", "base64")).to_text()), 1)
    assert e.stats()["decoders"] == 0x18
    f = engine.lib().gm_debug_loc_decoders
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    assert [f(e.h, 0), f(e.h, 1), f(e.h, 2)] == [0x18, 0x08, -1]
    e.load(blob.make_blob(CONF, {}, sigs.SigSet(RULES, ("gzip",)).to_text()), 2)
    assert e.stats()["decoders"] == 0x10 and f(e.h, 1) == 0
