"""gm_multipart_bodies (gm_multipart.inc: a wave per multipart body) against the grammar restated in
Python (mp_reference.py), byte for byte with length and flags: one batch holds every case."""

import base64

import numpy as np
import pytest

import mp_reference as ref
from gpumatch import engine, records

pytestmark = pytest.mark.gpu

CD = b'Content-Disposition: form-data; '


def ct(B):
    return b"multipart/form-data; boundary=" + B


def mp(parts, B=b"XbX", nl=b"\r\n", close=True, pre=b""):
    """parts: (header lines, content or None for a part with no empty line)"""
    out = pre
    for hdrs, content in parts:
        out += b"--" + B + nl + nl.join(hdrs) + (nl if content is None else nl + nl + content + nl)
    return out + (b"--" + B + b"--" + nl if close else b"")


def two(nl=b"\r\n", B=b"XbX", **kw):
    return mp([([CD + b'name="a"'], b"one <1>"), ([CD + b'name="b"; filename="f.txt"', b"Content-Type: text/plain"], b"two")],
              B, nl, **kw)


def b64_part(data, nl, cols=76, tail=b""):
    t = base64.b64encode(data)
    return ([CD + b'name="f"', b"Content-Transfer-Encoding: base64"],
            nl.join(t[i:i + cols] for i in range(0, len(t), cols)) + tail)


def qp_part(content):
    return ([CD + b"name=q", b"content-transfer-encoding:  Quoted-Printable "], content)


def cases():
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    data = rng.integers(0, 256, 3072, dtype=np.uint8).tobytes()
    fill = (b"lorem ipsum dolor sit amet " * 50)
    c = [("crlf", ct(b"XbX"), two()), ("lf", ct(b"XbX"), two(b"\n")),
         ("quoted_boundary", b'multipart/form-data; boundary="XbX"; charset=x', two()),
         ("boundary_second", b"Multipart/Mixed; charset=utf-8; Boundary=XbX", two())]
    c += [(f"boundary_{k}", ct(b"b" * k), two(B=b"b" * k)) for k in (1, 62, 63, 64, 70, 71)]
    c += [(f"delim_at_{k}", ct(b"XbX"), two(pre=b"p" * (k - 1) + b"\n")) for k in range(1000, 1041)]
    c += [("wrong_boundary", ct(b"XbX"), two(pre=b"a\n--XbY\r\nzz\r\n")),
          ("d_then_x", ct(b"XbX"), mp([([CD + b"name=a"], b"1\r\n--XbXx\r\n2")])),
          ("d_spaces_tabs", ct(b"XbX"), b"--XbX \t \r\n" + CD + b"name=a\r\n\r\nv\r\n--XbX--\r\n"),
          ("epilogue_with_d", ct(b"XbX"), two() + b"epilogue\r\n--XbX\r\n" + CD + b"name=late\r\n\r\nno\r\n"),
          ("no_close", ct(b"XbX"), two(close=False)), ("no_close_bare", ct(b"XbX"), two(close=False)[:-2]),
          ("no_delimiter", ct(b"XbX"), b"just text\r\n-- XbX\r\n"),
          ("preamble", ct(b"XbX"), two(pre=b"This is a preamble.\r\n")),
          ("empty_content", ct(b"XbX"), mp([([CD + b"name=e"], b"")])),
          ("no_empty_line", ct(b"XbX"), mp([([CD + b"name=h", b"X-Other: 1"], None), ([CD + b"name=n"], b"x")])),
          ("parts_64", ct(b"XbX"), mp([([CD + b"name=p%d" % k], b"v%d" % k) for k in range(64)])),
          ("parts_65", ct(b"XbX"), mp([([CD + b"name=p%d" % k], b"v%d" % k) for k in range(65)])),
          ("quoted_escape", ct(b"XbX"), mp([([CD + b'name="a\\"b"; filename="c:\\\\d\\'], b"v")])),
          ("token_name", ct(b"XbX"), mp([([CD + b"name=tok;filename=t.bin"], b"v")])),
          ("filename_alone", ct(b"XbX"), mp([([b"content-disposition: attachment; filename=only.txt"], b"v")])),
          ("filename_star", ct(b"XbX"), mp([([CD + b"name=u; filename*=UTF-8''%3Cscript%3E%2"], b"v")])),
          ("name_in_value", ct(b"XbX"), mp([([CD + b'filename="x; name=hidden' + b"y" * 80 + b'"; name=real'], b"v")])),
          ("mixed_case_header", ct(b"XbX"), mp([([b"cOnTeNt-DiSpOsItIoN: form-data; NAME=mc", b"CONTENT-TYPE: Application/JSON"],
                                                  b'{"a": 1}')])),
          ("long_name", ct(b"XbX"), mp([([CD + b'name="' + b"n\\\\" * 70 + b'"; filename=' + b"f" * 150], b"v")])),
          ("b64_crlf", ct(b"XbX"), mp([b64_part(data, b"\r\n")])), ("b64_lf", ct(b"XbX"), mp([b64_part(data, b"\n")], nl=b"\n")),
          ("b64_partial", ct(b"XbX"), mp([b64_part(data[:1000], b"\r\n", 76, b"QU")])),
          ("b64_stray", ct(b"XbX"), mp([b64_part(data[:500], b" = \r\n", 61, b"==")])),
          ("qp_mix", ct(b"XbX"), mp([qp_part(b"a=3Db==41c=\r\nd=\ne=3cscript=3E =ZZ " + fill[:300] + b"=4")])),
          ("qp_lone_end", ct(b"XbX"), mp([qp_part(b"tail =")])),
          ("large_random", ct(b"XbX"), mp([([CD + b'name="blob"; filename="r.bin"'], rnd)])),
          ("not_multipart", b"application/json", two()), ("no_content_type", None, two()),
          ("no_boundary", b"multipart/form-data", two()), ("empty_body", ct(b"XbX"), b"")]
    c += [(f"qp_at_{k}", ct(b"XbX"), mp([qp_part(fill[:k] + b"=3C" + fill[:70])])) for k in range(1000, 1041)]
    return c


CASES = cases()


@pytest.fixture(scope="module")
def views():
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    # (URI lengths differ, so the bodies start at every alignment)
    reqs, arena = records.from_dicts([{"host": "a.example.com", "uri": "/" + "u" * (i % 37), "body": b, "port": 80,
                                       "headers": [("Accept", "*/*")] + ([("Content-Type", t)] if t is not None else [])}
                                      for i, (_, t, b) in enumerate(CASES)])
    return engine.Engine(0).multipart_bodies(reqs, arena)


def test_reference_delimiters_in_large_random():
    body = dict((c[0], c[2]) for c in CASES)["large_random"]
    assert len(ref.delimiters(body, b"XbX")) == 2   # no accidental match in the random content


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_multipart_matches_reference(views, i):
    _, t, body = CASES[i]
    assert views[i] == ref.view(body, t)
