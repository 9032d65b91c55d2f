"""gm_xml_bodies (gm_xml.inc: a wave per XML body, a parallel finite-state scan) against the grammar
restated in Python (xml_reference.py), byte for byte: one batch holds every case."""

import numpy as np
import pytest

import xml_reference as ref
from gpumatch import engine, records

FILL = b"lorem ipsum dolor sit amet " * 50
TAIL = b' mid <z q="1&amp;2">t&#65;il</z> end'
SLID = {"comment": b"<!--x-->", "cdata": b"<![CDATA[a<b]]>", "numref": b"&#x0000003c;",
        "attrs": b"<a b=\"&lt;\" c='>'>", "pi": b"<?p ?>"}
LONG = b"x-- ]] > \" ' <q> &lt; " * 110   # > 2 KiB, no terminator of a comment, CDATA section or string


def cases():
    rnd = np.random.default_rng(13).integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    X = b"text/xml"
    c = [(f"{name}_at_{k}", X, FILL[:k] + s + TAIL) for name, s in SLID.items() for k in range(1000, 1041)]
    c += [("long_comment", X, b"a<!--" + LONG + b"-->b" + TAIL), ("long_cdata", X, b"a<![CDATA[" + LONG + b"]]>b" + TAIL),
          ("long_dq", X, b'a<t v="' + LONG.replace(b'"', b"'") + b'">b' + TAIL),
          ("long_sq", X, b"a<t v='" + LONG.replace(b"'", b'"') + b"'>b" + TAIL)]
    edge = [b"a<!-->b", b"a<?>b", b"a<![CDATA[x]]]>b", b"<![CDATA[a<![CDATA[b]]>c]]>d", b"a<![CDATA]]>b", b"a<!->b",
            b"a<!--->b", b"a<![CDATA[]]>b", b"<t a=\"it's\" b='say \"hi\"'>x", b"<t a=\"1>2\" b='3>4'>x", b"a<t <u>b",
            b"<!DOCTYPE d [ <!ENTITY e \"v\"> <!-- > --> ]>after", b"<!DOCTYPE d [ x ] [ > ]>after>", b"a<!-- open", b"a<![CDATA[open ]]",
            b"a<![CDATA[", b"a<![CDAT", b"a<?open ?", b"a<!DOCTYPE [ open", b"a<t open", b"a<t v=\"open &lt; ", b"a<t v='open", b"ab<",
            b"ab<!", b"ab<!-", b"]]>--> ?> plain > text"]
    c += [(f"edge_{i}", X, b) for i, b in enumerate(edge)]
    refs = [b"&#x7F;&#x80;&#x7FF;&#x800;&#xFFFF;&#x10000;&#x10FFFF;", b"&#127;&#128;&#2047;&#2048;&#65535;&#65536;&#1114111;",
            b"a&#0;b&#xD800;c&#xDFFF;d&#x110000;e&#1114112;f", b"&#123456789;&#x123456789;&#00000060;&#X0000003C;", b"tail &lt",
            b"tail &#x3c", b"&LT;&Lt;&lt &lt;&gt;&amp;&quot;&apos;", b"&amp;lt;&amp;#60;", b"<![CDATA[&lt;&#60;]]>&lt;",
            b"a<!-- &lt; -->b<?p &gt;?>c<t &amp; v='&apos;&#39;'>", b"&;&#;&#x;&#xg;&&lt;&#6&lt;", b"&#x3c;" * 300]
    c += [(f"refs_{i}", X, b) for i, b in enumerate(refs)]
    doc = b"<?xml version='1.0'?><r a=\"1\">t&lt;</r>"
    c += [("sel_text_xml", X, doc), ("sel_soap", b"application/soap+xml; charset=utf-8", doc[21:]),
          ("sel_svg_case", b"Image/SVG+XML", doc[21:]), ("sel_prolog", None, doc),
          ("sel_bom_ws_prolog", None, b"\xef\xbb\xbf \r\n\t" + doc), ("sel_upper_prolog", None, b"<?XML" + doc[5:]),
          ("sel_json", b"application/json", doc[21:]), ("sel_json_prolog", b"application/json", doc),
          ("sel_none", None, doc[21:]), ("sel_empty", X, b""), ("large_random", X, rnd)]
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
    return engine.Engine(0).xml_bodies(reqs, arena)


def test_reference_size_bound():
    taken = [ref.view(b, t) for _, t, b in CASES]
    assert all(v is None or len(v) <= len(b) for v, (_, _, b) in zip(taken, CASES))
    assert sum(v is None for v in taken) == 4   # <?XML, application/json, no header and no prolog, the empty body


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_xml_matches_reference(views, i):
    _, t, body = CASES[i]
    assert views[i] == ref.view(body, t)
