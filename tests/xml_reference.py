"""The xml grammar of include/gpumatch.h restated as a plain serial Python scanner (bytes.find, one
re.sub for the references): what gm_xml_bodies is compared with.
view(body, content_type) -> X or None."""

import re

REF = re.compile(rb"&(?:(lt|gt|amp|quot|apos)|#([0-9]{1,8})|#[xX]([0-9A-Fa-f]{1,8}));")
NAMED = {b"lt": b"<", b"gt": b">", b"amp": b"&", b"quot": b'"', b"apos": b"'"}


def _ref(m):
    if m[1]:
        return NAMED[m[1]]
    v = int(m[2]) if m[2] else int(m[3], 16)
    return chr(v).encode("utf-8") if 1 <= v <= 0x10FFFF and not 0xD800 <= v <= 0xDFFF else m[0]


def chardata(b):
    return REF.sub(_ref, b)


def selected(body, content_type):
    if not body:
        return False
    if content_type is not None and b"xml" in content_type.lower():
        return True
    b = body[3:] if body[:3] == b"\xef\xbb\xbf" else body
    return b.lstrip(b" \t\r\n").startswith(b"<?xml")


def _until(body, pat, start):
    """(end of the construct, where its content ends): after the first pat at >= start, else the body's end"""
    q = body.find(pat, start)
    return (len(body), len(body)) if q < 0 else (q + len(pat), q)


def view(body, content_type):
    if not selected(body, content_type):
        return None
    out, p, n = [], 0, len(body)
    while p < n:
        lt = body.find(b"<", p)
        if lt < 0:
            lt = n
        out.append(chardata(body[p:lt]))
        if lt == n:
            break
        p = lt
        if body.startswith(b"<!--", p):
            p, _ = _until(body, b"-->", p + 2)
        elif body.startswith(b"<![CDATA[", p):
            p, e = _until(body, b"]]>", p + 9)
            out.append(body[lt + 9:e])
        elif body.startswith(b"<?", p):
            p, _ = _until(body, b"?>", p + 1)
        elif body.startswith(b"<!", p):
            subset, p = False, p + 2
            while p < n:
                c = body[p]
                p += 1
                if c == 0x5B:
                    subset = True
                elif c == 0x5D:
                    subset = False
                elif c == 0x3E and not subset:
                    break
        else:
            out.append(b"\n")
            p += 1
            while p < n:
                c = body[p:p + 1]
                p += 1
                if c == b">":
                    break
                if c in (b'"', b"'"):
                    q = body.find(c, p)
                    if q < 0:
                        out.append(chardata(body[p:]))
                        p = n
                    else:
                        out.append(chardata(body[p:q]) + b"\n")
                        p = q + 1
    return b"".join(out)
