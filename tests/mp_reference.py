"""The multipart grammar of include/gpumatch.h restated in plain Python (bytes.find / partition,
base64.b64decode on the filtered alphabet, re.sub for the escapes): what gm_multipart_bodies is
compared with.  view(body, content_type) -> (M, flags) or None."""

import base64
import re

PARAM = re.compile(rb'(?is)(?<=[; \t])(?:(filename\*)=([^; \t\r\n]*)|'
                   rb'(filename|name)=(?:"((?:\\.|[^"\\]|\\\Z)*)"?|([^; \t\r\n]*)))')


def boundary(ct):
    if ct is None or ct[:10].lower() != b"multipart/" or b";" not in ct:
        return None
    m = re.search(rb'(?i)(?<=[; \t])boundary=(?:"([^"]*)|([^; \t]*))', ct[ct.find(b";"):])
    b = None if not m else m[1] if m[1] is not None else m[2]
    return b if b is not None and 1 <= len(b) <= 70 else None


def delimiters(body, B):
    return list(re.finditer(rb"(?:\A|(?<=\n))" + re.escape(b"--" + B) + rb"(?:(--)|[ \t\r]*\n)", body))


def part_view(part):
    hdr, content, q = {}, None, 0
    while q < len(part):
        e = part.find(b"\n", q)
        line = part[q:] if e < 0 else part[q:e]
        if e >= 0 and line in (b"", b"\r"):
            content = part[e + 1:]
            break
        name, colon, val = line[:-1].partition(b":") if line.endswith(b"\r") else line.partition(b":")
        if colon:
            hdr.setdefault(name.lower(), val)
        q = len(part) if e < 0 else e + 1
    par = {}
    for m in PARAM.finditer(hdr.get(b"content-disposition", b"")):
        if m[1]:
            t = m[2].split(b"'", 2)
            v = re.sub(rb"%([0-9A-Fa-f]{2})", lambda x: bytes([int(x[1], 16)]), t[2]) if len(t) == 3 else None
            par.setdefault(b"filename*", v)
        else:
            par.setdefault(m[3].lower(), re.sub(rb"(?s)\\(.)", rb"\1", m[4]) if m[4] is not None else m[5])
    enc = hdr.get(b"content-transfer-encoding", b"").strip(b" \t").lower()
    if content is not None and enc == b"base64":
        f = re.sub(rb"[^A-Za-z0-9+/]", b"", content)
        content = base64.b64decode(f[:len(f) // 4 * 4])
    elif content is not None and enc == b"quoted-printable":
        content = re.sub(rb"=([0-9A-Fa-f]{2})|=\r?\n", lambda x: bytes([int(x[1], 16)]) if x[1] else b"", content)
    pieces = [par.get(b"name"), par.get(b"filename"), par.get(b"filename*"), content]
    return b"".join(p + b"\n" for p in pieces if p is not None), b"json" in hdr.get(b"content-type", b"").lower()


def view(body, ct):
    B = boundary(ct)
    ms = delimiters(body, B) if B is not None and body else []
    if not ms:
        return None
    out, json, n = b"", False, 0
    for k, m in enumerate(ms):
        if m[1] or n == 64:
            break
        part = body[m.end():ms[k + 1].start() if k + 1 < len(ms) else len(body)]
        part = part[:-1] if part.endswith(b"\n") else part
        part = part[:-1] if part.endswith(b"\r") else part
        o, j = part_view(part)
        out, json, n = out + o, json or j, n + 1
    return out, n << 8 | int(json)
