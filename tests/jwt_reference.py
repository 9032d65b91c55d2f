"""gm_auth_jwt's grammar (include/gpumatch.h, gm_jwt.inc) restated in plain Python: hmac, hashlib,
base64, json.  `outcome` is what out_auth holds for one request whose location has an auth record.
(It assumes what the tests keep to: well-formed UTF-8 JSON and member names without escapes.)"""

import base64
import hashlib
import hmac
import json
import re

NONE, OK, DENY, DEFER = 0, 1, 2, 3
NO_TOKEN, MALFORMED, ALG_NONE, SIGNATURE, EXPIRED, NOT_YET, ALG, STALE = range(1, 9)
HASHED = (SIGNATURE, EXPIRED, NOT_YET)   # DENY reasons of a token that reached the HMAC kernel


def code(c, reason=0):
    return c | reason << 8


def b64d(s):
    return base64.urlsafe_b64decode(s + "=" * (-len(s) % 4))


def b64e(b):
    return base64.urlsafe_b64encode(b).rstrip(b"=").decode()


def jwk_keys(jwk_text):
    """[(kid or None, key bytes)] of a JWK set, the first eight."""
    return [(k.get("kid"), b64d(k["k"])) for k in json.loads(jwk_text)["keys"]][:8]


def sign(key, header, payload):
    """A token: header (dict) and payload (dict, or the payload's bytes as they are), HS256 under key."""
    body = payload if isinstance(payload, bytes) else json.dumps(payload, separators=(",", ":")).encode()
    msg = b64e(json.dumps(header, separators=(",", ":")).encode()) + "." + b64e(body)
    return msg + "." + b64e(hmac.new(key, msg.encode(), hashlib.sha256).digest())


def source_value(req, src):
    """The token source's value: src None (Authorization: Bearer) or ("cookie" | "arg" | "http", name)."""
    hdrs = [(k.lower().replace("-", "_"), v) for k, v in req.get("headers", [])]
    if src is None:
        v = next((v for k, v in hdrs if k == "authorization"), None)
        return v[6:].lstrip(" ") if v is not None and re.match(r"(?i)bearer ", v) else None
    kind, name = src
    if kind == "http":
        return next((v for k, v in hdrs if k == name), None)
    parts = req.get("args", "").split("&") if kind == "arg" else \
        [c.strip(" ") for k, v in hdrs if k == "cookie" for c in v.split(";")]
    return next((p[len(name) + 1:] for p in parts if p.lower().startswith(name + "=")), None)


def time_claim(v):
    if isinstance(v, int) and not isinstance(v, bool) and abs(v) < 10 ** 18:
        return v
    if isinstance(v, str) and re.fullmatch(r"[0-9]{1,18}", v):
        return int(v)
    raise ValueError(v)


def outcome(value, keys, now, leeway=0):
    tok = (value or "").split(" ")[0]
    if not tok:
        return code(DENY, NO_TOKEN)
    seg = tok.split(".")
    if len(seg) != 3 or not all(re.fullmatch(r"[A-Za-z0-9_-]+", s) for s in seg) or len(seg[2]) != 43 or \
            any(len(s) % 4 == 1 for s in seg[:2]):
        return code(DENY, MALFORMED)
    try:
        hdr = json.loads(b64d(seg[0]))
        alg = hdr["alg"] if isinstance(hdr, dict) else None
    except (ValueError, KeyError):
        alg = None
    if not isinstance(alg, str):
        return code(DENY, MALFORMED)
    if alg != "HS256":
        return code(DENY, ALG_NONE) if alg == "none" else code(DEFER, ALG)
    kid = hdr.get("kid")
    cand = [k for i, k in keys if isinstance(kid, str) and i == kid] or [k for _, k in keys]
    msg = (seg[0] + "." + seg[1]).encode()
    if not any(hmac.compare_digest(hmac.new(k, msg, hashlib.sha256).digest(), b64d(seg[2])) for k in cand):
        return code(DENY, SIGNATURE)
    try:
        pl = json.loads(b64d(seg[1]))
        exp, nbf = (time_claim(pl[c]) if c in pl else None for c in ("exp", "nbf"))
    except (ValueError, TypeError):
        return code(DENY, MALFORMED)
    if not isinstance(pl, dict):
        return code(DENY, MALFORMED)
    if exp is not None and not exp + leeway > now:
        return code(DENY, EXPIRED)
    if nbf is not None and not nbf <= now + leeway:
        return code(DENY, NOT_YET)
    return code(OK)
