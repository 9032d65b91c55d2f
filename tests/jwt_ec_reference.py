"""gm_auth_jwt's grammar for a key set that holds an EC key (include/gpumatch.h), restated with Python ints over jwt_rsa_reference.
A key is (kid or None, key): an `oct` key's bytes, an RSA key's int n, or a P-256 key's affine point (x, y); None is the point at infinity."""

import functools
import hashlib
import json
import os

import jwt_reference as ref
import jwt_rsa_reference as rsa

P = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
B = 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b
G = (0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296,
     0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5)
SIGNATURE, DEFER_ALG = ref.code(ref.DENY, ref.SIGNATURE), ref.code(ref.DEFER, ref.ALG)


def add(a, b):   # every case: either at infinity, a = b (a doubling), a = -b
    if a is None or b is None:
        return a or b
    if a[0] == b[0] and (a[1] + b[1]) % P == 0:
        return None
    lam = (3 * a[0] * a[0] - 3) * pow(2 * a[1], -1, P) if a == b else (b[1] - a[1]) * pow(b[0] - a[0], -1, P)
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def mul(k, a):
    return functools.reduce(lambda r, bit: add(add(r, r), a if bit == "1" else None), bin(k % N)[2:], None)


def lift_x(x):   # the curve's point with this x (< p) and an even y; None if there is none
    y = pow((x ** 3 - 3 * x + B) % P, (P + 1) // 4, P)
    return (x, P - y if y & 1 else y) if (y * y - x ** 3 + 3 * x - B) % P == 0 else None


def digest(msg):
    return int.from_bytes(hashlib.sha256(msg.encode()).digest(), "big")


def verify(msg, r, s, q):
    pt = 1 <= r < N and 1 <= s < N and add(mul(digest(msg) * pow(s, -1, N), G), mul(r * pow(s, -1, N), q))
    return bool(pt) and pt[0] % N == r


def message(header, payload):
    return ".".join(ref.b64e(json.dumps(x, separators=(",", ":")).encode()) for x in (header, payload))


def token(msg, r, s):
    return msg + "." + ref.b64e(r.to_bytes(32, "big") + s.to_bytes(32, "big"))


def sign(d, header, payload, k=None):   # under the private key d, with the nonce k (default: derived from the message and d)
    msg = message(header, payload)
    k = k or digest(msg + "/%x" % d) % (N - 1) + 1
    r = mul(k, G)[0] % N
    return token(msg, r, pow(k, -1, N) * (digest(msg) + r * d) % N)


def forged(msg, u1, u2):   # a token whose verification computes u1 G + u2 Q for the chosen u1 != 0 and u2
    s = digest(msg) * pow(u1, -1, N) % N
    return token(msg, u2 * s % N, s)


def keyless(msg, pt, s):   # (Q, r): the public key under which (r = x_pt mod n, s) verifies msg; no private key is known
    r, w = pt[0] % N, pow(s, -1, N)
    minus = mul(digest(msg) * w, G)
    return mul(pow(r * w, -1, N), add(pt, (minus[0], P - minus[1]))), r


def jwk(q, kid=None):
    return {"kty": "EC", "crv": "P-256", **{c: ref.b64e(v.to_bytes(32, "big")) for c, v in zip("xy", q)}, **({"kid": kid} if kid else {})}


def fixture_key():   # (d, Q)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jwt", "ec-p256.private.jwk.json")) as f:
        d, x, y = (int.from_bytes(ref.b64d(v), "big") for v in map(json.load(f)["keys"][0].get, "dxy"))
    return d, (x, y)


def jwk_keys(jwk_text):
    return [(k.get("kid"), tuple(int.from_bytes(ref.b64d(k[c]), "big") for c in "xy")) if k["kty"] == "EC" else
            rsa.jwk_keys(json.dumps({"keys": [k]}))[0] for k in json.loads(jwk_text)["keys"]][:8]


def outcome(value, keys, now, leeway=0):
    ec = [(i, k) for i, k in keys if isinstance(k, tuple)]
    seg = (value or "").split(" ")[0].split(".")
    long = bool(ec) and len(seg) == 3 and len(seg[2]) == 86
    # shape, header and alg as ever over the other keys (86 characters pass the shape check as 43 do)
    base = rsa.outcome(".".join(seg[:2] + ["A" * 43]) if long else value, [k for k in keys if k not in ec], now, leeway)
    if not ec or base not in (SIGNATURE, DEFER_ALG):
        return base
    hdr = json.loads(ref.b64d(seg[0]))
    if hdr["alg"] != "ES256":   # HS256 with 86 characters is MALFORMED, RS256 with 86 stays SIGNATURE
        return ref.code(ref.DENY, ref.MALFORMED) if long and hdr["alg"] == "HS256" else base
    r, s = (int.from_bytes(ref.b64d(seg[2])[k:k + 32], "big") if long else 0 for k in (0, 32))   # (another admitted length: none)
    cand = [k for i, k in ec if isinstance(hdr.get("kid"), str) and i == hdr["kid"]] or [k for _, k in ec]
    if not any(verify(seg[0] + "." + seg[1], r, s, q) for q in cand):
        return SIGNATURE
    return ref.outcome(ref.sign(b"c", {"alg": "HS256"}, ref.b64d(seg[1])), [(None, b"c")], now, leeway)   # the claims, as of an HS256 token that verifies
