"""gm_auth_jwt's grammar for a key set that holds an RSA key (include/gpumatch.h), restated with hashlib and
pow over jwt_reference.  A key is (kid or None, key): an `oct` key's bytes, or the int n of an RSA key."""

import hashlib
import json
import os

import jwt_reference as ref

DIGEST_INFO = bytes.fromhex("3031300d060960864801650304020105000420")


def jwk_keys(jwk_text):
    return [(k.get("kid"), ref.b64d(k["k"]) if k["kty"] == "oct" else int.from_bytes(ref.b64d(k["n"]), "big"))
            for k in json.loads(jwk_text)["keys"]][:8]


def fixture_key(name, kid=None):
    """(n, d, the public JWK) of tests/golden/jwt/<name>.private.jwk.json."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jwt", name + ".private.jwk.json")) as f:
        k = json.load(f)["keys"][0]
    pub = {"kty": "RSA", "n": k["n"], "e": k["e"], **({"kid": kid} if kid else {})}
    return int.from_bytes(ref.b64d(k["n"]), "big"), int.from_bytes(ref.b64d(k["d"]), "big"), pub


def encoding(msg, k):
    return b"\x00\x01" + b"\xff" * (k - 54) + b"\x00" + DIGEST_INFO + hashlib.sha256(msg).digest()


def sign(n, d, header, payload, add=0):
    """An RS256 token under the private key (n, d); `add` is added to the signature's integer."""
    msg = ".".join(ref.b64e(json.dumps(x, separators=(",", ":")).encode()) for x in (header, payload))
    k = (n.bit_length() + 7) // 8
    return msg + "." + ref.b64e((pow(int.from_bytes(encoding(msg.encode(), k), "big"), d, n) + add).to_bytes(k, "big"))


def outcome(value, keys, now, leeway=0):
    rsa = [(i, k) for i, k in keys if isinstance(k, int)]
    octs = [(i, k) for i, k in keys if not isinstance(k, int)]
    seg = (value or "").split(" ")[0].split(".")
    if not rsa:
        return ref.outcome(value, keys, now, leeway)
    sig = seg[2] if len(seg) == 3 else ""
    long = len(sig) in (342, 512, 683)
    # the HS256 grammar over the oct keys (of the token with a 43-character segment 3, if it has a long one)
    base = ref.outcome(".".join(seg[:2] + ["A" * 43]) if long else value, octs, now, leeway)
    hdr = json.loads(ref.b64d(seg[0])) if base == ref.code(ref.DEFER, ref.ALG) else {}
    if hdr.get("alg") != "RS256":   # shape, header and alg as ever; HS256 with a long segment 3 is MALFORMED
        return ref.code(ref.DENY, ref.MALFORMED) if long and base == ref.code(ref.DENY, ref.SIGNATURE) else base
    if not long:
        return ref.code(ref.DENY, ref.SIGNATURE)
    kid = hdr.get("kid")
    cand = [k for i, k in rsa if isinstance(kid, str) and i == kid] or [k for _, k in rsa]
    msg = (seg[0] + "." + seg[1]).encode()
    for n in cand:
        k = (n.bit_length() + 7) // 8
        s = int.from_bytes(ref.b64d(sig)[:k], "big")
        if len(sig) == (4 * k + 2) // 3 and s < n and pow(s, 65537, n) == int.from_bytes(encoding(msg, k), "big"):
            # verified: the claims as of an HS256 token that verifies
            return ref.outcome(ref.sign(b"c", {"alg": "HS256"}, ref.b64d(seg[1])), [(None, b"c")], now, leeway)
    return ref.code(ref.DENY, ref.SIGNATURE)
