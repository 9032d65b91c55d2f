"""RS256 through gm_auth_jwt (gm_jwt.inc: k_jwt_rsa, a lane per token) against the grammar restated in
Python (jwt_rsa_reference.py) and against spelled-out codes."""

import json

import pytest

import jwt_reference as ref
import jwt_rsa_reference as rsa
from gpumatch import blob, engine, records
from test_auth_jwt_rsa import CONF   # one server, one auth_jwt location /p, key file /k

pytestmark = pytest.mark.gpu
NOW = 1_700_000_000
RS = {"alg": "RS256", "typ": "JWT"}
OK, SIG, MAL = ref.code(ref.OK), ref.code(ref.DENY, ref.SIGNATURE), ref.code(ref.DENY, ref.MALFORMED)
B64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return engine.Engine(0)


def check(eng, jwks, toks, want, pads=None):
    """The tokens (an X-Pad header of pads[i] bytes before Authorization) under the set jwks give `want`, as the restatement says."""
    eng.load(blob.make_blob(None, {"c": CONF}, jwks={"/k": json.dumps({"keys": jwks})}), 1)
    items = [{"uri": "/p", "host": "a.example.com", "port": 80,
              "headers": ([("X-Pad", "p" * pads[i])] if pads else []) + [("Authorization", "Bearer " + t)]} for i, t in enumerate(toks)]
    reqs, arena = records.from_dicts(items)
    verdicts, _ = eng.match_host(reqs, arena)
    got = [hex(g) for g in eng.auth_jwt(reqs, arena, verdicts, NOW)]
    assert got == [hex(w) for w in want]
    keys = rsa.jwk_keys(json.dumps({"keys": jwks}))
    assert got == [hex(rsa.outcome(t, keys, NOW)) for t in toks]


def flip(tok, pos):
    """The token with the top bit of its signature's character `pos` flipped (a bit of the integer: no surplus bit)."""
    at = tok.rindex(".") + 1 + pos if pos >= 0 else len(tok) + pos
    return tok[:at] + B64[B64.index(tok[at]) ^ 32] + tok[at + 1:]


@pytest.mark.parametrize("name", ["rsa-2048", "rsa-3072", "rsa-4096", "rsa-2048-carry"])
def test_every_size_verifies_and_rejects(eng, name):
    n, d, pub = rsa.fixture_key(name)
    good = [rsa.sign(n, d, RS, {"sub": "user-%d" % i}) for i in range(64)]
    chars = len(good[0]) - good[0].rindex(".") - 1
    forged = [flip(t, pos) for pos in (-1, 0, chars // 2) for t in good]
    check(eng, [pub], good + forged, [OK] * 64 + [SIG] * 192)


def test_signature_not_below_the_modulus(eng):
    n, d, pub = rsa.fixture_key("rsa-2048")
    i = next(i for i in range(64) if ref.b64d(rsa.sign(n, d, RS, {"sub": i}).split(".")[2]) < (2 ** 2048 - n).to_bytes(256, "big"))
    check(eng, [pub], [rsa.sign(n, d, RS, {"sub": i}), rsa.sign(n, d, RS, {"sub": i}, add=n)], [OK, SIG])


def test_padding_boundaries_and_alignment(eng):
    n, d, pub = rsa.fixture_key("rsa-2048")
    sizes = (55, 56, 63, 64, 65, 119)
    toks = [rsa.sign(n, d, RS, {"s": "x" * ((size - 37) * 3 // 4 - 8)}) for size in sizes]
    assert tuple(t.rindex(".") for t in toks) == sizes
    check(eng, [pub], toks + [toks[5]] * 16, [OK] * 22, pads=[0] * 6 + list(range(16)))


def test_mixed_set(eng):
    (na, da, pa), (nb, db, pb), (n4, d4, _) = rsa.fixture_key("rsa-2048", "a"), rsa.fixture_key("rsa-3072", "b"), rsa.fixture_key("rsa-4096")
    okey, nbytes = b"an oct key", na.to_bytes(256, "big")
    late = rsa.sign(nb, db, dict(RS, kid="b"), {"exp": NOW - 1})
    msg = rsa.sign(na, da, RS, {}).rsplit(".", 1)[0]
    cases = [(ref.sign(okey, {"alg": "HS256"}, {"sub": "u"}), OK),
             (ref.sign(nbytes, {"alg": "HS256"}, {"sub": "u"}), SIG),            # an RSA key is never an HMAC key
             (rsa.sign(nb, db, dict(RS, kid="b"), {"sub": "u"}), OK),
             (rsa.sign(nb, db, dict(RS, kid="zz"), {"sub": "u"}), OK),          # falls back to both RSA keys: the second verifies
             (rsa.sign(na, da, RS, {"sub": "u"}), OK),
             (rsa.sign(n4, d4, RS, {"sub": "u"}), SIG),                          # no candidate of that size
             (msg + "." + "A" * 43, SIG), (msg + "." + "A" * 100, MAL),
             (rsa.sign(na, da, dict(RS, alg="RS384"), {}), ref.code(ref.DEFER, ref.ALG)),
             (late, ref.code(ref.DENY, ref.EXPIRED)), (flip(late, 7), SIG)]
    check(eng, [{"kty": "oct", "k": ref.b64e(okey)}, pa, pb], [t for t, _ in cases], [w for _, w in cases])


def test_oct_only_set_answers_as_before(eng):
    n, d, _ = rsa.fixture_key("rsa-2048")
    check(eng, [{"kty": "oct", "k": ref.b64e(b"k")}], [rsa.sign(n, d, RS, {"sub": "u"})], [MAL])
