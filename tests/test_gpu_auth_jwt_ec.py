"""ES256 through gm_auth_jwt (gm_jwt.inc: k_jwt_ec; gm_p256.hpp) against jwt_ec_reference.py's restatement and against spelled-out codes."""

import json

import pytest

import jwt_ec_reference as ec
import jwt_reference as ref
import jwt_rsa_reference as rsa
from gpumatch import blob, records
from test_auth_jwt_rsa import CONF   # one server, one auth_jwt location /p, key file /k
from test_gpu_auth_jwt_rsa import MAL, NOW, OK, RS, SIG, eng, flip   # noqa: F401 (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu
ES, ALG, n = {"alg": "ES256", "typ": "JWT"}, ref.code(ref.DEFER, ref.ALG), ec.N
D, Q = ec.fixture_key()
PUB, MSG = ec.jwk(Q), ec.message(ES, {"sub": "nobody"})
E = ec.digest(MSG) % n


def check(eng, jwks, toks, want, pads=None):
    """The tokens (an X-Pad header of pads[i] bytes before Authorization) under the set jwks give `want`, as the restatement says."""
    eng.load(blob.make_blob(None, {"c": CONF}, jwks={"/k": json.dumps({"keys": jwks})}), 1)
    reqs, arena = records.from_dicts([{"uri": "/p", "host": "a.example.com", "port": 80, "headers":
                                       [("X-Pad", "p" * (pads[i] if pads else 0)), ("Authorization", "Bearer " + t)]} for i, t in enumerate(toks)])
    got = [hex(g) for g in eng.auth_jwt(reqs, arena, eng.match_host(reqs, arena)[0], NOW)]
    assert got == [hex(w) for w in want]
    assert got == [hex(ec.outcome(t, ec.jwk_keys(json.dumps({"keys": jwks})), NOW)) for t in toks]


def test_signed_and_forged(eng):
    good = [ec.sign(D, ES, {"sub": "user-%d" % i}) for i in range(64)]
    forged = [flip(t, pos) for pos in (0, 43, -1) for t in good]   # a bit of r, of s, and of the last character (s's bit 1)
    check(eng, [PUB], good + forged, [OK] * 64 + [SIG] * 192)


# (u1, u2) steering u1 G + u2 Q, Q = D G: after k joint 2-bit windows the accumulator is (u1 >> 256 - 2 k) G + (u2 >> 256 - 2 k) Q
A = next(a for a in range(1, 64) if -a * D % n < n // 4)
B = next(b for b in range(1, 4096) if D * (1 - 4 * b) * pow(4, -1, n) % n < 2 ** 250)
STEERED = {"infinity_at_the_end": (-5 * D % n, 5),
           "infinity_until_the_last_window": (1, 1),
           # all but the last window sum to -A D G + A Q: the addend is minus the accumulator there, then G is added
           "meets_its_negative": (4 * (-A * D % n) + 1, 4 * A),
           # U G + B Q = Q / 4 after the prefix, so two doublings give Q and the window (0, 1) adds Q: a doubling
           "addend_equals_accumulator": (16 * (D * (1 - 4 * B) * pow(4, -1, n) % n) + 1, (4 * B + 1) * 4)}


@pytest.mark.parametrize("case", sorted(STEERED))
def test_steered_scalars(eng, case):
    check(eng, [PUB], [ec.forged(ec.message(ES, {"sub": "m%d" % i}), *STEERED[case]) for i in range(3)], [SIG] * 3)


@pytest.mark.parametrize("pt,s,r", [(ec.mul(12345, ec.G), 0x7654321, None),
                                    (ec.lift_x(n + 3), 0x1234567, 3),   # x_R >= n: only (r + n) Z^2 = X accepts
                                    # u1 = 1 and the smallest u2 with R = G + u2 Q: at infinity until the last windows
                                    (next(p for p in (ec.lift_x(E * u % n) for u in range(1, 64)) if p), E, None)],
                         ids=["any_point", "r_plus_n", "u1_is_one"])
def test_keyless_tokens_verify_and_range(eng, pt, s, r):
    q, got = ec.keyless(MSG, pt, s)
    assert r in (None, got)
    cases = [(got, s, OK), (got, n - s, OK), (got, s ^ 2, SIG), (0, s, SIG), (got, 0, SIG), (n, s, SIG), (got, n, SIG),
             (got, min(s + n, 2 ** 256 - 1), SIG)]   # (high s verifies; s + n where 256 bits hold it)
    check(eng, [ec.jwk(q)], [ec.token(MSG, a, b) for a, b, _ in cases], [w for _, _, w in cases])


def test_hash_boundaries_and_alignment(eng):
    sizes = (55, 56, 63, 64, 65, 119)
    toks = [ec.sign(D, ES, {"s": "x" * ((size - 37) * 3 // 4 - 8)}) for size in sizes]
    assert tuple(t.rindex(".") for t in toks) == sizes
    check(eng, [PUB], toks + [toks[5]] * 16, [OK] * 22, pads=[0] * 6 + list(range(16)))


def test_mixed_set(eng):
    (na, da, pa), d2, okey, msg = rsa.fixture_key("rsa-2048", "r"), D * 7 % n, b"an oct key", ec.message(ES, {})
    late = ec.sign(d2, dict(ES, kid="b"), {"exp": NOW - 1})
    cases = [(ec.sign(D, dict(ES, kid="a"), {"sub": "u"}), OK),
             (ec.sign(d2, dict(ES, kid="zz"), {"sub": "u"}), OK),               # falls back to both EC keys: the second verifies
             (ec.sign(d2, dict(ES, kid="a"), {"sub": "u"}), SIG),               # the kid names the other key
             (msg + "." + "A" * 43, SIG), (msg + "." + "A" * 342, SIG), (msg + "." + "A" * 100, MAL),
             (ec.token(ec.message({"alg": "HS256"}, {}), 1, 1), MAL), (ec.token(ec.message({"alg": "RS256"}, {}), 1, 1), SIG),
             (ec.sign(D, dict(ES, alg="ES384"), {}), ALG),
             (late, ref.code(ref.DENY, ref.EXPIRED)), (flip(late, 7), SIG),
             (ref.sign(okey, {"alg": "HS256"}, {"sub": "u"}), OK), (ref.sign(b"other", {"alg": "HS256"}, {"sub": "u"}), SIG),
             (rsa.sign(na, da, dict(RS, kid="r"), {"sub": "u"}), OK), (rsa.sign(na, da, RS, {"sub": "u"}, add=1), SIG)]
    jwks = [{"kty": "oct", "k": ref.b64e(okey)}, pa, dict(PUB, kid="a"), ec.jwk(ec.mul(d2, ec.G), "b")]
    check(eng, jwks, [t for t, _ in cases], [w for _, w in cases])


def test_set_without_an_ec_key_answers_as_before(eng):
    tok = ec.sign(D, ES, {"sub": "u"})
    check(eng, [{"kty": "oct", "k": ref.b64e(b"k")}], [tok, tok.rsplit(".", 1)[0] + "." + "A" * 43], [MAL, ALG])
