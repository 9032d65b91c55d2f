"""P-256 public keys in a JWK set (compile-only context): which sets compile, which are rejected like a bad RSA key."""

import pytest

import jwt_ec_reference as ec
from gpumatch import engine
from test_auth_jwt_rsa import compiled, rsa_jwk

PUB = dict(ec.jwk(ec.fixture_key()[1], "k1"), d="c2tpcHBlZA", use="sig", alg="ES256")   # (further members are skipped)


def test_mixed_set_compiles():   # (Q = G: the table's entry G + Q is a doubling)
    assert compiled([{"kty": "oct", "k": "c2VjcmV0"}, rsa_jwk(), PUB, ec.jwk(ec.G)]) == (0, [], ("r", engine.GM_NONE))


@pytest.mark.parametrize("change", [{"crv": "P-384"}, {"x": PUB["x"][4:]}, {"y": ec.jwk((0, ec.fixture_key()[1][1] ^ 1))["y"]}, {"x": ec.jwk((ec.P, 0))["x"]},
                                    ec.jwk((ec.G[0], ec.P - ec.G[1]))],   # (Q = -G: the table's entry G + Q is the point at infinity)
                         ids=["p384", "x_31_bytes", "off_curve", "x_is_p", "q_is_minus_g"])
def test_ec_key_the_engine_does_not_take(change):
    assert compiled([{"kty": "oct", "k": "c2VjcmV0"}, dict(PUB, **change)]) == (1, ["location /p: auth_jwt r"], None)
