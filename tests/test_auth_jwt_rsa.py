"""RSA public keys in a JWK set (compile-only context): which sets compile, which stay rejected as before."""

import json

import pytest

import jwt_reference as ref
import jwt_rsa_reference as rsa
from gpumatch import blob, engine

CONF = ("upstream up { server 10.0.0.1:80; }\nserver { listen 80; server_name a.example.com;\n"
        "location /p { auth_jwt_key_file /k; auth_jwt \"r\"; proxy_pass http://up; } }\n")


def rsa_jwk(name="rsa-2048"):
    return dict(rsa.fixture_key(name)[2], d="c2tpcHBlZA", p="AQAB")   # (private members are skipped)


def compiled(keys):
    e = engine.Engine(compile_only=True)
    e.load(blob.make_blob(None, {"c": CONF}, jwks={"/k": json.dumps({"keys": keys})}), 1)
    return e.stats()["n_rejected_other"], e.rejects(), e.auth_info(0)


def test_mixed_set_compiles():
    assert compiled([{"kty": "oct", "k": "c2VjcmV0"}, rsa_jwk(), rsa_jwk("rsa-4096")]) == (0, [], ("r", engine.GM_NONE))


def big(v):
    return ref.b64e(v.to_bytes((v.bit_length() + 7) // 8, "big"))


N = int.from_bytes(ref.b64d(rsa_jwk()["n"]), "big")


@pytest.mark.parametrize("change", [{"e": "Aw"}, {"n": big(N >> 1024 | 1)}, {"n": big(N << 1 | 1)}, {"n": big(N - 1)}],
                         ids=["e_3", "1024_bits", "2049_bits", "even"])
def test_rsa_key_the_engine_does_not_take(change):
    n, rejects, info = compiled([{"kty": "oct", "k": "c2VjcmV0"}, dict(rsa_jwk(), **change)])
    assert (n, rejects, info) == (1, ["location /p: auth_jwt r"], None)
