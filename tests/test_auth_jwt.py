"""auth_jwt in the generation compiler (compile-only context): a Plus config's auth_jwt is accepted
only with a GM_ENTRY_JWK entry for its key file, and then every location gets the auth record nginx's
inheritance gives it, read back through gm_auth_info."""

import os

import pytest

from gpumatch import blob, engine

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jwt")
SRV, OWN = "/etc/nginx/secrets/default-srv-jwk", "/etc/nginx/secrets/default-own-jwk"
LOGIN = "location @login_url_default-ing { internal; return 302 https://login.example.com; }"
# locations in config order: 0 @login_url..., 1 /api, 2 /open, 3 /own, 4 /plain, 5 /loc
CONF = """
upstream up { server 10.0.0.1:80; }
server { listen 80; server_name a.example.com;
  auth_jwt_key_file %s;
  auth_jwt "srv realm";
  error_page 401 @login_url_default-ing;
  %%s
  location /api { proxy_pass http://up; }
  location /open { auth_jwt off; proxy_pass http://up; }
  location /own { auth_jwt_key_file %s; auth_jwt "own realm" token=$cookie_auth; auth_jwt_leeway 1m30s; proxy_pass http://up; }
}
server { listen 80; server_name b.example.com;
  location /plain { proxy_pass http://up; }
  location /loc { auth_jwt_key_file %s; auth_jwt "loc realm" token=$arg_jwt; proxy_pass http://up; }
}
""" % (SRV, OWN, OWN)
# what the compiler said of this config before it knew GM_ENTRY_JWK (and says without the entry)
REJECTS = ["server: auth_jwt srv realm", "server: error_page 401 @login_url_default-ing",
           "location @login_url_default-ing: internal", "location /own: auth_jwt own realm token=$cookie_auth",
           "location /loc: auth_jwt loc realm token=$arg_jwt"]
NONE = engine.GM_NONE


def jwk(name):
    with open(os.path.join(GOLD, name)) as f:
        return f.read()


def compiled(jwks, login=LOGIN):
    e = engine.Engine(compile_only=True)
    e.load(blob.make_blob(None, {"plus": CONF % login}, jwks=jwks), 1)
    s = e.stats()
    return s["n_rejected_other"], e.rejects(), s["n_auth_locations"], [e.auth_info(i) for i in range(s["n_locations"])]


RSA = '{"keys":[{"kty":"oct","k":"c2VjcmV0"},{"kty":"RSA","n":"sXchDaQebHnPiGvyDOAT4saGEUetSyo9MKLOoWFsueri","e":"AQAB"}]}'


@pytest.mark.parametrize("jwks", [None, {"/etc/nginx/secrets/other-jwk": jwk("jwt-secret.jwk.json")},
                                  {SRV: RSA, OWN: RSA}, {SRV: '{"keys":[{"kty":"oct","k":"c2Vj', OWN: '{"keys":[]}'}],
                         ids=["no_entry", "other_file", "rsa_key", "unparsable"])
def test_rejected_exactly_as_before(jwks):
    n, rejects, n_auth, info = compiled(jwks)
    assert (n, rejects) == (len(REJECTS), REJECTS) and any("auth_jwt" in r for r in rejects)
    assert n_auth == 0 and info == [None] * 6


def test_records_follow_nginx_inheritance():
    n, rejects, n_auth, info = compiled({SRV: jwk("jwt-secret.jwk.json"), OWN: jwk("jwt-minion-secret.jwk.json")})
    assert (n, rejects) == (0, [])
    assert n_auth == 3
    # /api inherits the server's; `auth_jwt off` clears it; /own replaces realm and key file and keeps the
    # inherited login location; the second server has no server-level auth and no login url
    assert info == [None, ("srv realm", 0), None, ("own realm", 0), None, ("loc realm", NONE)]


def test_only_the_server_key_file():
    n, rejects, n_auth, info = compiled({SRV: jwk("jwt-secret.jwk.json")})
    assert rejects == REJECTS[3:] and n == 2
    assert n_auth == 1 and info == [None, ("srv realm", 0), None, None, None, None]


@pytest.mark.parametrize("login", ["", LOGIN.replace("internal;", "internal; add_header X y;"), LOGIN.replace("302", "301")],
                         ids=["missing", "extra_directive", "not_302"])
def test_login_location_of_another_shape_keeps_the_server_rejected(login):
    n, rejects, n_auth, info = compiled({SRV: jwk("jwt-secret.jwk.json"), OWN: jwk("jwt-secret.jwk.json")}, login)
    assert "server: auth_jwt srv realm" in rejects and "server: error_page 401 @login_url_default-ing" in rejects
    assert info[:-1] == [None] * (len(info) - 1) and info[-1] == ("loc realm", NONE)
