"""gm_auth_jwt (gm_jwt.inc: HMAC-SHA-256 on the GPU, a lane per token) against the grammar restated in
Python (jwt_reference.py): the reference project's own tokens and key sets, the SHA-256 padding
boundaries, every text alignment, and one shuffled batch of mixed lengths, keys, sources and outcomes."""

import json
import os

import numpy as np
import pytest

import jwt_reference as ref
from gpumatch import blob, engine, records

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jwt")
TOKENS = ["jwt-secrets-token.jwt", "jwt-auth-master-token.jwt", "jwt-auth-minion-token.jwt"]
SETS = ["jwt-secret", "jwt-secret-updated", "jwt-master-secret", "jwt-minion-secret"]
HS = {"alg": "HS256", "typ": "JWT"}
NOW = 1_700_000_000
EXP = 1577836800   # the minion token's "exp", a string


def gold(name):
    with open(os.path.join(GOLD, name)) as f:
        return f.read().strip()


def conf(locs):
    """One server; locs: (path, key file or None, directives after auth_jwt_key_file)."""
    body = "".join("location %s { %s proxy_pass http://up; }\n" % (p, "auth_jwt_key_file %s; %s" % (f, d) if f else d)
                   for p, f, d in locs)
    return "upstream up { server 10.0.0.1:80; }\nserver { listen 80; server_name a.example.com;\n%s}\n" % body


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU test without a GPU"
    return engine.Engine(0)


def run(eng, items, now):
    """out_auth of the requests (dicts for records.from_dicts) under the loaded generation."""
    reqs, arena = records.from_dicts([dict(host="a.example.com", port=80, **it) for it in items])
    verdicts, _ = eng.match_host(reqs, arena)
    return verdicts, eng.auth_jwt(reqs, arena, verdicts, now)


def bearer(tok, pad=None):
    return {"uri": "/p", "headers": ([("X-Pad", "p" * pad)] if pad is not None else []) + [("Authorization", "Bearer " + tok)]}


def sized(key, n, hdr=HS, claims={}):
    """A token whose signing input is n bytes long (a byte shorter where base64 has no such length,
    longer where the claims alone are): the value of claim "s" pads the payload."""
    p64 = n - len(ref.b64e(json.dumps(hdr, separators=(",", ":")).encode())) - 1
    base = len(json.dumps(dict(claims, s=""), separators=(",", ":")))
    return ref.sign(key, hdr, dict(claims, s="x" * max(0, (p64 - (p64 % 4 == 1)) * 3 // 4 - base)))


@pytest.mark.parametrize("leeway", [0, 60])
@pytest.mark.parametrize("jwk", SETS)
def test_reference_fixtures(eng, jwk, leeway):
    keys = ref.jwk_keys(gold(jwk + ".jwk.json"))
    eng.load(blob.make_blob(None, {"c": conf([("/p", "/k", 'auth_jwt "r"; auth_jwt_leeway %ds;' % leeway)])},
                            jwks={"/k": gold(jwk + ".jwk.json")}), 1)
    toks = [gold(t) for t in TOKENS]
    for now in (EXP + leeway - 1, EXP + leeway):
        _, got = run(eng, [bearer(t) for t in toks], now)
        assert list(got) == [ref.outcome(t, keys, now, leeway) for t in toks]
        good = keys[0][1] == b"fantasticjwt"   # the master and secrets tokens' key; the minion token's is awesomejwt
        late = ref.code(ref.DENY, ref.EXPIRED) if now == EXP + leeway else ref.code(ref.OK)
        bad = ref.code(ref.DENY, ref.SIGNATURE)
        assert list(got) == ([ref.code(ref.OK)] * 2 + [bad] if good else [bad] * 2 + [late])


def test_padding_boundaries_and_alignment(eng):
    key = b"boundary key"
    eng.load(blob.make_blob(None, {"c": conf([("/p", "/k", 'auth_jwt "r";')])},
                            jwks={"/k": json.dumps({"keys": [{"kty": "oct", "k": ref.b64e(key)}]})}), 1)
    sizes = (55, 56, 63, 64, 65, 119, 120, 128)
    toks = [sized(key, n) for n in sizes]
    assert tuple(t.rindex(".") for t in toks) == sizes
    forged = [t[:-43] + ("B" if t[-43] == "A" else "A") + t[-42:] for t in toks]
    # and one token at every text offset mod 16: the X-Pad header before it grows a byte at a time
    items = [bearer(t) for t in toks + forged] + [bearer(toks[5], pad) for pad in range(16)]
    _, got = run(eng, items, NOW)
    assert list(got) == [ref.code(ref.OK)] * 8 + [ref.code(ref.DENY, ref.SIGNATURE)] * 8 + [ref.code(ref.OK)] * 16
    assert list(got) == [ref.outcome(ref.source_value(it, None), [(None, key)], NOW) for it in items]


@pytest.mark.parametrize("n", [64, 65, 70])
def test_token_ends_the_arena(eng, n):
    """The token is the payload's, and the arena's, last bytes: $arg_t of a record with nothing after
    $args, the arena ending with it on a 16-byte boundary."""
    key = b"k"
    eng.load(blob.make_blob(None, {"c": conf([("/p", "/k", 'auth_jwt "r" token=$arg_t;')])},
                            jwks={"/k": json.dumps({"keys": [{"kty": "oct", "k": ref.b64e(key)}]})}), 7)
    args = b"t=" + sized(key, n).encode()
    uri = b"/p" + b"u" * (-(2 + len(args)) % 16)
    reqs = np.zeros(1, dtype=records.REQ_DTYPE)
    reqs["uri_len"], reqs["args_len"], reqs["port"] = len(uri), len(args), 80
    arena = np.frombuffer(uri + args, dtype=np.uint8)
    assert len(arena) % 16 == 0
    verdicts = np.zeros(1, dtype=records.VERDICT_DTYPE)
    verdicts["gen"], verdicts["location_id"], verdicts["action"] = 7, 0, 0   # a PROXY verdict at /p
    assert list(eng.auth_jwt(reqs, arena, verdicts, NOW)) == [ref.code(ref.OK)]


def test_shuffled_batch(eng):
    rng = np.random.default_rng(14)
    k1, k64, k65, ka, kb = b"1", bytes(range(64)), bytes(range(65)), b"first key", b"second key"
    sets = {"/k1": [(None, k1)], "/k64": [("a", k64)], "/k65": [(None, k65)], "/k2": [("k1", ka), ("k2", kb)]}
    jwks = {f: json.dumps({"keys": [dict(kty="oct", k=ref.b64e(k), **({"kid": i} if i else {})) for i, k in ks]})
            for f, ks in sets.items()}
    # path -> (key file, token source, leeway)
    locs = {"/b": ("/k1", None, 0), "/c": ("/k64", ("cookie", "auth"), 0), "/a": ("/k65", ("arg", "jwt"), 30),
            "/h": ("/k2", ("http", "x_token"), 0), "/open": (None, None, 0), "/ret": ("/k1", None, 0)}
    directive = {None: "", "cookie": " token=$cookie_auth", "arg": " token=$arg_jwt", "http": " token=$http_x_token"}
    eng.load(blob.make_blob(None, {"c": conf(
        [(p, f, ('auth_jwt "r"%s; auth_jwt_leeway %ds;' % (directive[s and s[0]], lw) if f else "auth_jwt off;") +
          (" return 204;" if p == "/ret" else "")) for p, (f, s, lw) in locs.items()])}, jwks=jwks), 3)

    def req(path, tok):
        src = locs[path][1]
        if src is None:
            return {"uri": path, "headers": [("Accept", "*/*"), ("Authorization", "bEARER  " + tok)]}
        if src[0] == "cookie":
            return {"uri": path, "headers": [("Cookie", "lang=en; auth=%s; theme=dark" % tok)]}
        if src[0] == "arg":
            return {"uri": path, "args": "page=2&jwt=%s&x=1" % tok}
        return {"uri": path, "headers": [("X-Token", tok)]}

    items, blocks = [], set()
    for i in range(470):   # 1 .. 40 SHA blocks, every location, good and forged signatures, claims in and out of date
        path = ["/b", "/c", "/a", "/h"][i % 4]
        key = {"/b": k1, "/c": k64, "/a": k65, "/h": kb}[path]
        # /h: the second key by its kid, by fallback from a kid no key has, and with no kid at all
        hdr = dict(HS, **({"kid": ["k2", "zz"][i % 8 // 4]} if path == "/h" and i % 16 != 15 else {}))
        claims = [{}, {"exp": NOW + 5}, {"exp": str(NOW - 40)}, {"nbf": NOW + 31}, {"nbf": NOW + 30}][i % 5]
        tok = sized(key if i % 7 else b"another key", 64 * (1 + i % 40) - 9, hdr, claims)
        blocks.add((tok.rindex(".") + 9 + 63) // 64)
        items.append(req(path, tok))
    assert blocks >= set(range(1, 41))
    good = ref.sign(k1, HS, {"sub": "u"})
    items += [{"uri": "/b"}, {"uri": "/b", "headers": [("Authorization", "Basic dTpw")]},                  # no token
              req("/b", good + "="), req("/b", good[:-1]), req("/b", ref.sign(k1, HS, b"[1]")),             # malformed
              req("/b", ref.sign(k1, HS, {"exp": 1.5})), req("/b", ref.sign(k1, {"typ": "JWT"}, {})),
              req("/b", ref.sign(k1, {"alg": "none"}, {})), req("/b", ref.sign(k1, {"alg": "HS384"}, {})),  # none; defer
              req("/b", ref.sign(k1, {"alg": "RS256", "kid": "a"}, {})),
              req("/open", good), {"uri": "/ret", "headers": [("Authorization", "Bearer " + good)]},        # no auth; a return
              {"uri": "/nowhere"}, req("/b", good)]
    items = [items[i] for i in rng.permutation(len(items))]
    items += [{"uri": "/open"}] * (512 - len(items))
    stale = next(i for i, it in enumerate(items) if it == req("/b", good))
    reqs, arena = records.from_dicts([dict(host="a.example.com", port=80, **it) for it in items])
    verdicts, _ = eng.match_host(reqs, arena)
    verdicts["gen"][stale] = 2   # a verdict of the generation before
    want = []
    for i, it in enumerate(items):
        f, src, lw = locs.get(it["uri"], (None, None, 0))
        want.append(ref.code(ref.DEFER, ref.STALE) if i == stale else ref.code(ref.NONE) if f is None or it["uri"] == "/ret"
                    else ref.outcome(ref.source_value(it, src), sets[f], NOW, lw))
    hashed = [w for w in want if w == ref.code(ref.OK) or (w & 0xFF == ref.DENY and w >> 8 in ref.HASHED)]
    assert len(hashed) >= 400 and {w >> 8 for w in want} == set(range(9))   # every reason of the table is there
    got = eng.auth_jwt(reqs, arena, verdicts, NOW)
    assert [hex(g) for g in got] == [hex(w) for w in want]
