#!/usr/bin/env python3
"""gm_auth_jwt throughput: requests that carry `Authorization: Bearer <HS256 token>` at one auth_jwt
location -- tokens of the reference fixtures' sizes (142 to 167 bytes of signing input) with a share
of 1 KiB-claims tokens mixed in -- verified by the lane-per-token HMAC kernels (gm_jwt.inc).  HIP
events around each call, warm-up first, the spread of the repeats reported; every outcome is compared
with tests/jwt_reference.py on the distinct tokens.  A second batch whose tokens say HS384 stops
after k_jwt_find (DEFER), so the find + order share of the call is known and the HMAC + claims
share follows by difference.  Python's single-thread hmac over the same tokens is timed as context.
Prints one JSON line.

`--alg RS256` is the RSA leg instead: one 2048-bit key (tests/golden/jwt/rsa-2048), 512 distinct tokens
cycled over the batch (a tenth of them forged), verified by k_jwt_rsa (a lane per token, Montgomery
products); outcomes are compared with tests/jwt_rsa_reference.py on the distinct tokens, the same
batch saying RS384 gives the find + order share, and the restatement's own pow() is timed as context.

`--alg ES256` is the ECDSA leg: the P-256 key of tests/golden/jwt/ec-p256, 512 distinct tokens (a tenth forged),
verified by k_jwt_ec (a lane per token; gm_p256.hpp); outcomes are compared with tests/jwt_ec_reference.py, the
same batch saying ES384 gives the find + order share.

    python scripts/bench_jwt.py [--n 1000000] [--reps 10] [--warmup 3] [--large 0.1]
    python scripts/bench_jwt.py --alg RS256 [--n 65536]
    python scripts/bench_jwt.py --alg ES256 [--n 65536]
"""

import argparse
import hashlib
import hmac
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-plus_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jwt_ec_reference as ec  # noqa: E402
import jwt_reference as ref  # noqa: E402
import jwt_rsa_reference as rsa  # noqa: E402
from gpumatch import blob, engine, records  # noqa: E402

KEY = b"fantasticjwt"
NOW = 1_700_000_000
CONF = ("upstream up { server 10.0.0.1:80; }\nserver { listen 80; server_name a.example.com;\n"
        "location / { auth_jwt_key_file /k; auth_jwt \"api\"; proxy_pass http://up; } }\n")
POOL = 8192   # distinct tokens, cycled over the batch


def tokens(alg, large, rng):
    out = []
    for i in range(POOL):
        claims = {"name": "Quotation System", "sub": "q%05x" % i, "iss": "My API Gateway"}   # (the fixtures' claims)
        if rng.random() < large:
            claims["pad"] = "x" * int(rng.integers(700, 800))
        if i % 3 == 0:
            claims["exp"] = NOW + 3600 if i % 9 else NOW - 1
        out.append(ref.sign(KEY, {"typ": "JWT", "alg": alg, "kid": "0001"}, claims))
    return out


def batch(n, toks):
    lines = [b"Authorization: Bearer " + t.encode() + b"\r\n" for t in toks]
    pick = np.arange(n) % len(lines)
    lens = np.array([len(x) for x in lines], dtype=np.uint64)[pick]
    base = np.concatenate([[0], np.cumsum((lens + 1 + 15) & ~np.uint64(15))]).astype(np.uint64)
    arena = np.zeros(int(base[-1]) + 16, np.uint8)
    for k in range(len(lines)):
        src = np.frombuffer(b"/" + lines[k], np.uint8)
        idx = base[:-1][pick == k]
        arena[(idx[:, None] + np.arange(len(src), dtype=np.uint64)[None, :]).astype(np.int64)] = src
    rq = np.zeros(n, dtype=records.REQ_DTYPE)
    rq["base"], rq["uri_len"], rq["hdr_len"], rq["port"] = base[:-1], 1, lens, 80
    return rq, arena


def timed(e, a, dev, toks, n):
    """(ms of each repeat, out_auth) of gm_auth_jwt over n requests that cycle through toks."""
    import torch
    rq, arena = batch(n, toks)
    ver = np.zeros(n, dtype=records.VERDICT_DTYPE)
    ver["gen"], ver["location_id"] = 1, 0
    d_ver = torch.from_numpy(ver.view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(n, dtype=torch.int32, device=dev)
    d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).to(dev)
    d_ar = torch.from_numpy(arena).to(dev)
    ms = []
    for k in range(a.warmup + a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        e.auth_jwt_ptr(d_rq.data_ptr(), d_ar.data_ptr(), len(arena), n, d_ver.data_ptr(), NOW, d_out.data_ptr(), 0)
        t1.record()
        e.sync(0)
        t1.synchronize()
        if k >= a.warmup:
            ms.append(t0.elapsed_time(t1))
    return ms, d_out.cpu().numpy().view(np.uint32)


def rsa_leg(a, e, dev):
    n = a.n if a.n != 1_000_000 else 65536
    nn, d, pub = rsa.fixture_key("rsa-2048", "0001")
    e.load(blob.make_blob(None, {"c": CONF}, jwks={"/k": json.dumps({"keys": [pub]})}), 1)
    res = {}
    for alg in ("RS256", "RS384"):
        toks = [rsa.sign(nn, d, {"typ": "JWT", "alg": alg, "kid": "0001"}, {"sub": "q%05x" % i, "iss": "My API Gateway"}, add=i % 10 == 9)
                for i in range(512)]
        ms, got = timed(e, a, dev, toks, n)
        t0 = time.perf_counter()
        want = np.array([rsa.outcome(t, [("0001", nn)], NOW) for t in toks], dtype=np.uint32)
        cpu_s = (time.perf_counter() - t0) / len(toks)
        assert np.array_equal(got, want[np.arange(n) % len(toks)]), alg
        res[alg] = (float(np.median(ms)), ms, cpu_s)
    med, ms, cpu_s = res["RS256"]
    rsa_ms = med - res["RS384"][0]
    print(json.dumps({"bench": "jwt_rs256", "n": n, "modulus_bits": 2048, "distinct_tokens": 512, "ms_median": round(med, 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "reps": a.reps, "tokens_per_s": round(n / med * 1e3),
                      "ms_find_order_median": round(res["RS384"][0], 4), "ms_hash_rsa_claims_by_difference": round(rsa_ms, 4),
                      "montgomery_products_per_s": round(18 * n / rsa_ms * 1e3), "multiply_adds_per_s": round(18 * 2 * 64 * 64 * n / rsa_ms * 1e3),
                      "python_restatement_tokens_per_s_one_thread": round(1 / cpu_s), "csrc_hash": engine.build_hash()}))


def ec_leg(a, e, dev):
    n = a.n if a.n != 1_000_000 else 65536
    d, q = ec.fixture_key()
    pub = ec.jwk(q, "0001")
    e.load(blob.make_blob(None, {"c": CONF}, jwks={"/k": json.dumps({"keys": [pub]})}), 1)
    res = {}
    for alg in ("ES256", "ES384"):
        toks = [ec.sign(d, {"typ": "JWT", "alg": alg, "kid": "0001"}, {"sub": "q%05x" % i, "iss": "My API Gateway"}) for i in range(512)]
        toks = [t[:-2] + ("A" if t[-2] != "A" else "B") + t[-1] if i % 10 == 9 else t for i, t in enumerate(toks)]   # (a tenth forged)
        ms, got = timed(e, a, dev, toks, n)
        t0 = time.perf_counter()
        want = np.array([ec.outcome(t, [("0001", q)], NOW) for t in toks], dtype=np.uint32)
        cpu_s = (time.perf_counter() - t0) / len(toks)
        assert np.array_equal(got, want[np.arange(n) % len(toks)]), alg
        res[alg] = (float(np.median(ms)), ms, cpu_s)
    med, ms, cpu_s = res["ES256"]
    ec_ms = med - res["ES384"][0]
    # per token: 128 x (2 doublings of 8 + a mixed addition of 11) + 5 field products, about 330 scalar products
    print(json.dumps({"bench": "jwt_es256", "n": n, "curve": "P-256", "distinct_tokens": 512, "ms_median": round(med, 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "reps": a.reps, "tokens_per_s": round(n / med * 1e3),
                      "ms_find_order_median": round(res["ES384"][0], 4), "ms_hash_ec_claims_by_difference": round(ec_ms, 4),
                      "field_products_per_s": round((128 * 27 + 5) * n / ec_ms * 1e3),
                      "multiply_adds_per_s": round(((128 * 27 + 5) * 64 + 330 * 128) * n / ec_ms * 1e3),
                      "python_restatement_tokens_per_s_one_thread": round(1 / cpu_s), "csrc_hash": engine.build_hash()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alg", choices=["HS256", "RS256", "ES256"], default="HS256")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--large", type=float, default=0.1, help="share of 1 KiB-claims tokens")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_jwt.py needs a GPU"
    dev = torch.device("cuda", 0)
    e = engine.Engine(0)
    if a.alg == "RS256":
        return rsa_leg(a, e, dev)
    if a.alg == "ES256":
        return ec_leg(a, e, dev)
    e.load(blob.make_blob(None, {"c": CONF}, jwks={"/k": json.dumps({"keys": [{"kty": "oct", "k": ref.b64e(KEY), "kid": "0001"}]})}), 1)
    assert e.stats()["n_auth_locations"] == 1
    ver = np.zeros(a.n, dtype=records.VERDICT_DTYPE)
    ver["gen"], ver["location_id"] = 1, 0   # PROXY verdicts at the location (what gm_match_batch gives them)
    d_ver = torch.from_numpy(ver.view(np.uint8).reshape(-1).copy()).to(dev)
    d_out = torch.zeros(a.n, dtype=torch.int32, device=dev)
    res = {}
    for alg in ("HS256", "HS384"):
        toks = tokens(alg, a.large, np.random.default_rng(20240))
        rq, arena = batch(a.n, toks)
        d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).to(dev)
        d_ar = torch.from_numpy(arena).to(dev)
        ms = []
        for k in range(a.warmup + a.reps):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            e.auth_jwt_ptr(d_rq.data_ptr(), d_ar.data_ptr(), len(arena), a.n, d_ver.data_ptr(), NOW, d_out.data_ptr(), 0)
            t1.record()
            e.sync(0)
            t1.synchronize()
            if k >= a.warmup:
                ms.append(t0.elapsed_time(t1))
        got = d_out.cpu().numpy().view(np.uint32)
        want = np.array([ref.outcome(t, [("0001", KEY)], NOW) for t in toks], dtype=np.uint32)
        assert np.array_equal(got, want[np.arange(a.n) % POOL]), alg
        res[alg] = (ms, toks)
    ms, toks = res["HS256"]
    sin = np.array([t.rindex(".") for t in toks])[np.arange(a.n) % POOL]
    compresses = int(((sin + 9 + 63) // 64 + 2).sum())
    msgs = [t[:t.rindex(".")].encode() for t in toks]
    t0 = time.perf_counter()
    for m in msgs:
        hmac.new(KEY, m, hashlib.sha256).digest()
    cpu_s = (time.perf_counter() - t0) / len(msgs)
    med, find = float(np.median(ms)), float(np.median(res["HS384"][0]))
    print(json.dumps({"bench": "jwt", "n": a.n, "mix": "%d%% fixture-size tokens (signing input %d..%d B), %d%% with 1 KiB of claims"
                      % (round(100 * (1 - a.large)), sin.min(), sin[sin < 512].max(), round(100 * a.large)),
                      "signing_bytes": int(sin.sum()), "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "reps": a.reps, "tokens_per_s": round(a.n / med * 1e3), "sha256_compresses_per_s": round(compresses / med * 1e3),
                      "ms_find_order_median": round(find, 4), "ms_hmac_claims_by_difference": round(med - find, 4),
                      "cpu_hmac_tokens_per_s_one_thread": round(1 / cpu_s), "csrc_hash": engine.build_hash()}))


if __name__ == "__main__":
    main()
