#!/usr/bin/env python3
"""gm_xml_bodies throughput: the C4 workload's request bodies, each wrapped as a SOAP-like XML
document -- a prolog, a comment, namespaced elements with quoted attributes, the body's text split
into elements with its markup characters as named / numeric references, one CDATA section in five
elements -- parsed by the wave-per-body kernel (gm_xml.inc).  HIP events around each call, warm-up
first, the spread of the repeats reported; the first distinct bodies' views are compared with
tests/xml_reference.py.  Prints one JSON line.

    python scripts/bench_xml.py [--n 200000] [--reps 10] [--warmup 3]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-plus_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import xml_reference as ref  # noqa: E402
from gpumatch import engine, records, workloads  # noqa: E402

HDR = b"Content-Type: text/xml; charset=utf-8\r\n"
ESC = {0x3C: b"&lt;", 0x3E: b"&gt;", 0x26: b"&amp;", 0x22: b"&quot;", 0x27: b"&#39;", 0x5D: b"&#x5d;"}


def wrap(raw):
    out = [b'<?xml version="1.0" encoding="UTF-8"?>\n<!-- generated request -->\n'
           b'<soap:Envelope xmlns:soap="http://schemas.xmlsoap.org/soap/envelope/" xmlns:m="urn:example:orders">\n'
           b' <soap:Header><m:Trace id="7f3a" hop=\'2\'/></soap:Header>\n <soap:Body>\n  <m:Submit>\n']
    for k, i in enumerate(range(0, len(raw), 48)):
        piece = raw[i:i + 48]
        if k % 5 == 4:
            out.append(b'   <m:Blob seq="%d"><![CDATA[' % k + piece.replace(b"]]>", b"]] >") + b"]]></m:Blob>\n")
        else:
            out.append(b'   <m:Field seq="%d" kind="text">' % k + b"".join(ESC.get(c, bytes([c])) for c in piece) + b"</m:Field>\n")
    out.append(b"  </m:Submit>\n </soap:Body>\n</soap:Envelope>\n")
    return b"".join(out)


def xml_batch(n, seed, repeat=1):
    """n records that hold a Content-Type header and a body: gen_c4's bodies (cycled, `repeat` of
    them joined), wrapped: a few KB each"""
    ss = workloads.c4_sigset(400, 100)
    reqs, arena = records.gen_c4(max(n // 4, 1000), ss, seed=seed)
    body = reqs["base"] + reqs["uri_len"] + reqs["args_len"] + reqs["hdr_len"]
    raws = [arena[int(b):int(b) + int(k)].tobytes() for b, k in zip(body, reqs["body_len"]) if k]
    docs = [HDR + wrap(b" ".join(raws[i:i + repeat])) for i in range(0, len(raws) - repeat + 1, repeat)]
    pick = np.arange(n) % len(docs)
    lens = np.array([len(docs[k]) for k in pick], dtype=np.uint64)
    base = np.concatenate([[0], np.cumsum((lens + 15) & ~np.uint64(15))]).astype(np.uint64)
    out = np.zeros(int(base[-1]) + 16, np.uint8)
    for k, b in zip(pick, base[:-1]):
        out[int(b):int(b) + len(docs[k])] = np.frombuffer(docs[k], np.uint8)
    rq = np.zeros(n, dtype=records.REQ_DTYPE)
    rq["base"], rq["hdr_len"], rq["body_len"] = base[:-1], len(HDR), lens - len(HDR)
    return rq, out, docs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_xml.py needs a GPU"
    rq, arena, docs = xml_batch(a.n, 20191)
    dev = torch.device("cuda", 0)
    e = engine.Engine(0)
    d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).to(dev)
    d_ar = torch.from_numpy(arena).to(dev)
    cap = len(arena) + 16
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(a.n, dtype=torch.int64, device=dev)
    d_len = torch.zeros(a.n, dtype=torch.int32, device=dev)
    ms = []
    for k in range(a.warmup + a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        e.xml_bodies_ptr(d_rq.data_ptr(), d_ar.data_ptr(), len(arena), a.n, d_out.data_ptr(), cap, d_off.data_ptr(),
                         d_len.data_ptr(), 0)
        t1.record()
        e.sync(0)
        t1.synchronize()
        if k >= a.warmup:
            ms.append(t0.elapsed_time(t1))
    ln, off, out = d_len.cpu().numpy().view(np.uint32), d_off.cpu().numpy(), d_out.cpu().numpy()
    assert (ln != engine.GM_NONE).all()   # every body taken
    for i in range(min(64, a.n, len(docs))):
        assert out[off[i]:off[i] + ln[i]].tobytes() == ref.view(docs[i][len(HDR):], b"text/xml"), i
    body_bytes, med = int(rq["body_len"].sum()), float(np.median(ms))
    print(json.dumps({"bench": "xml", "n": a.n, "body_bytes": body_bytes, "view_bytes": int(ln.astype(np.int64).sum()),
                      "mix": "SOAP-like: 48-byte fields, references for markup characters, 1 CDATA section in 5 fields, a comment",
                      "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "reps": a.reps, "gpu_GBps": round(body_bytes / med / 1e6, 3),
                      "bodies_per_s": round(a.n / med * 1e3), "csrc_hash": engine.build_hash()}))


if __name__ == "__main__":
    main()
