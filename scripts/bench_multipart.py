#!/usr/bin/env python3
"""gm_multipart_bodies throughput: the C4 workload's request bodies, each wrapped as a three-part
multipart/form-data body -- the first third verbatim, the second third base64 at 76 columns, the rest
as the string of a JSON part -- parsed by the wave-per-body kernel (gm_multipart.inc).  HIP events
around each call, warm-up first, the spread of the repeats reported.  Prints one JSON line.

    python scripts/bench_multipart.py [--n 200000] [--reps 10] [--warmup 3]
"""

import argparse
import base64
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-plus_amd"))

from gpumatch import engine, records, workloads  # noqa: E402

B = b"----gmBenchBoundary7MA4YWxkTrZu0gW"
HDR = b"Content-Type: multipart/form-data; boundary=" + B + b"\r\n"


def wrap(raw):
    k = len(raw) // 3
    t = base64.b64encode(raw[k:2 * k])
    b64 = b"\r\n".join(t[i:i + 76] for i in range(0, len(t), 76))
    js = b'{"v": "' + raw[2 * k:].replace(b"\\", b"/").replace(b'"', b"'") + b'"}'
    d = b"--" + B + b"\r\nContent-Disposition: form-data; "
    return (d + b'name="text"\r\n\r\n' + raw[:k] + b"\r\n" +
            d + b'name="file"; filename="upload.bin"\r\nContent-Transfer-Encoding: base64\r\n\r\n' + b64 + b"\r\n" +
            d + b'name="meta"\r\nContent-Type: application/json\r\n\r\n' + js + b"\r\n--" + B + b"--\r\n")


def multipart_batch(n, seed):
    """n records that hold a Content-Type header and a body: gen_c4's bodies (cycled), wrapped."""
    ss = workloads.c4_sigset(400, 100)
    reqs, arena = records.gen_c4(max(n // 4, 1000), ss, seed=seed)
    body = reqs["base"] + reqs["uri_len"] + reqs["args_len"] + reqs["hdr_len"]
    mp = [HDR + wrap(arena[int(b):int(b) + int(k)].tobytes()) for b, k in zip(body, reqs["body_len"]) if k]
    pick = np.arange(n) % len(mp)
    lens = np.array([len(mp[k]) for k in pick], dtype=np.uint64)
    base = np.concatenate([[0], np.cumsum((lens + 15) & ~np.uint64(15))]).astype(np.uint64)
    out = np.zeros(int(base[-1]) + 16, np.uint8)
    for k, b in zip(pick, base[:-1]):
        out[int(b):int(b) + len(mp[k])] = np.frombuffer(mp[k], np.uint8)
    rq = np.zeros(n, dtype=records.REQ_DTYPE)
    rq["base"], rq["hdr_len"], rq["body_len"] = base[:-1], len(HDR), lens - len(HDR)
    return rq, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_multipart.py needs a GPU"
    rq, arena = multipart_batch(a.n, 20191)
    dev = torch.device("cuda", 0)
    e = engine.Engine(0)
    d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).to(dev)
    d_ar = torch.from_numpy(arena).to(dev)
    cap = len(arena) + 16
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(a.n, dtype=torch.int64, device=dev)
    d_len = torch.zeros(a.n, dtype=torch.int32, device=dev)
    d_flg = torch.zeros(a.n, dtype=torch.int32, device=dev)
    ms = []
    for k in range(a.warmup + a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        e.multipart_bodies_ptr(d_rq.data_ptr(), d_ar.data_ptr(), len(arena), a.n, d_out.data_ptr(), cap, d_off.data_ptr(),
                               d_len.data_ptr(), d_flg.data_ptr(), 0)
        t1.record()
        e.sync(0)
        t1.synchronize()
        if k >= a.warmup:
            ms.append(t0.elapsed_time(t1))
    ln, fl = d_len.cpu().numpy().view(np.uint32), d_flg.cpu().numpy()
    assert (ln != engine.GM_NONE).all() and (fl == (3 << 8 | 1)).all()   # every body parsed: three parts, one JSON
    body_bytes, med = int(rq["body_len"].sum()), float(np.median(ms))
    print(json.dumps({"bench": "multipart", "n": a.n, "body_bytes": body_bytes, "view_bytes": int(ln.astype(np.int64).sum()),
                      "mix": "3 parts per body: 1/3 verbatim, 1/3 base64 at 76 columns, 1/3 JSON",
                      "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "reps": a.reps, "gpu_GBps": round(body_bytes / med / 1e6, 3),
                      "bodies_per_s": round(a.n / med * 1e3), "csrc_hash": engine.build_hash()}))


if __name__ == "__main__":
    main()
