#!/usr/bin/env python3
"""gm_inflate_bodies throughput: the C4 workload's request bodies, each gzipped at level 6, inflated
by the wave-per-stream kernel (gm_inflate.inc); Python's zlib over the same bodies on a thread pool
beside it as context.  HIP events around each call, warm-up first, the spread of the repeats
reported.  Prints one JSON line.

    python scripts/bench_inflate.py [--n 200000] [--reps 10] [--warmup 3] [--threads 16]
"""

import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-plus_amd"))

from gpumatch import engine, records, workloads  # noqa: E402


def gzip_batch(n, seed):
    """n records that hold only a body: the bodies of gen_c4 (cycled over those that have one)."""
    ss = workloads.c4_sigset(400, 100)
    reqs, arena = records.gen_c4(max(n // 4, 1000), ss, seed=seed)
    body = reqs["base"] + reqs["uri_len"] + reqs["args_len"] + reqs["hdr_len"]
    raw = [arena[int(b):int(b) + int(k)].tobytes() for b, k in zip(body, reqs["body_len"]) if k]
    co = [zlib.compressobj(6, zlib.DEFLATED, 31) for _ in raw]
    gz = [c.compress(r) + c.flush() for c, r in zip(co, raw)]
    pick = np.arange(n) % len(gz)
    lens = np.array([len(gz[k]) for k in pick], dtype=np.uint64)
    base = np.concatenate([[0], np.cumsum((lens + 15) & ~np.uint64(15))]).astype(np.uint64)
    out = np.zeros(int(base[-1]) + 16, np.uint8)
    for k, b in zip(pick, base[:-1]):
        g = gz[k]
        out[int(b):int(b) + len(g)] = np.frombuffer(g, np.uint8)
    rq = np.zeros(n, dtype=records.REQ_DTYPE)
    rq["base"], rq["body_len"] = base[:-1], lens
    return rq, out, [gz[k] for k in pick], int(sum(len(raw[k]) for k in pick))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_inflate.py needs a GPU"
    rq, arena, bodies, raw_bytes = gzip_batch(a.n, 20191)
    dev = torch.device("cuda", 0)
    e = engine.Engine(0)
    d_rq = torch.from_numpy(rq.view(np.uint8).reshape(-1).copy()).to(dev)
    d_ar = torch.from_numpy(arena).to(dev)
    cap = 8 * len(arena) + 16
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(a.n, dtype=torch.int64, device=dev)
    d_len = torch.zeros(a.n, dtype=torch.int32, device=dev)
    ms = []
    for k in range(a.warmup + a.reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        e.inflate_bodies_ptr(d_rq.data_ptr(), d_ar.data_ptr(), len(arena), a.n, d_out.data_ptr(), cap, d_off.data_ptr(),
                             d_len.data_ptr(), 0)
        t1.record()
        e.sync(0)
        t1.synchronize()
        if k >= a.warmup:
            ms.append(t0.elapsed_time(t1))
    ln = d_len.cpu().numpy().view(np.uint32)
    out_bytes = int(ln[ln != engine.GM_NONE].astype(np.int64).sum())
    assert out_bytes == raw_bytes, (out_bytes, raw_bytes)   # every body inflated whole
    with ThreadPoolExecutor(a.threads) as ex:   # (zlib releases the GIL)
        t = time.perf_counter()
        list(ex.map(lambda b: zlib.decompress(b, wbits=31), bodies, chunksize=1024))
        cpu_s = time.perf_counter() - t
    med = float(np.median(ms))
    print(json.dumps({"bench": "inflate", "n": a.n, "gzip_bytes": int(rq["body_len"].sum()), "inflated_bytes": out_bytes,
                      "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                      "reps": a.reps, "gpu_GBps": round(out_bytes / med / 1e6, 3),
                      "zlib_threads": a.threads, "zlib_GBps": round(out_bytes / cpu_s / 1e9, 3),
                      "csrc_hash": engine.build_hash()}))


if __name__ == "__main__":
    main()
