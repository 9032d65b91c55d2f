#!/usr/bin/env python3
"""gm_ws_messages throughput on two traffic shapes: segments of many small text frames (64-byte
payloads, every eighth message in two fragments, a ping now and then) and segments of one large
binary frame -- parsed by the wave-per-segment kernel (gm_ws.inc).  HIP events around each call,
warm-up first, the spread of the repeats reported; the distinct segments' views and results are
compared with tests/ws_reference.py.  Beside them, as context: a device-to-device copy of the same
bytes (the roofline of a pass that reads and writes every byte once) and the rate of the Python
restatement on one CPU thread.  Prints one JSON line per shape.

    python scripts/bench_ws.py [--mb 512] [--reps 10] [--warmup 3]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ingress-plus_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ws_reference as ref  # noqa: E402
from gpumatch import engine  # noqa: E402

TEXT = b"GET /api/v1/items?id=17&q=lorem+ipsum+dolor+sit+amet HTTP chat line "


def small_frames(rng, seg_bytes=16384):
    out, k = [], 0
    while sum(map(len, out)) + 80 <= seg_bytes:
        key, body = rng.integers(0, 256, 4, dtype=np.uint8).tobytes(), (TEXT * 2)[k % 7:k % 7 + 64]
        if k % 8 == 7:
            out += [ref.frame(1, body[:40], fin=False, key=key), ref.frame(0, body[40:], key=key)]
        else:
            out.append(ref.frame(1, body, key=key))
        if k % 32 == 31:
            out.append(ref.frame(9, b"keepalive", key=key))
        k += 1
    return b"".join(out)


def one_large_frame(rng, payload=65536):
    return ref.frame(2, rng.integers(0, 256, payload, dtype=np.uint8).tobytes(), key=rng.integers(0, 256, 4, dtype=np.uint8).tobytes())


def shape_batch(make, distinct, total_bytes, seed):
    """`distinct` segments cycled up to total_bytes, each at a 16-byte aligned offset of one wire buffer"""
    rng = np.random.default_rng(seed)
    segs = [make(rng) for _ in range(distinct)]
    n = max(total_bytes // len(segs[0]), 1)
    pick = np.arange(n) % distinct
    lens = np.array([len(segs[k]) for k in pick], dtype=np.uint64)
    base = np.concatenate([[0], np.cumsum((lens + 15) & ~np.uint64(15))]).astype(np.uint64)
    wire = np.zeros(int(base[-1]) + 16, np.uint8)
    for k, b in zip(pick, base[:-1]):
        wire[int(b):int(b) + len(segs[k])] = np.frombuffer(segs[k], np.uint8)
    sg = np.zeros(n, dtype=engine.WS_SEG_DTYPE)
    sg["off"], sg["len"] = base[:-1], lens
    return wire, sg, segs


def timed(fn, warmup, reps):
    import torch
    ms = []
    for k in range(warmup + reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if k >= warmup:
            ms.append(t0.elapsed_time(t1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_ws.py needs a GPU"
    dev = torch.device("cuda", 0)
    e = engine.Engine(0)
    for name, make, distinct in (("small_frames", small_frames, 64), ("one_large_frame", one_large_frame, 8)):
        wire, sg, segs = shape_batch(make, distinct, a.mb << 20, 20260)
        n, in_bytes = len(sg), int(sg["len"].sum())
        d_wire = torch.from_numpy(wire).to(dev)
        d_segs = torch.from_numpy(sg.view(np.uint8).reshape(-1).copy()).to(dev)
        d_out = torch.empty(in_bytes + 16, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n, dtype=torch.int64, device=dev)
        d_len = torch.zeros(n, dtype=torch.int32, device=dev)
        d_res = torch.zeros(4 * n, dtype=torch.int32, device=dev)

        def call():
            e.ws_messages(d_wire.data_ptr(), d_segs.data_ptr(), n, d_out.data_ptr(), in_bytes, d_off.data_ptr(),
                          d_len.data_ptr(), d_res.data_ptr(), 0)
        ms = timed(call, a.warmup, a.reps)
        e.sync(0)
        ln, off, out = d_len.cpu().numpy().view(np.uint32), d_off.cpu().numpy(), d_out.cpu().numpy()
        res = d_res.cpu().numpy().view(engine.WS_RESULT_DTYPE)
        t0 = time.perf_counter()
        exp = [ref.parse(s) for s in segs]
        py_s = time.perf_counter() - t0
        for i in range(min(n, 2 * distinct)):
            view, status, reason, consumed, stop, n_messages = exp[i % distinct]
            assert out[off[i]:off[i] + ln[i]].tobytes() == view, i
            assert tuple(int(x) for x in res[i]) == (status | reason << 8, consumed, stop, n_messages), i
        cp = timed(lambda: d_out[:in_bytes].copy_(d_wire[:in_bytes]), a.warmup, a.reps)
        med = float(np.median(ms))
        print(json.dumps({"bench": "ws", "shape": name, "segments": n, "segment_bytes": len(segs[0]),
                          "frames_per_segment": sum(1 for _ in _frames(segs[0])), "input_bytes": in_bytes,
                          "view_bytes": int(ln.astype(np.int64).sum()), "messages": int(res["n_messages"].astype(np.int64).sum()),
                          "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "reps": a.reps,
                          "gpu_GBps": round(in_bytes / med / 1e6, 3),
                          "d2d_copy_ms_median": round(float(np.median(cp)), 4),
                          "d2d_copy_GBps": round(in_bytes / float(np.median(cp)) / 1e6, 3),
                          "python_reference_MBps": round(sum(map(len, segs)) / py_s / 1e6, 3),
                          "csrc_hash": engine.build_hash()}), flush=True)


def _frames(seg):
    """the offsets of a well-formed segment's frames"""
    p = 0
    while p < len(seg):
        len7 = seg[p + 1] & 127
        ext = 2 if len7 == 126 else 8 if len7 == 127 else 0
        p += 6 + ext + (int.from_bytes(seg[p + 2:p + 2 + ext], "big") if ext else len7)
        yield p


if __name__ == "__main__":
    main()
