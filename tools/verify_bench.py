#!/usr/bin/env python3
"""Time BatchCodec.verify on the headline batch beside BatchCodec.decode.

k=10, m=4, 256 x 4 MiB objects, an inline_crc32 full stripe in HBM, all 14
fragments present.  After a warm-up, verify and a plain decode of the same
batch with 4 erasures alternate in one process, each call between two device
events; the medians are reported with the bytes verify reads (headers and
payloads) over its time, in TB/s and as a share of the 7.0 TB/s single-stream
read of profiles/r06c_membench_roof_dmapat.txt.

    python tools/verify_bench.py [--calls 20] [--warmup 3] [--out profiles/verify_bench.json]

For the kernels' own times, run it under `rocprofv3 --kernel-trace --stats`
(a run of its own; counters in another).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROOF_TBS = 7.0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-obj", type=int, default=256)
    ap.add_argument("--obj-len", type=int, default=4 << 20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import torch
    from pyeclib_amd import batch
    k, m, n_obj, obj_len = 10, 4, a.n_obj, a.obj_len
    dev = torch.device("cuda:0")
    codec = batch.BatchCodec(k, m, inline_crc32=True)
    bs = codec.blocksize(obj_len)
    objs = torch.randint(0, 256, (n_obj, obj_len), dtype=torch.uint8, device=dev)
    stripes = batch.stripe_buffer(n_obj, k, m, bs, device=dev)
    codec.encode(objs, obj_len, parity=stripes[:, k:], data=stripes[:, :k])
    out = torch.empty_like(objs)
    res = torch.empty((n_obj, 2), dtype=torch.int32, device=dev)
    full = (1 << (k + m)) - 1
    lost = full & ~((1 << 1) | (1 << 4) | (1 << 5) | (1 << 12))
    masks = [lost] * n_obj

    # what is timed must be right: a clean batch reports nothing, one flipped
    # payload bit is found, the decode returns the objects
    codec.verify(stripes, obj_len, out=res)
    codec.decode(stripes, obj_len, masks, out)
    torch.cuda.synchronize()
    assert not bool(res.any()), "clean stripes reported"
    assert torch.equal(out, objs), "decode differs"
    stripes[n_obj - 1, 13, 80 + bs - 1] ^= 1
    assert codec.verify(stripes, obj_len)[n_obj - 1].tolist() == [0, 1 << 13]
    stripes[n_obj - 1, 13, 80 + bs - 1] ^= 1

    for _ in range(a.warmup):
        codec.verify(stripes, obj_len, out=res)
        codec.decode(stripes, obj_len, masks, out)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.calls)]
    for e0, e1, e2 in ev:
        e0.record()
        codec.verify(stripes, obj_len, out=res)
        e1.record()
        codec.decode(stripes, obj_len, masks, out)
        e2.record()
    torch.cuda.synchronize()
    verify_us = [e0.elapsed_time(e1) * 1e3 for e0, e1, _ in ev]
    decode_us = [e1.elapsed_time(e2) * 1e3 for _, e1, e2 in ev]
    v, d = statistics.median(verify_us), statistics.median(decode_us)
    read = n_obj * (k + m) * (80 + bs)
    tbs = read / (v * 1e-6) / 1e12
    result = {
        "tool": "verify_bench", "device": torch.cuda.get_device_name(0),
        "k": k, "m": m, "n_obj": n_obj, "obj_len": obj_len, "blocksize": bs,
        "calls": a.calls, "warmup": a.warmup,
        "verify_us": round(v, 2), "verify_us_min": round(min(verify_us), 2),
        "verify_us_max": round(max(verify_us), 2),
        "decode_us": round(d, 2), "decode_us_min": round(min(decode_us), 2),
        "decode_us_max": round(max(decode_us), 2),
        "verify_over_decode": round(v / d, 4),
        "verify_bytes_read": read, "verify_read_tbs": round(tbs, 3),
        "share_of_7_0_tbs_read": round(tbs / ROOF_TBS, 4),
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
