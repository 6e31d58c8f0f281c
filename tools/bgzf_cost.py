#!/usr/bin/env python3
"""Cost of the BGZF path against the plain independent-block path.

Times jdgpu_bgzf_deflate_device / jdgpu_bgzf_inflate_device (--mode bgzf) or
jdgpu_deflate_device / jdgpu_inflate_device (--mode blocks) on device-resident
level-6 text at one block size, with the per-kernel times of jdgpu_prof_read
from one extra profiled step, and prints one JSON line.  JDAMD_LIB selects the
library, so --mode blocks can be run against a build of the parent commit.

    python tools/bgzf_cost.py --mode bgzf   --mib 1024
    JDAMD_LIB=.../libjdeflate_amd.so python tools/bgzf_cost.py --mode blocks --mib 1024
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jdeflate_amd as J  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]


def dmalloc(n):
    p = ctypes.c_void_p()
    if hip.hipMalloc(ctypes.byref(p), max(n, 16)):
        raise MemoryError(n)
    return p.value


def d2h(d, n):
    hip.hipDeviceSynchronize()
    b = ctypes.create_string_buffer(n)
    hip.hipMemcpy(b, d, n, 2)
    return b.raw


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    hip.hipDeviceSynchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        hip.hipDeviceSynchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    J.prof_enable(True)
    fn()
    hip.hipDeviceSynchronize()
    prof = {k: round(v[0], 4) for k, v in J.prof_read().items()}
    J.prof_enable(False)
    return {"median_ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "kernels_ms": prof}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("bgzf", "blocks"), required=True)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--blocksize", type=int, default=65280)
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    bs = a.blocksize
    n = (a.mib << 20) // bs * bs
    nb = n // bs
    data = J.corpus_text(n, seed=1)
    d_in = dmalloc(n)
    hip.hipMemcpy(d_in, data.ctypes.data, n, 1)
    d_tot, d_back = dmalloc(8), dmalloc(n + bs)
    res = {"mode": a.mode, "bytes": n, "blocksize": bs, "level": a.level,
           "lib": os.environ.get("JDAMD_LIB", "default")}
    if a.mode == "bgzf":
        cap = J.bgzf_bound(n, bs)
        d_out, d_bo, d_err = dmalloc(cap), dmalloc(8 * nb), dmalloc(4 * (nb + 1))
        res["deflate"] = timed(lambda: J.bgzf_deflate_device(d_in, n, d_out, cap, d_bo, d_tot, level=a.level,
                                                            blocksize=bs), a.steps, a.warmup)
        total = int.from_bytes(d2h(d_tot, 8), "little")
        res["compressed"] = total
        res["inflate"] = timed(lambda: J.bgzf_inflate_device(d_out, total, d_back, n, d_tot, d_err, nb + 1),
                               a.steps, a.warmup)
        assert d2h(d_back, 1 << 20) == data[:1 << 20].tobytes()
    else:
        cap = J.bound(n, bs)
        d_out, d_cs, d_co = dmalloc(cap), dmalloc(4 * nb), dmalloc(8 * nb)
        d_us, d_err = dmalloc(4 * nb), dmalloc(4 * nb)
        res["deflate"] = timed(lambda: J.deflate_device(d_in, n, d_out, cap, d_cs, d_co, d_tot, level=a.level,
                                                       blocksize=bs), a.steps, a.warmup)
        total = int.from_bytes(d2h(d_tot, 8), "little")
        res["compressed"] = total
        res["inflate"] = timed(lambda: J.inflate_device(d_out, total, d_co, d_cs, nb, d_back, d_us, d_err,
                                                       blocksize=bs), a.steps, a.warmup)
        assert d2h(d_back, 1 << 20) == data[:1 << 20].tobytes()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
