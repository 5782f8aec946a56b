#!/usr/bin/env python3
"""B independent MSMs of n terms (jj_msm_batch) against the same rows as a loop of jj_msm_begin / jj_msm_finish jobs, three in flight
(the context's three MSM lanes), both over device-resident inputs and timed in the same process, alternating.  One JSON line per
(B, n, points_shared) with B n <= 2^22; `verified`: 16 rows of the batch equal jj_msm of the same row (itself held to the oracle by the GPU suite).
  python tools/msm_batch_bench.py                 (needs an MI355X)
  python tools/msm_batch_bench.py --only B,n      one size only (e.g. under a kernel trace)"""
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from jubjub_amd import Engine  # noqa: E402

eng = Engine(0)
dev = torch.device("cuda", 0)
only = None
if "--only" in sys.argv:
    only = tuple(int(x) for x in sys.argv[sys.argv.index("--only") + 1].split(","))


def batch_ms(S, P, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = eng.msm_batch(S, P)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def jobs_ms(S, P, inflight=3):
    B = S.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    jobs, res = [], [None] * B
    for b in range(B):
        jobs.append((b, eng.msm_begin(S[b], P if P.dim() == 2 else P[b])))
        if len(jobs) > inflight:
            i, j = jobs.pop(0)
            res[i] = eng.msm_finish(j)
    for i, j in jobs:
        res[i] = eng.msm_finish(j)
    return (time.perf_counter() - t0) * 1e3, res


for B in (only[0],) if only else (64, 1024, 4096):
    for n in (only[1],) if only else (16, 64, 256, 1024, 4096):
        if B * n > (1 << 22) or (only and (B, n) != only):
            continue
        S = eng.synth_bytes32(B * n, 11 + n, 0, device=dev).reshape(B, n, 32)
        for shared in (0, 1):
            P = eng.random_points(n if shared else B * n, 12 + n, 0, subgroup=False, device=dev)
            P = P if shared else P.reshape(B, n, 64)
            batch_ms(S, P, 2)                                                  # warm-up: workspaces, code objects
            jobs_ms(S[:8], P if shared else P[:8])
            reps = max(3, min(50, (1 << 22) // (B * n)))
            tb, tj = [], []
            for _ in range(3):                                                 # alternating, best of three each
                t, out = batch_ms(S, P, reps)
                tb.append(t)
                t, res = jobs_ms(S, P)
                tj.append(t)
            h = out.cpu().numpy()
            rows = [int(b) for b in torch.linspace(0, B - 1, 16).long()]
            one = [eng.msm(S[b], P if shared else P[b]) for b in rows]
            verified = all((h[b] == res[b]).all() and (h[b] == o.cpu().numpy()).all() for b, o in zip(rows, one))
            b_ms, j_ms = min(tb), min(tj)
            print(json.dumps({"B": B, "n": n, "points_shared": shared, "batch_ms": round(b_ms, 4), "batch_terms_per_s": round(B * n / b_ms * 1e3),
                              "jobs_ms": round(j_ms, 3), "jobs_terms_per_s": round(B * n / j_ms * 1e3), "speedup": round(j_ms / b_ms, 2),
                              "verified": bool(verified)}), flush=True)
