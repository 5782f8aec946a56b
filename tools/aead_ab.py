#!/usr/bin/env python3
"""What the tag check of a trial decryption costs on the device (jj_aead_open, jj_aead_seal, jj_poly1305, Engine.ka_open_aead), on the GPU box:
    python tools/aead_ab.py [--log2n 10 16 20] [--rounds 3]
    python tools/aead_ab.py --worker trace      (nothing is timed: every call once at the smallest size, for rocprofv3 --kernel-trace)

This driver opens no GPU itself: it starts one worker process per route and round, one at a time, each under a time limit, and stops at the
first worker that does not end well.  The order of the routes is reversed in every other round.  The routes:
  chacha20_xor   jj_chacha20_xor at the same len and stride (what the MAC and the second read add: measurement 1)
  aead_open, aead_seal, poly1305    the three new calls
  ka_kdf, ka_open_aead    jj_ka_kdf alone and Engine.ka_open_aead (what tag-checked trial decryption costs over the key agreement: measurement 2)
  host    what a caller had before (measurement 3): keys and rows copied to the host, EVP_chacha20_poly1305 of the system's libcrypto through
          ctypes in one thread and in 16 processes (the copies are inside the time); left out, with a line that says so, where libcrypto does
          not load
Inputs and results of the device routes are on the device.  A worker times ONE route, at every size in turn.
The full-note shape: len 564 in a stride of 580, zero nonce, empty aad.  The rows are sealed on the device under the keys of the key
agreement and every other tag is broken, so both verdicts occur; the time cannot depend on them (no branch on the verdict).  Every worker warms
up, holds 64 rows to the restatement of tests/aead_cases.py and reports host-clock seconds per call over a window of --seconds of work (one
pass where a pass is longer).  Median [min .. max] of the rounds, and the bytes a call moves per row over the measured time (measurement 4).
The output is profiles/aead_ab.txt, under the expectation written before the run."""
import argparse
import ctypes
import ctypes.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
PERSONAL = b"Zcash_SaplingKDF"
FLAGS = 1 | 32 | 64
LEN, STRIDE = 564, 580
DEVICE_ROUTES = ("chacha20_xor", "aead_open", "aead_seal", "poly1305", "ka_kdf", "ka_open_aead")
# bytes a call moves per row: the row read (twice by open), the key, the result
BYTES = {"chacha20_xor": LEN + 32 + LEN, "aead_open": 2 * (LEN + 16) + 32 + LEN + 1, "aead_seal": LEN + 32 + LEN + 16, "poly1305": LEN + 32 + 16}


def _evp():
    name = ctypes.util.find_library("crypto")
    if not name:
        return None
    try:
        lib = ctypes.CDLL(name)
        lib.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
        lib.EVP_chacha20_poly1305.restype = ctypes.c_void_p
        lib.EVP_DecryptInit_ex.argtypes = [ctypes.c_void_p] * 5
        lib.EVP_CIPHER_CTX_ctrl.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.EVP_DecryptUpdate.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int]
        lib.EVP_DecryptFinal_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        lib.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        return lib
    except (OSError, AttributeError):
        return None


def _evp_open_block(args):
    """(keys, rows) as bytes -> (plaintext, zeros where the tag fails; ok bytes)"""
    keys, rows = args
    lib = _evp()
    ctx = lib.EVP_CIPHER_CTX_new()
    lib.EVP_DecryptInit_ex(ctx, lib.EVP_chacha20_poly1305(), None, None, None)
    lib.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 12, None)
    n = len(keys) // 32
    out = ctypes.create_string_buffer(n * LEN)
    ok = bytearray(n)
    outl, nonce, base = ctypes.c_int(0), bytes(12), ctypes.addressof(out)
    for i in range(n):
        row = rows[i * STRIDE:i * STRIDE + LEN + 16]
        lib.EVP_DecryptInit_ex(ctx, None, None, keys[32 * i:32 * i + 32], nonce)
        lib.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, row[LEN:])                          # EVP_CTRL_AEAD_SET_TAG
        lib.EVP_DecryptUpdate(ctx, base + i * LEN, ctypes.byref(outl), row, LEN)
        if lib.EVP_DecryptFinal_ex(ctx, base + i * LEN, ctypes.byref(outl)) > 0:
            ok[i] = 1
        else:
            ctypes.memset(base + i * LEN, 0, LEN)
    lib.EVP_CIPHER_CTX_free(ctx)
    return out.raw, bytes(ok)


def worker(args):
    import numpy as np
    import torch

    from jubjub_amd import Engine
    from tests import aead_cases as AC
    from tests import ka_cases as KC

    route = args.worker
    pool = None
    if route == "host":
        if _evp() is None:
            print("RESULT " + json.dumps({"no libcrypto": 1}), flush=True)
            return
        import multiprocessing

        pool = multiprocessing.get_context("fork").Pool(16)              # forked BEFORE this process opens the GPU: the children never have it open
    eng = Engine(0)
    sk = KC.SCALARS[-1]

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    def window(fn):
        per = timed(fn, 1)
        if per > args.seconds:
            return per if per > 2.0 else timed(fn, 1)
        timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    out = {}
    for log2n in ([min(args.log2n)] if route == "trace" else args.log2n):
        n = 1 << log2n
        encs = eng.compress(eng.random_points(n, 0xCAFE, 0, subgroup=True, device="cuda"))
        keys, kok = eng.ka_kdf(sk, encs, PERSONAL, FLAGS)
        assert bool(kok.all())
        plain = torch.randint(0, 256, (n, LEN), dtype=torch.uint8, device="cuda")
        rows = torch.zeros((n, STRIDE), dtype=torch.uint8, device="cuda")
        rows[:, :LEN + 16] = eng.aead_seal(keys, plain)
        rows[1::2, LEN + 5] ^= 0x20                                      # every other tag broken
        want_ok = (torch.arange(n, device="cuda") % 2 == 0).to(torch.uint8)
        hk, hr = keys[:64].cpu().numpy(), rows[:64].cpu().numpy()
        want_plain, want_ok64 = AC.open_rows(hk, hr, LEN)
        got, ok = eng.aead_open(keys, rows)
        assert np.array_equal(got[:64].cpu().numpy(), want_plain) and np.array_equal(ok[:64].cpu().numpy(), want_ok64) and bool((ok == want_ok).all())
        assert bool((got[0::2] == plain[0::2]).all()) and not bool(got[1::2].any())
        if route != "host":
            got2, ok2 = eng.ka_open_aead(sk, encs, rows, PERSONAL, FLAGS)
            assert bool((got2 == got).all()) and bool((ok2 == ok).all())
            tags = eng.poly1305(keys, rows, LEN)
            assert np.array_equal(tags[:64].cpu().numpy(), AC.mac_rows(hk, hr, LEN))
            eng.chacha20_xor(keys, rows, None, 1, LEN)
            if route == "trace":
                torch.cuda.synchronize()
                continue
            o_plain, o_ok = torch.empty_like(got), torch.empty_like(ok)
            o_seal, o_tag, o_xor = torch.empty((n, LEN + 16), dtype=torch.uint8, device="cuda"), torch.empty_like(tags), torch.empty_like(got)
            calls = {"chacha20_xor": lambda: eng.chacha20_xor(keys, rows, None, 1, LEN, out=o_xor),
                     "aead_open": lambda: eng.aead_open(keys, rows, out=(o_plain, o_ok)),
                     "aead_seal": lambda: eng.aead_seal(keys, plain, out=o_seal),
                     "poly1305": lambda: eng.poly1305(keys, rows, LEN, out=o_tag),
                     "ka_kdf": lambda: eng.ka_kdf(sk, encs, PERSONAL, FLAGS),
                     "ka_open_aead": lambda: eng.ka_open_aead(sk, encs, rows, PERSONAL, FLAGS)}
            out["%s %d" % (route, log2n)] = window(calls[route])
        else:
            def hosted(procs):
                k, r = keys.cpu().numpy().tobytes(), rows.cpu().numpy().tobytes()
                if procs == 1:
                    parts = [_evp_open_block((k, r))]
                else:
                    step = -(-n // procs)
                    parts = pool.map(_evp_open_block, [(k[32 * o:32 * (o + step)], r[STRIDE * o:STRIDE * (o + step)]) for o in range(0, n, step)])
                return b"".join(p[0] for p in parts), b"".join(p[1] for p in parts)

            hp, hok = hosted(16)
            assert hp == got.cpu().numpy().tobytes() and hok == ok.cpu().numpy().tobytes()      # libcrypto and the device agree on every row
            out["host EVP x16 %d" % log2n] = window(lambda: hosted(16))
            out["host EVP x1 %d" % log2n] = window(lambda: hosted(1))
    if pool is not None:
        pool.close()
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", choices=list(DEVICE_ROUTES) + ["host", "trace"])
    ap.add_argument("--log2n", type=int, nargs="+", default=[10, 16, 20])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one worker")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    results = {}
    for rnd in range(args.rounds):
        order = DEVICE_ROUTES + ("host",)
        for route in (order if rnd % 2 == 0 else order[::-1]):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", route, "--seconds", str(args.seconds), "--log2n"] + [str(x) for x in args.log2n]
            res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
            line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
            if res.returncode != 0 or not line:
                print("STOP: worker %s of round %d ended with %d; nothing more is started\n%s" % (route, rnd, res.returncode, res.stderr[-2000:]))
                return 3
            for k, v in json.loads(line[0][7:]).items():
                results.setdefault(k, []).append(v)
            print("# round %d, %s: done" % (rnd, route), flush=True)
    if results.pop("no libcrypto", None):
        print("# the system's libcrypto does not load here: no host route")
    print("# full-note rows (len %d in a stride of %d, zero nonce, empty aad); seconds of host clock per call, device-resident data for the device routes" % (LEN, STRIDE))
    print("# %d alternating rounds of one process per route; median [min .. max]; GB/s = the bytes the call moves per row over the median" % args.rounds)
    print("%-18s %8s %12s %24s %12s %10s" % ("route", "log2 n", "ms per call", "[min .. max]", "M rows / s", "GB/s"))
    for key in sorted(results, key=lambda k: (int(k.rsplit(" ", 1)[1]), k)):
        v = sorted(results[key])
        name, log2n = key.rsplit(" ", 1)
        med, n = v[len(v) // 2], 1 << int(log2n)
        rate = "%10.1f" % (BYTES[name] * n / med / 1e9) if name in BYTES else "%10s" % "-"
        print("%-18s %8s %12.3f %24s %12.2f %s" % (name, log2n, med * 1e3, "[%.3f .. %.3f]" % (v[0] * 1e3, v[-1] * 1e3), n / med / 1e6, rate))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
