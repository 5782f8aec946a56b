#!/usr/bin/env python3
"""A/B of the batch Schnorr check with the terms of equal keys folded (jj_sigbatch_keyed_begin) against jj_sigbatch_begin on the expanded arrays,
on the GPU box:   python tools/sig_keyed_ab.py [--log2n 10 16 20] [--rounds 5] [--trace-one LOG2N]

One process, device-resident inputs, valid batches: n signatures under K keys in equal groups (K = 8, 256, n/4, n; a K above n is left out), made
on the device with the library itself (keys and nonces by jj_fixedbase_mul + jj_compress, s = k + c sk by jj_fr_mul / jj_fr_add).  Every route is
warmed up and EVERY run's verdict is checked (the identity); then the routes ALTERNATE in `rounds` rounds (host clock around work that ends with the
verdict on the host).  Signatures per second: median [min .. max] of the rounds.
  k1 / k4   jj_sigbatch_keyed_begin + jj_msm_finish, one job at a time / four jobs in flight (begin four, then finish the oldest and begin the next)
  a1 / a4   jj_sigbatch_begin + jj_msm_finish on the expanded arrays (a32[k] repeated over its group), the same two ways
--trace-one LOG2N: nothing is timed; ONE keyed call (K = 256) and ONE expanded call after a warm-up of each, for a kernel-trace run
(rocprofv3 --kernel-trace -- python tools/sig_keyed_ab.py --trace-one 20).
The output is profiles/sig_keyed_ab.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 16, 20])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--trace-one", type=int, default=0, metavar="LOG2N")
    args = ap.parse_args()
    import numpy as np
    import torch

    from jubjub_amd import Engine
    from tests import sig_batch_cases as SC

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    base = SC.bases()["prime"]
    base_dev = torch.from_numpy(np.array(base)).to(dev)
    tab = eng.fixedbase_table(base, 13)
    ident = bytes(SC.IDENTITY)

    def material(n):
        """n secret keys, nonces and challenges (canonical Fr elements) and weights on the device; the n keys and the n R encodings"""
        sk, nonce, c = [eng.synth_scalars(n, seed, device=dev) for seed in (0x6B10, 0x6B11, 0x6B12)]
        z = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(0x6B13))
        z[:, 0] |= 1
        return sk, nonce, c, z, eng.compress(eng.fixedbase_mul(tab, sk)), eng.compress(eng.fixedbase_mul(tab, nonce))

    def grouped(n, K, sk, nonce, c, keys_all):
        """equal groups: signature i is checked under key i * K // n"""
        offsets = (np.arange(K + 1, dtype=np.uint64) * np.uint64(n)) // np.uint64(K)
        g = torch.from_numpy(np.repeat(np.arange(K), np.diff(offsets.astype(np.int64)))).to(dev)
        s = eng.field_binary("fr", "add", nonce, eng.field_binary("fr", "mul", c, sk[g].contiguous()))
        return keys_all[:K].contiguous(), offsets, keys_all[g].contiguous(), s

    if args.trace_one:
        n, K = 1 << args.trace_one, 256
        sk, nonce, c, z, keys_all, r = material(n)
        keys, offsets, a, s = grouped(n, K, sk, nonce, c, keys_all)
        for _ in range(2):                                   # the second pass is the one to read: workspaces exist
            assert bytes(eng.msm_finish(eng.sigbatch_keyed_begin(base_dev, keys, offsets, r, s, c, z))) == ident
            torch.cuda.synchronize()
            assert bytes(eng.msm_finish(eng.sigbatch_begin(base_dev, r, a, s, c, z))) == ident
            torch.cuda.synchronize()
        print("traced: n = 2^%d, K = %d: keyed call, expanded call (twice each, the first pass allocates)" % (args.trace_one, K))
        tab.close()
        eng.close()
        return

    print("# batch Schnorr verification, keys folded against expanded: %d alternating rounds, device-resident inputs, valid batches, equal groups;"
          " signatures/s: median [min .. max] of the rounds" % args.rounds)
    print("%-6s %-8s %-52s %14s %30s %12s" % ("log2n", "K", "route", "median sig/s", "[min .. max]", "ms per batch"))
    for lg in args.log2n:
        n = 1 << lg
        sk, nonce, c, z, keys_all, r = material(n)
        for K in sorted({k for k in (8, 256, n // 4, n) if k <= n}):
            keys, offsets, a, s = grouped(n, K, sk, nonce, c, keys_all)

            def keyed():
                return eng.sigbatch_keyed_begin(base_dev, keys, offsets, r, s, c, z)

            def expanded():
                return eng.sigbatch_begin(base_dev, r, a, s, c, z)

            def one(begin):
                return lambda k: all(bytes(eng.msm_finish(begin())) == ident for _ in range(k))

            def four(begin):
                def fn(jobs):
                    q, ok = [], True
                    for _ in range(jobs):
                        q.append(begin())
                        if len(q) == 4:
                            ok &= bytes(eng.msm_finish(q.pop(0))) == ident
                    while q:
                        ok &= bytes(eng.msm_finish(q.pop(0))) == ident
                    return ok
                return fn

            def timed(fn, batches):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ok = fn(batches)
                torch.cuda.synchronize()
                assert ok, "a route rejected a valid batch"
                return (time.perf_counter() - t0) / batches

            routes = {
                "k1 sigbatch_keyed_begin + msm_finish, one job": one(keyed),
                "a1 sigbatch_begin (expanded) + msm_finish, one job": one(expanded),
                "k4 sigbatch_keyed_begin, four jobs in flight": four(keyed),
                "a4 sigbatch_begin (expanded), four jobs in flight": four(expanded),
            }
            reps = {}
            for name, fn in routes.items():                  # warm-up, and enough batches per window for args.seconds of work
                timed(fn, 4)
                per = timed(fn, 4)
                reps[name] = max(4, min(4096, int(args.seconds / per) + 1))
            res = {k: [] for k in routes}
            for _ in range(args.rounds):
                for name, fn in routes.items():
                    res[name].append(timed(fn, reps[name]))
            med, lo, hi = {}, {}, {}
            for name in routes:
                v = sorted(res[name])
                med[name], lo[name], hi[name] = v[len(v) // 2], v[0], v[-1]
                print("%-6d %-8d %-52s %14.0f %30s %12.4f" % (lg, K, name, n / med[name], "[%.0f .. %.0f]" % (n / v[-1], n / v[0]), med[name] * 1e3))
            k = {x.split()[0]: x for x in routes}

            def ratio(a_, k_):
                """median ratio, and whether the two routes' ranges of rounds are apart"""
                apart = hi[k[k_]] < lo[k[a_]] or hi[k[a_]] < lo[k[k_]]
                return "%.3f%s" % (med[k[a_]] / med[k[k_]], "" if apart else " (inside the spread)")

            print("%-6d %-8d keyed over expanded, ratios of the medians: one job %s, four in flight %s   (batches per window: %s)"
                  % (lg, K, ratio("a1", "k1"), ratio("a4", "k4"), ", ".join("%s %d" % (x.split()[0], reps[x]) for x in routes)))
            sys.stdout.flush()
    tab.close()
    eng.close()


if __name__ == "__main__":
    main()
