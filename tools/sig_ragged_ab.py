#!/usr/bin/env python3
"""A/B of one verdict per segment in one call (jj_sigbatch_ragged) against the two routes a caller had before it, on the GPU box:
    python tools/sig_ragged_ab.py [--log2n 16 20] [--rounds 5] [--locate-log2n 20] [--trace-one LOG2N]

One process, device-resident inputs, valid batches: n signatures under n keys, made on the device with the library itself (keys and nonces by
jj_fixedbase_mul + jj_compress, s = k + c sk by jj_fr_mul / jj_fr_add).  Every route is warmed up and EVERY run's verdicts are checked; then the
routes ALTERNATE in `rounds` rounds (host clock around work that ends with the verdicts on the host).  Signatures per second: median [min .. max].
  g   ONE jj_sigbatch_ragged call over all S segments
  a   one jj_sigbatch_begin + jj_msm_finish job per segment, four in flight.  With more than --job-cap segments the route runs over the first
      --job-cap segments only and its rate is that of the signatures they hold (a job costs the same whichever segment it is)
  b   the per-signature route over all n: jj_decompress x 2 + jj_point_neg + jj_fixedvar_mul_vartime_compressed, table 13
Shapes: 16 equal segments (the first round of a bisection), n / 64 segments of 64, n segments of 1, geometric lengths of mean 16.
Then Engine.sigbatch_locate (fanout 16) with 1 and with 16 failing signatures planted, against route b over the whole batch (which finds them too:
its per-signature comparison is the list).
--trace-one LOG2N: nothing is timed; ONE call (n / 64 segments of 64) after a warm-up, for a kernel-trace run
(rocprofv3 --kernel-trace -- python tools/sig_ragged_ab.py --trace-one 20).
The output is profiles/sig_ragged_ab.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--locate-log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--job-cap", type=int, default=1024, help="route a: segments per pass, at most")
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
    ident_row = torch.from_numpy(np.array(SC.IDENTITY)).to(dev)

    def material(n):
        """n valid signatures on the device: r, a (encodings), s, c (canonical Fr elements), z (odd weights)"""
        sk, nonce, c = [eng.synth_scalars(n, seed, device=dev) for seed in (0x6C10, 0x6C11, 0x6C12)]
        z = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(0x6C13))
        z[:, 0] |= 1
        s = eng.field_binary("fr", "add", nonce, eng.field_binary("fr", "mul", c, sk))
        return eng.compress(eng.fixedbase_mul(tab, nonce)), eng.compress(eng.fixedbase_mul(tab, sk)), s, c, z

    def shapes(n):
        rng = np.random.default_rng(0x6C14)
        geo = []
        while sum(geo) < n:
            geo += [int(x) - 1 for x in rng.geometric(1.0 / 17, 4096)]
        cut = np.minimum(np.cumsum(geo), n)
        cut = cut[:int(np.argmax(cut >= n)) + 1]
        return [("16 equal segments", (np.arange(17, dtype=np.uint64) * np.uint64(n)) // np.uint64(16)),
                ("n/64 segments of 64", np.arange(0, n + 1, 64, dtype=np.uint64)),
                ("n segments of 1", np.arange(n + 1, dtype=np.uint64)),
                ("geometric lengths, mean 16", np.concatenate([[0], cut]).astype(np.uint64))]

    def per_signature(r, a, s, c):
        """route b: the compressed [s]B - [c]A of every signature beside its R -> the indices that differ"""
        rp, rok = eng.decompress(r, 0)
        ap_, aok = eng.decompress(a, 0)
        enc = eng.fixedvar_mul_vartime_compressed(tab, s, c, eng.point_neg(ap_))
        bad = (enc != r).any(dim=1) | (rok == 0) | (aok == 0)
        return torch.nonzero(bad).reshape(-1).tolist()

    def timed(fn, batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok = fn(batches)
        torch.cuda.synchronize()
        assert ok, "a route gave a wrong verdict"
        return (time.perf_counter() - t0) / batches

    def alternate(routes, seconds):
        """warm-up, batches per window for `seconds` of work, then the alternating rounds -> {route: sorted seconds per batch}, {route: batches}"""
        reps = {}
        for name, fn in routes.items():
            timed(fn, 2)
            per = timed(fn, 2)
            reps[name] = max(2, min(4096, int(seconds / per) + 1))
        res = {k: [] for k in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                res[name].append(timed(fn, reps[name]))
        return {k: sorted(v) for k, v in res.items()}, reps

    def apart(x, y):
        return x[-1] < y[0] or y[-1] < x[0]

    if args.trace_one:
        n = 1 << args.trace_one
        r, a, s, c, z = material(n)
        offsets = np.arange(0, n + 1, 64, dtype=np.uint64)
        for _ in range(2):                                   # the second pass is the one to read: workspaces exist
            out = eng.sigbatch_ragged(base_dev, offsets, r, a, s, c, z)
            assert bool((out == ident_row).all().item())
            torch.cuda.synchronize()
        print("traced: n = 2^%d, %d segments of 64: one call, twice (the first pass allocates)" % (args.trace_one, n // 64))
        tab.close()
        eng.close()
        return

    print("# one verdict per segment: %d alternating rounds, device-resident inputs, valid batches; signatures/s: median [min .. max] of the rounds" % args.rounds)
    print("%-6s %-28s %-58s %14s %30s %12s" % ("log2n", "shape", "route", "median sig/s", "[min .. max]", "ms per pass"))
    for lg in args.log2n:
        n = 1 << lg
        r, a, s, c, z = material(n)
        for shape, offsets in shapes(n):
            S = len(offsets) - 1
            o = [int(x) for x in offsets]
            m = min(S, args.job_cap)                         # route a: the first m segments
            covered = o[m]

            def ragged(k):
                ok = True
                for _ in range(k):
                    ok &= bool((eng.sigbatch_ragged(base_dev, offsets, r, a, s, c, z) == ident_row).all().item())
                return ok

            def jobs(k):
                ok = True
                for _ in range(k):
                    q = []
                    for g in range(m):
                        lo, hi = o[g], o[g + 1]
                        if hi == lo:
                            continue                         # an empty segment: the identity without a job
                        q.append(eng.sigbatch_begin(base_dev, r[lo:hi], a[lo:hi], s[lo:hi], c[lo:hi], z[lo:hi]))
                        if len(q) == 4:
                            ok &= bytes(eng.msm_finish(q.pop(0))) == ident
                    while q:
                        ok &= bytes(eng.msm_finish(q.pop(0))) == ident
                return ok

            def each(k):
                return all(per_signature(r, a, s, c) == [] for _ in range(k))

            routes = {"g  one sigbatch_ragged call": ragged,
                      "a  one sigbatch_begin job per segment, four in flight": jobs,
                      "b  decompress x2 + point_neg + fixedvar_mul_vartime_compressed(13)": each}
            sigs = {"g": n, "a": covered, "b": n}
            res, reps = alternate(routes, args.seconds)
            for name in routes:
                v, cnt = res[name], sigs[name.split()[0]]
                note = "" if cnt == n else "   (first %d segments, %d signatures)" % (m, cnt)
                print("%-6d %-28s %-58s %14.0f %30s %12.4f%s" % (lg, shape, name, cnt / v[len(v) // 2], "[%.0f .. %.0f]" % (cnt / v[-1], cnt / v[0]), v[len(v) // 2] * 1e3, note))
            k = {x.split()[0]: x for x in routes}
            per = {x: [t / sigs[x] for t in res[k[x]]] for x in sigs}          # seconds per signature
            med = {x: sorted(per[x])[len(per[x]) // 2] for x in per}
            print("%-6d %-28s S = %d; ragged over jobs %.2f%s, ragged over per-signature %.2f%s   (passes per window: %s)"
                  % (lg, shape, S, med["a"] / med["g"], "" if apart(sorted(per["a"]), sorted(per["g"])) else " (inside the spread)",
                     med["b"] / med["g"], "" if apart(sorted(per["b"]), sorted(per["g"])) else " (inside the spread)",
                     ", ".join("%s %d" % (x.split()[0], reps[x]) for x in routes)))
            sys.stdout.flush()

    n = 1 << args.locate_log2n
    r, a, s, c, z = material(n)
    print("# Engine.sigbatch_locate (fanout 16) against the per-signature route over the whole batch, n = 2^%d; ms per search: median [min .. max]" % args.locate_log2n)
    for planted in (1, 16):
        rng = np.random.default_rng(0x6C20 + planted)
        where = sorted(int(x) for x in rng.choice(n, planted, replace=False))
        sb = s.clone()
        sb[torch.tensor(where, device=dev), 1] ^= 1          # s differs in bit 8: still below r (the top byte is untouched)
        want = [(i, "reject") for i in where]
        bound, calls = eng._lib.jj_sigbatch_ragged, []
        eng._lib.jj_sigbatch_ragged = lambda *x: (calls.append(1), bound(*x))[1]
        assert eng.sigbatch_locate(base_dev, r, a, sb, c, z) == want
        eng._lib.jj_sigbatch_ragged = bound
        routes = {"locate": lambda k: all(eng.sigbatch_locate(base_dev, r, a, sb, c, z) == want for _ in range(k)),
                  "b  per-signature": lambda k: all(per_signature(r, a, sb, c) == where for _ in range(k))}
        res, reps = alternate(routes, args.seconds)
        for name in routes:
            v = res[name]
            print("%-3d planted  %-20s %10.3f ms  [%.3f .. %.3f]%s" % (planted, name, v[len(v) // 2] * 1e3, v[0] * 1e3, v[-1] * 1e3,
                                                                       "   (%d sigbatch_ragged calls per search)" % len(calls) if name == "locate" else ""))
        lo_, b_ = res["locate"], res["b  per-signature"]
        print("%-3d planted  per-signature over locate %.2f%s" % (planted, b_[len(b_) // 2] / lo_[len(lo_) // 2], "" if apart(lo_, b_) else " (inside the spread)"))
        sys.stdout.flush()
    tab.close()
    eng.close()


if __name__ == "__main__":
    main()
