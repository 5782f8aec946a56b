#!/usr/bin/env python3
"""A/B of batch Schnorr verification as one MSM job (jj_sigbatch_begin) against what a caller could do before it, on the GPU box:
python tools/sig_batch_ab.py [--log2n 10 16 20] [--rounds 5]

One process, device-resident inputs (valid signatures over one prime-order base, built with the oracle as in tests/sig_batch_cases.py), every
route warmed up and its verdict checked, then the routes ALTERNATE in `rounds` rounds (host clock around work that ends with the verdict on the
host).  Signatures per second: median [min .. max] of the rounds.
  a1  jj_sigbatch_begin + jj_msm_finish, one job at a time
  a4  the same, four jobs in flight (begin four, then finish the oldest and begin the next)
  b   the same check composed from the entry points that existed before: jj_decompress x 2 into one points array, jj_fr_mul for z c and z s,
      the products z s copied to the host and summed there (numpy column sums of 32-bit words, one Python integer reduction), the two ok arrays
      reduced with torch, the scalar array assembled on the device, jj_msm, three jj_point_double on the result
  c   the per-signature route: jj_decompress x 2, jj_point_neg, jj_fixedvar_mul_vartime_compressed on a table of width 13 ([s]B - [c]A, compressed),
      compared with the encodings of R on the device
The output is profiles/sig_batch_ab.txt."""
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
    ap.add_argument("--seconds", type=float, default=0.25, help="work per timed window, at least")
    args = ap.parse_args()
    import numpy as np
    import torch

    from jubjub_amd import Engine
    from tests import sig_batch_cases as SC

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    R_MOD = SC.R
    base = SC.bases()["prime"]
    base_dev = torch.from_numpy(np.array(base)).to(dev)
    tab13 = eng.fixedbase_table(base, 13)
    ident = bytes(SC.IDENTITY)
    print("# batch Schnorr verification A/B: %d alternating rounds, device-resident inputs, valid batches; signatures/s: median [min .. max] of the rounds" % args.rounds)
    print("%-6s %-58s %14s %34s %12s" % ("log2n", "route", "median sig/s", "[min .. max]", "ms per batch"))
    for lg in args.log2n:
        n = 1 << lg
        r, a, s, c, z, _, _ = SC._valid(n, "prime")
        r, a, s, c, z = [torch.from_numpy(np.array(x)).to(dev) for x in (r, a, s, c, z)]
        z32 = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        z32[:, :16] = z
        pts = torch.empty((2 * n + 1, 64), dtype=torch.uint8, device=dev)
        oks = torch.empty((2 * n,), dtype=torch.uint8, device=dev)
        scal = torch.empty((2 * n + 1, 32), dtype=torch.uint8, device=dev)
        pts[2 * n] = base_dev
        scal[:n] = z32

        def a1():
            return bytes(eng.msm_finish(eng.sigbatch_begin(base_dev, r, a, s, c, z))) == ident

        def a4(jobs):
            q, ok = [], True
            for _ in range(jobs):
                q.append(eng.sigbatch_begin(base_dev, r, a, s, c, z))
                if len(q) == 4:
                    ok &= bytes(eng.msm_finish(q.pop(0))) == ident
            while q:
                ok &= bytes(eng.msm_finish(q.pop(0))) == ident
            return ok

        def b():
            eng.decompress(r, 0, out=(pts[:n], oks[:n]))
            eng.decompress(a, 0, out=(pts[n:2 * n], oks[n:]))
            scal[n:2 * n] = eng.field_binary("fr", "mul", z32, c)
            zs = eng.field_binary("fr", "mul", z32, s)
            _, s_ok = eng.field_unary_ok("fr", "from_bytes", s)
            good = bool(oks.min().item()) and bool(s_ok.min().item())
            w = zs.cpu().numpy().view("<u4").astype(np.uint64).sum(axis=0)               # eight column sums below 2^52
            sigma = sum(int(x) << (32 * i) for i, x in enumerate(w)) % R_MOD
            scal[2 * n] = torch.from_numpy(np.frombuffer(((R_MOD - sigma) % R_MOD).to_bytes(32, "little"), dtype=np.uint8).copy()).to(dev)
            out = eng.msm(scal, pts).reshape(1, 64)
            for _ in range(3):
                out = eng.point_double(out)
            return good and bytes(np.asarray(out.cpu() if hasattr(out, "cpu") else out).reshape(64)) == ident

        def cc():
            rp, rok = eng.decompress(r, 0)
            ap_, aok = eng.decompress(a, 0)
            enc = eng.fixedvar_mul_vartime_compressed(tab13, s, c, eng.point_neg(ap_))
            return bool(rok.min().item()) and bool(aok.min().item()) and bool(torch.equal(enc, r))

        def timed(fn, batches):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ok = fn(batches)
            torch.cuda.synchronize()
            assert ok, "a route rejected a valid batch"
            return (time.perf_counter() - t0) / batches

        routes = {
            "a1 sigbatch_begin + msm_finish, one job": lambda k: all(a1() for _ in range(k)),
            "a4 sigbatch_begin + msm_finish, four jobs in flight": a4,
            "b  decompress x2 + fr_mul x2 + host sum + msm (composed)": lambda k: all(b() for _ in range(k)),
            "c  decompress x2 + point_neg + fixedvar_mul_vartime_compressed(13)": lambda k: all(cc() for _ in range(k)),
        }
        reps = {}
        for name, fn in routes.items():                     # warm-up, and enough batches per window for args.seconds of work
            timed(fn, 4)
            per = timed(fn, 4)
            reps[name] = max(4, min(4096, int(args.seconds / per) + 1))
        res = {k: [] for k in routes}
        for _ in range(args.rounds):
            for name, fn in routes.items():
                res[name].append(timed(fn, reps[name]))
        med = {}
        for name in routes:
            v = sorted(res[name])
            med[name] = v[len(v) // 2]
            print("%-6d %-58s %14.0f %34s %12.4f" % (lg, name, n / med[name], "[%.0f .. %.0f]" % (n / v[-1], n / v[0]), med[name] * 1e3))
        k = {x.split()[0]: x for x in routes}
        print("%-6d ratios of the medians: a1 / b = %.3f, a4 / b = %.3f, a1 / c = %.3f, a4 / c = %.3f   (batches per window: %s)"
              % (lg, med[k["b"]] / med[k["a1"]], med[k["b"]] / med[k["a4"]], med[k["c"]] / med[k["a1"]], med[k["c"]] / med[k["a4"]],
                 ", ".join("%s %d" % (x.split()[0], reps[x]) for x in routes)))
        sys.stdout.flush()
    tab13.close()
    eng.close()


if __name__ == "__main__":
    main()
