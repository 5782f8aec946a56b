#!/usr/bin/env python3
"""A/B of one verdict per signature in one call (jj_sigverify_each) against the four-call composed route a caller had before it, on the GPU box:
    python tools/sig_each_ab.py --parent-lib PATH [--variant-lib PATH --variant-name NAME] [--log2n 10 16 20] [--widths 13 10] [--rounds 5]
    python tools/sig_each_ab.py --trace-one LOG2N            (nothing is timed: one call after a warm-up, for rocprofv3 --kernel-trace --stats)

The comparison must not run on the code under test, and a process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this
driver opens no GPU itself: it starts one worker process per route and round, one at a time, each under a time limit, and stops at the first
worker that does not end well.  Rounds ALTERNATE over the routes:
  call      jj_sigverify_each on the shipped library, both modes
  variant   the same call on another build of the library (--variant-lib; jubjub_amd.build.build_variant, or the shipped build of a tree with a
            patch applied -- experiments/sig_each_fused/k_sig_each.patch: the fused kernel this route was measured against and lost to)
  composed  jj_decompress x 2 + jj_point_neg + jj_fixedvar_mul_vartime_compressed + the caller's byte compare, on a build of the PARENT commit
Every worker makes its own device-resident valid batches (n signatures under n keys, made with the library itself), warms every shape up,
checks EVERY run's verdicts and reports the host-clock seconds per call of one window of --seconds of work per shape.  Median [min .. max] of
the rounds.  The locate section (2^20, 0 / 1 / 16 failing signatures planted): Engine.sig_locate and Engine.sigbatch_locate on the shipped
library, the composed route (whose compare is the list) on the parent's.  The decoder section: one jj_decompress over 2^21 encodings (with the
copy that makes r32 | a32 contiguous) against two over 2^20, which is the choice jj_sigverify_each had to make.
The output is profiles/sig_each_ab.txt."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


# ---- worker: one library, one route, every shape once ---------------------------------------------------------------------------------------
def worker(args):
    from jubjub_amd import _lib

    if b"jj_sigverify_each" not in open(_lib.LIB_PATH, "rb").read():      # (by its bytes: loading it here would bring in a HIP runtime ahead of torch's)
        assert args.worker in ("composed", "composed-locate"), "this library has no jj_sigverify_each"
        _lib._SIGS.pop("jj_sigverify_each")                  # the parent's build: the binding must not ask for the symbol
    import numpy as np
    import torch

    from jubjub_amd import Engine
    from tests import sig_batch_cases as SC

    eng = Engine(0)
    dev = torch.device("cuda", 0)
    base = SC.bases()["prime"]
    base_dev = torch.from_numpy(np.array(base)).to(dev)
    tabs = {w: eng.fixedbase_table(base, w) for w in args.widths}

    def material(n):
        """n valid signatures on the device: r, a (encodings), s, c (canonical Fr elements), z (odd weights)"""
        t = tabs[args.widths[0]]
        sk, nonce, c = [eng.synth_scalars(n, seed, device=dev) for seed in (0x6C10, 0x6C11, 0x6C12)]
        z = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(0x6C13))
        z[:, 0] |= 1
        s = eng.field_binary("fr", "add", nonce, eng.field_binary("fr", "mul", c, sk))
        return eng.compress(eng.fixedbase_mul(t, nonce)), eng.compress(eng.fixedbase_mul(t, sk)), s, c, z

    def composed(tab, r, a, s, c):
        """the per-signature route: the compressed [s]B - [c]A of every signature beside its R -> the indices that differ"""
        rp, rok = eng.decompress(r, 0)
        ap_, aok = eng.decompress(a, 0)
        enc = eng.fixedvar_mul_vartime_compressed(tab, s, c, eng.point_neg(ap_))
        bad = (enc != r).any(dim=1) | (rok.reshape(-1) == 0) | (aok.reshape(-1) == 0)
        return torch.nonzero(bad).reshape(-1).tolist()

    def each(tab, r, a, s, c, cofactored):
        v = eng.sigverify_each(tab, r, a, s, c, cofactored=cofactored)
        return torch.nonzero(v != 1).reshape(-1).tolist()

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok = all(fn() for _ in range(k))
        torch.cuda.synchronize()
        assert ok, "a route gave a wrong verdict"
        return (time.perf_counter() - t0) / k

    def window(fn):
        timed(fn, 2)
        per = timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    out = {}
    if args.worker == "trace":
        n = 1 << args.trace_one
        r, a, s, c, z = material(n)
        for _ in range(2):                                   # the second pass is the one to read: workspaces exist
            assert each(tabs[args.widths[0]], r, a, s, c, True) == []
            torch.cuda.synchronize()
        print("traced: n = 2^%d, table %d: one call, twice (the first pass allocates)" % (args.trace_one, args.widths[0]))
    elif args.worker in ("call", "variant", "composed"):
        for lg in args.log2n:
            n = 1 << lg
            r, a, s, c, z = material(n)
            for w in args.widths:
                if args.worker == "composed":
                    out["%d w%d composed" % (lg, w)] = window(lambda: composed(tabs[w], r, a, s, c) == [])
                else:
                    out["%d w%d cofactored" % (lg, w)] = window(lambda: each(tabs[w], r, a, s, c, True) == [])
                    out["%d w%d cofactorless" % (lg, w)] = window(lambda: each(tabs[w], r, a, s, c, False) == [])
            if args.worker == "call":
                # the decoder over r32 | a32: one launch needs the two arrays side by side first
                both = torch.empty((2 * n, 32), dtype=torch.uint8, device=dev)

                def one_launch():
                    both[:n] = r
                    both[n:] = a
                    return bool(eng.decompress(both, 0)[1].all().item())
                out["%d decoder one launch over 2n (with the copy)" % lg] = window(one_launch)
                both[:n] = r
                both[n:] = a
                out["%d decoder one launch over 2n (copy not counted)" % lg] = window(lambda: bool(eng.decompress(both, 0)[1].all().item()))
                out["%d decoder two launches of n" % lg] = window(lambda: bool(eng.decompress(r, 0)[1].all().item()) and bool(eng.decompress(a, 0)[1].all().item()))
    else:
        n = 1 << args.locate_log2n
        w = args.widths[0]
        r, a, s, c, z = material(n)
        for planted in (0, 1, 16):
            rng = np.random.default_rng(0x6C20 + planted)
            where = sorted(int(x) for x in rng.choice(n, planted, replace=False))
            sb = s.clone()
            if planted:
                sb[torch.tensor(where, device=dev), 1] ^= 1  # s differs in bit 8: still below r (the top byte is untouched)
            want = [(i, "reject") for i in where]
            if args.worker == "composed-locate":
                out["%d planted composed" % planted] = window(lambda: composed(tabs[w], r, a, sb, c) == where)
            else:
                out["%d planted sig_locate" % planted] = window(lambda: eng.sig_locate(base_dev, tabs[w], r, a, sb, c, z) == want)
                out["%d planted sigbatch_locate" % planted] = window(lambda: eng.sigbatch_locate(base_dev, r, a, sb, c, z) == want)
                out["%d planted sigverify_each alone" % planted] = window(lambda: each(tabs[w], r, a, sb, c, True) == where)
    for t in tabs.values():
        t.close()
    eng.close()
    print("RESULT " + json.dumps(out))


# ---- driver: no GPU in this process ---------------------------------------------------------------------------------------------------------
def run_worker(route, lib, args, limit=300):
    env = dict(os.environ)
    env.pop("JJ_LIB_PATH", None)
    if lib:
        env["JJ_LIB_PATH"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", route, "--seconds", str(args.seconds), "--locate-log2n", str(args.locate_log2n),
           "--trace-one", str(args.trace_one), "--log2n"] + [str(x) for x in args.log2n] + ["--widths"] + [str(x) for x in args.widths]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if p.returncode:
        sys.stdout.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("worker %s ended with %d; nothing more is started on the GPU" % (route, p.returncode))
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if not line:
        sys.stdout.write(p.stdout)
        return {}
    return json.loads(line[-1][7:])


def apart(x, y):
    return x[-1] < y[0] or y[-1] < x[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[10, 16, 20])
    ap.add_argument("--widths", type=int, nargs="*", default=[13, 10])
    ap.add_argument("--locate-log2n", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--parent-lib", default="", help="libjubjub_hip.so built from the parent commit: the composed route runs on it")
    ap.add_argument("--variant-lib", default="", help="another build of the library that has jj_sigverify_each")
    ap.add_argument("--variant-name", default="variant", help="what the variant build is, for the report")
    ap.add_argument("--trace-one", type=int, default=0, metavar="LOG2N")
    ap.add_argument("--worker", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.trace_one:
        run_worker("trace", "", args)
        return
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: the composed route must run on a build of the parent commit"
    routes = [("call", ""), ("composed", args.parent_lib)] + ([("variant", args.variant_lib)] if args.variant_lib else [])
    res = {}
    for _ in range(args.rounds):
        for route, lib in routes:
            for k, v in run_worker(route, lib, args).items():
                res.setdefault((route, k), []).append(v)
    res = {k: sorted(v) for k, v in res.items()}
    med = lambda v: v[len(v) // 2]      # noqa: E731
    print("# one verdict per signature: %d alternating rounds of one process per route, device-resident valid batches; median [min .. max] of the rounds" % args.rounds)
    print("# call: jj_sigverify_each on the shipped library%s;" % ("; variant: the same call on %s" % args.variant_name if args.variant_lib else ""))
    print("# composed: decompress x2 + point_neg + fixedvar_mul_vartime_compressed + compare on the PARENT commit's library")
    print("%-6s %-6s %-38s %12s %26s %14s" % ("log2n", "table", "route", "ms per call", "[min .. max]", "signatures/s"))
    for lg in args.log2n:
        n = 1 << lg
        for w in args.widths:
            rows = [("call", "cofactored"), ("call", "cofactorless"), ("variant", "cofactored"), ("variant", "cofactorless"), ("composed", "composed")]
            for route, mode in rows:
                v = res.get((route, "%d w%d %s" % (lg, w, mode)))
                if v:
                    print("%-6d %-6d %-38s %12.4f %26s %14.0f" % (lg, w, "%s %s" % (route, mode) if route != "composed" else "composed (cofactorless rule)", med(v) * 1e3,
                                                                 "[%.4f .. %.4f]" % (v[0] * 1e3, v[-1] * 1e3), n / med(v)))
            c, f, fl = res.get(("composed", "%d w%d composed" % (lg, w))), res.get(("call", "%d w%d cofactorless" % (lg, w))), res.get(("call", "%d w%d cofactored" % (lg, w)))
            fb = res.get(("variant", "%d w%d cofactored" % (lg, w)))
            if c and f:
                print("%-6d %-6d composed over the call: cofactorless %.3f%s, cofactored %.3f%s" % (lg, w, med(c) / med(f), "" if apart(c, f) else " (inside the spread)",
                                                                                                    med(c) / med(fl), "" if apart(c, fl) else " (inside the spread)"))
            if fb and fl:
                print("%-6d %-6d variant over the call (cofactored): %.3f%s" % (lg, w, med(fb) / med(fl), "" if apart(fb, fl) else " (inside the spread)"))
        d = [res.get(("call", "%d decoder %s" % (lg, x))) for x in ("one launch over 2n (with the copy)", "one launch over 2n (copy not counted)", "two launches of n")]
        if all(d):
            print("%-6d decoder over R and A: one launch with the copy %.4f ms [%.4f .. %.4f], one launch without it %.4f ms [%.4f .. %.4f], two launches %.4f ms [%.4f .. %.4f]"
                  % (lg, med(d[0]) * 1e3, d[0][0] * 1e3, d[0][-1] * 1e3, med(d[1]) * 1e3, d[1][0] * 1e3, d[1][-1] * 1e3, med(d[2]) * 1e3, d[2][0] * 1e3, d[2][-1] * 1e3))
        sys.stdout.flush()
    # the locate section
    loc = {}
    for _ in range(args.rounds):
        for route, lib in (("locate", ""), ("composed-locate", args.parent_lib)):
            for k, v in run_worker(route, lib, args).items():
                loc.setdefault(k, []).append(v)
    loc = {k: sorted(v) for k, v in loc.items()}
    print("# which signatures fail, n = 2^%d, table %d; ms per search: median [min .. max]" % (args.locate_log2n, args.widths[0]))
    for planted in (0, 1, 16):
        for name in ("sig_locate", "sigbatch_locate", "sigverify_each alone", "composed"):
            v = loc["%d planted %s" % (planted, name)]
            print("%-3d planted  %-24s %10.3f ms  [%.3f .. %.3f]" % (planted, name, med(v) * 1e3, v[0] * 1e3, v[-1] * 1e3))
        s, b, c = (loc["%d planted %s" % (planted, x)] for x in ("sig_locate", "sigbatch_locate", "composed"))
        print("%-3d planted  sigbatch_locate over sig_locate %.2f%s, composed over sig_locate %.2f%s" % (planted, med(b) / med(s), "" if apart(b, s) else " (inside the spread)",
                                                                                                     med(c) / med(s), "" if apart(c, s) else " (inside the spread)"))


if __name__ == "__main__":
    main()
