#!/usr/bin/env python3
"""A/B of the windowed Pedersen commitment (jj_pedersen_commit_vartime) on the note-commitment shape, on the GPU box:
    python tools/commit_ab.py --parent-lib PATH --split-lib PATH [--log2n 20 16 10] [--rounds 3]

A process loads ONE library (JJ_LIB_PATH is read when jubjub_amd is imported), so this driver opens no GPU itself: it starts one worker process
per route and round, one at a time, each under a time limit, and stops at the first worker that does not end well.  Rounds ALTERNATE:
  new     this commit's library: (a) the call with a gathered rbase (window_bits 13: the fused walk), (b) the call with the default LDS rbase
          (k_pedersen_commit, then the table's own kernel with chain = 1); and Engine.note_check end to end at the sizes up to 2^16
  split   a probe build of this commit (python -c "from jubjub_amd import build as b; b.build_variant(PATH, ['-DJJ_EXPERIMENTS',
          '-DJJ_COMMIT_PROBE_SPLIT'])"): the call with rbase 13 in the two-launch form, k_pedersen_commit up to the message's end and then
          k_fixedbase_gather with chain = 1 -- what the fused walk has to beat
  parent  (c) what a caller had before, on a build of the PARENT commit: the three sources packed into rows of 72 bytes (torch.cat; timed
          separately), then jj_pedersen_hash_vartime(JJ_PEDERSEN_POINT) + jj_fixedbase_mul (rbase 13) + jj_point_add + the u-coordinates copied out
The shape: four segments of 63 chunks, the prefix 0b111111, 64 bits at byte 12 of rows of 52 bytes, then two arrays of 32 bytes: 582 bits.
Inputs and results stay on the device.  Every worker warms up, holds one unit per size to the restatement of tests/commit_cases.py and reports
host-clock seconds per call over a window of --seconds of work.  Median [min .. max] of the rounds.  The output is profiles/commit_ab.txt."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
FIELDS = ((0, 12, 64), (1, 0, 256), (2, 0, 256))
PREFIX, PREFIX_BITS, SEG_CHUNKS, GATHERED = 0b111111, 6, 63, 13
PLAIN_LEN = 564


def worker(args):
    import numpy as np
    import torch

    from jubjub_amd import Engine, _lib
    from tests import commit_cases as CC
    from tests import pedersen_cases as PC

    J = PC.J                                                           # the restatement's point arithmetic, through the case module as tools/pedersen_ab.py takes it

    route = args.worker
    if route == "parent":
        blob = open(_lib.LIB_PATH, "rb").read()
        for name in [k for k in _lib._SIGS if k.encode() not in blob]:
            _lib._SIGS.pop(name)                                       # the parent's build: the binding must not ask for the symbols it lacks
    eng = Engine(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0xC0117)
    gens, rpt = CC.gens_of("four"), CC.bases()["R"]
    ped = eng.pedersen_table(CC.gens_bytes("four"), SEG_CHUNKS, 0)
    r13 = eng.fixedbase_table(PC.point_bytes(rpt).copy(), GATHERED)
    lds = eng.fixedbase_table(PC.point_bytes(rpt).copy(), 0)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k

    def window(fn):
        per = timed(fn, 1)
        timed(fn, 2)
        return timed(fn, max(2, min(4096, int(args.seconds / per) + 1)))

    def check(label, got, srcs, r, unit):
        bits = [1] * PREFIX_BITS
        for s, off, nb in FIELDS:
            row = srcs[s][unit].cpu().numpy()
            bits += [(int(row[off + (k >> 3)]) >> (k & 7)) & 1 for k in range(nb)]
        k = int.from_bytes(r[unit].cpu().numpy().tobytes(), "little") & ((1 << 252) - 1)
        h = J.affine_to_extended(PC.expected(gens, SEG_CHUNKS, bits))
        want = J.ext_to_affine(J.ext_add(h, J.affine_to_extended(J.scalar_mul_fast(rpt, k))))
        assert bytes(got[unit].cpu().numpy()[:32]) == want[0].to_bytes(32, "little"), (route, label, unit)

    out = {}
    for lg in args.log2n:
        n = 1 << lg
        srcs = [torch.randint(0, 256, (n, w), dtype=torch.uint8, device=dev, generator=gen) for w in (52, 32, 32)]
        r = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=gen)
        res = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        unit = int(np.random.default_rng(lg).integers(0, n))
        if route in ("new", "split"):
            tag = "a" if route == "new" else "a'"
            what = "fused walk" if route == "new" else "two launches: k_pedersen_commit, k_fixedbase_gather chain = 1"
            out["%d %s: pedersen_commit, rbase %d (%s)" % (lg, tag, GATHERED, what)] = window(lambda: eng.pedersen_commit(ped, r13, srcs, FIELDS, r, PREFIX, PREFIX_BITS, out=res))
            check(tag, res, srcs, r, unit)
        if route == "new":
            out["%d b: pedersen_commit, default LDS rbase" % lg] = window(lambda: eng.pedersen_commit(ped, lds, srcs, FIELDS, r, PREFIX, PREFIX_BITS, out=res))
            check("b", res, srcs, r, unit)
            if lg <= 16:
                plain = torch.randint(0, 256, (n, PLAIN_LEN), dtype=torch.uint8, device=dev, generator=gen)
                plain[:, 0] = 2
                ivk = np.frombuffer((0x1234567 ** 9 % J.R_MOD).to_bytes(32, "little"), dtype=np.uint8)
                args_nc = (ivk, plain, r, ped, lds, b"JJ_gd_ab", bytes(64), b"JJ_ExpandSeed_ab")
                out["%d note_check end to end, default LDS rbase, epk checked" % lg] = window(lambda: eng.note_check(*args_nc, epk=res))
        if route == "parent":
            def pack():
                return torch.cat([srcs[0][:, 12:20], srcs[1], srcs[2]], dim=1)

            rows = pack()

            def composed():
                h = eng.pedersen_hash(ped, rows, ((0, 576),), PREFIX, PREFIX_BITS, point=True)
                res.copy_(eng.point_add(h, eng.fixedbase_mul(r13, r))[:, :32])

            out["%d c: parent commit, pedersen_hash + fixedbase_mul (rbase %d) + point_add + u on pre-packed rows" % (lg, GATHERED)] = window(composed)
            out["%d c: parent commit, packing the three sources into rows of 72 bytes (torch.cat)" % lg] = window(pack)
            check("c", res, srcs, r, unit)
    for t in (ped, r13, lds):
        t.close()
    eng.close()
    print("RESULT " + json.dumps(out))


# ---- driver: no GPU in this process ---------------------------------------------------------------------------------------------------------
def run_worker(route, lib, args, limit=300):
    env = dict(os.environ)
    env.pop("JJ_LIB_PATH", None)
    if lib:
        env["JJ_LIB_PATH"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--worker", route, "--seconds", str(args.seconds), "--log2n"] + [str(x) for x in args.log2n]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    if p.returncode:
        sys.stdout.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("worker %s ended with %d; nothing more is started on the GPU" % (route, p.returncode))
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    return json.loads(line[-1][7:]) if line else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="*", default=[20, 16, 10])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.2, help="work per timed window, at least")
    ap.add_argument("--parent-lib", default="", help="libjubjub_hip.so built from the parent commit: route c runs on it")
    ap.add_argument("--split-lib", default="", help="probe build of this commit with -DJJ_EXPERIMENTS -DJJ_COMMIT_PROBE_SPLIT")
    ap.add_argument("--worker", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: route c must run on a build of the parent commit"
    assert args.split_lib and os.path.exists(args.split_lib), "--split-lib: the two-launch form runs on a probe build"
    res = {}
    for _ in range(args.rounds):
        for route, lib in (("new", ""), ("split", args.split_lib), ("parent", args.parent_lib)):
            for k, v in run_worker(route, lib, args).items():
                res.setdefault(k, []).append(v)
    res = {k: sorted(v) for k, v in res.items()}
    med = lambda v: v[len(v) // 2]      # noqa: E731
    print("# windowed Pedersen commitment, the note shape (582 bits, four segments): %d alternating rounds of one process per route;" % args.rounds)
    print("# median [min .. max] of the rounds, ms per call; inputs and results on the device")
    for lg in args.log2n:
        print("n = 2^%d" % lg)
        for k in sorted(res):
            if k.startswith("%d " % lg):
                v = res[k]
                print("  %-110s %10.4f ms  [%.4f .. %.4f]   %8.2f M units/s" % (k.split(" ", 1)[1], med(v) * 1e3, v[0] * 1e3, v[-1] * 1e3, (1 << lg) / med(v) / 1e6))
        fused = next((res[k] for k in res if k.startswith("%d a:" % lg)), None)
        split = next((res[k] for k in res if k.startswith("%d a':" % lg)), None)
        if fused and split:
            gain, spread = med(split) - med(fused), max(fused[-1] - fused[0], split[-1] - split[0])
            print("  fused against two launches: %+.4f ms, the larger range %.4f ms -> %s" % (gain * 1e3, spread * 1e3, "AHEAD" if gain > spread else "BEHIND" if -gain > spread else "within the ranges"))


if __name__ == "__main__":
    main()
