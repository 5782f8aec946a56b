#!/usr/bin/env python3
"""
bench.py — headline benchmark of the MI355X Jubjub engine (BASELINE.json metric: Jubjub scalar-muls/sec).

  python bench.py --gpus N --steps K --warmup W [--workload varbase|fixedbase|msm|decompress] [--log2n L] [--scaling weak|strong]
                  [--dump-outputs DIR]

One "step" = PASSES back-to-back passes of the hot path over one batch of synthetic inputs already resident in HBM (the
pass count per workload is fixed below and reported in `config`, it only makes the timed region long enough for the
clocks to settle; `value` is units per second either way).
N = 1 default workload: BASELINE.json configs[1] — 2^20 variable-base scalar-muls (random Fr x random curve points).
N > 1: one process per GPU.  When this script is started WITHOUT a launcher (no WORLD_SIZE in the environment) it spawns
the N ranks itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT) and relays rank 0's single JSON
line; under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` it uses the ranks it is given.
--scaling weak   : every rank runs 2^log2n units (independent shards, no data-path collective; the MSM workload all-gathers
                   one 8 KB record of window sums per rank over RCCL, copies the gathered records to the host once and runs ONE
                   host tail -- window sums, Horner, one inversion -- on every rank).
--msm-partition  : terms  = rank g owns terms [g n/G, (g+1) n/G) and all their windows;
                   window = rank g owns windows g, g + G, ... of ALL terms (every rank holds the whole batch; strong scaling only).
--msm-async D    : D MSMs in flight (N = 1: jj_msm_begin / jj_msm_finish; N > 1 over RCCL with --msm-exchange c: jj_msm_allgather_begin):
                   the exchange and the host tail of one overlap the kernels of the next.
--msm-contexts K : N = 1: K contexts (streams + workspaces) on the one GPU, one host thread each, the step's MSMs dealt among them:
                   sustained throughput (the dependent chains of one MSM leave most of the GPU idle); `ms_per_pass` is then the
                   aggregate time per MSM, not the latency of one.
--scaling strong : 2^log2n units IN TOTAL, cut into contiguous shards (BASELINE configs[3]: 2^20-term MSM over 8 GPUs;
                   configs[4]: 2^26 encodings over 8 GPUs with --log2n 26).
--host-buffers   : pageable | pinned: the timed region is the C-ABI call on HOST arrays (H2D + kernels + D2H, pipelined by the
                   library); `metric` says so, `pcie_inclusive` is true and `roofline.pcie` prices both directions against the link.
                   This is never the headline value (that one has its inputs resident in HBM).  `--workload msm`: jj_msm on host arrays
                   (96 bytes per term in, one 64-byte point out; the library sums 2^19 terms and more in passes whose copies run beside
                   the kernels).
Rank 0 prints ONE JSON line.

Inputs come from the library's counter-based generators (jj_synth_scalars / jj_random_points: Group::random semantics,
reference src/lib.rs:1244-1267, over splitmix64 streams indexed by the GLOBAL unit index), so any rank — and the host-side
checker — can reproduce any unit without moving data.

The JSON carries:
  roofline     integer-VALU roofline of the dominant kernel (this path is carry-free integer multiply-add work, not HBM- or
               MFMA-bound): achieved = algorithmic IMAD32/s with the SURVEY §8(d) convention (field mul = 128, square = 100
               IMAD32) for the field operations THAT KERNEL runs, divided by that kernel's HIP-event duration; peak =
               v_mad_u64_u32 rate measured live on this device (jj_peak_imad32).  `hbm` gives the algorithmic HBM bytes/s
               beside the 8 TB/s peak; `traffic` the PMC-measured fabric bytes per launch from profiles/traffic.json when
               that file was collected for exactly this build of the kernels (source hash), else null.
  verified     a strided sample of the LAST timed output (every 2^10-th unit of rank 0's shard, plus the injected edge
               encodings for the decoder) recomputed by the oracle from the unit indices: true / false.
  cpu_baseline the oracle's C port of the reference algorithm (exact 252-step ladder, 4x64 Montgomery limbs) timed on this
               box's host cores on a bounded sample: one thread and all cores, CPU model stated (N = 1 only).
  dump_outputs with --dump-outputs DIR: the .npy files written from the last timed step's output and how their rows were sampled.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
NOMINAL_PEAK_IMAD32 = 1024 * 16 * 2.4e9   # 1024 SIMDs x 16 lanes x 2.4 GHz boost clock: one 32x32+64 multiply-add per lane per 4-cycle wave64 issue
PCIE_PEAK_GBPS = 63.0    # host link: PCIe Gen5 x16, per direction (what the link measures on this pool: profiles/r4_pcie_probe.txt)
SEED = 0x4A55424A5542
POINT_SEED = SEED ^ 0x9E3779B97F4A7C15
RAW_SEED = SEED ^ 0x5DEECE66D

# Field-operation counts of the algorithms the kernels actually run, per unit, split into the dominant
# kernel ("main": what roofline.kernel_ms times) and the normalisation tail that follows it.
# IMAD32 convention: M = 128, S = 100.
WORK = {
    # k_varbase_ct3 (jj_varbase_mul, the constant-time default since round 5): 2 from_words; table {P, 2P, 3P, 4P}: 4 to_niels x 2M, two doublings,
    # one addition 8M; the carry window's addition + 84 window additions x 8M; 252 doublings x (3S + 4M: 2UV is a product here, jj_curve.h).
    # normalisation tail: tail_work() below
    "varbase": {"S": 252 * 3 + 2 * 3, "M": 2 + 4 * 2 + 2 * 4 + 8 + 85 * 8 + 252 * 4, "bytes": 32 + 64 + 64},
    # k_fixedbase_comb (default, --fb-window 0/7): 32 mixed additions x 7M + three doublings (3S + 4M each); --fb-window 6: k_fixedbase, 43 x 7M
    "fixedbase": {"S": 9, "M": 32 * 7 + 12, "bytes": 32 + 64},
    # Pippenger, c = 16: per term 2M load + 2M to_niels + 16 windows x 7M mixed add; bucket reduce 2 x 10M per bucket
    # (16 x 2^15 buckets / 2^20 terms -> +10M); the 240-doubling Horner tail is per MSM (on the host), not per term
    # (the entry below is the 16-window case, 2^18 terms and more; run() recomputes it from the window count of the record)
    "msm": {"S": 0, "M": 2 + 2 + 16 * 7 + 10, "bytes": 32 + 64},
    # k_decompress (the flag kernels run after it and show up in tail_ms): two decode passes (2 x (1M + 1S + 1M)), shared
    # inversion (3M + (253S+61M)/32), u^2 1M, sqrt = a^((t-1)/2) (220S + 52M, sliding windows) + 2M + 24S + 6M digit
    # extraction + 4 canonical forms + 4M table multiplies + verify (1S + 2M), 1 to_plain (v's bytes are the input's, -u = q - u)
    "decompress": {"S": 2 + 8 + 220 + 24 + 1, "M": 4 + 3 + 2 + 1 + 52 + 2 + 6 + 4 + 4 + 2 + 1, "bytes": 32 + 65},
}


def tail_work(wl, n, cus=256):
    """field operations per unit of the normalisation that follows the ladder kernels: 6M per point + one inversion (255S + 75M) per
    chunk; the chunk length is the one normalize_launch (jj_abi.hip) picks for n units"""
    if wl not in ("varbase", "fixedbase"):
        return 0, 0
    lanes = cus * 64 * 8
    chunk = 64 if n >= lanes * 128 else (32 if n >= lanes * 32 else (16 if n >= lanes * 4 else 4))
    return -(-255 // chunk), 6 + -(-75 // chunk)


# k_varbase (jj_varbase_mul_vartime: per-lane table {0..16}P in memory, signed 5-bit windows): 2 from_words + to_niels(P) 2M; table: to_niels 2M +
# 15 x (mixed add 7M + to_niels 2M); 51 additions x 8M; 250 doublings x (3S + 4M)
WORK_VARTIME = {"S": 250 * 3, "M": 2 + 2 + 2 + 15 * 9 + 51 * 8 + 250 * 4}
REFERENCE_WORK = {"varbase": {"S": 1008, "M": 2774}, "fixedbase": {"S": 1008, "M": 2520}}   # the reference's own ladders
# passes per step: ~0.33 s of kernels per step, so that the default --steps 20 keeps the GPU busy for 6-7 s (a 5-second utilisation sampler around the
# run then sees it; rounds 1-4 ran ~50 ms steps: 1 s of GPU work inside a 40 s process)
PASSES = {"varbase": 24, "fixedbase": 12, "msm": 256, "decompress": 20}
DEFAULT_LOG2N = {"varbase": 20, "fixedbase": 24, "msm": 20, "decompress": 23}
UNIT = {"varbase": "scalar-muls/s", "fixedbase": "scalar-muls/s", "msm": "terms/s", "decompress": "points/s"}
GEN_U = 0x62EDCBB8BF3787C88B0F03DDD60A8187CAF55D1B29BF81AFE4B3D35DF1A7ADFE   # generator (u, 11), reference src/lib.rs:1380-1396
SAMPLE_STRIDE = 1 << 10
# --dump-outputs: an output of more rows than this keeps a fixed sample of DUMP_ROWS of them, drawn with DUMP_SEED (16 MB of float32 at 64 bytes per row)
DUMP_ROWS = 1 << 16
DUMP_SEED = 0x44554D50
BLOCK_LOG2 = 14          # besides the strided sample: one CONTIGUOUS block of 2^14 units (whole waves, whole workgroups) recomputed by the oracle
# edge encodings injected into the decoder's input at fixed global indices: (index, kind)
INJECT_FIRST, INJECT_STEP = 1000, 4096
# JJ_BENCH_FAULT_INJECT=1 flips one bit of the CHECKER's expected values (never of the product's output): the run must then report
# "verified": false and exit with status 3 (tests/test_gpu_dist.py::test_bench_exits_3_when_verification_fails)
FAULT = os.environ.get("JJ_BENCH_FAULT_INJECT") == "1"


def imad32(s, m):
    return 100 * s + 128 * m


def host_bytes(x):
    """numpy view of a small result that may be a numpy array or a torch tensor on any device"""
    import numpy as np

    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def dump_outputs(d, out):
    """--dump-outputs: the arrays of one step's output (a tensor / array of result bytes, or the decoder's (points, ok) pair) as
    d/out.npy (and d/ok.npy), float32 with one element per byte, rows in unit order; above DUMP_ROWS rows the same seeded sample of
    rows for every run of the same batch size.  Returns what the JSON line records about it."""
    import numpy as np

    arrays = dict(zip(("out", "ok"), out if isinstance(out, tuple) else (out,)))
    n = arrays["out"].shape[0] if arrays["out"].ndim > 1 else 1           # the MSM returns one 64-byte point
    rows = None
    if n > DUMP_ROWS:
        rows = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_ROWS, replace=False))
    os.makedirs(d, exist_ok=True)
    files = {}
    for name, x in arrays.items():
        if rows is not None and hasattr(x, "cpu"):
            import torch

            x = x[torch.from_numpy(rows).to(x.device)]                   # gathered on the device: only the sample crosses to the host
        elif rows is not None:
            x = np.asarray(x)[rows]
        h = host_bytes(x).astype(np.float32)
        np.save(os.path.join(d, name + ".npy"), h)
        files[name + ".npy"] = list(h.shape)
    return {"dir": d, "files": files, "rows_of": n,
            "sample": None if rows is None else "%d rows drawn without replacement by numpy default_rng(%#x).choice(%d, %d), sorted" % (DUMP_ROWS, DUMP_SEED, n, DUMP_ROWS)}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="varbase", choices=sorted(WORK))
    ap.add_argument("--log2n", type=int, default=None, help="log2 of the batch: per GPU (weak) or in total (strong); default 20 varbase/msm, 24 fixedbase, 23 decompress")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"])
    ap.add_argument("--passes", type=int, default=0, help="passes per step (default: per workload, see PASSES)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="varbase workload: skip the fixed-base side measurements (clean per-kernel profiles)")
    ap.add_argument("--fb-window", type=int, default=0, help="fixed-base table: 0/7 = signed comb in LDS (default: 32 additions + 3 doublings), 6 = signed 6-bit windows in LDS (43 additions), both with the constant-time shuffle select; 8..16 = table gathered from L2 / Infinity Cache")
    ap.add_argument("--decompress-flags", type=int, default=13,
                    help="jj_decompress flags: 1 ZIP-216 | 2 torsion-free (order-8 Tate pairing; --opt torsion_check_ladder=1 for the [r]P ladder) | 4 reject small order | 8 clear cofactor (default 13 = BASELINE config 5: decode + small-order check + mul_by_cofactor)")
    ap.add_argument("--msm-partition", default="terms", choices=["terms", "window"], help="multi-rank MSM: cut by terms or by windows (see the module docstring)")
    ap.add_argument("--msm-async", type=int, default=1, help="MSM workload: jobs in flight per context (1 = synchronous jj_msm / jj_msm_allgather calls)")
    ap.add_argument("--msm-contexts", type=int, default=1, help="N = 1 MSM workload: contexts (each with its own stream and workspaces) driven by as many host threads on the one GPU: "
                    "the latency-bound tails of one MSM overlap the sort / accumulation of another")
    ap.add_argument("--host-buffers", default=None, choices=["pageable", "pinned", "fresh", "pooled"],
                    help="time the C-ABI call on HOST arrays (the path a drop-in caller takes) instead of device-resident tensors: pinned = page-locked "
                         "buffers from jj_host_alloc, pageable = plain numpy memory (page-locked in place by every call); inputs and result buffers are "
                         "allocated once and reused; fresh = pageable inputs and a NEWLY ALLOCATED pageable result array on every call (what a caller that "
                         "returns a new Vec per call does: the pages of the result are faulted in inside the call); the JSON gains roofline.pcie; "
                         "varbase / fixedbase / decompress, N = 1")
    ap.add_argument("--compressed", action="store_true", help="varbase / fixedbase: 32-byte compressed results (jj_*_mul_compressed)")
    ap.add_argument("--msm-exchange", default="c", choices=["c", "torch"],
                    help="multi-rank MSM over the nccl backend: c = the whole exchange behind the C ABI (jj_ctx_set_comm + jj_msm_allgather on an RCCL "
                         "communicator of this process's own); torch = jj_msm_partial + torch.distributed.all_gather + jj_msm_combine")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only for plumbing tests)")
    ap.add_argument("--opt", action="append", default=[], metavar="KEY=VALUE", help="jj_ctx_set_option for every context of the run (repeatable), e.g. --opt msm_lanes=1 --opt msm_front1=0; "
                    "host_tail_scalar=1 is process-wide.  The library reads no JJ_* environment variable.")
    ap.add_argument("--cpu-seconds", type=float, default=8.0, help="target wall time of each CPU baseline sample")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="rank 0: write what the last timed step returned as DIR/<name>.npy, float32, one element per result byte (out.npy; the decoder "
                         "also ok.npy); an output of more than %d rows keeps the same seeded sample of %d rows in every run" % (DUMP_ROWS, DUMP_ROWS))
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


# ------------------------------------------------------------------------------------------------ self-launch
def spawn_ranks(a):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) and relay rank 0's line."""
    import torch

    ndev = torch.cuda.device_count()
    if ndev < a.gpus and "JJ_BENCH_FORCE_DEVICE" not in os.environ:
        print("bench.py: --gpus %d but only %d device(s) visible; refusing to report a smaller run as n_gpus=%d "
              "(set JJ_BENCH_FORCE_DEVICE=0 to stack the ranks on one GPU for a plumbing check)" % (a.gpus, ndev, a.gpus), file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    return max(abs(rc) for rc in rcs)


# ------------------------------------------------------------------------------------------------ traffic (PMC) record
def build_id():
    """hash of the kernel sources: profiles/traffic.json is only valid for the build it was collected on"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "jubjub_amd", "csrc")
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fh:
            h.update(f.encode() + b"\0" + fh.read())
    return h.hexdigest()[:16]


def traffic_record(workload, log2n):
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        rec = json.load(open(path))
    except Exception:
        return None, "profiles/traffic.json not present"
    if rec.get("build_id") != build_id():
        return None, "profiles/traffic.json was collected on build %s, this is %s: refused (re-run tools/collect_traffic.py)" % (rec.get("build_id"), build_id())
    e = rec.get("workloads", {}).get("%s:%d" % (workload, log2n))
    if not e:
        return None, "profiles/traffic.json has no entry for %s at 2^%d" % (workload, log2n)
    return e, None


# ------------------------------------------------------------------------------------------------ oracle leg (checker + CPU baseline)
def injected_encodings():
    """the 2 ZIP-216 non-canonical encodings (reference src/lib.rs:1894-1907) and the 8 small-order encodings, as bytes"""
    from oracle import jubjub_ref as J

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
    enc = [bytes(e) for e in g["zip216_noncanonical"]["encodings"]]
    for p in g["EIGHT_TORSION_raw"]["points"]:
        pt = (sum(int(h, 16) << (64 * i) for i, h in enumerate(p["u"])) % J.Q, sum(int(h, 16) << (64 * i) for i, h in enumerate(p["v"])) % J.Q)
        enc.append(J.affine_to_bytes(pt))
    return enc


def decoder_input_for(i, inj):
    from oracle import jubjub_ref as J

    if i >= INJECT_FIRST and (i - INJECT_FIRST) % INJECT_STEP == 0 and (i - INJECT_FIRST) // INJECT_STEP < len(inj):
        return inj[(i - INJECT_FIRST) // INJECT_STEP]
    if i % 16 == 15:
        return J.synth_bytes32(i, RAW_SEED)
    return J.affine_to_bytes(J.synth_point(i, POINT_SEED)[0])


def verify_sample(wl, a, lo, n, out, ok, msm_inputs, idx=None):
    """Recomputes every SAMPLE_STRIDE-th unit of rank 0's shard (or the units `idx`) with the oracle, from the unit indices alone."""
    import numpy as np

    from oracle import c_oracle as O
    from oracle import jubjub_ref as J

    b32 = lambda k: np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint8)
    pt64 = lambda p: np.concatenate([b32(p[0]), b32(p[1])])
    strided = idx is None
    idx = list(range(0, n, SAMPLE_STRIDE)) if strided else list(idx)
    if wl == "decompress":
        inj = injected_encodings()
        if strided:
            idx = sorted(set(idx) | {i - lo for i in range(INJECT_FIRST, INJECT_FIRST + INJECT_STEP * len(inj), INJECT_STEP) if lo <= i < lo + n})
        enc = np.stack([np.frombuffer(decoder_input_for(lo + i, inj), dtype=np.uint8) for i in idx])
        eo, ek = O.decompress(enc, a.decompress_flags)
        if FAULT:
            eo = eo.copy(); eo.reshape(-1)[0] ^= 1
        got_o, got_k = out[idx].cpu().numpy(), ok[idx].cpu().numpy()
        return bool((got_k == ek).all() and (got_o == eo).all()), len(idx)
    if wl == "msm":
        # the whole shard: the oracle's OpenMP MSM over the terms rank 0 reduced (inputs copied back once, outside the timed region)
        s, p = msm_inputs
        # up to 2^18 terms: the fold of ladders (the reference's own semantics); above: the bucket method of the same oracle library (equal
        # to the fold for every window width: tests/test_oracle_c.py), which keeps a 2^22-term check to seconds
        want = O.msm(s.cpu().numpy(), p.cpu().numpy()) if s.shape[0] <= (1 << 18) else O.msm_pippenger(s.cpu().numpy(), p.cpu().numpy(), 13)
        if FAULT:
            want = want.copy(); want.reshape(-1)[0] ^= 1
        got = out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)
        return bool((got.reshape(64) == want.reshape(64)).all()), int(s.shape[0])
    scal = np.stack([b32(J.synth_scalar(lo + i, SEED)) for i in idx])
    if wl == "fixedbase":
        want = O.fixedbase_mul(scal, pt64((GEN_U, 11)))
    else:
        pts = np.stack([pt64(J.synth_point(lo + i, POINT_SEED)[0]) for i in idx])
        want = O.varbase_mul(scal, pts)
    if a.compressed:
        want = O.compress(want)
    if FAULT:
        want = want.copy(); want.reshape(-1)[0] ^= 1
    return bool((out[idx].cpu().numpy() == want).all()), len(idx)


def cpu_info():
    model, n_logical = "unknown", os.cpu_count() or 1
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    try:
        affinity = len(os.sched_getaffinity(0))
    except Exception:
        affinity = n_logical
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    return {"model": model, "logical_cpus": n_logical, "affinity": affinity, "cgroup_cpu_quota": quota}


def cpu_baseline(workload, target_s):
    """Times the oracle's C port of the reference algorithm on the host cores: one thread and all cores."""
    import ctypes

    import numpy as np

    from oracle import c_oracle as O
    from oracle import jubjub_ref as J

    omp = ctypes.CDLL("libgomp.so.1")
    omp.omp_get_max_threads.restype = ctypes.c_int
    info = cpu_info()
    # threads = the CPUs this process may actually use: the logical CPUs of its affinity mask, capped by the cgroup quota (a container
    # that sees 256 logical CPUs but is throttled to 16 runs 16 threads, not 128 or 256)
    effective = min(info["affinity"], int(-(-info["cgroup_cpu_quota"] // 1)) if info["cgroup_cpu_quota"] else info["affinity"])
    all_threads = max(1, min(int(omp.omp_get_max_threads()), effective))
    base = np.frombuffer(J.GENERATOR[0].to_bytes(32, "little") + J.GENERATOR[1].to_bytes(32, "little"), dtype=np.uint8)
    rng = np.random.default_rng(2024)

    def run(n):
        s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        s[:, 31] &= 0x0F
        if workload == "fixedbase":
            t0 = time.perf_counter(); O.fixedbase_mul(s, base); return time.perf_counter() - t0
        pts = O.fixedbase_mul(s[::-1].copy(), base)
        if workload == "decompress":
            enc = O.compress(pts)
            t0 = time.perf_counter(); O.decompress(enc, 1); return time.perf_counter() - t0
        if workload == "msm":
            t0 = time.perf_counter(); O.msm(s, pts); return time.perf_counter() - t0
        t0 = time.perf_counter(); O.varbase_mul(s, pts); return time.perf_counter() - t0

    def measure(threads, seconds):
        omp.omp_set_num_threads(threads)
        probe = max(32, 16 * threads)
        t = run(probe)                                                  # warm-up + first calibration
        n = int(max(probe, min(1 << 18, probe * 1.0 / max(t, 1e-6))))   # ~1 s sample for a stable rate estimate
        t = run(n)
        n = int(max(probe, min(1 << 22, n * seconds / max(t, 1e-6))))   # the reported sample: ~`seconds` of wall time
        t = run(n)
        return n / t, n, t

    one, n1, t1 = measure(1, min(target_s, 4.0))
    allc, na, ta = measure(all_threads, target_s)
    res = {"value": allc, "unit": UNIT[workload], "cores": all_threads, "threads": all_threads, "effective_cpus": effective, "kind": "port",
           "single_thread": {"value": one, "sample_units": n1, "seconds": t1},
           "all_cores": {"value": allc, "threads": all_threads, "sample_units": na, "seconds": ta, "speedup_over_one_thread": allc / one},
           "cpu": info,
           "sample": "%d units (%d threads) / %d units (one thread) of the same synthetic workload, reference algorithm (exact 252-step ladder / "
                     "per-point decode), oracle/jubjub_oracle.c -O3 + OpenMP" % (na, all_threads, n1),
           "note": "threads = cores = the CPUs this process can really use: min(affinity mask, cgroup CPU quota), NOT the logical CPUs the box "
                   "shows (`cpu.logical_cpus`); the rate is this container's, not the whole host's"}
    if workload == "msm":
        # the bucket method on the CPU beside the naive fold of ladders (the reference's own semantics, lib.rs:183-193)
        workload = "msm_pippenger"
        omp.omp_set_num_threads(all_threads)
        n = 1 << 20
        s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        s[:, 31] &= 0x0F
        small = O.fixedbase_mul(s[:4096][::-1].copy(), base)
        pts = np.ascontiguousarray(small[np.arange(n) % 4096])           # 2^20 terms over 4096 distinct points: the bucket method does not care
        t0 = time.perf_counter(); O.msm_pippenger(s, pts, 13); tp = time.perf_counter() - t0
        res["pippenger"] = {"value": n / tp, "unit": "terms/s", "threads": all_threads, "terms": n, "seconds": tp, "window_bits": 13,
                            "note": "oracle/jubjub_oracle.c jjo_msm_pippenger: unsigned 13-bit windows, one bucket array per window, windows in parallel; "
                                    "the reference itself has no MSM algorithm (its Sum is the fold measured as `value`)"}
    omp.omp_set_num_threads(all_threads)
    return res


# ------------------------------------------------------------------------------------------------ one rank
def run(a):
    import numpy as np
    import torch
    import torch.distributed as dist

    from jubjub_amd import Engine
    from jubjub_amd.dist import shard_bounds

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1 or os.environ.get("JJ_BENCH_FORCE_DIST") == "1"   # the latter: 1-rank RCCL plumbing check
    dev_index = int(os.environ.get("JJ_BENCH_FORCE_DEVICE", local_rank))      # plumbing tests: several ranks on one GPU
    dev = torch.device("cuda", dev_index)
    torch.cuda.set_device(dev)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:                    # 1-rank plumbing runs without a launcher: any free port
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        os.environ.setdefault("RANK", str(rank))
        os.environ.setdefault("WORLD_SIZE", str(world))
        if a.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=a.backend)
    n_gpus = world
    if a.gpus != n_gpus:
        if rank == 0:
            print("bench.py: --gpus %d but the launcher started %d rank(s); refusing to mislabel the run" % (a.gpus, world), file=sys.stderr)
        return 2
    ctx_options = {kv.split("=", 1)[0]: int(kv.split("=", 1)[1]) for kv in a.opt}
    eng = Engine(dev_index, options=ctx_options)

    wl = a.workload
    log2n = a.log2n if a.log2n is not None else DEFAULT_LOG2N[wl]
    total = (1 << log2n) * (n_gpus if a.scaling == "weak" else 1)
    by_window = wl == "msm" and a.msm_partition == "window" and n_gpus > 1
    if by_window and a.scaling != "strong":
        if rank == 0:
            print("bench.py: --msm-partition window cuts ONE batch by windows: use it with --scaling strong", file=sys.stderr)
        return 2
    lo, hi = (0, total) if by_window else shard_bounds(total, rank, n_gpus)     # window partition: every rank holds the whole batch
    n = hi - lo
    passes = a.passes or PASSES[wl]

    # ---- synthetic inputs, generated on the device from the global unit indices, resident in HBM before the timed region
    scalars = eng.synth_scalars(n, SEED, lo, device=dev)
    base = torch.from_numpy(np.frombuffer(GEN_U.to_bytes(32, "little") + (11).to_bytes(32, "little"), dtype=np.uint8).copy()).to(dev)
    table = eng.fixedbase_table(base, a.fb_window)
    points = enc = None
    if wl in ("varbase", "msm", "decompress"):
        points = eng.random_points(n, POINT_SEED, lo, subgroup=False, device=dev)   # Group::random: points of the full group (order 8r)
        assert bool(eng.predicate("is_on_curve", points[:4096]).all())
    if wl == "decompress":
        # 15/16 valid encodings, 1/16 raw PRNG bytes (off-curve, >= q, sign noise), edge encodings injected at fixed indices
        enc = eng.compress(points)
        raw = eng.synth_bytes32(n, RAW_SEED, lo, device=dev)
        gi = torch.arange(lo, hi, device=dev)
        m = (gi % 16) == 15
        enc[m] = raw[m]
        if True:
            g = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
            zip216 = [bytes(e) for e in g["zip216_noncanonical"]["encodings"]]
            tors = np.array([[b for b in (sum(int(h, 16) << (64 * i) for i, h in enumerate(p[c])) % (1 << 256)).to_bytes(32, "little")]
                             for p in g["EIGHT_TORSION_raw"]["points"] for c in ("u", "v")], dtype=np.uint8).reshape(8, 64)
            tors_enc = eng.compress(torch.from_numpy(tors).to(dev))
            inj = torch.cat([torch.tensor([list(z) for z in zip216], dtype=torch.uint8, device=dev), tors_enc])
            for k in range(inj.shape[0]):
                gidx = INJECT_FIRST + INJECT_STEP * k
                if lo <= gidx < hi:
                    enc[gidx - lo] = inj[k]
        points = None

    rccl_comm = None
    exchange_fallback = None
    if wl == "msm" and distributed and a.backend == "nccl" and a.msm_exchange == "c":
        # the exchange behind the C ABI on a communicator of this process's own.  It is set up and TRIED ONCE on a small slice against the
        # torch.distributed exchange of the same records; if any rank fails (library, communicator, the all-gather itself) or the two disagree,
        # EVERY rank falls back to --msm-exchange torch and the line says why ("msm_exchange_fallback"): the run still has to verify.
        from jubjub_amd.dist import RcclComm

        err = None
        try:
            if os.environ.get("JJ_BENCH_BREAK_C_EXCHANGE") == str(rank):       # tests: this rank's set-up fails
                raise RuntimeError("JJ_BENCH_BREAK_C_EXCHANGE")
            rccl_comm = RcclComm(rank, world)      # the ncclUniqueId travels over torch.distributed; a rank that cannot load RCCL fails all of them
            eng.set_comm(rccl_comm)
        except Exception as e:                     # noqa: BLE001 -- whatever went wrong is the reason recorded
            err = "%s: %s" % (type(e).__name__, e)
        every = [None] * world
        dist.all_gather_object(every, err)
        if not any(every):
            k = min(n, 4096)
            try:
                got = np.asarray(eng.msm_allgather(scalars[:k], points[:k], "window" if by_window else "terms")).tobytes()
                rec = eng.msm_partial(scalars[:k], points[:k], rank, world) if by_window else eng.msm_partial(scalars[:k], points[:k])
                recs = [torch.empty_like(rec) for _ in range(world)]
                dist.all_gather(recs, rec)
                want = np.asarray(eng.msm_combine(torch.stack(recs))).tobytes()
                if got != want:
                    err = "trial MSM over the C exchange differs from the torch.distributed exchange"
            except Exception as e:                 # noqa: BLE001
                err = "%s: %s" % (type(e).__name__, e)
            dist.all_gather_object(every, err)
        bad = [(r, e) for r, e in enumerate(every) if e]
        if bad:
            exchange_fallback = "rank %d: %s" % bad[0]
            if rccl_comm is not None:
                eng.set_comm(None)
                rccl_comm = None                   # (not destroyed: ncclCommDestroy of a half-working communicator may itself wait for the others)
            if rank == 0:
                print("bench.py: C-level MSM exchange unavailable (%s); falling back to --msm-exchange torch" % exchange_fallback, file=sys.stderr)
    host = a.host_buffers
    if host and (distributed or (wl == "msm" and (host in ("fresh", "pooled") or a.msm_async > 1 or a.msm_contexts > 1))):
        if rank == 0:
            print("bench.py: --host-buffers covers one GPU (msm: pinned | pageable, synchronous jj_msm calls: the result is 64 bytes, there is no result array to be fresh)", file=sys.stderr)
        return 2
    out_w = 32 if (a.compressed and wl in ("varbase", "fixedbase")) else 64
    if host:
        # the caller's side of the boundary: inputs in host memory, result buffers allocated ONCE and reused by every pass
        halloc = eng.host_alloc if host == "pinned" else (lambda shape: np.empty(shape, np.uint8))

        def to_host(t):
            h = halloc(tuple(t.shape))
            h[...] = t.cpu().numpy()
            return h

        h_scalars = to_host(scalars) if wl in ("varbase", "fixedbase", "msm") else None
        h_points = to_host(points) if wl in ("varbase", "msm") else None
        h_enc = to_host(enc) if wl == "decompress" else None
        if host == "pooled":
            # the caller returns a NEW result object per call (-> Vec): result buffers come from the library's pool (jj_result_acquire), the previous
            # call's buffer is given back only AFTER the next one was acquired, so consecutive calls never write into the same object
            h_out, h_ok = None, None
        else:
            h_out = halloc((n, out_w) if wl != "msm" else (64,))
            h_ok = halloc((n,)) if wl == "decompress" else None
            h_out[...] = 0                                            # touched once (a fresh pageable result buffer would be faulted in inside the first call)
            if h_ok is not None:
                h_ok[...] = 0

    def one_pass_device():
        if wl == "varbase":
            return eng.varbase_mul_compressed(scalars, points) if a.compressed else eng.varbase_mul(scalars, points)
        if wl == "fixedbase":
            return eng.fixedbase_mul_compressed(table, scalars) if a.compressed else eng.fixedbase_mul(table, scalars)
        if wl == "msm":
            return eng.msm(scalars, points)
        return eng.decompress(enc, a.decompress_flags)

    call_s = [0.0]                                                 # host-buffer modes: time spent inside the C-ABI calls themselves

    def one_pass():
        nonlocal h_out, h_ok
        if host == "fresh":
            h_out = None; h_ok = None                              # (the previous result array itself is released when the caller drops it: `out = step()`)
            h_out = np.empty((n, out_w), np.uint8)
            h_ok = np.empty((n,), np.uint8) if wl == "decompress" else None
        if host == "pooled":
            prev = (h_out, h_ok)
            h_out = eng.result_acquire((n, out_w))                 # a DIFFERENT buffer than the one the previous call filled (that one is still out)
            h_ok = eng.result_acquire((n,)) if wl == "decompress" else None
            assert prev[0] is None or prev[0].ctypes.data != h_out.ctypes.data
            eng.result_release(prev[0]); eng.result_release(prev[1])    # the caller has consumed (converted / copied) the previous result by now
        if host:
            tc = time.perf_counter()
            if wl == "varbase":
                r = (eng.varbase_mul_compressed if a.compressed else eng.varbase_mul)(h_scalars, h_points, out=h_out)
            elif wl == "fixedbase":
                r = (eng.fixedbase_mul_compressed if a.compressed else eng.fixedbase_mul)(table, h_scalars, out=h_out)
            elif wl == "msm":
                r = eng.msm(h_scalars, h_points)                   # 96 bytes per term in, 64 bytes out: passes of the terms, copies beside the kernels
                h_out[...] = r
            else:
                r = eng.decompress(h_enc, a.decompress_flags, out=(h_out, h_ok))
            call_s[0] += time.perf_counter() - tc
            return r
        if wl != "msm":
            return one_pass_device()
        if not distributed:
            return eng.msm(scalars, points)
        if rccl_comm is not None:
            # the whole exchange behind ONE C-ABI call: record -> ncclAllGather (RCCL over xGMI) -> one D2H -> one host tail
            return eng.msm_allgather(scalars, points, "window" if by_window else "terms")
        # every rank: its record of window sums (8 KB, stays on the device), all_gather, ONE copy to the host, ONE host tail
        rec = eng.msm_partial(scalars, points, rank, world) if by_window else eng.msm_partial(scalars, points)
        if a.backend == "nccl":
            recs = [torch.empty_like(rec) for _ in range(world)]
            dist.all_gather(recs, rec)                          # RCCL over xGMI; EC addition is not a reduce op
            return eng.msm_combine(torch.stack(recs))
        recs = [torch.empty(rec.shape, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(recs, rec.cpu())
        return eng.msm_combine(torch.stack(recs))

    # --msm-contexts K: K engines on this GPU, each driven by its own host thread on its own torch stream
    msm_engs = [eng]
    if wl == "msm" and not distributed and a.msm_contexts > 1:
        import threading

        msm_engs += [Engine(dev_index, options=ctx_options) for _ in range(a.msm_contexts - 1)]
        msm_streams = [torch.cuda.Stream(dev) for _ in msm_engs]

    def msm_series(e, count):
        """`count` MSMs on engine e, --msm-async jobs in flight; returns the last point"""
        o, pend = None, []
        for _ in range(count):
            if a.msm_async > 1:
                pend.append(e.msm_begin(scalars, points))
                if len(pend) == a.msm_async:
                    o = e.msm_finish(pend.pop(0))
            else:
                o = e.msm(scalars, points)
        for j in pend:
            o = e.msm_finish(j)
        return o

    def step():
        o = None
        if len(msm_engs) > 1:
            K = len(msm_engs)
            outs = [None] * K

            def work(i):
                with torch.cuda.stream(msm_streams[i]):
                    outs[i] = msm_series(msm_engs[i], passes // K + (1 if i < passes % K else 0))
                msm_streams[i].synchronize()

            torch.cuda.synchronize(dev)
            th = [threading.Thread(target=work, args=(i,)) for i in range(K)]
            [t.start() for t in th]
            [t.join() for t in th]
            return outs[0]
        if wl == "msm" and a.msm_async > 1 and (not distributed or rccl_comm is not None):
            pend = []                                           # a sliding window of jobs: begin the next before finishing the oldest
            begin = eng.msm_begin if not distributed else (lambda s_, p_: eng.msm_allgather_begin(s_, p_, "window" if by_window else "terms"))
            for _ in range(passes):                             # (distributed: jj_msm_allgather_begin -- every rank begins the same jobs in the same order)
                pend.append(begin(scalars, points))
                if len(pend) == a.msm_async:
                    o = eng.msm_finish(pend.pop(0))
            for j in pend:
                o = eng.msm_finish(j)
            return o
        for _ in range(passes):
            o = one_pass()
        return o

    def barrier():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(a.warmup):
        step()
    peak_before = eng.peak_imad32_samples(5) if rank == 0 else None     # the roofline denominator, sampled on both sides of the timed region
    barrier()
    eng.profile(True)
    call_s[0] = 0.0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    torch.cuda.synchronize(dev)
    t_own = time.perf_counter() - t0                                    # this rank's own work done (device drained), before it waits for the others
    call_in_timed = call_s[0]
    barrier()
    dt = time.perf_counter() - t0
    main_ms, tail_ms = eng.profile_read()
    eng.profile(False)
    peak_after = eng.peak_imad32_samples(5) if rank == 0 else None
    rank_ms = [t_own / a.steps * 1e3]
    if distributed:
        tcpu = "cpu" if a.backend != "nccl" else dev
        tmax = torch.tensor([dt], dtype=torch.float64, device=tcpu)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        mine = torch.tensor([t_own / a.steps * 1e3], dtype=torch.float64, device=tcpu)
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        rank_ms = [float(t.item()) for t in every]

    # a second, untimed pass over the same inputs on EVERY rank (the MSM's pass holds a collective): rank 0 compares all its units
    # with the timed output below
    dev_ref = None
    if host:
        # the timed output lives in host arrays: bring it back to the device for the checks below, and time the same entry point on
        # device-resident tensors in this process (the ratio host / device-resident is what the pipelining is judged by)
        out = torch.from_numpy(np.array(h_out)).to(dev)
        if wl == "decompress":
            out = (out, torch.from_numpy(np.array(h_ok)).to(dev))
        one_pass_device(); torch.cuda.synchronize(dev)
        eng.profile(True)
        t1 = time.perf_counter()
        for _ in range(2):
            o_dev = one_pass_device()
        torch.cuda.synchronize(dev)
        ddt = (time.perf_counter() - t1) / 2
        main_ms, tail_ms = eng.profile_read()
        eng.profile(False)
        dev_ref = {"value": n / ddt, "unit": UNIT[wl], "ms_per_pass": ddt * 1e3}
        del o_dev
        out2 = None if a.no_verify else one_pass_device()         # the independent second pass runs device-resident
    else:
        out2 = None if a.no_verify else one_pass()
    units_per_step = total * passes
    value = units_per_step * a.steps / dt
    res = {
        "metric": ("Jubjub scalar-muls/sec (%s)" % wl if wl in ("varbase", "fixedbase") else "Jubjub %s units/sec" % wl) +
                  (" -- C ABI on HOST buffers (%s), PCIe-inclusive: not the headline value" % host if host else ""),
        "value": value, "unit": UNIT[wl],
        "n_gpus": n_gpus, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": dt / a.steps * 1e3,
        "higher_is_better": True, "scaling": a.scaling, "vs_baseline": None,
        "dtype": "i32x9 (signed 29-bit limbs, v_mad_i64_i32 integer multiply-add)",
        "data": "synthetic",
        "config": {"workload": "%s, 2^%d units %s, %d passes per step (BASELINE.json configs[%d])" % (
            wl, log2n, "per GPU" if a.scaling == "weak" else "in total over %d GPU(s)" % n_gpus, passes, {"varbase": 1, "fixedbase": 2, "msm": 3, "decompress": 4}[wl]),
            "units_per_step": units_per_step, "passes_per_step": passes, "ms_per_pass": dt / a.steps / passes * 1e3,
            "scalars": "jj_synth_scalars: canonical Fr from splitmix64(seed + 4 i + j)", "points": "jj_random_points: Group::random rejection sampling (full group, order 8r), affine 64 B",
            "parallelism": ("window partition: rank g owns windows g, g + G, ... of all terms" if by_window else "contiguous shards, one process per GPU") +
                           ("; all_gather of one 8 KB record of window sums per rank (%s%s), one host tail" % (a.backend, ", behind the C ABI: jj_msm_allgather on this process's own RCCL communicator" if rccl_comm is not None else "") if wl == "msm" else "; no data-path collective")},
        "rccl_world_size": dist.get_world_size() if distributed else 1,
        "msm_exchange_fallback": exchange_fallback,
        # each rank's own time per step before the closing barrier (ms_per_step is the max over ranks, barrier included): stragglers show here
        "rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms), "per_rank": rank_ms},
    }
    if a.dump_outputs and rank == 0:
        res["dump_outputs"] = dump_outputs(a.dump_outputs, out)          # the last timed step's output (host modes: as copied back above)
    if host:
        res["pcie_inclusive"] = True
        res["config"]["host_buffers"] = {"pinned": "page-locked (jj_host_alloc), reused by every pass",
                                         "pageable": "pageable numpy memory, reused by every pass; the chunks pass through the context's page-locked staging slots (bounce path; --opt pipe_pageable_register=1: arrays that consist of whole pages are page-locked in place instead)",
                                         "pooled": "inputs: pageable numpy memory, reused; RESULT: a different page-locked buffer from the library's pool for every call (jj_result_acquire; the previous call's buffer is released after the next one was acquired)",
                                         "fresh": "pageable numpy memory; the RESULT array is newly allocated (np.empty) for every call: its pages are faulted in and page-locked inside the call"}[host]
        res["config"]["result_bytes"] = out_w if wl != "msm" else 64
        res["device_resident"] = dev_ref
        res["host_over_device_resident"] = value / dev_ref["value"]
    if wl == "msm" and not distributed and not host and a.msm_async <= 1 and len(msm_engs) == 1:
        # The timed region carries the HIP events the roofline's kernel_ms comes from: three hipEventRecord per call, which a 0.1-0.4 ms call feels.
        # The same synchronous call without them, after the timed region (not `value`): what a caller of jj_msm sees.
        one_pass(); torch.cuda.synchronize(dev)
        reps = max(8, min(passes * a.steps, 200))
        ts = []
        for _ in range(reps):
            t1 = time.perf_counter(); one_pass(); ts.append(time.perf_counter() - t1)
        torch.cuda.synchronize(dev)
        ts.sort()
        res["config"]["ms_per_call_without_events"] = {"median": ts[len(ts) // 2] * 1e3, "min": ts[0] * 1e3, "calls": reps,
                                                        "note": "jj_msm on the same device-resident inputs, profiling events off, wall time of each call through the Python mirror (host tail done when it returns; the 64 result bytes go to a new device tensor by a queued copy)"}
    if wl == "msm":
        res["config"]["msm_partition"] = a.msm_partition if n_gpus > 1 else None
        res["config"]["msm_jobs_in_flight"] = a.msm_async if (not distributed or rccl_comm is not None) else 1
        res["config"]["msm_contexts"] = len(msm_engs)
    rc = 0
    if rank == 0:
        w = dict(WORK[wl])
        if wl == "msm":
            # field operations of the algorithm this run used, from the window count W of a record (small batches: W = 64, per-term
            # table of 8 entries (7 x 9M) + W mixed-form additions of 8M; Pippenger: W additions of 7M + 2 x 9M per bucket)
            hdr = eng.msm_partial(scalars[: min(n, 1 << 24)], points[: min(n, 1 << 24)])[:16].cpu().numpy().view("<u4")
            W = int(hdr[2])
            if W == 64:
                w["M"] = 2 + 2 + 7 * 9 + W * 8
            else:
                c_, r_ = divmod(253, W)
                buckets = r_ * (1 << c_) + (W - r_) * (1 << (c_ - 1))
                w["M"] = 2 + 2 + W * 7 + -(-(buckets * 18) // n)
            res["config"]["msm_windows"] = W
        if wl == "fixedbase" and a.fb_window >= 8:
            w["S"], w["M"] = 0, -(-253 // a.fb_window) * 7   # ceil(253/w) mixed additions
        if wl == "fixedbase" and a.fb_window == 6:
            w["S"], w["M"] = 0, 43 * 7
        if main_ms and len(msm_engs) == 1:
            kern_ms = sum(main_ms) / len(main_ms)
            tail = sum(tail_ms) / len(tail_ms)
        else:                                                       # workloads without the event hooks: whole pass
            kern_ms, tail = dt / a.steps / passes * 1e3, 0.0
        samples = sorted(peak_before + peak_after)
        peak = samples[len(samples) // 2]                       # median of the 10 samples taken before and after the timed region
        work_main = imad32(w["S"], w["M"])
        achieved = n * work_main / (kern_ms * 1e-3)
        traffic, traffic_note = traffic_record(wl, log2n)
        tail_s, tail_m = tail_work(wl, n)
        res["roofline"] = {
            "bound": "valu_int32", "achieved": achieved / 1e12, "peak": peak / 1e12, "unit": "TIMAD32/s",
            "frac": achieved / peak,
            # the denominator: median of 5 + 5 single measurements (before / after the timed region) and their spread; frac_nominal uses the
            # data-sheet ceiling instead (1024 SIMDs x 16 lanes x 2.4 GHz), which no sustained integer load reaches on this part
            "peak_samples": {"before": [x / 1e12 for x in peak_before], "after": [x / 1e12 for x in peak_after], "median": peak / 1e12,
                             "min": samples[0] / 1e12, "max": samples[-1] / 1e12, "spread": (samples[-1] - samples[0]) / peak},
            # which peak `frac` uses, and why it is 10 % under the data-sheet product (round 6, profiles/r6_peak_clock.txt + r6_mad_banks.txt: one rocprofv3
            # pass with GRBM_GUI_ACTIVE / SQ_INSTS_VALU over k_peak_mad and k_varbase_ct3 in one process)
            "peak_kind": "measured: median of 5 + 5 launches of k_peak_mad (a pure v_mad_u64_u32 stream, 8 waves per SIMD) around the timed region; frac_nominal = the same work over 1024 SIMDs x 16 lanes x 2.4 GHz",
            "peak_attribution": "measured / nominal ~ 0.90 = clock 2.25-2.27 GHz of 2.4 under this load (0.94) x one multiply-add per 4.35 cycles per SIMD instead of 4 (0.92; independent of VGPR banks, operand kind and signedness; 5.2 cycles for a lone wave per SIMD, 4.4 for two); the ladder itself issues one VALU instruction per 4.08 cycles at 2.26 GHz",
            "frac_at_peak_max": achieved / samples[-1], "frac_at_peak_min": achieved / samples[0],
            "peak_nominal": NOMINAL_PEAK_IMAD32 / 1e12, "frac_nominal": achieved / NOMINAL_PEAK_IMAD32,
            "frac_min": (n * work_main / (min(main_ms) * 1e-3) / peak) if main_ms and len(msm_engs) == 1 else None,     # the fastest dispatch of the timed region
            # multiply-adds actually issued by the signed 9x29-bit representation (153 per mul, 117 per square) / measured peak
            "mad_issue_frac": n * (153 * w["M"] + 117 * w["S"]) / (kern_ms * 1e-3) / peak,
            "traffic": traffic["bytes_per_launch"] if traffic else None,
            "traffic_detail": traffic if traffic else traffic_note,
            "kernel": {"varbase": "k_varbase_ct3", "fixedbase": ("k_fixedbase_comb" if a.fb_window in (0, 7) else "k_fixedbase") if a.fb_window < 8 else "k_fixedbase_gather(w=%d)" % a.fb_window, "msm": "whole MSM: k_msm_accumulate(_seg) + sort / fix-up / reduce; Horner on the host", "decompress": "k_decompress"}[wl],
            "kernel_ms": kern_ms, "tail_ms": tail, "units_per_launch": n,
            "work_per_unit": {"field_squares": w["S"], "field_muls": w["M"], "imad32": work_main, "convention": "M=128,S=100 (SURVEY 8d); the kernel named above only",
                              "tail_kernel": {"field_squares": tail_s, "field_muls": tail_m, "imad32": imad32(tail_s, tail_m)}},
            "whole_pass_frac": n * (work_main + imad32(tail_s, tail_m)) / ((kern_ms + tail) * 1e-3) / peak,
            "reference_algorithm_imad32": imad32(REFERENCE_WORK[wl]["S"], REFERENCE_WORK[wl]["M"]) if wl in REFERENCE_WORK else None,
            "hbm": {"achieved": n * w["bytes"] / (kern_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": n * w["bytes"] / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, "bytes_per_unit": w["bytes"]},
            "build_id": build_id(),
        }
        if host:
            in_b = {"varbase": 96, "fixedbase": 32, "decompress": 32, "msm": 96}[wl]
            out_b = (out_w + (1 if wl == "decompress" else 0)) if wl != "msm" else 64.0 / n
            per_pass = dt / a.steps / passes
            h2d, d2h = n * in_b / per_pass / 1e9, n * out_b / per_pass / 1e9
            res["roofline"]["note"] = "kernel_ms / frac: the same entry point on device-resident tensors in this process (2 passes after the timed region)"
            res["roofline"]["pcie"] = {
                "bound": "pcie", "link": "PCIe Gen5 x16: 63 GB/s per direction (32 GT/s x 16 lanes, 128b/130b), full duplex",
                "bytes_per_unit": {"h2d": in_b, "d2h": out_b}, "h2d_GBps": h2d, "d2h_GBps": d2h, "peak_GBps": PCIE_PEAK_GBPS,
                "frac": max(h2d, d2h) / PCIE_PEAK_GBPS, "frac_h2d": h2d / PCIE_PEAK_GBPS, "frac_d2h": d2h / PCIE_PEAK_GBPS,
                "link_bound_units_per_s": PCIE_PEAK_GBPS * 1e9 / max(in_b, out_b),
                "kernel_bound_units_per_s": dev_ref["value"],
                "ms_per_pass": per_pass * 1e3,
                # the time inside the C-ABI calls alone, and (fresh mode) what the CALLER spends per pass allocating the next result array and
                # releasing the previous one (mmap / munmap of 1 GB of touched pages: any implementation that returns a new array per call pays it)
                "call_ms_per_pass": call_in_timed / a.steps / passes * 1e3,
                "units_per_s_inside_the_call": units_per_step * a.steps / call_in_timed,
                "caller_alloc_free_ms_per_pass": (dt - call_in_timed) / a.steps / passes * 1e3 if host == "fresh" else None,
                "bound_by": "kernels" if dev_ref["value"] < PCIE_PEAK_GBPS * 1e9 / max(in_b, out_b) else "link",
                "frac_of_min_bound": value / min(dev_ref["value"], PCIE_PEAK_GBPS * 1e9 / max(in_b, out_b)),
            }
        if wl == "msm":
            res["msm_result"] = bytes(host_bytes(out).reshape(64).tolist()).hex()     # the point every rank ends up with
        if not a.no_verify:
            o, k = (out if isinstance(out, tuple) else (out, None))
            if wl == "msm" and n_gpus > 1 and not by_window:
                # the timed output is the all-rank sum; rank 0's own shard is re-reduced and compared with the oracle here,
                # the sum of a whole multi-rank run is compared in tests/test_gpu_dist.py
                o = eng.msm(scalars, points)
                res["verified_note"] = "rank 0's shard vs the oracle (the all-rank sum is checked by tests/test_gpu_dist.py)"
            okv, cnt = verify_sample(wl, a, lo, n, o, k, (scalars, points))
            res["verified"], res["verified_units"] = okv, cnt
            if wl != "msm":
                # one CONTIGUOUS block of 2^14 units (256 whole waves) recomputed by the oracle as well: a defect tied to a lane, wave or
                # workgroup position that a stride-1024 sample can step over shows here
                bn = min(n, 1 << BLOCK_LOG2)
                b0 = ((n // 2) // bn) * bn if n >= 2 * bn else 0
                okb, cntb = verify_sample(wl, a, lo, n, o, k, None, idx=range(b0, b0 + bn))
                res["verified_block"] = {"ok": okb, "first_unit": lo + b0, "units": cntb}
                okv = okv and okb
            # every unit of the timed output against a fresh pass over the same inputs, compared on the device (the oracle sample
            # above checks one unit in 2^10; this ties all the others to a second, independent run)
            o2v, k2 = (out2 if isinstance(out2, tuple) else (out2, None))
            if wl == "msm":
                same = bool((host_bytes(out) == host_bytes(o2v)).all())
            else:
                same = bool(torch.equal(o, o2v)) and (k2 is None or bool(torch.equal(k, k2)))
            res["all_units_equal_second_pass"] = same
            if not (okv and same):
                rc = 3
        if wl == "varbase" and not a.no_extras and n_gpus == 1 and not host:
            # the other half of BASELINE.json's metric at ITS config (2^24 fixed-base scalar-muls), same process, outside the timed region above
            fn = 1 << 24
            fs = eng.synth_scalars(fn, SEED, 0, device=dev)
            fo = None
            for _ in range(2):                                      # warm-up: the 1 GB output and the library's workspaces get allocated here
                fo = None
                fo = eng.fixedbase_mul(table, fs)
            torch.cuda.synchronize(dev)
            eng.profile(True)
            t1 = time.perf_counter()
            for _ in range(4):
                fo = None                                           # release the previous 1 GB output to torch's caching allocator first
                fo = eng.fixedbase_mul(table, fs)
            torch.cuda.synchronize(dev)
            fdt = (time.perf_counter() - t1) / 4
            fm, _ft = eng.profile_read()
            eng.profile(False)
            fw = WORK["fixedbase"]
            fkm = sum(fm) / max(len(fm), 1)
            res["fixed_base"] = {"value": fn / fdt, "unit": "scalar-muls/s per GPU", "units_per_pass": fn, "ms_per_pass": fdt * 1e3, "kernel_ms": fkm,
                                 "roofline_frac": fn * imad32(fw["S"], fw["M"]) / (fkm * 1e-3) / peak,
                                 "window_select": "signed comb (8 teeth, 8 column blocks: 32 additions + 3 doublings), 140 KiB table staged in LDS, ds_bpermute constant-time select"}
            if not a.no_verify:
                res["fixed_base"]["verified"], _ = verify_sample("fixedbase", a, 0, fn, fo, None, None)
            wt = eng.fixedbase_table(base, 16)                      # wide-window alternative (64 MB table in the Infinity Cache, per-lane gather)
            for _ in range(2):
                fo = None
                fo = eng.fixedbase_mul(wt, fs)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(4):
                fo = None
                fo = eng.fixedbase_mul(wt, fs)
            torch.cuda.synchronize(dev)
            res["fixed_base_wide_window"] = {"value": fn * 4 / (time.perf_counter() - t1), "unit": "scalar-muls/s per GPU", "units_per_pass": fn,
                                              "window_bits": 16, "table": "64 MB (one 128-byte line per entry), Infinity-Cache resident, variable-time gather: 16 additions per scalar"}
            if not a.no_verify:
                res["fixed_base_wide_window"]["verified"], _ = verify_sample("fixedbase", a, 0, fn, fo, None, None)
            wt.close()
            del fs, fo
        if wl == "varbase" and not a.no_extras and n_gpus == 1 and not host:
            # the variable-time ladder (jj_varbase_mul_vartime: per-lane window table in memory, signed 5-bit windows, digit-dependent addresses) on the same batch
            for _ in range(2):
                co = eng.varbase_mul_vartime(scalars, points)
            torch.cuda.synchronize(dev)
            eng.profile(True)
            t1 = time.perf_counter()
            for _ in range(4):
                co = eng.varbase_mul_vartime(scalars, points)
            torch.cuda.synchronize(dev)
            cdt = (time.perf_counter() - t1) / 4
            cm, _ct = eng.profile_read()
            eng.profile(False)
            ckm = sum(cm) / max(len(cm), 1)
            cw = WORK_VARTIME
            res["varbase_vartime"] = {"value": n / cdt, "unit": "scalar-muls/s per GPU", "units_per_pass": n, "ms_per_pass": cdt * 1e3, "kernel_ms": ckm, "kernel": "k_varbase",
                                      "roofline_frac": n * imad32(cw["S"], cw["M"]) / (ckm * 1e-3) / peak, "work_per_unit": cw,
                                      "relative_to_default": (n / cdt) / value,
                                      "note": "jj_varbase_mul_vartime: the window table of every lane lives in memory and is read at a digit-dependent address (rounds 1-4's default); for public scalars"}
            if not a.no_verify:
                res["varbase_vartime"]["verified"], _ = verify_sample("varbase", a, lo, n, co, None, None)
                res["varbase_vartime"]["equals_default_ladder_all_units"] = bool(torch.equal(co, out))
            res["value_vartime"] = n / cdt
        if wl == "varbase":
            # the headline IS the constant-time ladder: jj_varbase_mul has no scalar-dependent address or branch (the reference's conditional_select
            # discipline, src/lib.rs:334-343, 357-379)
            res["value_constant_time"] = res["value"]
        if not a.no_cpu_baseline and n_gpus == 1:
            res["cpu_baseline"] = cpu_baseline(wl, a.cpu_seconds)
        emit(json.dumps(res))
    if rccl_comm is not None:
        eng.set_comm(None)
        rccl_comm.close()
    table.close()
    for e in msm_engs[1:]:
        e.close()
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    return rc


_OUT_FD = None


def emit(line):
    """the ONE line of rank 0, written to the process's real stdout (see main)"""
    if _OUT_FD is None:
        print(line)
        sys.stdout.flush()
    else:
        os.write(_OUT_FD, (line + "\n").encode())


def main():
    global _OUT_FD
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(a))
    # Native libraries print on stdout too (RCCL writes a version banner at its first communicator, through C stdio: when stdout is a
    # pipe it surfaces at process exit, after the JSON line).  The rank keeps its real stdout for the JSON line alone and points fd 1 at
    # stderr for everything else.
    sys.stdout.flush()
    _OUT_FD = os.dup(1)
    os.dup2(2, 1)
    sys.exit(run(a))


if __name__ == "__main__":
    main()
