#!/usr/bin/env python3
"""
The kernel reach ledger: which GPU test file launches which kernel of the library (profiles/kernel_reach_ledger.json).
The ledger is a record of a trace and lives beside the other records under profiles/, where a change that adds a kernel can write it again.
tests/kernel_reach.json and tests/kernel_reach_ledger.json are the ledgers of earlier commits; they are kept as they were and no longer read.

  python tools/kernel_reach.py --trace DIR [--files test_gpu_a.py,test_gpu_b.py]     on the GPU box
      For every tests/test_gpu_*.py except test_gpu_dist.py (it only spawns bench.py ranks): one untraced pytest process, timed, then
          rocprofv3 --kernel-trace -d <dir> -o <file stem> -- python -m pytest tests/<file> -q -m gpu
      under `timeout -k 10` (three times the untraced wall time plus 60 s).  Kernel trace only: no counters, no other tracing.  The kernel
      names are read from every result database under <dir> (child processes write their own) the way tools/rocpd_summary.py reads the
      `kernels` table, and land with their dispatch counts and launch sizes in DIR/<file stem>.json.  The run stops at the first step that
      faults, aborts or runs into its limit and starts nothing more on the GPU after it; a file whose tests fail is recorded as failed.
  python tools/kernel_reach.py --ledger DIR                                          no GPU (compiles the library's assembly, ~2 minutes)
      Matches the traced names of namespace jj against the .amdhsa_kernel symbols of tools/gfx_asm.assembly() -- both brought to one form
      with one demangler (llvm-cxxfilt of the ROCm toolchain, c++filt where that is not installed), `.kd` stripped -- and writes profiles/kernel_reach_ledger.json.  A traced jj kernel that no compiled
      kernel matches is an error.
  python tools/kernel_reach.py DIR                                                   both in turn
  python tools/kernel_reach.py --add DIR                                             no GPU: a new GPU test file that adds no kernel -- the files
      traced into DIR (--trace DIR --files test_gpu_new.py) enter the committed ledger, every other file's entries and the header stay
  python tools/kernel_reach.py --add DIR --add-kernels                               no GPU: the same for a change whose new kernels only its new
      test files launch -- the compiled kernels the ledger lacks enter it first (the library's assembly is compiled, ~2 minutes)
  python tools/kernel_reach.py --check                                               no GPU: the committed ledger as a table
"""
import argparse
import datetime
import glob
import json
import os
import re
import shutil
import sqlite3
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER = os.path.join(ROOT, "profiles", "kernel_reach_ledger.json")
CXXFILT = ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt")     # the first one installed; both sides of the match go through the same one
SKIP = {"test_gpu_dist.py"}
STOP = {124: "time limit", 137: "time limit (killed)", 134: "abort", 139: "segmentation fault", -6: "abort", -11: "segmentation fault", -9: "killed"}
HEADER_KEYS = ("build_id", "commit", "cus", "date", "device", "rocm")


def gpu_files():
    return sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")) if os.path.basename(f) not in SKIP)


# ---- names -----------------------------------------------------------------------------------------------------------------------------
def demangle(names):
    names = list(names)
    if not names:
        return []
    tool = next((shutil.which(c) for c in CXXFILT if shutil.which(c)), None)
    if tool is None:
        raise RuntimeError("no demangler found (looked for %s)" % ", ".join(CXXFILT))
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names)
    return out


def canonical(name):
    """one form for a demangled kernel name: no `.kd`, no return type, no parameter list -- `jj::k_normalize<4>`, `jj::k_field_op<jj::FqP, (jj::FieldOp)2>`"""
    s = name.strip()
    if s.endswith(".kd"):
        s = s[:-3]
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):                 # the parameter list opens at the first `(` outside template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut].strip()
    depth = 0
    for i in range(len(s) - 1, -1, -1):        # the return type ends at the last blank outside template brackets
        if s[i] == ">":
            depth += 1
        elif s[i] == "<":
            depth -= 1
        elif s[i] == " " and depth == 0:
            s = s[i + 1:]
            break
    return re.sub(r"\s+", " ", s)


def canonical_all(raw):
    """raw trace or symbol names -> canonical names (mangled ones go through the demangler first)"""
    raw = [r[:-3] if r.endswith(".kd") else r for r in raw]
    idx = [i for i, r in enumerate(raw) if r.startswith("_Z")]
    for i, d in zip(idx, demangle([raw[i] for i in idx])):
        raw[i] = d
    return [canonical(r) for r in raw]


def compiled_kernels(asm=None):
    """canonical names of the .amdhsa_kernel symbols of the library's gfx950 assembly"""
    if asm is None:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from gfx_asm import assembly

        asm = assembly()
    syms = re.findall(r"\.amdhsa_kernel (\S+)", asm)
    names = canonical_all(syms)
    assert len(set(names)) == len(names), "two kernel symbols with one canonical name"
    return sorted(names)


# ---- trace (GPU box) ---------------------------------------------------------------------------------------------------------------------
def read_trace(dirname):
    """{raw kernel name: [dispatches, smallest grid_x x workgroup_x, largest]} over every result database under dirname"""
    out = {}
    dbs = sorted(glob.glob(os.path.join(dirname, "**", "*.db"), recursive=True))
    for path in dbs:
        db = sqlite3.connect(path)
        # the smallest and the largest launch by grid_x, each with its own workgroup_x
        for name, cnt in db.execute("select name, count(*) from kernels group by name").fetchall():
            lo = db.execute("select grid_x, workgroup_x from kernels where name = ? order by grid_x asc, workgroup_x asc limit 1", (name,)).fetchone()
            hi = db.execute("select grid_x, workgroup_x from kernels where name = ? order by grid_x desc, workgroup_x desc limit 1", (name,)).fetchone()
            e = out.setdefault(name, [0, list(lo), list(hi)])
            e[0] += cnt
            if lo[0] < e[1][0]:
                e[1] = list(lo)
            if hi[0] > e[2][0]:
                e[2] = list(hi)
        db.close()
    return out, len(dbs)


def device_header():
    """device name and CU count from a child process: this one starts the test processes and never opens the GPU itself"""
    code = "import json, torch; p = torch.cuda.get_device_properties(0); print(json.dumps({'device': p.name, 'cus': int(p.multi_processor_count)}))"
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout
    h = json.loads(out.strip().splitlines()[-1])
    ver = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"))), ".info", "version")
    h.update(rocm=open(ver).read().strip() if os.path.exists(ver) else "unknown", date=datetime.date.today().isoformat())
    return h


def step(cmd, limit, log):
    t0 = time.time()
    with open(log, "w") as f:
        rc = subprocess.run(["timeout", "-k", "10", str(int(limit))] + cmd, cwd=ROOT, stdout=f, stderr=subprocess.STDOUT, env=dict(os.environ, TMPDIR="/tmp")).returncode
    return rc, time.time() - t0


def faulted(rc, log):
    if rc in STOP:
        return STOP[rc]
    text = open(log, errors="replace").read()
    for needle in ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "Fatal Python error", "core dumped"):
        if needle in text:
            return needle
    return None


def trace(outdir, files, untraced_limit):
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "header.json"), "w") as f:
        json.dump(device_header(), f, indent=1, sort_keys=True)
    for name in files:
        stem = name[:-3]
        test = [sys.executable, "-m", "pytest", "tests/" + name, "-q", "-m", "gpu"]
        rc0, t_plain = step(test, untraced_limit, os.path.join(outdir, stem + ".untraced.log"))
        print("%-34s untraced %7.1f s rc %d" % (name, t_plain, rc0), flush=True)
        why = faulted(rc0, os.path.join(outdir, stem + ".untraced.log"))
        if why:
            print("STOP: %s untraced ended with %s; nothing more is started on the GPU" % (name, why), flush=True)
            return 3
        limit = 3 * t_plain + 60
        tmp = os.path.join("/tmp", "kernel_reach_%d_%s" % (os.getpid(), stem))
        shutil.rmtree(tmp, ignore_errors=True)
        rc1, t_traced = step(["rocprofv3", "--kernel-trace", "-d", tmp, "-o", stem, "--"] + test, limit, os.path.join(outdir, stem + ".traced.log"))
        print("%-34s traced   %7.1f s rc %d (limit %.0f s)" % (name, t_traced, rc1, limit), flush=True)
        why = faulted(rc1, os.path.join(outdir, stem + ".traced.log"))
        if why:
            print("STOP: %s traced ended with %s; nothing more is started on the GPU" % (name, why), flush=True)
            shutil.rmtree(tmp, ignore_errors=True)
            return 3
        kernels, ndb = read_trace(tmp)
        shutil.rmtree(tmp, ignore_errors=True)
        with open(os.path.join(outdir, stem + ".json"), "w") as f:
            json.dump({"file": name, "untraced_s": round(t_plain, 1), "traced_s": round(t_traced, 1), "untraced_rc": rc0, "traced_rc": rc1, "databases": ndb,
                       "kernels": kernels}, f, indent=1, sort_keys=True)
        print("%-34s %d databases, %d kernel names" % (name, ndb, len(kernels)), flush=True)
    return 0


# ---- ledger (no GPU) -------------------------------------------------------------------------------------------------------------------
def source_stamp():
    sys.path.insert(0, ROOT)
    import bench

    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        dirty = subprocess.run(["git", "status", "--porcelain", "--", "jubjub_amd", "tests"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
        if dirty:
            commit += " + uncommitted changes (the sources of build_id)"
    except (OSError, subprocess.CalledProcessError):
        commit = "unknown"
    return {"commit": commit, "build_id": bench.build_id()}


def build_ledger(outdir, asm=None):
    compiled = compiled_kernels(asm)
    header = json.load(open(os.path.join(outdir, "header.json")))
    header.update(source_stamp())
    kernels = {k: {"files": {}, "grid_x_by_workgroup_x": None} for k in compiled}
    times, failed, strays = {}, [], []
    for path in sorted(glob.glob(os.path.join(outdir, "test_gpu_*.json"))):
        rec = json.load(open(path))
        times[rec["file"]] = {"untraced_s": rec["untraced_s"], "traced_s": rec["traced_s"]}
        if rec["untraced_rc"] or rec["traced_rc"]:
            failed.append("%s (untraced rc %d, traced rc %d)" % (rec["file"], rec["untraced_rc"], rec["traced_rc"]))
        raws = sorted(rec["kernels"])
        for raw, name in zip(raws, canonical_all(raws)):
            if not name.startswith("jj::"):
                continue                                       # torch, RCCL, the runtime's own copy kernels
            if name not in kernels:
                strays.append("%s: %s (%s)" % (rec["file"], name, raw))
                continue
            cnt, lo, hi = rec["kernels"][raw]
            e = kernels[name]
            e["files"][rec["file"]] = e["files"].get(rec["file"], 0) + cnt
            cur = e["grid_x_by_workgroup_x"]
            e["grid_x_by_workgroup_x"] = [lo if not cur or lo[0] < cur[0][0] else cur[0], hi if not cur or hi[0] > cur[1][0] else cur[1]]
    if strays:
        raise SystemExit("traced jj kernels that match no compiled kernel:\n  " + "\n  ".join(strays))
    if failed:
        raise SystemExit("test files that did not pass while traced; the ledger is not written:\n  " + "\n  ".join(failed))
    missing = [f for f in gpu_files() if f not in times]
    if missing:
        raise SystemExit("no trace of: " + ", ".join(missing))
    for e in kernels.values():
        g = e.pop("grid_x_by_workgroup_x")
        e["smallest"], e["largest"] = ("%d x %d" % tuple(g[0]), "%d x %d" % tuple(g[1])) if g else (None, None)
    write_ledger({"header": header, "kernels": kernels, "seconds": times})
    return kernels


def add_to_ledger(outdir, new_kernels=False):
    """--add: the per-file results in outdir replace those files' entries in the committed ledger; every other file's counts, and the header of
    the full trace, stay.  For a change that adds GPU test files and, with new_kernels (--add-kernels), the kernels only they launch: a
    compiled kernel the ledger lacks enters it without a launch, and the traced files are then expected to give it one.  A name the ledger
    holds and the library no longer compiles is an error either way: that takes a trace of every file."""
    ledger = json.load(open(LEDGER))
    kernels = ledger["kernels"]
    if new_kernels:
        compiled = set(compiled_kernels())
        gone = sorted(set(kernels) - compiled)
        if gone:
            raise SystemExit("in the ledger but no longer compiled: %s: trace every file again" % ", ".join(gone))
        for name in sorted(compiled - set(kernels)):
            kernels[name] = {"files": {}, "largest": None, "smallest": None}
            print("new kernel: %s" % name)
    for path in sorted(glob.glob(os.path.join(outdir, "test_gpu_*.json"))):
        rec = json.load(open(path))
        if rec["untraced_rc"] or rec["traced_rc"]:
            raise SystemExit("%s did not pass while traced (untraced rc %d, traced rc %d); the ledger is not written" % (rec["file"], rec["untraced_rc"], rec["traced_rc"]))
        for e in kernels.values():
            e["files"].pop(rec["file"], None)
        raws = sorted(rec["kernels"])
        for raw, name in zip(raws, canonical_all(raws)):
            if not name.startswith("jj::"):
                continue
            if name not in kernels:
                raise SystemExit("%s launched %s, which the ledger does not name: trace every file again" % (rec["file"], name))
            cnt, lo, hi = rec["kernels"][raw]
            e = kernels[name]
            e["files"][rec["file"]] = e["files"].get(rec["file"], 0) + cnt
            size = lambda s: int(s.split(" x ")[0])      # noqa: E731
            if not e["smallest"] or lo[0] < size(e["smallest"]):
                e["smallest"] = "%d x %d" % tuple(lo)
            if not e["largest"] or hi[0] > size(e["largest"]):
                e["largest"] = "%d x %d" % tuple(hi)
        ledger["seconds"][rec["file"]] = {"untraced_s": rec["untraced_s"], "traced_s": rec["traced_s"]}
    missing = [f for f in gpu_files() if f not in ledger["seconds"]]
    if missing:
        raise SystemExit("no trace of: " + ", ".join(missing))
    write_ledger(ledger)
    return kernels


def write_ledger(ledger, path=None):
    """sorted keys, one kernel per line"""
    path = path or LEDGER
    lines = ["{", ' "header": %s,' % json.dumps(ledger["header"], sort_keys=True), ' "kernels": {']
    ks = sorted(ledger["kernels"])
    lines += ["  %s: %s%s" % (json.dumps(k), json.dumps(ledger["kernels"][k], sort_keys=True), "," if i + 1 < len(ks) else "") for i, k in enumerate(ks)]
    lines += [" },", ' "seconds": {']
    fs = sorted(ledger["seconds"])
    lines += ["  %s: %s%s" % (json.dumps(f), json.dumps(ledger["seconds"][f], sort_keys=True), "," if i + 1 < len(fs) else "") for i, f in enumerate(fs)]
    lines += [" }", "}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def check(path=None):
    led = json.load(open(path or LEDGER))
    h = led["header"]
    print("# %s, %s CUs, ROCm %s, traced %s at %s (build_id %s)" % (h["device"], h["cus"], h["rocm"], h["date"], h["commit"], h["build_id"]))
    print("%-72s %5s %10s  %s" % ("kernel", "files", "dispatches", "smallest .. largest grid_x x workgroup_x"))
    for k in sorted(led["kernels"]):
        e = led["kernels"][k]
        print("%-72s %5d %10d  %s .. %s" % (k, len(e["files"]), sum(e["files"].values()), e["smallest"], e["largest"]))
    un = [k for k, e in led["kernels"].items() if not sum(e["files"].values())]
    print("# %d kernels, %d never launched%s" % (len(led["kernels"]), len(un), (": " + ", ".join(sorted(un))) if un else ""))
    print("%-34s %10s %10s" % ("file", "untraced_s", "traced_s"))
    for f in sorted(led["seconds"]):
        print("%-34s %10.1f %10.1f" % (f, led["seconds"][f]["untraced_s"], led["seconds"][f]["traced_s"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir", nargs="?", help="directory of the per-file results (both phases in turn)")
    ap.add_argument("--trace", metavar="DIR")
    ap.add_argument("--ledger", metavar="DIR")
    ap.add_argument("--add", metavar="DIR", help="no GPU: put the files traced into DIR (--trace DIR --files ...) into the committed ledger, the other files' entries kept")
    ap.add_argument("--add-kernels", action="store_true", help="with --add: kernels the library compiles and the ledger lacks enter it (compiles the assembly, ~2 minutes)")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--files", default="", help="comma-separated subset of the GPU test files (a long suite is traced over several calls into one DIR)")
    ap.add_argument("--untraced-limit", type=int, default=600, help="seconds allowed to a file's untraced run")
    a = ap.parse_args()
    if a.check:
        return check()
    if a.add:
        add_to_ledger(a.add, a.add_kernels)
        return 0
    files = [f for f in a.files.split(",") if f] or gpu_files()
    assert all(f in gpu_files() for f in files), files
    if a.trace or a.dir:
        rc = trace(a.trace or a.dir, files, a.untraced_limit)
        if rc:
            return rc
    if a.ledger or a.dir:
        kernels = build_ledger(a.ledger or a.dir)
        print("%s: %d kernels, %d never launched" % (os.path.relpath(LEDGER, ROOT), len(kernels), sum(1 for e in kernels.values() if not e["files"])))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
