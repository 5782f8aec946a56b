"""
Code generation of k_pedersen_commit (jubjub_amd/csrc/jj_pedersen.h, jj_kernels.h), from hipcc's gfx950 assembly of the shipped source (no GPU
needed): the kernel exists and uses NO scratch -- the accumulator, the prefetched entry, the scalar of the blinding walk and the window's bits
stay in registers, and the choice among the call's sources is made by compares, not by an indexed read of the kernel's arguments --, the plan
is read with scalar loads (its addresses are wave-uniform), the rows of every source are read as dwords joined by v_alignbit_b32 and never as
bytes or halfwords, and the table entries arrive as sixteen-byte vector loads.  No VGPR count is pinned; the count is printed into the test's
message for the record (DESIGN.md has the figure of the day).
"""
import collections
import os
import re
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gfx_asm import assembly  # noqa: E402

from tests.test_codegen import kernel_body, resources  # noqa: E402

KERNEL = "k_pedersen_commit"


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that launches the kernel


def test_kernel_exists_and_uses_no_scratch(asm):
    vgpr, scratch = resources(asm, KERNEL)
    print("%s: %d VGPRs, %d bytes of scratch" % (KERNEL, vgpr, scratch))
    assert scratch == 0, "%s: %d bytes of scratch at %d VGPRs" % (KERNEL, scratch, vgpr)
    assert 0 < vgpr <= 256, "%s: %d VGPRs" % (KERNEL, vgpr)
    assert not re.findall(r"^\s+scratch_", kernel_body(asm, KERNEL), re.M)


def test_plan_by_scalar_loads_rows_through_a_funnel_shift_entries_by_vector_loads(asm):
    vgpr, _ = resources(asm, KERNEL)
    body = kernel_body(asm, KERNEL)
    ops = collections.Counter(line.split()[0] for line in body.splitlines() if re.match(r"^\s+[vsg]\w+_", line))
    print("%s: %d VGPRs; %s" % (KERNEL, vgpr, {o: v for o, v in ops.items() if "load" in o}))
    assert ops["v_alignbit_b32"] >= 1, "%s (%d VGPRs): no v_alignbit_b32" % (KERNEL, vgpr)
    assert sum(v for o, v in ops.items() if o.startswith("s_load_dword")) >= 4, "the plan is not read by scalar loads"
    # a piece is two dword loads; nothing in the bit extraction is a sub-dword load
    assert ops["global_load_dword"] >= 2, dict(ops)
    assert not [o for o in ops if re.match(r"(global|flat|buffer)_load_(u|s)(byte|short)", o)], dict(ops)
    assert not [o for o in ops if o.startswith("flat_load") or o.startswith("buffer_load")], dict(ops)
    assert ops["global_load_dwordx4"] >= 6, "the table entries do not arrive as sixteen-byte vector loads"
