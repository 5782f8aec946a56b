"""
Code generation of the Pedersen kernels (jubjub_amd/csrc/jj_pedersen.h, jj_kernels.h), from hipcc's gfx950 assembly of the shipped source (no
GPU needed): k_pedersen_gather and k_pedersen_scalars exist and use NO scratch -- the accumulator, the prefetched entry and the window's bits
stay in registers --, the plan is read with scalar loads (its addresses are wave-uniform: a vector load per plan word would put the layout's
arithmetic into every lane), the rows are read as dwords joined by v_alignbit_b32, and the gather kernel's table entry arrives as sixteen-byte
vector loads.  No VGPR count is pinned; the counts are printed into the test's message for the record (DESIGN.md has the figures of the day).
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

KERNELS = ("k_pedersen_gather", "k_pedersen_scalars", "k_affine_u")


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that launches the kernels


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_exists_and_uses_no_scratch(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0, "%s: %d bytes of scratch at %d VGPRs" % (kernel, scratch, vgpr)
    assert 0 < vgpr <= 256, "%s: %d VGPRs" % (kernel, vgpr)
    assert not re.findall(r"^\s+scratch_", kernel_body(asm, kernel), re.M), kernel


@pytest.mark.parametrize("kernel", KERNELS[:2])
def test_plan_is_read_by_scalar_loads_and_rows_through_a_funnel_shift(asm, kernel):
    vgpr, _ = resources(asm, kernel)
    body = kernel_body(asm, kernel)
    ops = collections.Counter(line.split()[0] for line in body.splitlines() if re.match(r"^\s+[vsg]\w+_", line))
    assert ops["v_alignbit_b32"] >= 1, "%s (%d VGPRs): no v_alignbit_b32" % (kernel, vgpr)
    assert sum(v for o, v in ops.items() if o.startswith("s_load_dword")) >= 4, "%s: the plan is not read by scalar loads" % kernel
    # a piece is two dword loads; nothing else in the bit extraction is a vector load
    assert ops["global_load_dword"] >= 2 and not ops["global_load_ubyte"] and not ops["global_load_ushort"], (kernel, dict(ops))
    if kernel == "k_pedersen_gather":
        assert ops["global_load_dwordx4"] >= 6, "%s: the table entry does not arrive as vector loads" % kernel
