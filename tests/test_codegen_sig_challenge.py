"""
Code generation of k_sig_challenge (jubjub_amd/csrc/jj_blake2b.h, jj_kernels.h), from hipcc's gfx950 assembly of the shipped source (no GPU
needed): the three instantiations (no part, one, two) exist and use NO scratch -- the message schedule is resolved at compile time, so the 16
message words, the working vector and the state stay in registers; a run-time-indexed m[sigma[r][k]] would send them to private memory --, the
rotations are v_alignbit_b32 on the halves and not 64-bit shifts, and a challenge leaves as sixteen-byte vector stores.  No VGPR count is
pinned; the counts are printed into the test's message for the record (DESIGN.md has the figures of the day: 96, five waves per SIMD).
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

KERNELS = ("k_sig_challengeILi0", "k_sig_challengeILi1", "k_sig_challengeILi2")


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that launches the kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_exists_and_uses_no_scratch(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0, "%s: %d bytes of scratch at %d VGPRs: the message words or the state left the registers" % (kernel, scratch, vgpr)
    assert 0 < vgpr <= 512, "%s: %d VGPRs" % (kernel, vgpr)


@pytest.mark.parametrize("kernel", KERNELS)
def test_rotations_are_funnel_shifts_and_stores_are_vectors(asm, kernel):
    vgpr, _ = resources(asm, kernel)
    body = kernel_body(asm, kernel)
    ops = collections.Counter(line.split()[0] for line in body.splitlines() if re.match(r"^\s+[vsg]\w+_", line))
    # two compressions are inlined (block 0 with the parts, the loop's block): 2 x 96 G x 3 rotations x 2 halves
    assert ops["v_alignbit_b32"] >= 2 * 96 * 6, "%s (%d VGPRs): %d v_alignbit_b32" % (kernel, vgpr, ops["v_alignbit_b32"])
    assert ops["v_lshlrev_b64"] + ops["v_lshrrev_b64"] < 16, "%s (%d VGPRs): the rotations went through 64-bit shifts" % (kernel, vgpr)
    assert len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) == 2 and not re.findall(r"^\s+global_store_(byte|short|dword)\s", body, re.M), kernel
