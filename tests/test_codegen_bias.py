"""
Code-generation census of the ladder step with q-biased sums (jubjub_amd/csrc/jj_mont.h mont_xdbladd), from hipcc's gfx950 assembly (no GPU
needed).  The step lost its two carry steps and must not have gained anything in their place: the loop of k_varbase_mont is at most 1711
instructions (1759 with the carries), still 1248 v_mad_i64_i32, at most 18 v_bfi_b32 and no v_bitop3_b32; the kernel, split into the ladder
and the y-recovery with the base point loaded in between, uses no scratch memory and at most 168 VGPRs (three waves per SIMD).
"""
import collections
import re

import pytest

from test_codegen import ladder_loop, resources


@pytest.fixture(scope="module")
def asm():
    from gfx_asm import assembly

    return assembly(["jj_abi"])


MONT = "14k_varbase_montE"      # the ladder, not k_varbase_mont_x1
LOOP_MAX = 1711                 # what hipcc gives for the shipped source; the bias is worth it up to 1715


def test_biased_ladder_loop_census(asm):
    loop = ladder_loop(asm, MONT)
    ops = collections.Counter(l.split()[0] for l in loop.splitlines() if re.match(r"^\s+[vs]_", l))
    total = sum(ops.values())
    print("k_varbase_mont loop: %d instructions, %d v_mad_i64_i32, %d v_bfi_b32, %d v_bitop3_b32" % (total, ops["v_mad_i64_i32"], ops["v_bfi_b32"], ops["v_bitop3_b32"]))
    assert ops["v_mad_i64_i32"] == 1248, ops["v_mad_i64_i32"]
    assert ops["v_bfi_b32"] <= 18, ops["v_bfi_b32"]
    assert ops["v_bitop3_b32"] == 0, ops["v_bitop3_b32"]
    assert LOOP_MAX <= 1715 and total <= LOOP_MAX, total


def test_split_kernel_has_no_scratch_and_three_waves(asm):
    vgpr, scratch = resources(asm, MONT)
    print("k_varbase_mont: %d VGPRs, %d bytes of scratch" % (vgpr, scratch))
    assert scratch == 0 and vgpr <= 168, (vgpr, scratch)
