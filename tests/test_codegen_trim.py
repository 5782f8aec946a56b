"""
Code-generation census of the trimmed ladder step and of the kernels that invert by divsteps, from hipcc's gfx950 assembly (no GPU needed):
k_varbase_mont's loop selects only the two inputs of the doubling (18 v_bfi_b32, none re-expanded into v_bitop3_b32) and is no longer than
1760 instructions; neither it nor the two batch-inversion kernels (k_varbase_mont_x1, every k_normalize instance) uses scratch memory.
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


def test_mont_ladder_loop_selects_two_elements_and_is_short(asm):
    loop = ladder_loop(asm, MONT)
    ops = collections.Counter(l.split()[0] for l in loop.splitlines() if re.match(r"^\s+[vs]_", l))
    total = sum(ops.values())
    print("k_varbase_mont loop: %d instructions, %d v_bfi_b32, %d v_bitop3_b32, %d v_mad_i64_i32" % (total, ops["v_bfi_b32"], ops["v_bitop3_b32"], ops["v_mad_i64_i32"]))
    assert ops["v_bfi_b32"] <= 18, ops["v_bfi_b32"]
    assert ops["v_bitop3_b32"] == 0, ops["v_bitop3_b32"]
    assert total <= 1760, total


def test_inversion_kernels_and_the_ladder_have_no_scratch(asm):
    names = [m.group(1) for m in re.finditer(r"\.amdhsa_kernel (\S+)", asm)]
    normalize = [n for n in names if "k_normalize" in n]
    assert len(normalize) >= 4, normalize                 # CHUNK = 4, 16, 32, 64
    for needle in [MONT, "k_varbase_mont_x1"] + normalize:
        vgpr, scratch = resources(asm, needle)
        assert scratch == 0, (needle, vgpr, scratch)
