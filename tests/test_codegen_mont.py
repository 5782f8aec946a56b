"""
Code-generation census of the default constant-time ladder, k_varbase_mont (jubjub_amd/csrc/jj_mont.h), from hipcc's gfx950 assembly (no GPU
needed): its loop has no load, store or shuffle at all and one branch (the bit counter's), no kernel spills, the register count allows three
waves per SIMD, and the products stay single multiply-adds with pinned column carries.  k_varbase_ct3 stays compiled (vb_ct_window=3).
"""
import collections
import re

import pytest

from test_codegen import kernel_body, ladder_loop, resources


@pytest.fixture(scope="module")
def asm():
    from gfx_asm import assembly

    return assembly(["jj_abi"])


MONT = "14k_varbase_montE"      # the ladder, not k_varbase_mont_x1


def test_mont_ladder_loop_has_no_memory_access_and_one_branch(asm):
    loop = ladder_loop(asm, MONT)
    assert not re.search(r"^\s+((?:global|ds|buffer|scratch|flat|s_load|s_buffer)[a-z0-9_]*)\s", loop, re.M), "k_varbase_mont touches memory inside its loop"
    assert len(re.findall(r"^\s+s_cbranch", loop, re.M)) == 1 and not re.search(r"^\s+(s_setpc|s_swappc|s_call|s_branch)", loop, re.M)
    ops = collections.Counter(l.split()[0] for l in loop.splitlines() if re.match(r"^\s+[vs]_", l))
    # one bit per iteration: 4 squares + 5 products (4 x 117 + 5 x 153 = 1233 multiply-adds) and the a24 scale
    assert 1233 <= ops["v_mad_i64_i32"] <= 1233 + 18, ops["v_mad_i64_i32"]
    assert ops["v_lshl_add_u64"] * 40 < ops["v_mad_i64_i32"]
    assert ops["v_mov_b32_e32"] * 6 < ops["v_mad_i64_i32"]


@pytest.mark.parametrize("needle,max_vgpr", [(MONT, 168), ("k_varbase_mont_x1", 256), ("k_varbase_ct3", 256)])
def test_mont_kernels_have_no_scratch(asm, needle, max_vgpr):
    vgpr, scratch = resources(asm, needle)
    assert scratch == 0 and vgpr <= max_vgpr, (needle, vgpr, scratch)
