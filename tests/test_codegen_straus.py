"""
Code generation of the two-term ladder kernels (k_varbase_mul2<W, SHARED>, jubjub_amd/csrc/jj_straus.h), from hipcc's gfx950 assembly of the
shipped source (no GPU needed), with the checks of tests/test_codegen.py: the four instantiations exist, none uses scratch or more than 256
VGPRs (two waves per SIMD), the hottest block's products are pinned and selected as single multiply-adds, and the kernel reads its per-lane
tables with sixteen-byte loads.  No VGPR count other than the cap is pinned.
"""
import os
import re
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gfx_asm import assembly  # noqa: E402

from tests.test_codegen import kernel_body, ladder_block, resources  # noqa: E402

KERNELS = ["k_varbase_mul2ILi5ELb0", "k_varbase_mul2ILi5ELb1", "k_varbase_mul2ILi4ELb0", "k_varbase_mul2ILi4ELb1"]


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that holds the ladder kernels


@pytest.mark.parametrize("needle", KERNELS)
def test_kernel_exists_without_scratch_within_256_vgprs(asm, needle):
    vgpr, scratch = resources(asm, needle)
    assert scratch == 0 and vgpr <= 256, (needle, vgpr, scratch)


@pytest.mark.parametrize("needle", KERNELS)
def test_products_are_pinned(asm, needle):
    best = ladder_block(asm, needle)
    mads, merges = best["mads"], best["v_lshl_add_u64"]
    assert mads > 600
    assert merges * 40 < mads, "column carries are re-joined with 64-bit adds again (%d for %d multiply-adds)" % (merges, mads)


@pytest.mark.parametrize("needle", KERNELS)
def test_products_are_single_multiply_adds(asm, needle):
    best = ladder_block(asm, needle)
    assert best["v_mov_b32_e32"] * 6 < best["mads"], "%d v_mov_b32 for %d multiply-adds: products are being expanded" % (best["v_mov_b32_e32"], best["mads"])


@pytest.mark.parametrize("needle", KERNELS)
def test_table_reads_are_sixteen_byte_loads(asm, needle):
    """two entries of nine 16-byte vectors per window (P's and Q's), and P's first entry ahead of the loop"""
    body = kernel_body(asm, needle)
    assert len(re.findall(r"^\s+global_load_dwordx4", body, re.M)) >= 18
    assert len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) >= 9
