"""
Code generation of the fused fixed + variable ladder kernel (k_varbase_fixed, jubjub_amd/csrc/jj_fixedvar.h), from hipcc's gfx950 assembly of the
shipped source (no GPU needed), with the checks of tests/test_codegen_straus.py: the kernel exists, uses no scratch and at most 256 VGPRs (two
waves per SIMD), the hottest block's products are pinned and selected as single multiply-adds, and both tables -- the lane's extended-Niels table
and the gathered affine-Niels table of the fixed base -- are read with sixteen-byte loads.  No VGPR count other than the cap is pinned.
"""
import os
import re
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gfx_asm import assembly  # noqa: E402

from tests.test_codegen import kernel_body, ladder_block, resources  # noqa: E402

KERNEL = "k_varbase_fixed"


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that holds the ladder kernels


def test_kernel_exists_without_scratch_within_256_vgprs(asm):
    vgpr, scratch = resources(asm, KERNEL)
    assert scratch == 0 and vgpr <= 256, (KERNEL, vgpr, scratch)


def test_products_are_pinned(asm):
    best = ladder_block(asm, KERNEL)
    mads, merges = best["mads"], best["v_lshl_add_u64"]
    assert mads > 600
    assert merges * 40 < mads, "column carries are re-joined with 64-bit adds again (%d for %d multiply-adds)" % (merges, mads)


def test_products_are_single_multiply_adds(asm):
    best = ladder_block(asm, KERNEL)
    assert best["v_mov_b32_e32"] * 6 < best["mads"], "%d v_mov_b32 for %d multiply-adds: products are being expanded" % (best["v_mov_b32_e32"], best["mads"])


def test_table_reads_are_sixteen_byte_loads(asm):
    """the lane's table: nine 16-byte vectors per entry, fetched ahead of the ladder's loop and in it, and stored nine at a time; the fixed
    base's table: seven 16-byte vectors per entry, fetched ahead of the fixed loop and in it; no entry word comes in through a narrower load
    (the only narrower loads are the two scalars' and the point's 32-byte rows: at most 4 x 2 dwordx4 or 32 single words)"""
    body = kernel_body(asm, KERNEL)
    assert len(re.findall(r"^\s+global_load_dwordx4", body, re.M)) >= 2 * 9 + 2 * 7
    assert len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) >= 9
    assert len(re.findall(r"^\s+global_load_dword\s", body, re.M)) <= 32
