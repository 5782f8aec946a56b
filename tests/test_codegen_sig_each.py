"""
Code generation of jj_sigverify_each's two kernels (k_sig_each_prep, k_sig_each_tail: jubjub_amd/csrc/jj_sig_each.h), from hipcc's gfx950 assembly
of the shipped source (no GPU needed): both exist and use no scratch, the tail's products are single multiply-adds as in the ladders, and a unit's
verdict leaves as one byte through a vector store -- no coordinate is stored.  The fused kernel k_sig_each measured slower than these two behind
the existing ladders and is not in the library (experiments/sig_each_fused, profiles/sig_each_ab.txt); its checks went with it.  No VGPR count
is pinned.
"""
import os
import re
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gfx_asm import assembly  # noqa: E402

from tests.test_codegen import kernel_body, ladder_block, resources  # noqa: E402

SMALL = ("k_sig_each_prep", "k_sig_each_tail")


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that holds the ladder kernels


@pytest.mark.parametrize("kernel", SMALL)
def test_small_kernels_exist_and_use_no_scratch(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    assert scratch == 0 and vgpr <= 128, (kernel, vgpr, scratch)       # one unit per lane at four waves per SIMD or more


def test_fused_kernel_is_not_shipped(asm):
    assert not re.search(r"\.amdhsa_kernel \S*10k_sig_eachE", asm)


def test_tail_products_are_single_multiply_adds(asm):
    best = ladder_block(asm, "k_sig_each_tail")
    assert best["mads"] > 100
    assert best["v_lshl_add_u64"] * 40 < best["mads"], "column carries are re-joined with 64-bit adds again (%d for %d multiply-adds)" % (best["v_lshl_add_u64"], best["mads"])
    assert best["v_mov_b32_e32"] * 6 < best["mads"], "%d v_mov_b32 for %d multiply-adds: products are being expanded" % (best["v_mov_b32_e32"], best["mads"])


@pytest.mark.parametrize("kernel", SMALL)
def test_verdict_leaves_as_one_byte_store(asm, kernel):
    """vector stores only: the verdict byte; the preparation also stores 32-byte rows (c mod r, -A, the identity) as sixteen-byte vectors"""
    body = kernel_body(asm, kernel)
    assert len(re.findall(r"^\s+global_store_byte", body, re.M)) >= 1
    assert not re.findall(r"^\s+global_store_dword\s", body, re.M)
    if kernel == "k_sig_each_tail":
        assert not re.findall(r"^\s+global_store_dwordx", body, re.M), "the tail stores a coordinate"
