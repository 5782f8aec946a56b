"""
Code generation of k_blake2s (jubjub_amd/csrc/jj_blake2s.h, jj_kernels.h: jj_blake2s, jj_group_hash), from hipcc's gfx950 assembly of the
shipped source (no GPU needed).

The kernel uses NO scratch: the message schedule is resolved at compile time, so the 16 message words, the working vector and the state stay in
registers; a run-time-indexed m[sigma[r][k]] would send them to private memory.  It holds ONE inlined compression -- the first block and the
later ones differ by values, not by code --, whose 80 G are 4 rotations each: 320 v_alignbit_b32, beside the 16 funnel shifts of the one
message fill (word j of a block from two neighbouring aligned dwords) and nothing else; no rotation goes through a shift pair.  A block's
message bytes are read as at most 17 aligned dwords (16 words at any byte offset) and nothing narrower; the prefix's tail and the midstate
arrive as kernel arguments through the scalar unit.  A digest leaves as two sixteen-byte stores.  The VGPR count is pinned at what the
compiler shows, 50: the whole kernel fits the 64 registers of eight waves per SIMD.
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

KERNEL = "9k_blake2sE"


@pytest.fixture(scope="module")
def asm():
    return assembly(["jj_abi"])    # the translation unit that launches the kernel


@pytest.fixture(scope="module")
def ops(asm):
    return collections.Counter(line.split()[0] for line in kernel_body(asm, KERNEL).splitlines() if re.match(r"^\s+[vsg]\w+_", line))


def test_kernel_uses_no_scratch_and_50_vgprs(asm):
    vgpr, scratch = resources(asm, KERNEL)
    print("k_blake2s: %d VGPRs, %d bytes of scratch" % (vgpr, scratch))
    assert scratch == 0, "%d bytes of scratch at %d VGPRs: the message words or the state left the registers" % (scratch, vgpr)
    assert vgpr == 50, vgpr
    body = kernel_body(asm, KERNEL)
    assert not re.search(r"^\s+(scratch_|buffer_)", body, re.M)


def test_one_compression_with_320_rotations(ops):
    # 80 G x 4 rotations, ONE compression in the kernel, and the 16 funnel shifts of the one message fill
    assert ops["v_alignbit_b32"] == 320 + 16, ops["v_alignbit_b32"]
    assert ops["v_lshlrev_b32_e32"] + ops["v_lshrrev_b32_e32"] + ops["v_lshl_or_b32"] < 16, "rotations through shift pairs"
    assert ops["v_lshlrev_b64"] + ops["v_lshrrev_b64"] <= 2                     # address arithmetic only
    assert ops["v_perm_b32"] == 0 and ops["v_alignbyte_b32"] == 0               # no rotation by 8 or 16 turned into another instruction


def test_message_loads_per_block_and_vector_stores(asm, ops):
    body = kernel_body(asm, KERNEL)
    # 16 words at any byte offset are 17 aligned dwords at the most; ONE fill in the kernel, inside the block loop
    loads = {k: v for k, v in ops.items() if k.startswith("global_load") or k.startswith("flat_load")}
    assert set(loads) == {"global_load_dword"} and 1 <= loads["global_load_dword"] <= 17, loads
    assert not re.findall(r"^\s+global_load_(ubyte|sbyte|ushort|sshort|short)", body, re.M)
    # the midstate, the tail and the other arguments come through the scalar unit
    assert ops["s_load_dwordx16"] + ops["s_load_dwordx8"] >= 2
    assert len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) == 2 and not re.findall(r"^\s+global_store_(byte|short|dword|dwordx2|dwordx3)\s", body, re.M)
    assert not re.search(r"^\s+(s_setpc|s_swappc|s_call)", body, re.M)
