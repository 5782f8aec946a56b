"""
Code generation of the kernels of jj_ka_kdf_each and jj_blake2b, from hipcc's gfx950 assembly of the shipped source (no GPU needed).

k_varbase_mont_ka_each (both instantiations: without and with the cofactor's doublings) is the ladder of k_varbase_mont with the doublings of
k_varbase_mont_ka behind it: the loop has k_varbase_mont's count of conditional branches (one: the bit counter's), of v_bfi_b32 and of
v_mad_i64_i32 per bit, no v_cndmask, no scalar select, no memory access and no call; the kernel uses no scratch and at most 168 VGPRs (three
waves per SIMD).

k_blake2b<32|64>: no scratch -- every index into m[] is a compile-time constant --, at most 128 VGPRs (the cap tests/test_codegen_ka.py holds
k_ka_kdf to; four waves per SIMD and more), the rotations are v_alignbit_b32 (ONE compression is inlined: the block loop's), the rows move as
dwords, and no 64-bit shift pairs beyond the handful test_hash_is_one_compression allows.
"""
import collections
import re

import pytest

from test_codegen import kernel_body, ladder_loop, resources
from test_codegen_ka import MEM, MONT, census

EACH = ("k_varbase_mont_ka_eachILb0", "k_varbase_mont_ka_eachILb1")
B2B = ("k_blake2bILi32", "k_blake2bILi64")


@pytest.fixture(scope="module")
def asm():
    from gfx_asm import assembly

    return assembly(["jj_abi"])


@pytest.mark.parametrize("kernel", EACH)
def test_ladder_loop_matches_k_varbase_mont(asm, kernel):
    ref, new = census(ladder_loop(asm, MONT)), census(ladder_loop(asm, kernel))
    print("k_varbase_mont %r\n%s %r" % (ref, kernel, new))
    assert ref["cbranch"] == 1 and ref["v_bfi_b32"] >= 18
    assert new["cbranch"] == ref["cbranch"], "another conditional branch in the loop: on a bit of a key?"
    assert new["v_bfi_b32"] == ref["v_bfi_b32"], "the masked selects are no longer v_bfi_b32"
    assert new["cndmask"] == ref["cndmask"] == 0 and new["s_cselect"] == ref["s_cselect"] == 0
    assert new["mads"] == ref["mads"]
    loop = ladder_loop(asm, kernel)
    assert not re.search(MEM, loop, re.M), "%s touches memory inside its loop" % kernel
    assert not re.search(r"^\s+(s_setpc|s_swappc|s_call|s_branch)", loop, re.M)


@pytest.mark.parametrize("kernel", EACH)
def test_ladder_kernel_resources(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0 and vgpr <= 168, (kernel, vgpr, scratch)


@pytest.mark.parametrize("kernel", B2B)
def test_hash_kernel_resources(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0 and 0 < vgpr <= 128, (kernel, vgpr, scratch)


@pytest.mark.parametrize("kernel", B2B)
def test_hash_rotations_and_dword_rows(asm, kernel):
    body = kernel_body(asm, kernel)
    ops = collections.Counter(line.split()[0] for line in body.splitlines() if re.match(r"^\s+[vsg]\w+_", line))
    print("%s: %r" % (kernel, {k: ops[k] for k in ("v_alignbit_b32", "v_lshlrev_b64", "v_lshrrev_b64", "global_load_dword", "global_store_dwordx4", "v_cndmask_b32_e32")}))
    assert 96 * 6 - 16 <= ops["v_alignbit_b32"] <= 96 * 6, (kernel, ops["v_alignbit_b32"])          # 96 G x 3 rotations x 2 halves: one compression, written once
    assert ops["v_lshlrev_b64"] + ops["v_lshrrev_b64"] < 16, "%s: the rotations went through 64-bit shifts" % kernel
    assert not re.findall(r"^\s+global_(load|store)_(ubyte|sbyte|byte|short|ushort|sshort)", body, re.M)
    assert not re.findall(r"^\s+(scratch|buffer|flat)_", body, re.M)
    loads = sum(v for k, v in ops.items() if k.startswith("global_load_dword"))
    assert loads >= 32, (kernel, loads)                                                           # the 32 dwords of a block
    assert len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) == int(kernel[-2:]) // 16 and not re.findall(r"^\s+global_store_(byte|short|dword)\s", body, re.M)
