"""
Code generation of the kernels of jj_ka_kdf and jj_chacha20_xor, from hipcc's gfx950 assembly of the shipped source (no GPU needed).

k_varbase_mont_ka (both instantiations: without and with the cofactor's doublings) is the ladder of k_varbase_mont with ONE secret scalar for
all lanes.  A wave-uniform secret invites the compiler to turn the masked select of a ladder step into a scalar select or into a branch on a
bit of the key; the kernel reads the scalar through a per-lane address so that it cannot.  The pin: the loop of the new kernel has the same
number of conditional branches (one: the bit counter's) and the same number of v_bfi_b32 per bit as the loop of k_varbase_mont, no scalar
select, no v_cndmask, no memory access of any kind and no call; the kernel uses no scratch and at most 168 VGPRs (three waves per SIMD).
k_varbase_mont itself is held by tests/test_codegen_mont.py, which stays as it is.

k_ka_kdf (both instantiations) and k_chacha20_xor use no scratch; the cipher's rotations are v_alignbit_b32 -- 320 per block, one block's
rounds being the only ones in the kernel --, and its rows move as dwords.
"""
import collections
import re

import pytest

from test_codegen import kernel_body, ladder_loop, resources

MONT = "14k_varbase_montE"      # the ladder of jj_varbase_mul, not k_varbase_mont_x1 or k_varbase_mont_ka
KA = ("k_varbase_mont_kaILb0", "k_varbase_mont_kaILb1")
MEM = r"^\s+((?:global|ds|buffer|scratch|flat|s_load|s_buffer)[a-z0-9_]*)\s"


@pytest.fixture(scope="module")
def asm():
    from gfx_asm import assembly

    return assembly(["jj_abi"])


def census(loop):
    ops = collections.Counter(l.split()[0] for l in loop.splitlines() if re.match(r"^\s+[vs]_", l))
    return {"cbranch": len(re.findall(r"^\s+s_cbranch", loop, re.M)), "v_bfi_b32": ops["v_bfi_b32"],
            "cndmask": sum(v for k, v in ops.items() if k.startswith("v_cndmask")), "s_cselect": sum(v for k, v in ops.items() if k.startswith("s_cselect")),
            "mads": ops["v_mad_i64_i32"], "total": sum(ops.values())}


@pytest.mark.parametrize("kernel", KA)
def test_ladder_loop_matches_k_varbase_mont(asm, kernel):
    ref, new = census(ladder_loop(asm, MONT)), census(ladder_loop(asm, kernel))
    print("k_varbase_mont %r\n%s %r" % (ref, kernel, new))
    assert ref["cbranch"] == 1 and ref["v_bfi_b32"] >= 18                      # what is compared with: one select of two field elements per bit
    assert new["cbranch"] == ref["cbranch"], "another conditional branch in the loop: on a bit of the key?"
    assert new["v_bfi_b32"] == ref["v_bfi_b32"], "the masked selects are no longer v_bfi_b32"
    assert new["cndmask"] == ref["cndmask"] == 0 and new["s_cselect"] == ref["s_cselect"] == 0
    assert new["mads"] == ref["mads"]
    loop = ladder_loop(asm, kernel)
    assert not re.search(MEM, loop, re.M), "%s touches memory inside its loop" % kernel
    assert not re.search(r"^\s+(s_setpc|s_swappc|s_call|s_branch)", loop, re.M)


@pytest.mark.parametrize("kernel", KA)
def test_ladder_kernel_resources(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0 and vgpr <= 168, (kernel, vgpr, scratch)


def test_the_scalar_is_loaded_per_lane(asm):
    """the eight dwords of the key come through vector loads (global_load_*), never through the scalar unit (s_load_* of more than the kernel's
    arguments would put the key into scalar registers)"""
    for kernel in KA:
        body = kernel_body(asm, kernel)
        head = body.split(ladder_loop(asm, kernel)[:200])[0]                    # the code in front of the loop
        loads = collections.Counter(m.group(1) for m in re.finditer(r"^\s+(global_load_\w+)", head, re.M))
        dwords = sum(v * {"global_load_dword": 1, "global_load_dwordx2": 2, "global_load_dwordx3": 3, "global_load_dwordx4": 4}[k] for k, v in loads.items())
        assert dwords >= 8 + 9, (kernel, loads)                                 # the key's eight dwords and x1's nine limbs
        assert len(re.findall(r"^\s+s_(?:buffer_)?load", head, re.M)) == len(re.findall(r"^\s+s_(?:buffer_)?load", kernel_body(asm, MONT).split("v_mad_i64_i32")[0], re.M))


@pytest.mark.parametrize("kernel", ["k_ka_kdfILb0", "k_ka_kdfILb1", "k_chacha20_xor"])
def test_hash_and_cipher_use_no_scratch(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0 and 0 < vgpr <= 128, (kernel, vgpr, scratch)


def test_hash_is_one_compression(asm):
    for kernel, loads in (("k_ka_kdfILb0", 2), ("k_ka_kdfILb1", 4)):
        body = kernel_body(asm, kernel)
        ops = collections.Counter(line.split()[0] for line in body.splitlines() if re.match(r"^\s+[vsg]\w+_", line))
        assert 96 * 6 - 16 <= ops["v_alignbit_b32"] <= 96 * 6, (kernel, ops["v_alignbit_b32"])      # 96 G x 3 rotations x 2 halves, less what zero words fold away
        assert ops["v_lshlrev_b64"] + ops["v_lshrrev_b64"] < 16
        assert ops["global_load_dwordx4"] == loads and len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) == 2, (kernel, ops)
        assert not re.search(r"^\s+s_cbranch", body.split("global_load_dwordx4")[-1].split("global_store")[0], re.M)    # straight-line between the loads and the store


def test_cipher_rotations_and_dword_rows(asm):
    body = kernel_body(asm, "k_chacha20_xor")
    ops = collections.Counter(line.split()[0] for line in body.splitlines() if re.match(r"^\s+[vsg]\w+_", line))
    assert ops["v_alignbit_b32"] == 320, ops["v_alignbit_b32"]                  # 80 quarter rounds x 4 rotations, written once
    assert ops["v_lshlrev_b32_e32"] + ops["v_lshrrev_b32_e32"] < 8              # no shift pairs for the rotations
    assert ops["global_load_dwordx4"] == 2                                      # the key
    assert ops["global_load_dword"] >= 16 and ops["global_store_dword"] >= 16
    assert not re.findall(r"^\s+global_(load|store)_(ubyte|sbyte|byte|short|ushort)", body, re.M)
