"""
Code generation of k_poly1305, k_aead<false> (open) and k_aead<true> (seal), from hipcc's gfx950 assembly of the shipped source (no GPU needed).

Resources: no scratch and at most 128 VGPRs each (four waves per SIMD).

Memory: a row moves as single dwords -- global_load_dword / global_store_dword, never a byte or short access and never a fused 8-, 12- or
16-byte access, for which a row that starts on a multiple of 4 is not aligned (jj_poly1305.h: row_ld, row_st).  The only other accesses are
the two global_load_dwordx4 of the key (32-byte aligned), k_poly1305's one global_store_dwordx4 of the tag (tag16 + 16 i: 16-byte aligned) and
open's one global_store_byte, the verdict ok[i].

Rotations: a ChaCha20 rotation is v_alignbit_b32 with BOTH sources the same register, 320 per block function.  k_aead inlines the block
twice -- block 0 for the one-time key, and the data stream's loop -- and k_poly1305 not at all, so there are at most 640 and 0.  The count
in k_aead is 627, 13 short of 640: the compiler shares work between the two copies (the three column quarter-rounds of the first round that
do not touch the counter word, x1, x2, x3 with their columns, are the same values in block 0 and in every block of the loop: 12 rotations)
and drops what block 0 computes only for words it never hands out (words 0..7 are used).  Pinned: between 640 - 16 and 640, so a third copy of
the block function (or a rotation written as two shifts) fails.  Poly1305 uses the same instruction with two DIFFERENT sources as a funnel
shift, to cut 26-bit limbs out of neighbouring dwords (four for r, four per absorbed block, one per joined column): those are counted apart
and bounded by 4 + 6 per inlined absorb.

Products: one Poly1305 block is 25 v_mad_u64_u32 plus one for the wrap 5 c of the top column's carry into limb 0: 26.  k_poly1305 has ONE
absorb in its loop (the partial last block goes through the same one): 26, plus the address multiplication i * in_stride.  k_aead walks the
MAC in steps of up to 16 words held in registers -- one ChaCha20 block, or 16 loads in flight -- and absorbs up to four blocks a step with
constant register indices, so its ONE absorbing loop holds four absorbs: 104, for the aad, the ciphertext and the lengths alike, plus the
address multiplications (i * in_stride, i * out_row).  Pinned: 26 or 104 in the loop, at most 3 outside.

The verdict: behind the tag comparison (the last of the three asm barriers that hide a mask's history from the compiler, jj_poly1305.h: opaque)
open has the keystream pass and the store of ok.  Whatever could carry a lane's verdict into control flow or a select is absent there: no
v_cmp, no v_cndmask, no v_readfirstlane, no branch on EXEC, and VCC is written only as `s_and_b64 (s_andn2_b64) vcc, exec, s[..]` -- a uniform condition
from scalar registers, which hold len and the loop counter.  Every conditional branch there is therefore a loop back-edge or a forward branch
on len alone (the compiler writes the loop guard and the predicate on the last partial block as forward branches; a back-edge-only form is
not something the source can ask for).  The same holds for the Poly1305 arithmetic itself in all three kernels: no v_cmp and no v_cndmask
other than the `i < n` guard and selects under a scalar-register condition (the uniform predicates on the last block's length).
"""
import collections
import re

import pytest

from test_codegen import kernel_body, resources

KERNELS = {"k_poly1305": 1, "k_aeadILb0": 4, "k_aeadILb1": 4}          # -> absorbs inlined in the kernel's one absorbing loop
ROW_OPS = {"global_load_dword", "global_store_dword"}


@pytest.fixture(scope="module")
def asm():
    from gfx_asm import assembly

    return assembly(["jj_abi"])


def ops_of(text):
    return collections.Counter(line.split()[0] for line in text.splitlines() if re.match(r"^\s+[vsg]\w+_", line))


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_four_waves_per_simd(asm, kernel):
    vgpr, scratch = resources(asm, kernel)
    print("%s: %d VGPRs, %d bytes of scratch" % (kernel, vgpr, scratch))
    assert scratch == 0 and 0 < vgpr <= 128, (kernel, vgpr, scratch)
    assert not re.search(r"^\s+(scratch_|buffer_)", kernel_body(asm, kernel), re.M)


@pytest.mark.parametrize("kernel", KERNELS)
def test_rows_move_as_dwords(asm, kernel):
    body = kernel_body(asm, kernel)
    mem = collections.Counter(m.group(1) for m in re.finditer(r"^\s+((?:global|flat|ds)_\w+)", body, re.M))
    print(kernel, dict(mem))
    other = {k: v for k, v in mem.items() if k not in ROW_OPS}
    want = {"global_load_dwordx4": 2}
    if kernel == "k_poly1305":
        want["global_store_dwordx4"] = 1
    if kernel == "k_aeadILb0":
        want["global_store_byte"] = 1
    assert other == want, (kernel, other)
    assert mem["global_load_dword"] >= 4 and (kernel == "k_poly1305" or mem["global_store_dword"] >= 16)


@pytest.mark.parametrize("kernel", KERNELS)
def test_rotations_and_funnel_shifts(asm, kernel):
    body = kernel_body(asm, kernel)
    align = re.findall(r"^\s+v_alignbit_b32\s+\w+, (\w+), (\w+), ", body, re.M)
    rot = sum(1 for a, b in align if a == b)
    funnel = len(align) - rot
    print("%s: %d rotations, %d funnel shifts" % (kernel, rot, funnel))
    if kernel == "k_poly1305":
        assert rot == 0, (kernel, rot)
    else:
        assert 640 - 16 <= rot <= 640, (kernel, rot)                             # the block function inlined twice, never a third time
    assert 0 < funnel <= 4 + 6 * KERNELS[kernel], (kernel, funnel)
    assert ops_of(body)["v_lshlrev_b32_e32"] + ops_of(body)["v_lshrrev_b32_e32"] < 24 * KERNELS[kernel]      # no shift pairs for the rotations


@pytest.mark.parametrize("kernel", KERNELS)
def test_products_are_written_once_per_absorbing_loop(asm, kernel):
    body = kernel_body(asm, kernel)
    blocks = re.split(r"\n(?=\.LBB\d+_\d+:)", body)
    per_block = [len(re.findall(r"^\s+v_mad_u64_u32", b, re.M)) for b in blocks]
    total = sum(per_block)
    print("%s: %d v_mad_u64_u32 in all, per basic block %r" % (kernel, total, [c for c in per_block if c]))
    want = 26 * KERNELS[kernel]
    assert want <= total <= want + 3, (kernel, total)
    # they sit in 26s: every basic block holds a whole number of absorbs, or only address arithmetic (at most 3 in all)
    assert sum(c for c in per_block if c % 26 == 0) == want and sum(c for c in per_block if c % 26) <= 3, (kernel, per_block)
    assert ops_of(body)["v_mad_i64_i32"] == 0 and ops_of(body)["v_mul_hi_u32"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_lane_dependent_compare_or_select(asm, kernel):
    body = kernel_body(asm, kernel)
    cmps = re.findall(r"^\s+(v_cmpx?_\w+)\s+(.*)$", body, re.M)
    assert [c[0] for c in cmps] == ["v_cmp_gt_u64_e32"], (kernel, cmps)           # i < n
    for cond in re.findall(r"^\s+v_cndmask_b32\w*\s+\w+, [^,]+, [^,]+, (\S+)", body, re.M):
        assert re.fullmatch(r"s\[\d+:\d+\]", cond), (kernel, cond)                # a uniform condition held in scalar registers
    assert not re.search(r"^\s+v_readfirstlane", body, re.M)
    assert len(re.findall(r"^\s+s_cbranch_exec", body, re.M)) <= (3 if kernel == "k_poly1305" else 1)


@pytest.mark.parametrize("kernel", ["k_aeadILb0", "k_aeadILb1"])
def test_nothing_behind_the_tag_comparison_depends_on_the_verdict(asm, kernel):
    body = kernel_body(asm, kernel)
    barriers = [m.end() for m in re.finditer(r";;#ASMEND", body)]
    assert len(barriers) == (3 if kernel == "k_aeadILb0" else 1), (kernel, len(barriers))      # finish's mask; open: 0 - diff and the verdict's mask
    head, tail = body[:barriers[-1]], body[barriers[-1]:]
    if kernel == "k_aeadILb0":
        assert re.search(r"v_or3_b32|v_or_b32", head[-600:]) and "global_store_byte" in tail and 300 <= len(re.findall(r"^\s+v_alignbit_b32", tail, re.M)) <= 320
    assert not re.search(r"^\s+(v_cmp|v_cndmask|v_readfirstlane|s_cbranch_exec)", tail, re.M), kernel
    for line in re.findall(r"^\s+(\S+\s+vcc(?:_lo|_hi)?,.*)$", tail, re.M):
        assert re.match(r"s_andn?2?_b64\s+vcc, exec, s\[\d+:\d+\]", line), (kernel, line)          # VCC only from scalar registers
    branches = collections.Counter(re.findall(r"^\s+(s_cbranch_\w+)", tail, re.M))
    assert set(branches) <= {"s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz"}, (kernel, branches)
    # SCC is written by the scalar unit alone, and no scalar register is loaded from a vector one behind the comparison
    assert not re.search(r"^\s+(v_readlane|s_.*\bv\d+)", tail, re.M), kernel
