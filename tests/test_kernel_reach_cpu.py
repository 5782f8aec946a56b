"""
The reach contract (no GPU needed): tests/kernel_reach.json, written by tools/kernel_reach.py from kernel traces of the
GPU test files, names exactly the kernels the library compiles, and every one of them was launched by a traced file or stands in
kernel_reach_cases.NOT_REACHED with its reason.  A new kernel, a new instantiation or a stale name fails here until the tool has run again.
Kernel names only: the assembly is read for its .amdhsa_kernel symbols and nothing else.
"""
import json
import os
import sys

import pytest

import kernel_reach_cases as C

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_reach as K  # noqa: E402
from gfx_asm import assembly  # noqa: E402


@pytest.fixture(scope="module")
def compiled():
    return K.compiled_kernels(assembly())          # every translation unit of the library, compiled once, as tests/test_codegen.py does


@pytest.fixture(scope="module")
def ledger():
    return json.load(open(K.LEDGER))


def dispatches(entry):
    return sum(entry["files"].values())


def test_ledger_names_exactly_the_compiled_kernels(compiled, ledger):
    have, want = set(ledger["kernels"]), set(compiled)
    assert have == want, "run tools/kernel_reach.py again: compiled but not in the ledger %r, in the ledger but not compiled %r" % (sorted(want - have), sorted(have - want))


def test_every_kernel_is_reached_or_explained(ledger):
    for name, e in sorted(ledger["kernels"].items()):
        assert all(isinstance(v, int) and v > 0 for v in e["files"].values()), name
        if name in C.NOT_REACHED:
            assert C.NOT_REACHED[name].strip(), "%s: NOT_REACHED gives no reason" % name
            assert dispatches(e) == 0, "%s is launched by %r: take it out of NOT_REACHED" % (name, sorted(e["files"]))
        else:
            assert dispatches(e) >= 1, "%s is launched by no GPU test file and NOT_REACHED does not say why" % name
            assert e["smallest"] and e["largest"], name


def test_not_reached_names_compiled_kernels(compiled):
    assert not set(C.NOT_REACHED) - set(compiled), sorted(set(C.NOT_REACHED) - set(compiled))


def test_default_build_has_no_gather_select_kernels(compiled):
    """k_fixedbase<false> and k_fixedbase_comb<false> (JJ_FIXEDBASE_SELECT=gather) exist in -DJJ_EXPERIMENTS probe builds only: no call of the
    shipped library could launch them."""
    assert "jj::k_fixedbase<true>" in compiled and "jj::k_fixedbase_comb<true>" in compiled
    assert "jj::k_fixedbase<false>" not in compiled and "jj::k_fixedbase_comb<false>" not in compiled


def test_header_is_complete(ledger):
    h = ledger["header"]
    assert sorted(h) == sorted(K.HEADER_KEYS)
    assert all(str(h[k]).strip() and str(h[k]) != "unknown" for k in K.HEADER_KEYS), h
    assert isinstance(h["cus"], int) and h["cus"] > 0
    assert len(h["commit"].split()[0]) == 40 and len(h["date"]) == 10
    traced = set(ledger["seconds"])
    assert traced == set(K.gpu_files()), "GPU test files and traced files differ: %r" % sorted(traced ^ set(K.gpu_files()))
    for name, e in ledger["kernels"].items():
        assert set(e["files"]) <= traced, name
