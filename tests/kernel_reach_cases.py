"""
The reach contract's exceptions (tests/test_kernel_reach_cpu.py; tests/kernel_reach.json is written by tools/kernel_reach.py).

NOT_REACHED: {kernel as the ledger names it: reason}.  Only for kernels that have no arithmetic result to hold to the oracle; every other
compiled kernel must be launched by a GPU test file whose assertions compare that call's output with the oracle.  No GPU import here.
"""

NOT_REACHED = {
    "jj::k_peak_mad": "the multiply-add stream that jj_peak_imad32_samples times (bench.py's roofline denominator): its output is a sink nobody reads, "
                      "there is no result to compare with the oracle",
}
