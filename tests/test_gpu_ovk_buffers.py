"""
The buffer-discipline rows of jj_blake2b and jj_ka_kdf_each (tests/ovk_buffer_row.py) through the runner of tests/test_gpu_buffers.py (its Env,
checked_call, placements and skews): both entry points on pointers into the guarded arenas of tests/buffer_cases.py -- every size of the table
x every skew (0, 16, 496 and the mixed one) in one device arena, the host arenas and the mixed placements at the host sizes, n = 0 --: return
code 0, the output bytes equal to the restatement of tests/ovk_cases.py, not a byte written beside them, the inputs untouched -- the four bytes
between two rows of a strided source among them.
"""
import pytest

from tests import ovk_buffer_row as BR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", [BR.ROW_B2B, BR.ROW_EACH], ids=["jj_blake2b", "jj_ka_kdf_each"])
def test_buffer_discipline_rows(case):
    import test_gpu_buffers as TB

    env = TB.Env()
    try:
        for options in case.options:
            for n in TB.SIZES:
                for skew in TB.SKEW_SETS:
                    TB.checked_call(env, case, options, n, TB.placement(case, "dev", "dev"), skew)
            for n in TB.HOST_SIZES:
                for ins, outs in (("host", "host"), ("pinned", "pinned"), ("dev", "host"), ("host", "dev"), ("dev", "pinned")):
                    TB.checked_call(env, case, options, n, TB.placement(case, ins, outs), TB.MIXED_SKEW)
            for where in ("dev", "host"):
                for skew in (TB.SKEW_SETS[1], TB.MIXED_SKEW):
                    TB.checked_call(env, case, options, 0, TB.placement(case, where, where), skew)
    finally:
        env.close()
