"""-m gpu: the field operations of csrc/field.hpp on RAW limb images at their stated bounds, as the device compiles them
(the chain barriers, the v_mad_u64_u32 asm of the sparse moduli, mul32, the rolled inverse loop exist on the device
alone): the debug kernel of csrc/tu_debug.hip runs csrc/field_raw_ops.hpp on the cases of tests/field_cases.py, and the
results are checked against Python integers.  test_field_raw_cpu.py runs the same cases on a host build."""

import numpy as np
import pytest

import field_cases as FC
from gpu_util import need_gpu

pytestmark = pytest.mark.gpu


def device_runner():
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    ariths = {}

    def run(f, code, a, b, c, d):
        if f.cid not in ariths:
            ariths[f.cid] = B.Arith.init(f.cid)
        n = a.shape[0]
        a, b, c, d = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, b, c, d))
        out = np.full((n, 2 * f.NL), 0xFFFFFFFF, dtype=np.uint32)
        rc = _lib.lib().bpp_debug_field_raw_op(ariths[f.cid].handle, f.idx, code, a.ctypes.data, b.ctypes.data, c.ctypes.data,
                                               d.ctypes.data, n, out.ctypes.data)
        assert rc == 0, (f.name, code, rc)
        return out
    return run


@pytest.mark.parametrize("fname", list(FC.FIELDS))
def test_raw_field_ops_match_integers_on_device(fname):
    need_gpu()
    FC.run_and_check(fname, device_runner())


def test_mul_add_of_all_ones_limbs_on_device():
    """a = b = c = d = 2^360 - 1 on BLS12-381 Fp: 26 products of all-ones limbs in a middle column (test_field_raw_cpu.py)"""
    need_gpu()
    f = FC.FIELDS["bls12_381_fp"]
    v = FC.OVERFLOW_PROBE
    case = FC.Case("mul_add", FC.OP_CODE["mul_add"], [v] * 70, [v] * 70, [v] * 70, [v] * 70)   # more than one block
    FC.check(f, case, device_runner()(f, case.code, *FC.operand_arrays(f, case)))


def test_unknown_raw_op_is_an_error():
    need_gpu()
    import bulletproofsplus_amd as B
    from bulletproofsplus_amd import _lib
    a = B.Arith.init(0)
    z = np.zeros((1, 13), dtype=np.uint32)
    out = np.zeros((1, 26), dtype=np.uint32)
    for code in (-1, len(FC.OPS)):
        assert _lib.lib().bpp_debug_field_raw_op(a.handle, 0, code, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1,
                                                 out.ctypes.data) < 0
