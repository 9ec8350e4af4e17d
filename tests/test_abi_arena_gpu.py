"""GPU: the memory contract of the C ABI (include/dmcnet_hip.h), entry point by entry point.  Every case of
tests/abi_cases.py drives the library through ctypes as a foreign caller would, with buffers of exactly the promised size
inside a poisoned arena (tests/abi_arena.py): the return code, the guard bytes around every buffer, the inputs, the bit
identity of every output between a 0xFF-filled and a 0x00-filled run, and the absence of NaN are checked, then the outputs
are tied to a reference -- the ops.py wrapper that makes the same call, bit for bit, or an independent fp64 torch evaluation
(the C oracle for the integer kernels) at the tolerance of the kernel's own unit test; each case's ``check`` says which.

What this cannot see: a read outside a buffer whose value is discarded and cannot change a result.  It is not claimed."""
import pytest

from dmcnet_amd import _lib
from tests.abi_arena import run_case
from tests.abi_cases import CASES, DEV

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_abi_memory_contract(case):
    lib = _lib.load()
    old = {k: lib.dmc_get_option(k.encode()) for k in case.options}
    try:
        for k, v in case.options.items():
            _lib.check(lib.dmc_set_option(k.encode(), v), "dmc_set_option")
        try:
            bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
            if case.check is not None:
                case.check(bufs)
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):
                # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
                pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
            raise
    finally:
        for k, v in old.items():
            _lib.check(lib.dmc_set_option(k.encode(), v), "dmc_set_option")
