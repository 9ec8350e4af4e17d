"""CPU: the guarded-arena harness of tests/abi_arena.py notices what it claims to notice (Python stand-ins for an entry
point over CPU tensors, one defect each), and every entry point of the C ABI either has an arena case
(tests/abi_cases.py, run on the GPU by tests/test_abi_arena_gpu.py) or is listed here as launching nothing."""
import pytest
import torch

from dmcnet_amd import _lib
from tests import abi_arena as AA
from tests.abi_cases import CASES

CAP = 8 << 20
N = 1000          # odd byte sizes: 4000-byte buffers, so the 256-byte alignment leaves slack that must stay fill too


def _x():
    return torch.arange(N, dtype=torch.float32) * 0.25 - 3.0


def standin(defect=None):
    """y = 2 x through a (zeroed) workspace word, as an entry point over caller buffers would."""
    def case(a):
        x, y, ws = a.inp("x", _x()), a.out("y", (N,)), a.work("ws", 64)
        wsf = ws.u8.view(torch.float32)
        if defect != "stale_work":
            wsf.zero_()
        y.t.copy_(x.t * 2 + wsf[3])
        if defect == "unwritten":
            y.u8[4 * 17:4 * 18] = a.fill                      # element 17 keeps what the buffer held before
        if defect == "behind":
            a.mem[y.offset + y.nbytes] = 0x5A
        if defect == "front":
            a.mem[y.offset - 1] = 0x5A
        if defect == "alter_in":
            x.u8[123] ^= 1
        a.returned("standin", -1 if defect == "rc" else 0)
    return case


def test_correct_standin_passes():
    bufs = AA.run_case(standin(), device="cpu", capacity=CAP)
    assert torch.equal(bufs["y"].t, _x() * 2)
    for b in bufs.values():
        assert b.u8.data_ptr() % 256 == 0 and b.offset >= AA.MARGIN
    offs = sorted((b.offset, b.nbytes) for b in bufs.values())
    for (o0, n0), (o1, _) in zip(offs, offs[1:]):
        assert o1 - (o0 + n0) >= AA.MARGIN
    assert bufs["y"].nbytes == 4 * N and bufs["ws"].nbytes == 64           # exact sizes, no rounding


@pytest.mark.parametrize("defect,check", [("behind", "guard"), ("front", "guard"), ("unwritten", "ab"), ("stale_work", "ab"),
                                          ("alter_in", "in"), ("rc", "rc")])
def test_defective_standin_fails_its_check(defect, check):
    with pytest.raises(AA.ArenaViolation) as e:
        AA.run_case(standin(defect), device="cpu", capacity=CAP)
    assert e.value.check == check, str(e.value)
    if defect == "behind":
        assert "1 bytes behind OUT buffer 'y'" in str(e.value)
    if defect == "front":
        assert "1 bytes in front of OUT buffer 'y'" in str(e.value)


def test_nan_check_and_its_exemption():
    def case(nan_ok):
        def run(a):
            y = a.out("y", (4,), nan_ok=nan_ok)
            y.t.copy_(torch.tensor([1.0, float("nan"), 2.0, 3.0]))
            a.returned("standin", 0)
        return run
    with pytest.raises(AA.ArenaViolation) as e:
        AA.run_case(case(False), device="cpu", capacity=CAP)
    assert e.value.check == "nan"
    AA.run_case(case(True), device="cpu", capacity=CAP)


def test_refused_call_must_write_nothing():
    def case(writes):
        def run(a):
            y = a.out("y", (4,))
            if writes:
                y.t.fill_(1.0)
            a.returned("standin", -1)
        return run
    AA.run_case(case(False), device="cpu", capacity=CAP, expect_rc=-1)
    with pytest.raises(AA.ArenaViolation):
        AA.run_case(case(True), device="cpu", capacity=CAP, expect_rc=-1)


def test_inout_and_slack_are_part_of_the_buffer():
    def run(a):
        r = a.inout("running", torch.ones(5))
        f = a.inp("frames", torch.arange(10, dtype=torch.uint8), slack=16)
        assert f.nbytes == 26 and r.nbytes == 20
        r.t.mul_(0.5)
        a.returned("standin", 0)
    bufs = AA.run_case(run, device="cpu", capacity=CAP)
    assert torch.equal(bufs["running"].t, torch.full((5,), 0.5))


#: entry points that launch no kernel over caller buffers, and why they need no arena case
NOT_LAUNCHING = {
    "dmc_version": "returns a constant",
    "dmc_last_error": "returns the thread-local error text",
    "dmc_set_option": "host-side option table",
    "dmc_get_option": "host-side option table",
    "dmc_profile_mark": "launches an empty marker kernel: no buffers",
    "dmc_prepare_interp_taps": "host only: fills host arrays, no launch (tests/test_device_prep_cpu.py)",
    "dmc_maxpool3d_tf_out_shape": "host-side shape query",
}
_QUERY_SUFFIXES = ("_bytes", "_supported", "_stat_blocks", "_stat_blocks_k")
NOT_LAUNCHING.update({n: "size / capability query: integers in, an integer out" for n in _lib.SIGNATURES if n.endswith(_QUERY_SUFFIXES)})


def test_every_entry_point_has_an_arena_case_or_launches_nothing():
    covered = set()
    for c in CASES:
        covered.update(c.covers)
    not_launching = NOT_LAUNCHING
    for n in not_launching:
        if n.endswith(_QUERY_SUFFIXES):       # listed by its name alone: it must not be able to reach a caller buffer
            assert not any(t is _lib._P for t in _lib.SIGNATURES[n][1]), "%s takes a pointer: it needs an arena case" % n
    assert not (covered & set(not_launching)), sorted(covered & set(not_launching))
    unknown = covered - set(_lib.SIGNATURES)
    assert not unknown, "arena cases name entry points the library does not have: %s" % sorted(unknown)
    missing = sorted(set(_lib.SIGNATURES) - covered - set(not_launching))
    assert not missing, "entry points without an arena case (tests/abi_cases.py): %s" % missing
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


def test_every_case_calls_what_it_covers_with_well_typed_arguments():
    """A dry run of every case on the CPU (size queries are host code): each call must match the ctypes signature -- pointers
    where the header has pointers, integers and floats elsewhere, the right count -- and the case must call every entry point
    it claims to cover (an entry point that depends on the shape: in at least one case)."""
    lib = _lib.load()
    all_called, all_covered = set(), set()
    for c in CASES:
        old = {k: lib.dmc_get_option(k.encode()) for k in c.options}
        try:
            for k, v in c.options.items():
                assert lib.dmc_set_option(k.encode(), v) == 0
            a = AA.Arena(0, "cpu", c.capacity, dry=True)
            c.fn(a)
        finally:
            for k, v in old.items():
                assert lib.dmc_set_option(k.encode(), v) == 0
        called = {name for name, _ in a.rcs}
        assert called and called <= set(c.covers), (c.id, sorted(called - set(c.covers)))
        all_called |= called
        all_covered |= set(c.covers)
        for b in a.bufs:
            assert b.u8.data_ptr() % AA.ALIGN == 0 and b.nbytes > 0
    assert all_called == all_covered, sorted(all_covered - all_called)        # a shape-dependent call must happen in SOME case
