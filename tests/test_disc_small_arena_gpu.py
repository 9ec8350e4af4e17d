"""GPU: the memory contract of every launching dmc_disc_c8_* / dmc_disc_head_* entry point (csrc/disc_c8.hip, csrc/disc_head.hip)
on the guarded arenas of tests/abi_arena.py -- buffers of exactly the promised size with a megabyte of fill on both sides, once
over 0xFF and once over 0x00: nothing outside them is touched, inputs stay as they were, every output element is written and does
not depend on what the workspace or the guard bands held, and a refused call (a null pointer, a wrong stat_blocks, an unsupported
shape, a size at the 2^31 bound) writes nothing.  Each served case also holds its values to the bars of tests/disc_small_ref.py."""
import pytest
import torch

from dmcnet_amd import _lib
from tests import abi_cases
from tests import disc_small_ref as R
from tests.abi_arena import run_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 48 << 20
F64 = torch.float64


def within(got, ref, bar):
    return R.ratio(got, ref, bar) <= 1.0


def c8_fwd_case(shape, full):
    n, h, w = shape
    oh, ow = R.out_hw(h, w)

    def fn(a):
        d = R.c8_inputs(shape)
        nblk = _lib.load().dmc_disc_c8_stat_blocks(n, h, w)
        a.call("dmc_disc_c8_fwd", a.inp("x", d["x"]), a.inp("w", d["w"]), a.inp("bias", d["bias"]) if full else None,
               a.inp("keep", d["keep"]) if full else None, a.out("z", (n, oh, ow, 16)),
               a.out("stat_partials", (nblk, 16, 2), dtype=F64) if full else None, nblk if full else 0, n, h, w, int(full))

    def check(bufs):
        z64, bar = R.c8_forward(shape, full, full, int(full))
        assert within(bufs["z"].t, z64, bar)
        if full:
            zd = bufs["z"].t.double().cpu().reshape(-1, 16)
            s = bufs["stat_partials"].t.cpu().sum(0)
            for k, v in ((0, zd), (1, zd * zd)):
                assert within(s[:, k], v.sum(0), zd.shape[0] * 2.0 ** -53 * v.abs().sum(0))
    return fn, check


def c8_dgrad_case(shape):
    n, h, w = shape

    def fn(a):
        d = R.c8_inputs(shape)
        a.call("dmc_disc_c8_dgrad", a.inp("g", d["g"]), a.inp("w", d["w"]), a.out("dx", (n, h, w, 8)), n, h, w)

    def check(bufs):
        g = R.c8_grads(shape)
        assert within(bufs["dx"].t, g["dx"], g["dx_bar"])
    return fn, check


def c8_wgrad_case(shape, with_db):
    n, h, w = shape

    def fn(a):
        d = R.c8_inputs(shape)
        ws = a.work("workspace", _lib.load().dmc_disc_c8_wgrad_bytes(n, h, w))
        a.call("dmc_disc_c8_wgrad", a.inp("x", d["x"]), a.inp("g", d["g"]), a.out("dw", (16, 3, 3, 8)), a.out("db", (16,)) if with_db else None,
               ws, n, h, w)

    def check(bufs):
        g = R.c8_grads(shape)
        assert within(bufs["dw"].t, g["dw"], g["dw_bar"])
        if with_db:
            assert within(bufs["db"].t, g["db"], g["db_bar"])
    return fn, check


def head_fwd_case(shape):
    m, c, h, w = shape

    def fn(a):
        d = R.head_inputs(shape)
        a.call("dmc_disc_head_fwd", a.inp("x", d["x"]), a.inp("weight", d["weight"]), a.inp("bias", d["bias"]), a.out("validity", (m, 2)), m, c, h, w)

    def check(bufs):
        ref = R.head_ref(shape)
        assert within(bufs["validity"].t, ref["v"], ref["v_bar"])
    return fn, check


def head_bwd_case(shape, want):
    m, c, h, w = shape

    def fn(a):
        d = R.head_inputs(shape)
        x = a.inp("x", d["x"]) if "w" in want else None
        wt = a.inp("weight", d["weight"]) if "x" in want else None
        dv = a.inp("dvalidity", d["dv"])
        dx = a.out("dx", (m, h, w, c)) if "x" in want else None
        dw = a.out("dweight", (2, c * h * w)) if "w" in want else None
        db = a.out("dbias", (2,)) if "b" in want else None
        ws = a.work("workspace", _lib.load().dmc_disc_head_bwd_bytes(m, c, h, w)) if "w" in want else None
        a.call("dmc_disc_head_bwd", x, wt, dv, dx, dw, db, ws, m, c, h, w)

    def check(bufs):
        ref = R.head_ref(shape)
        for key, r in (("dx", "dx"), ("dweight", "dw"), ("dbias", "db")):
            if key in bufs:
                assert within(bufs[key].t, ref[r], ref[r + "_bar"]), key
    return fn, check


# ---- refused calls: the buffers a served call would write are there, and keep their fill

def _c8_small(a, n=1, h=4, w=6):
    d = R.c8_inputs((n, h, w))
    oh, ow = R.out_hw(h, w)
    return d, a.inp("x", d["x"]), a.inp("w", d["w"]), a.inp("g", d["g"]), oh, ow


def refused_c8_fwd_null_x(a):
    _, _, w, _, oh, ow = _c8_small(a)
    a.call("dmc_disc_c8_fwd", None, w, None, None, a.out("z", (1, oh, ow, 16)), None, 0, 1, 4, 6, 1)


def refused_c8_fwd_stat_blocks(a):
    _, x, w, _, oh, ow = _c8_small(a)
    a.call("dmc_disc_c8_fwd", x, w, None, None, a.out("z", (1, oh, ow, 16)), a.out("stat_partials", (2, 16, 2), dtype=F64), 2, 1, 4, 6, 1)


def refused_c8_fwd_odd(a):
    a.call("dmc_disc_c8_fwd", a.inp("x", R.rnd(1, (1, 7, 9, 8))), a.inp("w", R.rnd(2, (16, 3, 3, 8))), None, None, a.out("z", (1, 4, 5, 16)), None, 0,
           1, 7, 9, 1)


def refused_c8_dgrad_2g(a):         # N H W = 2^26: x would be 2^31 bytes
    _, _, w, g, _, _ = _c8_small(a)
    a.call("dmc_disc_c8_dgrad", g, w, a.out("dx", (1, 4, 6, 8)), 1024, 256, 256)


def refused_c8_wgrad_null_workspace(a):
    _, x, _, g, _, _ = _c8_small(a)
    a.call("dmc_disc_c8_wgrad", x, g, a.out("dw", (16, 3, 3, 8)), a.out("db", (16,)), None, 1, 4, 6)


def _head_small(a):
    d = R.head_inputs((1, 16, 2, 3))
    return a.inp("x", d["x"]), a.inp("weight", d["weight"]), a.inp("bias", d["bias"]), a.inp("dvalidity", d["dv"])


def refused_head_fwd_c24(a):
    a.call("dmc_disc_head_fwd", a.inp("x", R.rnd(1, (2, 2, 2, 24))), a.inp("weight", R.rnd(2, (2, 96))), a.inp("bias", R.rnd(3, (2,))),
           a.out("validity", (2, 2)), 2, 24, 2, 2)


def refused_head_fwd_null_bias(a):
    x, wt, _, _ = _head_small(a)
    a.call("dmc_disc_head_fwd", x, wt, None, a.out("validity", (1, 2)), 1, 16, 2, 3)


def refused_head_bwd_2g(a):         # M C H W = 2^31
    x, wt, _, dv = _head_small(a)
    a.call("dmc_disc_head_bwd", x, wt, dv, a.out("dx", (1, 2, 3, 16)), a.out("dweight", (2, 96)), a.out("dbias", (2,)), a.work("workspace", 768),
           32768, 16, 64, 64)


def refused_head_bwd_null_dvalidity(a):
    x, wt, _, _ = _head_small(a)
    a.call("dmc_disc_head_bwd", x, wt, None, a.out("dx", (1, 2, 3, 16)), a.out("dweight", (2, 96)), a.out("dbias", (2,)), a.work("workspace", 768),
           1, 16, 2, 3)


def refused_head_bwd_dweight_without_workspace(a):
    x, wt, _, dv = _head_small(a)
    a.call("dmc_disc_head_bwd", x, wt, dv, a.out("dx", (1, 2, 3, 16)), a.out("dweight", (2, 96)), None, None, 1, 16, 2, 3)


ARENA_CASES = []


def _add(id, covers, pair, **kw):
    fn, check = pair if isinstance(pair, tuple) else (pair, None)
    ARENA_CASES.append(abi_cases.Case(id, covers, fn, check=check, capacity=CAP, **kw))


for _shape in ((2, 18, 34), (1, 112, 112)):
    for _full in (True, False):
        _add("dmc_disc_c8_fwd-%s-%s" % (R.sid(_shape), "all" if _full else "bare"), ["dmc_disc_c8_fwd"], c8_fwd_case(_shape, _full))
    _add("dmc_disc_c8_dgrad-" + R.sid(_shape), ["dmc_disc_c8_dgrad"], c8_dgrad_case(_shape))
    for _db in (True, False):
        _add("dmc_disc_c8_wgrad-%s-%s" % (R.sid(_shape), "db" if _db else "nodb"), ["dmc_disc_c8_wgrad"], c8_wgrad_case(_shape, _db))
for _shape in ((12, 128, 14, 14), (37, 16, 2, 3)):
    _add("dmc_disc_head_fwd-" + R.sid(_shape), ["dmc_disc_head_fwd"], head_fwd_case(_shape))
    for _want in ("xwb", "x", "wb", "b"):
        _add("dmc_disc_head_bwd-%s-%s" % (R.sid(_shape), _want), ["dmc_disc_head_bwd"], head_bwd_case(_shape, _want))
_INV = abi_cases.DMC_E_INVALID
_add("dmc_disc_c8_fwd-refused-null-x", ["dmc_disc_c8_fwd"], refused_c8_fwd_null_x, expect_rc=_INV)
_add("dmc_disc_c8_fwd-refused-stat-blocks", ["dmc_disc_c8_fwd"], refused_c8_fwd_stat_blocks, expect_rc=_INV)
_add("dmc_disc_c8_fwd-refused-odd-size", ["dmc_disc_c8_fwd"], refused_c8_fwd_odd, expect_rc=_INV)
_add("dmc_disc_c8_dgrad-refused-2GiB", ["dmc_disc_c8_dgrad"], refused_c8_dgrad_2g, expect_rc=_INV)
_add("dmc_disc_c8_wgrad-refused-null-workspace", ["dmc_disc_c8_wgrad"], refused_c8_wgrad_null_workspace, expect_rc=_INV)
_add("dmc_disc_head_fwd-refused-C-24", ["dmc_disc_head_fwd"], refused_head_fwd_c24, expect_rc=_INV)
_add("dmc_disc_head_fwd-refused-null-bias", ["dmc_disc_head_fwd"], refused_head_fwd_null_bias, expect_rc=_INV)
_add("dmc_disc_head_bwd-refused-2G-elements", ["dmc_disc_head_bwd"], refused_head_bwd_2g, expect_rc=_INV)
_add("dmc_disc_head_bwd-refused-null-dvalidity", ["dmc_disc_head_bwd"], refused_head_bwd_null_dvalidity, expect_rc=_INV)
_add("dmc_disc_head_bwd-refused-no-workspace", ["dmc_disc_head_bwd"], refused_head_bwd_dweight_without_workspace, expect_rc=_INV)
# the shared list: tests/test_abi_arena_cpu.py counts these cases as the entry points' coverage and dry-runs them on the CPU
_known = {c.id for c in abi_cases.CASES}
abi_cases.CASES.extend(c for c in ARENA_CASES if c.id not in _known)


@pytest.mark.parametrize("case", ARENA_CASES, ids=[c.id for c in ARENA_CASES])
def test_disc_small_entries_memory_contract(case):
    try:
        bufs = run_case(case.fn, device=DEV, capacity=case.capacity, expect_rc=case.expect_rc)
        if case.check is not None:
            case.check(bufs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            # a faulted device serves nothing more: end the session here instead of launching the remaining cases on it
            pytest.exit("GPU fault in %s: %s" % (case.id, str(e).splitlines()[0]), returncode=3)
        raise


def test_every_launching_entry_point_has_a_case():
    covered = {n for c in ARENA_CASES for n in c.covers}
    launching = {n for n in _lib.SIGNATURES if n.startswith(("dmc_disc_c8_", "dmc_disc_head_")) and not n.endswith(("_supported", "_bytes", "_stat_blocks"))}
    assert covered == launching and len(launching) == 5
