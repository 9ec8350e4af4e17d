"""CPU: the shapes of tests/test_csm_walk_gpu.py reach what they claim -- several visits per wave in every persistent kernel of
conv_small.hip, a capped grid, waves that stop one visit early, an odd tile count, partial row segments -- the restated launch
geometry (tests/csm_walk_shapes.py) is the library's, and no other unit test of those kernels gets a wave past its first tile."""
import pytest

import dmcnet_amd
from tests.csm_walk_shapes import WALK_CASES, WALK_VISITS, out_map, plans, tile_count, wgrad_workspace_bytes

TILES = {WALK_CASES[0]: 21279, WALK_CASES[1]: 35465, WALK_CASES[2]: 42039, WALK_CASES[3]: 21279, WALK_CASES[4]: 2175}


@pytest.mark.parametrize("case", WALK_CASES)
def test_every_walk_case_meets_its_row_of_the_table(case):
    n, cin, h, w, cout, stride = case
    p = plans(case)
    assert tile_count(n, h, w, stride) == TILES[case]
    assert TILES[case] % 2 == 1                                    # the last tile pair is half empty
    assert out_map(h, w, stride)[1] % 16 != 0 and w % 16 != 0     # every row ends in a partial segment
    assert n * h * w < 1 << 24 and n * h * w * cin * 4 < 1 << 31   # csm_supported's own limits
    want_fd, want_wg = WALK_VISITS[case]
    for kind in ("fwd", "dgrad"):
        if want_fd is None:
            assert p[kind] is None, (case, kind)
            continue
        q = p[kind]
        assert q is not None and q.tiles == TILES[case]
        assert (q.vmin, q.vmax) == want_fd, (case, kind, q)
        assert q.vmax >= 3                                         # a third visit: half 0 runs, half 1 breaks (or runs again)
        assert q.vmin < q.vmax                                     # some waves stop one visit earlier
        assert q.grid == q.cap
    q = p["wgrad"]
    assert q is not None and q.units == (TILES[case] + 1) // 2
    assert (q.vmin, q.vmax) == want_wg, (case, q)
    assert q.vmax >= 3 and q.vmin < q.vmax and q.grid == q.cap


def test_two_full_rounds_of_the_double_buffer_are_covered():
    # four visits = both halves of the loop body twice, the fifth starts a third round and breaks in its middle
    assert any(plans(c)["fwd"] is not None and plans(c)["fwd"].vmin >= 4 for c in WALK_CASES)
    # every kernel of the file is walked by some case
    seen = {q.kernel for c in WALK_CASES for q in plans(c).values() if q is not None}
    assert seen == {"csm_conv<16>", "csm_conv<32>", "csm_conv_s2", "csm_dgrad_s2", "csm_wgrad<16>", "csm_wgrad<32>",
                    "csm_wgrad_s2<16>", "csm_wgrad_s2<32>"}


@pytest.fixture
def x3_arith():
    """The library's host-side queries follow the option conv_arith; 1 (bf16x3) selects conv_small.hip."""
    lib = dmcnet_amd._lib.load()
    before = lib.dmc_get_option(b"conv_arith")
    dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_arith", 1), "dmc_set_option")
    yield lib
    dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_arith", before), "dmc_set_option")


def test_the_mirror_is_the_library(x3_arith):
    lib = x3_arith
    for case in WALK_CASES:
        n, cin, h, w, cout, stride = case
        assert lib.dmc_conv_nhwc_supported(n, h, w, cin, cout, 3, 3, stride, 1) == 1, case
        q = plans(case)["fwd"]
        if q is not None:
            assert lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, 3, stride, 1) == q.grid, case
    for case in WALK_CASES[:2]:
        n, cin, h, w, cout, stride = case
        q = plans(case)["wgrad"]
        assert q.grid == 768
        assert lib.dmc_conv_nhwc_wgrad_bytes(n, h, w, cin, cout, 3, 3, stride, 1) == q.grid * cout * 9 * cin * 4 + 16, case
    for case in WALK_CASES:                                        # every case's workspace holds its kernel's partials
        n, cin, h, w, cout, stride = case
        got = lib.dmc_conv_nhwc_wgrad_bytes(n, h, w, cin, cout, 3, 3, stride, 1)
        assert got == wgrad_workspace_bytes(case), case
        assert got >= plans(case)["wgrad"].grid * cout * 9 * cin * 4, case


def _disc_block_unit_shapes():
    """The shapes test_disc_block_unit gives the NHWC convolutions: n = 5 frames of hw x (hw + 3), from its own parameter list."""
    from tests import test_hip_parity
    marks = [m for m in test_hip_parity.test_disc_block_unit.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "first,cin,cout,stride,use_bn,hw"
    return [(5, cin, hw, hw + 3, cout, stride) for first, cin, cout, stride, _, hw in marks[0].args[1] if not first]


def test_record_of_the_gap_no_other_unit_test_walks():
    """Every conv_small.hip shape of CONV_CASES and of test_disc_block_unit gives each wave at most ONE tile or tile pair:
    the loops of those kernels run as loops only at the shapes of this file (and in the 240-frame GAN step)."""
    from tests.test_hip_parity import CONV_CASES
    shapes = [(n, cin, h, w, cout, stride) for n, cin, h, w, cout, k, stride in CONV_CASES if k == 3]
    shapes += _disc_block_unit_shapes()
    # test_discriminator_train_mode_vs_oracle: 4 frames of 224 x 224 through blocks 16 -> 16 (112 x 112), 16 -> 32 / 2, 32 -> 32 (56 x 56)
    shapes += [(4, 16, 112, 112, 16, 1), (4, 16, 112, 112, 32, 2), (4, 32, 56, 56, 32, 1), (4, 32, 56, 56, 64, 2)]
    reached = set()
    for case in shapes:
        for kind, q in plans(case).items():
            if q is None:
                continue
            reached.add(q.kernel)
            assert q.vmax <= 1, (case, kind, q)
    # they do reach the kernels -- at one visit
    assert {"csm_conv<16>", "csm_conv<32>", "csm_conv_s2", "csm_dgrad_s2", "csm_wgrad<16>", "csm_wgrad<32>", "csm_wgrad_s2<16>",
            "csm_wgrad_s2<32>"} <= reached
    # test_disc_block_unit's only 16 -> 32 case has an odd height: the stride-2 forward epilogue is not in it
    assert all(plans(c)["fwd"] is None for c in _disc_block_unit_shapes() if c[5] == 2)
