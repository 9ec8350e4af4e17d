"""CPU: the kernel selection of conv_nhwc.hip as tests/conv_nhwc_plans.py restates it IS the library's (host queries only), the
cases of tests/test_conv_nhwc_cfgs_gpu.py and tests/test_conv_nhwc_wgrad_runs_gpu.py reach what they claim -- every tile
configuration that production selects, every row-walking weight-gradient kernel at three or more steps per workgroup -- and the
older unit tests reach none of it."""
import pytest

import dmcnet_amd
from tests import conv_nhwc_plans as P


@pytest.fixture
def options():
    """set(conv_arith, conv_cfg) on the library; both options are process-wide and restored afterwards."""
    lib = dmcnet_amd._lib.load()
    before = {name: lib.dmc_get_option(name) for name in (b"conv_arith", b"conv_cfg")}
    assert lib.dmc_get_option(b"conv_path") == 1                   # the mirror takes the default path

    def set_options(arith, cfg):
        dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_arith", arith), "dmc_set_option")
        dmcnet_amd._lib.check(lib.dmc_set_option(b"conv_cfg", cfg), "dmc_set_option")
        return lib

    yield set_options
    for name, value in before.items():
        dmcnet_amd._lib.check(lib.dmc_set_option(name, value), "dmc_set_option")


def _stat_blocks(lib, case):
    n, cin, h, w, cout, k, stride = case
    return lib.dmc_conv_nhwc_stat_blocks(n, h, w, cin, cout, k, stride, k // 2)


def _wgrad_bytes(lib, case):
    n, cin, h, w, cout, k, stride = case
    return lib.dmc_conv_nhwc_wgrad_bytes(n, h, w, cin, cout, k, k, stride, k // 2)


def _transposed(case):
    """The case whose FORWARD is the GEMM of one data-gradient class of a stride-1 case (Cin and Cout swapped): the library has
    no host query for the data gradient's tile, but its choice is the same function of (channels produced, pixels)."""
    n, cin, h, w, cout, k, stride = case
    return (n, cout, h, w, cin, k, 1)


# ---- the mirror is the library -----------------------------------------------------------------------------------------------------

def test_the_mirror_is_the_library_tile_choice(options):
    """dmc_conv_nhwc_stat_blocks = ceil(M / BM) of the mirror's choice, for every swept shape under every forced conv_cfg of the
    sweep (1 .. 13 and 1 .. 8, honoured or not) in both arithmetics, for the production shapes and the run cases."""
    checked = 0
    shapes = P.CFG_SHAPES + [_transposed(s) for s in P.CFG_SHAPES if s[6] == 1]
    for arith in (0, 1):
        for cfg in [0] + P.V3_FORCED + [11]:
            lib = options(arith, cfg)
            for case in shapes:
                assert _stat_blocks(lib, case) == P.stat_blocks(case, arith, cfg), (case, arith, cfg)
                checked += 1
        lib = options(arith, 0)
        for case in P.PRODUCTION + P.WGRAD_RUN_CASES + [P.GENERIC_SPLIT_CASE, P.V1_LARGE_CASE, P.V1_48_CASE]:
            if P.fwd_choice(case, arith).kernel != "conv_small":
                assert _stat_blocks(lib, case) == P.stat_blocks(case, arith), (case, arith)
                checked += 1
    assert checked > 200


def test_the_mirror_is_the_library_weight_gradient_plans(options):
    """dmc_conv_nhwc_wgrad_bytes = groups x Cout x KK x Cin x 4 + 16 of the mirror's plan: pins groups and, with it, per_group."""
    for arith in (0, 1):
        lib = options(arith, 0)
        cases = [c for c, a in P.WGRAD_RUN_SWEEP if a == arith] + [P.GENERIC_SPLIT_CASE, P.V1_LARGE_CASE]
        cases += [c for c in P.PRODUCTION if P.wgrad_plan(c, arith).kernel not in ("conv_small", "small")]
        for case in cases:
            n, cin, h, w, cout, k, stride = case
            p = P.wgrad_plan(case, arith)
            assert p.groups > 1
            assert _wgrad_bytes(lib, case) == p.groups * cout * k * k * cin * 4 + 16 == P.wgrad_bytes(case, arith), (case, arith, p)
            if p.per_group is not None:
                # groups pins per_group: it is the only length whose groups cover the steps with exactly that many workgroups
                fits = [pg for pg in range(1, p.steps + 1) if P.ceil_div(p.steps, pg) == p.groups]
                assert p.per_group == min(fits), (case, p)
                assert P.ceil_div(p.steps, P.ceil_div(p.steps, min(max(256 // p.tiles, 1), p.steps))) == p.groups


def test_forced_configurations_the_mirror_says_are_honoured():
    """The acceptance rules of conv_cfg, spelt out: 2 and 6 (configurations 1 and 5) for every Cout, 4 (configuration 3) for
    Cout % 256 == 0, 11 (configuration 10, removed) never, the others for Cout % 128 == 0."""
    assert [c for c in range(0, 15) if P.v3_honoured(c, 64)] == [2, 6]
    assert [c for c in range(0, 15) if P.v3_honoured(c, 128)] == [1, 2, 3, 5, 6, 7, 8, 9, 10, 12, 13]
    assert [c for c in range(0, 15) if P.v3_honoured(c, 256)] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13]
    assert [c for c in range(0, 15) if P.v2_honoured(c, 64)] == [1, 2, 3, 7, 8]
    assert [c for c in range(0, 15) if P.v2_honoured(c, 128)] == [1, 2, 3, 4, 5, 6, 7, 8]
    assert [c for c in range(0, 15) if P.v2_honoured(c, 32)] == []
    assert P.v3_choice(256, 297, 11) == P.v3_choice(256, 297, 0) == 6


# ---- record of the gap -------------------------------------------------------------------------------------------------------------

def _disc_block_unit_shapes():
    """The shapes test_disc_block_unit gives the NHWC convolutions: n = 5 frames of hw x (hw + 3), from its own parameter list."""
    from tests import test_hip_parity
    marks = [m for m in test_hip_parity.test_disc_block_unit.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "first,cin,cout,stride,use_bn,hw"
    return [(5, cin, hw, hw + 3, cout, 3, stride) for first, cin, cout, stride, _, hw in marks[0].args[1] if not first]


#: test_discriminator_train_mode_vs_oracle: 4 frames of 224 x 224 through the blocks behind the first
DISC_4_FRAMES = [(4, 16, 112, 112, 16, 3, 1), (4, 16, 112, 112, 32, 3, 2), (4, 32, 56, 56, 32, 3, 1), (4, 32, 56, 56, 64, 3, 2),
                 (4, 64, 28, 28, 64, 3, 1), (4, 64, 28, 28, 128, 3, 2), (4, 128, 14, 14, 128, 3, 1)]


def _reached(shapes):
    """{"conv3" | "conv2": configurations} and the largest per_group of a row-walking weight-gradient kernel, over both arithmetics
    under the automatic choice."""
    seen = {"conv3": set(), "conv2": set(), "conv_nhwc": set(), "conv_small": set()}
    per_group = {}
    for case in shapes:
        for arith in (0, 1):
            for c in P.launches(case, arith):
                seen[c.kernel].add(c.cfg)
            p = P.wgrad_plan(case, arith)
            if p.per_group is not None:
                per_group[p.kernel] = max(per_group.get(p.kernel, 0), p.per_group)
    return seen, per_group


def test_record_of_the_gap_older_unit_tests_reach_two_configurations_each():
    """CONV_CASES, test_disc_block_unit and the 4-frame discriminator choose only conv3 configurations 5 and 6, conv2
    configurations 0 and 2, never the 128-pixel first-generation tile or a split generic weight gradient, and give a
    weight-gradient workgroup at most two steps.  Asserted exactly, so that a change of those lists shows up here."""
    from tests.test_hip_parity import CONV_CASES
    shapes = list(CONV_CASES) + _disc_block_unit_shapes() + DISC_4_FRAMES
    seen, per_group = _reached(shapes)
    assert seen["conv3"] == {5, 6}
    assert seen["conv2"] == {0, 2}
    assert per_group == {"wgrad3<1>": 2, "wgrad3<2>": 2, "wgrad2<3,1>": 2, "wgrad2<3,2>": 1, "wgrad2<1,1>": 1, "wgrad2<1,2>": 1}
    for case in shapes:
        for arith in (0, 1):
            assert all(c.bm != 128 for c in P.launches(case, arith) if c.kernel == "conv_nhwc" and c.bn == 64), case
            p = P.wgrad_plan(case, arith)
            assert p.kernel != "generic" or p.groups == 1, case


# ---- production is covered ---------------------------------------------------------------------------------------------------------

def test_production_is_covered():
    """Every forward / data-gradient configuration the twelve production shapes select is one the GPU sweep launches, and every
    row-walking weight-gradient kernel they reach has a run case of three or more steps per workgroup."""
    assert len(P.PRODUCTION) == 12
    seen, per_group = _reached(P.PRODUCTION)
    swept = P.swept_configurations()
    assert seen["conv3"] == {1, 2, 5, 6, 11}                       # 256 x 64 (8 waves), 128 x 128 (4 x 2), 192 x 128, and the two of the gap
    assert seen["conv2"] == {0, 2, 3, 6, 8}
    assert seen["conv3"] <= swept["conv3"] and seen["conv2"] <= swept["conv2"]
    assert not seen["conv_nhwc"]
    # the sweep launches every configuration either switch statement has (conv3: 10 is gone; conv2: all nine)
    assert swept["conv3"] == set(P.V3_TILES) and swept["conv2"] == set(P.V2_TILES)
    assert min(per_group.values()) >= 7 and max(per_group.values()) == 105
    runs = {}
    for case, arith in P.WGRAD_RUN_SWEEP:
        p = P.wgrad_plan(case, arith)
        runs[p.kernel] = max(runs.get(p.kernel, 0), p.per_group)
    assert set(per_group) <= set(runs)
    assert all(runs[k] >= 3 for k in runs)
    assert set(runs) == {"wgrad3<1>", "wgrad3<2>", "wgrad2<3,1>", "wgrad2<3,2>", "wgrad2<1,1>", "wgrad2<1,2>"}


# ---- every run case meets its row --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", P.WGRAD_RUN_CASES)
def test_every_run_case_meets_its_row_of_the_table(case):
    kernel, steps, groups, per_group, last = P.WGRAD_RUNS[case]
    p = P.wgrad_plan(case, 1)
    assert (p.kernel, p.steps, p.groups, p.per_group, p.last) == (kernel, steps, groups, per_group, last)
    assert p.per_group >= 3                                         # both buffers are used twice
    assert (p.groups - 1) * p.per_group + p.last == p.steps and 1 <= p.last <= p.per_group


def test_the_run_cases_cover_short_last_groups_image_crossings_and_every_r():
    plans = {(c, a): P.wgrad_plan(c, a) for c, a in P.WGRAD_RUN_SWEEP}
    for (case, arith), p in plans.items():
        # three or more steps everywhere but the 14 x 14 stride-2 case under fp32 MFMA (9 steps of 7 rows in groups of 2: its
        # sibling of 20 images stands in)
        assert p.per_group >= 3 or (case, arith, p.per_group) == ((9, 256, 14, 14, 512, 3, 2), 0, 2), (case, arith, p)
    assert plans[(P.WGRAD2_S2_R7_CASE, 0)][:8] == ("wgrad2<3,2>", 7, 1, 20, 32, 7, 3, 2)
    for kernel in ("wgrad3<1>", "wgrad3<2>", "wgrad2<3,1>", "wgrad2<3,2>", "wgrad2<1,1>"):
        mine = [p for p in plans.values() if p.kernel == kernel and p.per_group >= 3]
        assert any(p.last < p.per_group for p in mine), kernel      # a last group shorter than the others
        assert any(P.crosses_images(p) > 0 for p in mine), kernel   # a run that moves to the next image
        if kernel != "wgrad2<1,1>":                                 # one row per step, and several
            assert any(p.r == 1 for p in mine) and any(p.r > 1 for p in mine), kernel
    p = plans[((25, 256, 14, 14, 256, 3, 1), 1)]
    assert P.crosses_images(p) == p.groups - 1                      # every full run of that case crosses (4 steps, 2 per image)
    assert plans[((20, 128, 28, 28, 256, 1, 2), 1)].per_group == 5 and P.crosses_images(plans[((20, 128, 28, 28, 256, 1, 2), 1)]) > 0
    # odd per_group: the run ends in the other buffer than an even one
    assert {p.per_group % 2 for p in plans.values()} == {0, 1}


def test_the_two_small_cases_reach_their_code(options):
    p = P.wgrad_plan(P.GENERIC_SPLIT_CASE, 1)
    assert (p.kernel, p.tiles, p.groups) == ("generic", 18, 3) and P.wgrad_plan(P.GENERIC_SPLIT_CASE, 0) == p
    from tests.test_hip_parity import CONV_CASES
    assert P.wgrad_plan((3, 48, 9, 7, 80, 3, 1), 1).groups == 1 and (3, 48, 9, 7, 80, 3, 1) in CONV_CASES
    for arith in (0, 1):
        c = P.fwd_choice(P.V1_LARGE_CASE, arith)
        assert (c.kernel, c.bm, c.bn, c.m) == ("conv_nhwc", 128, 64, 32768)
        (_, _, taps, d), = P.dgrad_choices(P.V1_LARGE_CASE, arith)
        assert (d.kernel, d.bm, d.bn, taps) == ("conv_nhwc", 128, 32, 9)
        # 48 output channels run on the 128 x 32 tile of launch_conv: the row count of the statistics is that tile's
        lib = options(arith, 0)
        n, cin, h, w, cout, k, stride = P.V1_48_CASE
        assert cout == 48 and _stat_blocks(lib, P.V1_48_CASE) == P.ceil_div(n * h * w, 128)
