"""CPU: the shape list of tests/test_x3s_wgrad_addr_gpu.py is accepted by the library's own plans and covers what it claims
(every width, N = 1, odd N, H != W, ragged last groups, several ci / co tiles)."""
import dmcnet_amd
from tests.wgrad_addr_shapes import X3Q_ADDR_CASES, X3S_ADDR_CASES, x3q_plan, x3s_plan


def test_every_address_case_is_supported_by_the_library():
    lib = dmcnet_amd._lib.load()
    for n, cin, h, w, cout in X3S_ADDR_CASES:
        p = x3s_plan(n, h, w, cin, cout)
        assert p is not None and lib.dmc_x3s_conv_wgrad_supported(n, h, w, cin, cout) == 1, (n, cin, h, w, cout)
        # the restated plan is the library's: the partials are [groups][Cout][9][Cin] floats (none for a single group)
        want = p["groups"] * cout * 9 * cin * 4 if p["groups"] > 1 else 0
        assert lib.dmc_x3s_conv_wgrad_bytes(n, h, w, cin, cout) == want, (n, cin, h, w, cout)
    for n, cin, h, w, cout in X3Q_ADDR_CASES:
        assert x3q_plan(n, h // 2, w // 2, cin, cout) is not None
        assert lib.dmc_x3q_conv_wgrad_supported(n, h // 2, w // 2, cin, cout) == 1, (n, cin, h, w, cout)


def test_address_cases_cover_the_corners():
    for width in (56, 28, 14, 7):
        cases = [c for c in X3S_ADDR_CASES if c[3] == width]
        plans = [x3s_plan(n, h, w, cin, cout) for n, cin, h, w, cout in cases]
        assert any(c[0] == 1 for c in cases), width
        assert any(c[0] % 2 == 1 and c[0] > 1 for c in cases), width
        assert width == 7 or any(c[2] != c[3] for c in cases), width
        assert any(p["steps"] % p["groups"] != 0 for p in plans), width          # a last group with fewer steps
        assert any(p["per_group"] > 1 for p in plans), width                      # the step-to-step walk is exercised
        assert any(c[1] != c[4] and p["tiles"] > 1 for c, p in zip(cases, plans)), width
    assert sorted({c[0] for c in X3Q_ADDR_CASES}) == [1, 3, 7]
    assert sorted({c[2] for c in X3Q_ADDR_CASES}) == [14, 28, 56]
