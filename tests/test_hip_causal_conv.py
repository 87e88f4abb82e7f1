"""The NextItNet block node alone on the GPU (Fh.causal_conv_block over csrc/causal_conv.hip): forward + backward of every case of
tests/test_nextitnet_host.py's CASES in full mode and in last mode against float64 autograd of that file's restatement on `out`,
`dx` and every parameter gradient, at the project's bar 1e-4 max(1e-2, max |ref|) per tensor; each run twice with equal bits;
the launch counters against the numbers DESIGN.md §23 documents (forward 2; backward 7 two-masked, 9 one-masked), the same
at B = 1 and B = 70, with the torch-path count unchanged; exact zeros in the weight gradients of taps that read padding only;
the ill-conditioned widths for finiteness and bit-identity; one case outside the kernel's limits on the counted torch path."""
import warnings

import pytest
import torch

from conftest import require_gpu
from test_nextitnet_host import CASES, ILL, bar, case_inputs, f64_results, run_block

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def launches(one_masked):
    """(forward, backward) launches of one block, whatever B: repack + block; repack + block + 2 per conv + the gamma / beta sum"""
    return 2, 3 + 2 * (3 if one_masked else 2)


def counted_run(case, mode):
    from rec_pangu_amd import hip
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = run_block(case, mode, DEV)
    torch.cuda.synchronize()
    return got, hip.launch_count() - n0, hip.torch_path_count() - t0


@pytest.mark.parametrize("mode", ["full", "last"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_block_against_float64(case, mode):
    require_gpu()
    one, C, k, d, Ls, B = case
    ref = f64_results(case)[mode]
    got, n, t = counted_run(case, mode)
    assert n == sum(launches(one)) and t == 0, (n, t)
    assert set(got) == set(ref)
    worst = 0.0
    for key, want in ref.items():
        err = float((got[key].double() - want).abs().max())
        worst = max(worst, err / bar(want))
        print(f"{case} {mode} {key}: max err {err:.3g} against bar {bar(want):.3g}")
        assert got[key].shape == want.shape and err <= bar(want), (key, err, bar(want))
    print(f"{case} {mode}: worst tensor at {worst:.3g} of the bar")
    again, n2, _ = counted_run(case, mode)
    assert n2 == n and all(torch.equal(got[key], again[key]) for key in got)  # two runs, the same bits
    if d >= Ls and k > 1:  # every tap but the last reads padding only: exact zeros, not small numbers
        for slot in ((1,) if one else (0, 1)):
            assert float(got[f"p{slot}"][:, :, :k - 1].abs().max()) == 0.0 and float(got[f"p{slot}"][:, :, k - 1].abs().max()) > 0


@pytest.mark.parametrize("mode", ["full", "last"])
@pytest.mark.parametrize("case", ILL, ids=str)
def test_a_layernorm_over_two_channels_is_finite_and_reproducible(case, mode):
    require_gpu()
    got, n, t = counted_run(case, mode)
    again, _, _ = counted_run(case, mode)
    assert n == sum(launches(case[0])) and t == 0
    for key, v in got.items():
        assert torch.isfinite(v).all() and torch.equal(v, again[key]), key


@pytest.mark.parametrize("one_masked", [0, 1])
def test_the_launch_count_does_not_depend_on_the_batch(one_masked):
    require_gpu()
    for mode in ("full", "last"):
        counts = [counted_run((one_masked, 16, 3, 2, 9, B), mode)[1:] for B in (1, 70)]
        assert counts[0] == counts[1] == (sum(launches(one_masked)), 0), (mode, counts)


def test_positions_behind_the_length_take_no_gradient_and_last_mode_writes_every_position():
    require_gpu()
    case = (0, 8, 3, 2, 7, 70)
    _, _, lens, _, _ = case_inputs(case)
    behind = torch.arange(7)[None, :] >= lens[:, None]
    for mode in ("full", "last"):
        dx = run_block(case, mode, DEV)["dx"]
        assert float(dx[behind].abs().max()) == 0.0 and float(dx[~behind].abs().max()) > 0
    # last mode at dilation 2: the read row depends on positions anchor - 2 i only; every other position holds an exact zero
    dx = run_block(case, "last", DEV)["dx"]
    anchor = torch.where(lens > 0, lens - 1, torch.full_like(lens, 6))
    off_grid = ((anchor[:, None] - torch.arange(7)[None, :]) % 2 != 0) | (torch.arange(7)[None, :] > anchor[:, None])
    assert float(dx[off_grid].abs().max()) == 0.0


def test_outside_the_limits_the_torch_path_is_counted_and_matches():
    require_gpu()
    from rec_pangu_amd import hip
    case = (0, 130, 3, 1, 8, 2)  # wider than the kernel takes
    assert not hip.causal_conv_fits(8, 130, 3, False)
    for mode in ("full", "last"):
        ref = f64_results(case)[mode]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got, n, t = counted_run(case, mode)
        assert (n, t) == (0, 1)
        for key, want in ref.items():
            assert float((got[key].double() - want).abs().max()) <= bar(want), key
