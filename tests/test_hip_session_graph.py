"""The session-graph kernels alone on the GPU (csrc/session_graph.hip): rp_session_graph bit for bit against the CPU path,
the gated graph cell forward and backward against the float64 dense-adjacency statement of tests/test_srgnn_host.py
(the project's per-tensor bar 1e-4 max(1e-2, max |ref|)), bit-identical runs, launch and torch-path counts, one shape just
outside the declared geometry on the counted torch path, and the row L2 normalisation with zero rows.

Shapes: L = 1 (no transition anywhere), 2, 5, 20 (three samples per workgroup), 50 (one sample per workgroup, a padded tile);
B = 1, 7 (a partial last workgroup at every L but 1 and 50) and 300; D = 12 (one padded column tile), 64, 128 (the largest
tile).  The float64 reference of every shape is computed once per module."""
import functools
import warnings

import pytest
import torch

from conftest import require_gpu
from test_srgnn_host import cell_dense, cell_params, l2_f64, random_sessions, within

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- rp_session_graph ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("Lh", [1, 2, 20, 50])
def test_session_graph_is_the_cpu_path_bit_for_bit(B, Lh):
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    gen = torch.Generator().manual_seed(B * 100 + Lh)
    hist = random_sessions(B, Lh, 9, gen)          # rows: a single item, full, all items equal, empty, a repeated transition
    if B > 5:
        hist[5] = torch.arange(1, Lh + 1)          # all distinct, descending ids below
        hist[6] = torch.arange(Lh, 0, -1) + 2 ** 31 - Lh // 2  # ids on both sides of 2^31
        if Lh >= 4:
            hist[-1, 1] = 0                        # a hole inside a session
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = Fh.session_graph(hist.to(DEV))
    torch.cuda.synchronize()
    assert hip.launch_count() == n0 + 1 and hip.torch_path_count() == t0
    want = Fh.session_graph(hist)
    for name, a, b in zip(("nodes", "alias", "count", "indeg", "outdeg"), got, want):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b), name


def test_session_graph_beyond_the_kernels_length_takes_the_counted_torch_path():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    Lh = hip.session_graph_geometry()["max_l"] + 1
    hist = random_sessions(5, Lh, 9, torch.Generator().manual_seed(0))
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = Fh.session_graph(hist.to(DEV))
    assert hip.launch_count() == n0 and hip.torch_path_count() == t0 + 1
    for a, b in zip(got, Fh.session_graph(hist)):
        assert torch.equal(a.cpu(), b)


# ---- the cell ------------------------------------------------------------------------------------------------------------------
CELL_SHAPES = [(1, 1, 64), (7, 1, 12), (7, 5, 64), (7, 5, 12), (300, 5, 12), (7, 20, 64), (300, 20, 64), (1, 20, 128),
               (7, 50, 12), (7, 50, 128), (1, 50, 64)]


@functools.lru_cache(maxsize=None)
def cell_case(B, Lh, Dh):
    """inputs and the float64 results of two chained steps + the read-back: computed once, shared, left unchanged"""
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(B * 1000 + Lh * 10 + Dh)
    hist = random_sessions(B, Lh, 7 if Lh <= 20 else 30, gen)
    _, alias, count, _, _ = Fh.session_graph(hist)
    h0 = torch.randn(B, Lh, Dh, generator=gen, dtype=torch.float64)
    w = [torch.randn(B, Lh, Dh, generator=gen, dtype=torch.float64), torch.randn(B, Dh, generator=gen, dtype=torch.float64),
         torch.randn(B, Lh, Dh, generator=gen, dtype=torch.float64)]
    p64 = cell_params(Dh, gen)
    ref = {}
    for steps in (1, 2):
        h = h0.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in p64]
        x = h
        for _ in range(steps - 1):
            x = cell_dense(x, alias, ps, False)
        seq, ht = cell_dense(x, alias, ps, True)
        ((seq * w[0]).sum() + (ht * w[1]).sum()).backward()
        ref[steps] = [t.detach() for t in [seq, ht, h.grad] + [p.grad for p in ps]]
    # one step that is not the final one: h' itself and its gradients
    h = h0.clone().requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in p64]
    hy = cell_dense(h, alias, ps, False)
    (hy * w[2]).sum().backward()
    ref[0] = [t.detach() for t in [hy, h.grad] + [p.grad for p in ps]]
    return alias, count, h0, w, p64, ref


def run_device(alias, h0, w, p64, steps):
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd.models.layers import SRGNNCell
    cell = SRGNNCell(h0.shape[-1]).to(DEV)
    with torch.no_grad():
        for p, v in zip(Fh._cell_params(cell), p64):
            p.copy_(v.to(torch.float32))
    h = h0.to(torch.float32).to(DEV).requires_grad_(True)
    al = alias.to(DEV)
    if steps == 0:
        hy = Fh.ggnn_cell(h, al, cell)
        (hy * w[2].to(torch.float32).to(DEV)).sum().backward()
        outs = [hy]
    else:
        seq, ht = cell.encode(al, h, steps)
        ((seq * w[0].to(torch.float32).to(DEV)).sum() + (ht * w[1].to(torch.float32).to(DEV)).sum()).backward()
        outs = [seq, ht]
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in outs + [h.grad] + [p.grad for p in Fh._cell_params(cell)]]


@pytest.mark.parametrize("steps", [0, 1, 2])
@pytest.mark.parametrize("B,Lh,Dh", CELL_SHAPES)
def test_cell_forward_and_backward_against_float64(B, Lh, Dh, steps):
    """steps 0: one step that is not the final one (h' and the gradient through dHout); 1 and 2: the chain ending in the
    read-back (the gradients through dseq_hidden and dht).  Every returned gradient; two runs with equal bits."""
    require_gpu()
    from rec_pangu_amd import hip
    alias, count, h0, w, p64, ref = cell_case(B, Lh, Dh)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    got = run_device(alias, h0, w, p64, steps)
    assert hip.torch_path_count() == t0 and hip.launch_count() - n0 >= 4 * max(steps, 1)
    again = run_device(alias, h0, w, p64, steps)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    names = (["h_out"] if steps == 0 else ["seq_hidden", "ht"]) + ["dh", "dW_in", "db_in", "dW_out", "db_out", "dW_ih", "db_ih",
                                                                     "dW_hh", "db_hh"]
    assert len(got) == len(ref[steps]) == len(names)
    for name, a, b in zip(names, got, ref[steps]):
        within(a, b, f"{B}x{Lh}x{Dh} steps {steps}: {name}")
    node = torch.arange(Lh)[None, :] < count[:, None]
    dh = got[1 if steps == 0 else 2]
    if (~node).any():
        assert float(dh[~node].abs().max()) == 0.0 and float(got[0][(alias < 0) if steps else ~node].abs().max()) == 0.0


def test_cell_forward_launches():
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.layers import SRGNNCell
    alias, _, h0, _, _, _ = cell_case(7, 20, 64)
    cell = SRGNNCell(64).to(DEV)
    h = h0.to(torch.float32).to(DEV)
    n0 = hip.launch_count()
    with torch.no_grad():
        Fh.ggnn_cell(h, alias.to(DEV), cell)
    assert hip.launch_count() - n0 == 2  # the padded weight copies + the cell


@pytest.mark.parametrize("Lh,Dh", [(65, 16), (6, 132)])
def test_a_shape_outside_the_geometry_takes_the_counted_torch_path(Lh, Dh):
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    from rec_pangu_amd.models.layers import SRGNNCell
    assert not hip.ggnn_fits(Lh, Dh)
    gen = torch.Generator().manual_seed(1)
    hist = random_sessions(5, Lh, 7, gen)
    alias = Fh.session_graph(hist)[1]
    torch.manual_seed(0)
    cell = SRGNNCell(Dh)
    h = torch.randn(5, Lh, Dh, generator=gen)
    want = cell.encode(alias, h, 1)
    dev = cell.to(DEV)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = dev.encode(alias.to(DEV), h.to(DEV), 1)
    assert hip.torch_path_count() == t0 + 1 and hip.launch_count() == n0
    within(got[0], want[0].detach(), "seq_hidden")
    within(got[1], want[1].detach(), "ht")


# ---- l2_normalize --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 4, 13, 301])
@pytest.mark.parametrize("Dh", [12, 64, 70])
def test_l2_normalize_forward_and_backward(M, Dh):
    require_gpu()
    from rec_pangu_amd import functional as Fh
    from rec_pangu_amd import hip
    gen = torch.Generator().manual_seed(M * 100 + Dh)
    x = torch.randn(M, Dh, generator=gen) * 3
    x[0] = 0                # a zero row: stays zero, passes a zero gradient
    if M > 2:
        x[2] = 1e-15        # a row below the clamp: dy / eps
    dy = torch.randn(M, Dh, generator=gen)
    xd = x.to(DEV).requires_grad_(True)
    n0, t0 = hip.launch_count(), hip.torch_path_count()
    y = Fh.l2_normalize(xd)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert hip.launch_count() == n0 + 2 and hip.torch_path_count() == t0
    wy, wdx = l2_f64(x, dy)
    keep = torch.ones(M, dtype=torch.bool)
    if M > 2:
        keep[2] = False     # (compared on its own scale: its gradient is 1e12 times dy)
        within(xd.grad[2] * 1e-12, wdx[2] * 1e-12, "dx of the row below the clamp")
        within(y[2], wy[2], "y of the row below the clamp")
    within(y[keep], wy[keep], "y")
    within(xd.grad[keep], wdx[keep], "dx")
    assert float(y[0].abs().max()) == 0.0 and float(xd.grad[0].abs().max()) == 0.0
    # any leading shape
    if M % 4 == 0 and M > 1:
        y3 = Fh.l2_normalize(x.to(DEV).view(M // 4, 4, Dh))
        assert y3.shape == (M // 4, 4, Dh) and torch.equal(y3.view(M, Dh), y.detach())
