"""The eleven kernels of csrc/wass.hip through the C ABI (rlt_wass_loss_workspace / _fwd / _bwd) against the float64 Sinkhorn
restatement of tests/wass_restate.py, one test id per row of its case table: B 1, 2, 3 (empty row lanes of the column
kernels), 63, 64, 65 (the 64-column block edge), 255, 256, 257 (the 256-thread stride of the row kernels, a second blockIdx.y
of the cost kernel, eb = 2), S 1 and S 300 (two trips of the cost kernel's staging loop), each at eps 1e-1 and 1e-3 and at
softmax scale 1 and 6.

`thresh` is chosen per case from the float64 stop sums (wass_restate.choose_stop), so that float32 and float64 stop at the same
iteration; tests/test_wass_restate.py checks on the CPU that one iteration more or fewer could not pass.  The tolerance is
measured per case (wass_restate.yardstick): four times the error of the same loop in torch float32 on the CPU against float64,
largest of five seeds, never below sixteen float32 ulps.  Three measures are checked (wass_restate.errors): the loss, dp over
the whole matrix, and dp row by row.  Each measure is held to four times float32's own error in that measure: the row measure
divides by as little as 1e-3 of the largest |dp|, and torch float32 itself is up to a thousand times further from float64 in
it than in the matrix norm, so the matrix-norm yardstick is one no float32 loop can meet row by row.

Also here: exhaustion of max_iter without a stop, the default threshold 0.1 through utils.losses.WassDistLoss with a gscale
other than 1, gscale NULL, a NaN-filled workspace behind NaN sentinels, reuse of a workspace that holds a longer history,
determinism, and the workspace size check.  rlt_wass_loss_bwd with a larger max_iter than the forward call is out of scope:
the workspace layout depends on max_iter, so the two calls must name the same one, and that is not tested.

What these tests found: with the sweep seeded as first written (gC = pi (1 - C / eps), gu and gv = sum pi C / eps) seven ids
exceeded 4x the yardstick in dp while loss and stop iteration were right - B2_S40_eps0.001_scale1 9.7x, the four B65_S1 cases
12.5x and 35x, the default-threshold cases B2_S40_eps0.001 4.08x and B257_S300_eps0.1 5.1x: terms of size pi C / eps entered gC
before they cancelled.  csrc/wass.hip now seeds the sweep with C - c_j, c_j the pi-weighted centre of column j (see its header);
the largest ratio is 3.4x (profiles/wass_restate_margins.md).

With RLT_WASS_MARGINS=<path> the measured table (K, thresh, yardstick, device errors) is written there as markdown; a copy of
one run is kept in profiles/wass_restate_margins.md."""
import os

import numpy as np
import pytest
import torch

import wass_restate as wr

pytestmark = pytest.mark.gpu

GUARD = 256          # sentinel floats behind every buffer
E_WORKSPACE = -3     # RLT_E_WORKSPACE
MID = "B65_S40_eps0.001_scale1"      # the mid-sized case of the structural tests
_ROWS = []


@pytest.fixture(scope="module")
def N():
    from rlt_hip import native
    native.load()
    yield native
    path = os.environ.get("RLT_WASS_MARGINS")
    if path and _ROWS:
        with open(path, "w") as f:
            f.write("| case | K | device K | thresh | yardstick loss | dp | row | device loss | dp | row | worst device / yardstick |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in _ROWS:
                f.write("| " + " | ".join(r) + " |\n")


def guarded(nbytes, dev):
    """NaN-filled float buffer of at least nbytes, NaN sentinels behind it -> (buffer, sentinel view)"""
    n = (max(int(nbytes), 16) + 3) // 4
    full = torch.full((n + GUARD,), float("nan"), device=dev)
    return full[:n], full[n:]


def iterations_done(ws, B, max_iter):
    """state[1] of the workspace (C | gC | four histories of (max_iter + 1) rows | du gu gv rowpart | state)"""
    off = 2 * B * B + 4 * (max_iter + 1) * B + 4 * B
    return int(ws.view(torch.int32)[off + 1].item())


def run(N, c, max_iter=wr.MAX_ITER, thresh=None, gscale=None, ws=None):
    """fwd + bwd through the C ABI -> loss (1,), dp (B,S), iterations done, all on the host; `ws` to reuse a workspace"""
    dev = torch.device("cuda")
    B, S = c["B"], c["S"]
    p, y = c["p"].to(dev), c["y"].to(dev)
    nbytes = N.query("rlt_wass_loss_workspace", B, max_iter)
    assert nbytes >= (2 * B * B + 4 * (max_iter + 1) * B + 4 * B) * 4 + 8
    if ws is None:
        ws = torch.zeros((nbytes + 3) // 4, device=dev)
    loss, dp = torch.full((1,), float("nan"), device=dev), torch.full((B, S), float("nan"), device=dev)
    thresh = c["thresh"] if thresh is None else thresh
    N.call("rlt_wass_loss_fwd", N.ptr(p), N.ptr(y), B, S, c["eps"], max_iter, thresh, N.ptr(loss), N.ptr(ws), nbytes, N.stream())
    N.call("rlt_wass_loss_bwd", N.ptr(p), N.ptr(y), N.ptr(gscale), B, S, c["eps"], max_iter, N.ptr(ws), nbytes, N.ptr(dp), N.stream())
    torch.cuda.synchronize()
    return loss.cpu(), dp.cpu(), iterations_done(ws, B, max_iter)


def judge(tag, c, loss, dp, k_dev, gain=1.0):
    """print the figures, record them for the margins table, then assert the three measures against the case's tolerances"""
    errs = wr.errors(float(loss) / gain, dp.double().numpy() / gain, c["loss64"], c["dp64"])
    worst = max(e / max(y, wr.FLOOR / wr.FACTOR) for e, y in zip(errs, c["yard"]))
    print(f"{tag}: K={c['K']} device K={k_dev} thresh={c['thresh']:.4g} yardstick={c['yard']} device={errs} tol={c['tol']}")
    _ROWS.append([tag, str(c["K"]), str(k_dev), f"{c['thresh']:.4g}"] + [f"{v:.2e}" for v in c["yard"]] + [f"{v:.2e}" for v in errs]
                 + [f"{worst:.2f}"])
    assert np.isfinite(dp.numpy()).all() and np.isfinite(float(loss))
    assert errs[0] <= c["tol"][0], ("loss", errs, c["tol"])
    assert errs[1] <= c["tol"][1], ("dp", errs, c["tol"])
    assert errs[2] <= c["tol"][2], ("dp row", errs, c["tol"])


@pytest.mark.parametrize("name", list(wr.CASES))
def test_case(N, name):
    c = wr.prepare(name)
    loss, dp, k_dev = run(N, c)
    judge(name, c, loss, dp, k_dev)
    if not wr.degenerate(c["B"], c["S"]):          # there the stop sum is rounding noise and the iteration is not observable
        assert k_dev == c["K"]


@pytest.mark.parametrize("name", list(wr.EXHAUST))
def test_exhaustion_without_a_stop(N, name):
    c = wr.prepare_exhaust(name)
    loss, dp, k_dev = run(N, c, max_iter=wr.EXHAUST_ITERS, thresh=0.0)
    assert k_dev == wr.EXHAUST_ITERS
    judge("exhaust_" + name, c, loss, dp, k_dev)


@pytest.mark.parametrize("name", list(wr.DEFAULT_CASES))
def test_default_threshold_through_the_loss_module(N, name):
    """the path run.py takes: thresh 0.1 fixed by ops.WassDistLossFn, gscale a non-null pointer to 3"""
    from utils import losses as hl
    c = wr.prepare_default(name)
    dev = torch.device("cuda")
    p = c["p"].to(dev).unsqueeze(2).requires_grad_(True)
    loss = hl.WassDistLoss(eps=c["eps"], max_iter=wr.MAX_ITER)(p, c["y"].to(dev))
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    assert tuple(p.grad.shape) == (c["B"], c["S"], 1)
    judge("default_" + name, c, loss.detach().cpu() * 3.0, p.grad.squeeze(2).cpu(), "-", gain=3.0)


def test_null_gscale_is_one(N):
    c = wr.prepare(MID)
    loss0, dp0, _ = run(N, c, gscale=None)
    loss1, dp1, _ = run(N, c, gscale=torch.ones(1, device="cuda"))
    assert torch.equal(loss0, loss1) and torch.equal(dp0, dp1)
    _, dp3, _ = run(N, c, gscale=torch.full((1,), 3.0, device="cuda"))
    assert float((dp3 - 3.0 * dp0).abs().max()) <= 4 * 2.0 ** -24 * float(dp3.abs().max())


def test_nan_workspace_and_sentinels(N):
    """nothing reads history it has not written, nothing writes past a buffer"""
    c = wr.prepare(MID)
    dev, B, S = torch.device("cuda"), c["B"], c["S"]
    p, y = c["p"].to(dev), c["y"].to(dev)
    nbytes = N.query("rlt_wass_loss_workspace", B, wr.MAX_ITER)
    ws, ws_end = guarded(nbytes, dev)
    loss, loss_end = guarded(4, dev)
    dp, dp_end = guarded(4 * B * S, dev)
    N.call("rlt_wass_loss_fwd", N.ptr(p), N.ptr(y), B, S, c["eps"], wr.MAX_ITER, c["thresh"], N.ptr(loss), N.ptr(ws), nbytes, N.stream())
    N.call("rlt_wass_loss_bwd", N.ptr(p), N.ptr(y), None, B, S, c["eps"], wr.MAX_ITER, N.ptr(ws), nbytes, N.ptr(dp), N.stream())
    torch.cuda.synchronize()
    k_dev = iterations_done(ws, B, wr.MAX_ITER)
    assert bool(torch.isnan(loss[1:]).all())          # guarded() rounds one float up to four
    judge("nan_workspace", c, loss[:1].cpu(), dp[:B * S].reshape(B, S).cpu(), k_dev)
    assert k_dev == c["K"]
    for end in (ws_end, loss_end, dp_end):
        assert bool(torch.isnan(end).all()), "sentinel overwritten"


def test_workspace_reuse_after_a_longer_run(N):
    """stale hu / hv / lrow / lcol rows beyond K, and `state`, from a run that went on for 20 iterations"""
    c = wr.prepare(MID)
    assert c["K"] < 20
    fresh = run(N, c, max_iter=20)
    nbytes = N.query("rlt_wass_loss_workspace", c["B"], 20)
    ws = torch.zeros((nbytes + 3) // 4, device="cuda")
    long_run = run(N, c, max_iter=20, thresh=0.0, ws=ws)
    assert long_run[2] == 20 and not torch.equal(long_run[1], fresh[1])
    again = run(N, c, max_iter=20, ws=ws)
    assert again[2] == fresh[2] == c["K"]
    assert torch.equal(again[0], fresh[0]) and torch.equal(again[1], fresh[1])
    relong = run(N, c, max_iter=20, thresh=0.0, ws=ws)          # the stop flag the short run left set must not survive
    assert relong[2] == 20 and torch.equal(relong[0], long_run[0]) and torch.equal(relong[1], long_run[1])


def test_determinism(N):
    """csrc/wass.hip: all reductions in a fixed order"""
    c = wr.prepare("B257_S7_eps0.001_scale1")
    a, b = run(N, c), run(N, c)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_short_workspace_is_refused(N):
    c = wr.prepare(MID)
    dev, B, S = torch.device("cuda"), c["B"], c["S"]
    p, y = c["p"].to(dev), c["y"].to(dev)
    nbytes = N.query("rlt_wass_loss_workspace", B, wr.MAX_ITER)
    ws = torch.full(((nbytes + 3) // 4,), float("nan"), device=dev)
    loss, dp = torch.full((1,), float("nan"), device=dev), torch.full((B, S), float("nan"), device=dev)
    lib = N.load()
    assert lib.rlt_wass_loss_fwd(N.ptr(p), N.ptr(y), B, S, c["eps"], wr.MAX_ITER, c["thresh"], N.ptr(loss), N.ptr(ws), nbytes - 1,
                                 N.stream()) == E_WORKSPACE
    assert lib.rlt_wass_loss_bwd(N.ptr(p), N.ptr(y), None, B, S, c["eps"], wr.MAX_ITER, N.ptr(ws), nbytes - 1, N.ptr(dp),
                                 N.stream()) == E_WORKSPACE
    torch.cuda.synchronize()
    for t in (ws, loss, dp):
        assert bool(torch.isnan(t).all()), "written despite the refusal"
