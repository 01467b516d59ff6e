"""Pins tests/reward_any_restate.py - the float64 restatement the device tests of rlt_reward_any_loss compare against - without a
GPU: to tests/loss_restate.py where the two overlap (F_1 is the F1 reward, gain (penalty, 1) is the DCG reward, the four losses
on that reward), to torch's float64 autograd for d(loss)/dp, and to a brute-force search over orderings for the ideal value;
and RewardSpec.parse to the text forms it documents."""
import itertools

import numpy as np
import pytest
import torch

import loss_restate as L
import reward_any_restate as R


def _labels(B, S, seed, grades=2):
    rng = np.random.default_rng(seed)
    y = (rng.random((B, S)) < 0.3).astype(np.float64) * rng.integers(1, grades, (B, S))
    y[0] = 0.0                                      # a list without a relevant document
    if B > 1:
        y[1] = grades - 1
    return y


def _p(B, S, seed):
    rng = np.random.default_rng(seed)
    e = np.exp(rng.normal(size=(B, S + 1)) * 2.0)
    return (e / e.sum(1, keepdims=True))[:, :S]     # strictly positive


@pytest.mark.parametrize("S", [1, 7, 40, 300])
def test_fbeta_one_is_the_f1_reward(S):
    y = _labels(6, S, S)
    assert np.abs(R.reward64(y, R.fbeta(1.0)) - L.reward(y, "f1")).max() <= 1e-15


@pytest.mark.parametrize("S", [1, 7, 40, 300])
@pytest.mark.parametrize("pen", [-1.0, -0.5, 0.0])
def test_gain_penalty_one_is_the_dcg_reward(S, pen):
    y = _labels(6, S, S + 1)
    assert np.abs(R.reward64(y, R.gain((pen, 1.0))) - L.reward(y, "dcg", pen)).max() <= 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("metric", ["f1", "dcg"])
def test_matrix_loss_is_the_reward_loss(kind, metric):
    for S, tau in ((1, 1.0), (5, 0.85), (40, 0.95), (300, 0.85)):
        y, p = _labels(5, S, 3 * S), _p(5, S, S + 11)
        per, loss, dp, r, _q = L.reward_loss(p, y, metric, kind, tau)
        got = R.loss(p, r, kind, tau)
        assert abs(got["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
        assert np.abs(got["per_list"] - per).max() <= 1e-12 * max(1.0, np.abs(per).max())
        assert np.abs(got["dp"] - dp).max() <= 1e-12 * max(1.0, np.abs(dp).max())


@pytest.mark.parametrize("kind", R.KINDS)
def test_dp_is_the_gradient_of_the_loss(kind):
    y, p = _labels(4, 23, 5, grades=3), _p(4, 23, 6)
    for spec, tau in ((R.fbeta(2.0), 0.85), (R.gain((-1, 1, 3), normalize=True), 0.95)):
        r = R.reward(y, spec)
        got = R.loss(p, r, kind, tau)
        pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        rt = torch.tensor(r.astype(np.float64))
        q = torch.softmax(rt / tau, dim=1)
        if kind == R.EXPECT:
            per = -(pt * rt).sum(1)
        elif kind == R.CE:
            per = -(q * pt.log()).sum(1)
        elif kind == R.KL:
            per = (q * (q.log() - pt.log())).sum(1)
        else:
            m = (pt + q) / 2
            per = 0.5 * ((q * (q.log() - m.log())).sum(1) + (pt * (pt.log() - m.log())).sum(1))
        loss = per.sum() / p.shape[0]
        loss.backward()
        assert abs(got["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        assert np.abs(got["dp"] - pt.grad.numpy()).max() <= 1e-12 * max(1.0, float(pt.grad.abs().max()))


def test_ideal_equals_brute_force_maximum_of_cum_s():
    """Non-increasing non-negative discounts, 3 grades, S <= 7: with no negative gain, ideal is the brute-force maximum of cum_S
    over all orderings of the list; with negative gains - which the ideal list leaves out - it is the maximum over all orderings
    of the best prefix value max(0, max_k cum_k)."""
    rng = np.random.default_rng(8)
    for S in range(1, 8):
        d = np.sort(rng.random(S))[::-1].copy()
        for gains in ((1.0, 2.0, 3.0), (0.5, 0.25, 4.0), (0.0, 1.0, 1.0), (0.0, 0.0, 0.0)):
            spec = R.gain(gains, discount=d, normalize=True)
            y = rng.integers(0, 3, (4, S)).astype(np.float64)
            got = R.ideal(y, spec)
            for b in range(4):
                g = [gains[int(t)] for t in y[b]]
                best = max(sum(gi * di for gi, di in zip(perm, d)) for perm in set(itertools.permutations(g)))
                assert abs(got[b] - best) <= 1e-12
        for gains in ((-1.0, 1.0, 3.0), (-1.0, -2.0, 0.5), (-1.0, -2.0, -3.0)):
            spec = R.gain(gains, discount=d, normalize=True)
            y = rng.integers(0, 3, (4, S)).astype(np.float64)
            got = R.ideal(y, spec)
            for b in range(4):
                g = [gains[int(t)] for t in y[b]]
                best = max(max(np.cumsum([gi * di for gi, di in zip(perm, d)]).max(), 0.0) for perm in set(itertools.permutations(g)))
                assert abs(got[b] - best) <= 1e-12


def test_normalised_reward_of_the_ideal_list_reaches_one():
    y = np.array([[2.0, 2.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    r = R.reward64(y, R.gain((-1.0, 1.0, 3.0), normalize=True))
    assert r[0].max() == pytest.approx(1.0, abs=1e-15) and np.argmax(r[0]) == 2
    assert np.all(r[1] == 0.0)                      # ideal 0: the reward is 0, not a division by zero


def test_grades_round_clamp_and_nan():
    y = np.array([[-3.0, 0.4, 0.6, 1.5, 2.5, 7.0, np.nan]])
    assert R.grades(y, 3).tolist() == [[0, 0, 1, 2, 2, 2, 0]]


@pytest.mark.parametrize("text", ["fbeta:2", "fbeta:0.5", "ndcg", "ndcg:-0.5", "gain:-1,1,3", "gain:-1,1,3:norm", "gain:0,1"])
def test_parse_round_trips(text):
    from utils.rewards import RewardSpec
    from rlt_hip import native as N
    spec, want = RewardSpec.parse(text), R.parse(text)
    assert (spec.family == N.REWARD_FBETA) == (want.family == "fbeta")
    if want.family == "fbeta":
        assert spec.beta == want.beta
    else:
        assert spec.gains == want.gains and spec.normalize == want.normalize and spec.discount is None
    again = RewardSpec.parse(str(spec))
    assert again == spec and str(again) == str(spec)
    assert RewardSpec.parse(spec) is spec and RewardSpec.is_spec(text) and RewardSpec.is_spec(spec)


def test_parse_names_the_constructors():
    from utils.rewards import RewardSpec
    assert RewardSpec.parse("fbeta:2") == RewardSpec.fbeta(2.0)
    assert RewardSpec.parse("ndcg") == RewardSpec.ndcg() == RewardSpec.gain((-1.0, 1.0), None, True)
    assert RewardSpec.parse("ndcg:-0.5") == RewardSpec.ndcg(-0.5)
    assert RewardSpec.parse("gain:-1,1,3:norm") == RewardSpec.gain((-1, 1, 3), normalize=True)
    assert RewardSpec.parse("gain:-1,1,3") != RewardSpec.gain((-1, 1, 3), normalize=True)
    assert not RewardSpec.is_spec("f1") and not RewardSpec.is_spec("dcg") and not RewardSpec.is_spec("nci")


@pytest.mark.parametrize("text", ["", "fbeta", "fbeta:", "fbeta:0", "fbeta:-1", "fbeta:x", "fbeta:nan", "ndcg:x", "gain", "gain:", "gain:1",
                                  "gain:1,,2", "gain:1,2:normal", "gain:1,2:norm:norm", "gain:1,2,3,4,5,6,7,8,9", "gain:1,inf", "f2", "dcg:1",
                                  "fbeta:1:2"])
def test_parse_rejects(text):
    from utils.rewards import RewardSpec
    with pytest.raises(ValueError):
        RewardSpec.parse(text)
    with pytest.raises(ValueError):
        RewardSpec.parse(None)
