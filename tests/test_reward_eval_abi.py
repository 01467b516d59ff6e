"""The C ABI of the evaluation pass in any cut reward without a GPU (include/rlt_hip.h: rlt_reward_eval_workspace,
rlt_reward_eval): symbols declared, bound and exported, the workspace query answers without a device, and every bad argument is
answered with its documented code, in the documented order, before any launch - host buffers stand in for device memory,
nothing is launched.  Then the Python surface that needs no device: --eval-reward, compare_reports(metric='reward') on small
files, and a CutReport without `reward=`."""
import ctypes

import numpy as np
import pytest

ARG, SHAPE, WORKSPACE, ALIGN = -1, -2, -3, -4
NAMES = ("rlt_reward_eval_workspace", "rlt_reward_eval")


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def _buf(nbytes):
    raw = (ctypes.c_uint8 * (nbytes + 64))()
    return raw, (ctypes.addressof(raw) + 63) // 64 * 64


def test_symbols(native):
    lib = native.load()
    for name in NAMES:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.rlt_abi_version() == 5                                       # additions only
    assert len(native._SIGNATURES["rlt_reward_eval"][1]) == 20


def test_workspace_query(native):
    q = lambda B, S=40, T=3: native.query("rlt_reward_eval_workspace", B, S, T)
    for B, S, T in ((0, 40, 3), (-3, 40, 3), (6, 0, 3), (6, -1, 3), (6, 1025, 3), (6, 40, -1), (6, 40, 65)):
        assert q(B, S, T) == 0, (B, S, T)
    for S, T in ((1, 0), (40, 0), (40, 64), (300, 19), (1023, 1), (1024, 64)):
        last = 0
        for B in list(range(1, 70)) + [255, 256, 257, 4095, 4096, 4097, 100000, 1 << 20, (1 << 31) - 1]:
            assert q(B, S, T) >= last and q(B, S, T) >= 8 * (2 * S + 3 + 3 * T), (B, S, T)
            last = q(B, S, T)
    assert q(6, 40, 64) > q(6, 40, 0) and q(6, 1024, 3) > q(6, 40, 3)


class Call:
    """A valid call of rlt_reward_eval on host buffers; each test breaks one argument."""

    def __init__(self, native, B=6, S=40, T=3):
        self.native, self.lib = native, native.load()
        self.B, self.S, self.T = B, S, T
        self.keep = []

        def buf(nbytes):
            raw, base = _buf(nbytes)
            self.keep.append(raw)
            return base
        self.y, self.r = buf(4 * B * S), buf(4 * B * S)
        self.k, self.r_at, self.better = buf(4 * B * 64), buf(4 * B * 64), buf(4 * B * 64)
        self.best, self.best_k = buf(4 * B), buf(4 * B)
        self.curve, self.hist, self.sums = buf(8 * 1026), buf(8 * 1026), buf(8 * (3 + 3 * 64))
        self.table = buf(native.query("rlt_dcg_table_bytes"))
        self.ws_bytes = native.query("rlt_reward_eval_workspace", B, S, 64)
        self.ws = buf(self.ws_bytes)
        self.fbeta = native.reward_spec_struct(native.REWARD_FBETA, beta=2.0)
        self.gain = native.reward_spec_struct(native.REWARD_GAIN, gains=(-1.0, 1.0, 3.0), normalize=True)

    def __call__(self, **kw):
        a = dict(labels=self.y, spec=self.fbeta, r_in=None, B=self.B, S=self.S, k=self.k, T=self.T, allow_empty=1, table=self.table,
                 accumulate=0, r_at=self.r_at, better=self.better, best=self.best, best_k=self.best_k, curve=self.curve,
                 hist=self.hist, sums=self.sums, ws=self.ws, ws_bytes=None)
        a.update(kw)
        if a["ws_bytes"] is None:
            a["ws_bytes"] = self.ws_bytes
        spec = None if a["spec"] is None else ctypes.byref(a["spec"])
        return self.lib.rlt_reward_eval(a["labels"], spec, a["r_in"], a["B"], a["S"], a["k"], a["T"], a["allow_empty"], a["table"],
                                        a["accumulate"], a["r_at"], a["better"], a["best"], a["best_k"], a["curve"], a["hist"],
                                        a["sums"], a["ws"], a["ws_bytes"], None)


@pytest.fixture()
def call(native):
    return Call(native)


NO_OUT = dict(r_at=None, better=None, best=None, best_k=None, curve=None, hist=None, sums=None)


def test_short_workspace_is_the_last_check(call):
    """Everything valid but the workspace: RLT_E_WORKSPACE, i.e. every other check passed - and nothing was launched."""
    assert call(ws_bytes=0) == WORKSPACE
    assert call(ws_bytes=call.native.query("rlt_reward_eval_workspace", call.B, call.S, call.T) - 1) == WORKSPACE
    assert call(spec=call.gain, ws_bytes=0) == WORKSPACE
    assert call(labels=None, spec=None, r_in=call.r, ws_bytes=0) == WORKSPACE
    assert call(T=0, k=None, r_at=None, better=None, ws_bytes=0) == WORKSPACE
    assert call(T=0, r_at=None, better=None, ws_bytes=0) == WORKSPACE       # k_in is not read at T = 0
    assert call(T=64, ws_bytes=0) == WORKSPACE
    for name in NO_OUT:                                                     # each output alone
        assert call(**{**NO_OUT, name: getattr(call, name), "ws_bytes": 0}) == WORKSPACE, name


def test_reward_source(call):
    assert call(r_in=call.r) == ARG                                         # both
    assert call(labels=None, spec=None) == ARG                              # neither
    assert call(spec=None) == ARG                                           # labels without a spec
    assert call(labels=None) == ARG                                         # a spec without labels
    assert call(labels=None, r_in=call.r) == ARG                            # a matrix and a spec
    assert call(spec=None, r_in=call.r) == ARG                              # a matrix and labels


def test_dimensions_cuts_and_outputs(call):
    for B, S in ((0, 40), (-1, 40), (6, 0), (6, -4)):
        assert call(B=B, S=S) == ARG
    for T in (-1, 65, 1000):
        assert call(T=T) == ARG
    assert call(k=None) == ARG                                              # T > 0 without cuts
    assert call(T=0) == ARG                                                 # r_at / better without cuts
    assert call(T=0, better=None) == ARG
    assert call(T=0, r_at=None) == ARG
    assert call(**NO_OUT) == ARG                                            # every output NULL
    assert call(ws=None) == ARG


def test_spec_ranges(call):
    N = call.native
    for beta in (0.0, -1.0, float("nan"), float("inf")):
        assert call(spec=N.reward_spec_struct(N.REWARD_FBETA, beta=beta)) == ARG, beta
    for n in (0, 1, 9, -2):
        bad = N.reward_spec_struct(N.REWARD_GAIN, gains=(0.0, 1.0))
        bad.n_grades = n
        assert call(spec=bad) == ARG, n
    for family in (-1, 2, 7):
        bad = N.reward_spec_struct(N.REWARD_FBETA, beta=1.0)
        bad.family = family
        assert call(spec=bad) == ARG, family
    assert call(spec=N.reward_spec_struct(N.REWARD_GAIN, gains=(0.0, float("nan"), 1.0))) == ARG
    assert call(spec=call.gain, table=None) == ARG                          # GAIN with neither discount nor table
    assert call(table=None, ws_bytes=0) == WORKSPACE                        # FBETA does not read it


def test_order_of_the_codes(call):
    """RLT_E_ARG before RLT_E_SHAPE before RLT_E_ALIGN before RLT_E_WORKSPACE."""
    assert call(S=1025, labels=call.y + 4, ws_bytes=0, T=65) == ARG
    assert call(S=1025, labels=call.y + 4, ws_bytes=0, ws=None) == ARG
    assert call(S=1025, labels=call.y + 4, ws_bytes=0) == SHAPE
    assert call(S=1028, ws=call.ws + 4, ws_bytes=0) == SHAPE
    assert call(labels=call.y + 4, ws_bytes=0) == ALIGN
    assert call(S=1024, ws_bytes=0) == WORKSPACE                            # 1024 itself is inside (the buffers are not touched)
    # a misaligned DCG table is RLT_E_ALIGN too: after a missing ws (ARG) and a long list (SHAPE), before the workspace
    bad = dict(spec=call.gain, table=call.table + 4)
    assert call(ws=None, **bad) == ARG
    assert call(S=1025, **bad) == SHAPE
    assert call(ws_bytes=0, **bad) == ALIGN


def test_alignment(call):
    """S % 4 == 0: rows are read 16 bytes at a time; float64 outputs, ws and the table 8 bytes; the rest 4."""
    assert call(labels=call.y + 4) == ALIGN and call(labels=call.y + 8) == ALIGN
    assert call(labels=None, spec=None, r_in=call.r + 4) == ALIGN
    assert call(S=39, labels=call.y + 4, ws_bytes=0) == WORKSPACE           # S % 4 != 0: 4-byte alignment suffices
    assert call(S=39, labels=call.y + 2) == ALIGN
    for name in ("curve", "hist", "sums", "ws"):
        assert call(**{name: getattr(call, name) + 4}) == ALIGN, name
    assert call(spec=call.gain, table=call.table + 4) == ALIGN
    for name in ("k", "r_at", "better", "best", "best_k"):
        assert call(**{name: getattr(call, name) + 2}) == ALIGN, name
        assert call(**{name: getattr(call, name) + 4, "ws_bytes": 0}) == WORKSPACE, name


# ---- the Python surface that needs no device -----------------------------------------------------------------------------
def test_eval_reward_flag():
    import run
    parse = run.build_parser().parse_args
    assert parse([]).eval_reward is None and run.eval_reward_spec(parse([])) is None
    assert run.compare_metric(parse(["--criterion", "ndcg"])) == "f1"       # without the flag: as before
    assert run.report_metric("ndcg") == "f1" and run.report_metric("dcg") == "dcg"
    from utils.rewards import RewardSpec
    args = parse(["--criterion", "fbeta:2", "--eval-reward", "criterion"])
    assert run.eval_reward_spec(args) == RewardSpec.fbeta(2.0) and run.compare_metric(args) == "reward"
    args = parse(["--criterion", "f1", "--eval-reward", "ndcg:-0.5"])       # a spec of its own under any criterion
    assert run.eval_reward_spec(args) == RewardSpec.ndcg(-0.5)
    assert run.eval_reward_text(run.eval_reward_spec(args)) == str(RewardSpec.ndcg(-0.5))
    for crit in ("f1", "dcg"):
        with pytest.raises(ValueError, match="criterion"):
            run.eval_reward_spec(parse(["--criterion", crit, "--eval-reward", "criterion"]))
    with pytest.raises(ValueError):
        run.eval_reward_spec(parse(["--eval-reward", "fbeta"]))
    with pytest.raises(SystemExit):                                         # main() refuses it before anything is built
        run.main(["--criterion", "f1", "--eval-reward", "criterion", "--use-conf", "0"])


def _write_report(path, reward=None, spec=None, n=12, seed=0):
    rng = np.random.default_rng(seed)
    cols = {"qid": np.asarray([f"q{i}" for i in range(n)]), "length": np.full(n, 40, dtype=np.int32),
            "f1": rng.random(n), "best_f1": np.ones(n)}
    if reward is not None:
        cols.update({"reward": reward.astype(np.float32), "best_reward": np.ones(n, dtype=np.float32)})
    if spec is not None:
        cols["reward_spec"] = np.asarray(spec)
    np.savez(path, **cols)
    return str(path)


def test_compare_reports_refuses_what_it_cannot_compare(tmp_path):
    from utils.compare import compare_reports
    rng = np.random.default_rng(1)
    a = _write_report(tmp_path / "a.npz", rng.random(12), "ndcg:-1.0")
    b = _write_report(tmp_path / "b.npz", rng.random(12), "fbeta:2.0")
    plain = _write_report(tmp_path / "plain.npz")
    with pytest.raises(ValueError, match="no 'reward' column"):
        compare_reports([a, plain], metric="reward", device="cpu")
    with pytest.raises(ValueError, match="no 'reward' column"):
        compare_reports([plain, a], metric="reward", device="cpu")
    with pytest.raises(ValueError, match="not comparable"):
        compare_reports([a, b], metric="reward", device="cpu")
    with pytest.raises(ValueError, match="metric"):
        compare_reports([a, b], metric="ndcg", device="cpu")
    import compare_reports as cli
    with pytest.raises(SystemExit):
        cli.main([a, b, "--metric", "ndcg"])
    with pytest.raises(ValueError, match="not comparable"):
        cli.main([a, b, "--metric", "reward"])


def test_cut_report_without_a_reward_has_no_new_keys():
    """per_query() and summary() of a report without `reward=` hold exactly the keys they held before; the state update() leaves
    behind is stood in for by host tensors, so no device is needed."""
    import inspect
    import torch
    from utils.report import CutReport
    from utils.sweep import CutSweep, tune_cut_rule
    for fn in (CutReport.__init__, CutSweep.__init__, tune_cut_rule):
        assert inspect.signature(fn).parameters["reward"].default is None
    B, S = 3, 4
    old = ("k", "p_k", "margin", "f1", "dcg", "best_f1", "best_f1_k", "best_dcg", "best_dcg_k", "better")
    rep = CutReport.__new__(CutReport)
    rep.S, rep.metric, rep.reward, rep._labelled, rep._n, rep._racc = S, "f1", None, True, B, None
    rep._parts = [{n: torch.ones(B, dtype=torch.int32 if n in ("k", "best_f1_k", "best_dcg_k", "better") else torch.float64) for n in old}]
    rep._acc = {"hist": torch.tensor([0.0, 3.0, 0.0, 0.0, 0.0], dtype=torch.float64), "pred_curve": torch.zeros(S, dtype=torch.float64),
                "reward_curve": torch.zeros(S, dtype=torch.float64), "sums": torch.tensor([1.0, 2.0, 3.0, 4.0, 3.0], dtype=torch.float64)}
    assert tuple(rep.per_query()) == old
    assert set(rep.summary()) == {"n", "hist", "mean_k", "f1", "dcg", "best_f1", "best_dcg", "regret_f1", "regret_dcg",
                                  "best_cut_share_f1", "best_cut_share_dcg"}
    assert rep.reward_text() is None
    # with reward state the new keys appear, and only they
    from utils.rewards import RewardSpec
    rep.reward = RewardSpec.ndcg()
    rep._racc = {"sums": torch.tensor([3.0, 2.5, 0.0, 1.5, 1.0, 4.0], dtype=torch.float64)}
    s = rep.summary()
    assert {k: s[k] for k in ("reward_spec", "reward", "best_reward", "best_cut_share_reward", "better_reward")} == \
        {"reward_spec": "ndcg:-1.0", "reward": 0.5, "best_reward": 2.5 / 3, "best_cut_share_reward": 1 / 3, "better_reward": 4 / 3}
    from rlt_hip import ops
    with pytest.raises(ValueError):
        ops.reward_eval()                                                    # neither reward source
