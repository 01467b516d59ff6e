"""The pairwise ranking losses (rlt_pair_rank_loss, ops.PairRankLossFn / ops.pair_rank, utils.losses.PairwiseRankLoss,
MtCutLoss(rerank_loss=...), run.py --rerank-loss) without a GPU: the C ABI is declared, bound and exported, argument errors are
answered in the stated order before any launch, and the Python surface imports and parses."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -4


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbols_declared_bound_exported(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    P, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    want = {"rlt_pair_rank_workspace": (Z, [I, I]),
            "rlt_pair_rank_loss": (I, [P, P, I, I, I, F, P, I, I, P, P, P, P, P, P, P, P, Z, P])}
    for name, (res, args) in want.items():
        assert name in native.EXPORTS
        fn = getattr(native.load(), name)
        assert fn.restype is res and list(fn.argtypes) == args
        assert (fn.restype, list(fn.argtypes)) == (native._SIGNATURES[name][0], native._SIGNATURES[name][1])
        proto = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert len(proto.split(",")) == len(args)
    assert native.load().rlt_abi_version() == 5
    assert re.search(r"#define RLT_PAIR_RANKNET\s+0\b", header) and re.search(r"#define RLT_PAIR_LAMBDARANK\s+1\b", header)
    assert (native.PAIR_RANKNET, native.PAIR_LAMBDARANK) == (0, 1)
    block = header[header.index("pairwise ranking losses"):header.index("#define RLT_PAIR_RANKNET")]
    for phrase in ("counting rank", "four lists per wavefront", "16, 8, 4, 4 or 2 lists per workgroup", "no atomics",
                   "Algorithmic bytes per list", "off 4", "off 8 bytes", "two calls give the same bits"):
        assert phrase in block, phrase


def test_workspace_query(native):
    q = native.load().rlt_pair_rank_workspace
    assert q(0, 40) == 0 and q(-1, 40) == 0 and q(4, 0) == 0 and q(4, 1025) == 0
    assert q(1, 1) == 8 and q(5, 1024) == 24
    sizes = [q(B, S) for S in (1, 64, 65, 300, 1024) for B in (1, 7, 4096, 1 << 20)]
    assert all(s % 8 == 0 and s > 0 for s in sizes)
    for S in (40, 300, 1024):
        prev = 0
        for B in (1, 2, 3, 100, 5000, 1 << 20, (1 << 31) - 1):
            assert q(B, S) >= prev
            prev = q(B, S)


def test_argument_errors_before_any_launch(native):
    lib = native.load()
    buf = (ctypes.c_uint8 * (1 << 16))()
    base = (ctypes.addressof(buf) + 15) & ~15
    x = ctypes.c_void_p(base)
    off = lambda n: ctypes.c_void_p(base + n)
    gains = (ctypes.c_float * 8)(0, 1, 3, 7, 15, 31, 63, 127)
    B, S = 4, 40
    big = lib.rlt_pair_rank_workspace(B, S)

    def call(score=x, labels=x, B=B, S=S, kind=1, sigma=1.0, gain=gains, n_grades=8, normalize=1, table=x, gscale=x,
             per_list=x, loss=x, dscore=x, rank=x, n_pairs=x, ws=x, ws_bytes=big):
        return lib.rlt_pair_rank_loss(score, labels, B, S, kind, sigma, gain, n_grades, normalize, table, gscale,
                                      per_list, loss, dscore, rank, n_pairs, ws, ws_bytes, None)
    inf, nan = float("inf"), float("nan")
    assert call(score=None) == E_ARG and call(labels=None) == E_ARG and call(ws=None) == E_ARG
    assert call(B=0) == E_ARG and call(B=-1) == E_ARG and call(S=0) == E_ARG and call(S=-5) == E_ARG
    assert call(kind=-1) == E_ARG and call(kind=2) == E_ARG
    assert call(sigma=0.0) == E_ARG and call(sigma=-1.0) == E_ARG and call(sigma=inf) == E_ARG and call(sigma=nan) == E_ARG
    assert call(n_grades=1) == E_ARG and call(n_grades=9) == E_ARG
    for bad in (inf, -inf, nan):
        g = (ctypes.c_float * 8)(0, 1, 3, bad, 15, 31, 63, 127)
        assert call(gain=g) == E_ARG
        assert call(gain=g, n_grades=3, ws_bytes=0) == E_WORKSPACE          # beyond n_grades the array is not read
    assert call(table=None) == E_ARG                            # LAMBDARANK needs the table
    assert call(per_list=None, loss=None, dscore=None, rank=None, n_pairs=None) == E_ARG      # nothing to write
    # the order: an argument error wins over the shape, the shape over the alignment, the alignment over the workspace
    assert call(S=1025) == E_SHAPE and call(S=1 << 20) == E_SHAPE
    assert call(S=1025, score=None) == E_ARG and call(S=1025, sigma=0.0) == E_ARG and call(S=1025, table=None) == E_ARG
    assert call(S=1025, score=off(2)) == E_SHAPE and call(S=1025, ws_bytes=0) == E_SHAPE
    for name in ("score", "labels", "gscale", "per_list", "loss", "dscore", "rank", "n_pairs"):
        assert call(**{name: off(2)}) == E_ALIGN and call(**{name: off(1)}) == E_ALIGN, name
    assert call(ws=off(4)) == E_ALIGN and call(table=off(4)) == E_ALIGN and call(ws=off(2)) == E_ALIGN
    assert call(score=off(2), kind=7) == E_ARG
    assert call(score=off(2), ws_bytes=0) == E_ALIGN
    assert call(ws_bytes=big - 1) == E_WORKSPACE and call(ws_bytes=0) == E_WORKSPACE
    assert call(kind=0, table=None, ws_bytes=0) == E_WORKSPACE  # RANKNET reads no table: the call got as far as the workspace
    assert call(gain=None, ws_bytes=0) == E_WORKSPACE and call(gscale=None, ws_bytes=0) == E_WORKSPACE


def test_python_surface_imports_without_gpu():
    import inspect
    from rlt_hip import ops
    from utils import losses
    sig = inspect.signature(losses.PairwiseRankLoss.__init__)
    assert [sig.parameters[n].default for n in ("kind", "sigma", "gains", "n_grades", "normalize")] == ["lambdarank", 1.0, None, 2, True]
    sig = inspect.signature(ops.pair_rank)
    assert [sig.parameters[n].default for n in ("kind", "sigma", "gains", "n_grades", "normalize")] == ["lambdarank", 1.0, None, 2, True]
    assert hasattr(ops.PairRankLossFn, "apply")
    assert losses.MtCutLoss().rerank_loss == "hinge" and losses.MtCutLoss().pairloss is None
    sig = inspect.signature(losses.MtCutLoss.__init__)
    assert sig.parameters["rerank_loss"].default == "hinge" and sig.parameters["rerank_sigma"].default == 1.0
    assert set(losses.MtCutLoss().state_dict()) == set(losses.MtCutLoss(rerank_loss="lambdarank").state_dict())
    mt = losses.MtCutLoss(rerank_loss="ranknet", rerank_sigma=40.0)
    assert (mt.pairloss.kind, mt.pairloss.sigma, mt.pairloss.n_grades) == ("ranknet", 40.0, 2)
    for bad in ({"kind": "listnet"}, {"sigma": 0.0}, {"sigma": float("nan")}, {"n_grades": 1}, {"n_grades": 9}, {"gains": (1.0,)}):
        with pytest.raises(ValueError):
            losses.PairwiseRankLoss(**bad)
    with pytest.raises(ValueError, match="rerank_loss"):
        losses.MtCutLoss(rerank_loss="softmax")
    assert losses.PairwiseRankLoss(gains=(0, 1, 3)).n_grades == 3


def test_run_parser_accepts_and_rejects_rerank_loss():
    import run
    parse = run.build_parser().parse_args
    assert parse([]).rerank_loss == "hinge" and parse([]).rerank_sigma == 1.0
    a = parse(["--rerank-loss", "lambdarank", "--rerank-sigma", "40"])
    assert (a.rerank_loss, a.rerank_sigma) == ("lambdarank", 40.0)
    assert parse(["--rerank-loss", "ranknet"]).rerank_loss == "ranknet" and parse(["--rerank-loss", "hinge"]).rerank_loss == "hinge"
    for bad in ("listnet", "", "LambdaRank"):
        with pytest.raises(SystemExit):
            parse(["--rerank-loss", bad])
    assert "softmax over positions" in run.__doc__ and "large sigma" in run.__doc__
