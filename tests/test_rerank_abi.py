"""The per-list sort (rlt_rerank_lists, ops.rerank_lists, model.rerank, utils/rerank.py, run.py --rerank-eval) without a GPU: the
C ABI is declared, bound and exported, argument errors are answered in the stated order before any launch, and the Python
surface imports and parses."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from rlt_hip import build, native
    build.build(verbose=False)
    native.load()
    return native


def test_symbol_declared_bound_exported(native):
    header = open(os.path.join(REPO, "include", "rlt_hip.h")).read()
    assert "rlt_rerank_lists" in native.EXPORTS
    fn = native.load().rlt_rerank_lists
    P, I = ctypes.c_void_p, ctypes.c_int
    assert fn.restype is I and list(fn.argtypes) == [P, I, I, P, P, I, P, P, P, P]
    assert (fn.restype, list(fn.argtypes)) == (native._SIGNATURES["rlt_rerank_lists"][0], native._SIGNATURES["rlt_rerank_lists"][1])
    proto = re.search(r"int rlt_rerank_lists\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == len(fn.argtypes)
    assert native.load().rlt_abi_version() == 5
    block = header[header.index("rerank, then truncate"):header.index("int rlt_rerank_lists(")]
    for phrase in ("TOTAL order", "permutation", "kind=\"stable\"", "read 4 S (1 + n), write up to 4 S (3 + n)", "overlap",
                   "off 4 bytes"):
        assert phrase in block, phrase


def test_argument_errors_before_any_launch(native):
    lib = native.load()
    buf = (ctypes.c_uint8 * (1 << 16))()
    base = ctypes.addressof(buf)
    x = ctypes.c_void_p(base)
    off = lambda n: ctypes.c_void_p(base + n)
    arr = lambda *ps: (ctypes.c_void_p * len(ps))(*[p.value if p is not None else None for p in ps])
    four, B, S = arr(x, x, x, x), 4, 40

    def call(pred=x, B=B, S=S, src=four, dst=four, n=4, perm=x, rank=x, sorted_pred=x):
        return lib.rlt_rerank_lists(pred, B, S, src, dst, n, perm, rank, sorted_pred, None)
    E_ARG, E_SHAPE, E_ALIGN = -1, -2, -4
    assert call(pred=None) == E_ARG
    assert call(B=0) == E_ARG and call(B=-1) == E_ARG and call(S=0) == E_ARG and call(S=-5) == E_ARG
    assert call(n=-1) == E_ARG and call(n=5) == E_ARG
    assert call(src=None) == E_ARG and call(dst=None) == E_ARG
    for t in range(4):
        holed = arr(*[None if i == t else x for i in range(4)])
        assert call(src=holed) == E_ARG and call(dst=holed) == E_ARG
    assert call(src=arr(x, x, None, None), dst=arr(x, x, None, None), n=3) == E_ARG
    assert call(n=0, src=None, dst=None, perm=None, rank=None, sorted_pred=None) == E_ARG       # nothing to write
    # the order: an argument error wins over the shape, the shape over the alignment
    assert call(S=1025) == E_SHAPE and call(S=1 << 20) == E_SHAPE
    assert call(S=1025, pred=None) == E_ARG and call(S=1025, n=5) == E_ARG
    assert call(S=1025, pred=off(2)) == E_SHAPE
    for name in ("pred", "perm", "rank", "sorted_pred"):
        assert call(**{name: off(2)}) == E_ALIGN and call(**{name: off(1)}) == E_ALIGN, name
    assert call(src=arr(x, x, x, off(2))) == E_ALIGN and call(dst=arr(off(6), x, x, x)) == E_ALIGN
    assert call(pred=off(2), n=5) == E_ARG


def test_python_surface_imports_without_gpu():
    import inspect
    from rlt_hip import ops
    from models import _common
    import models
    sig = inspect.signature(ops.rerank_lists)
    assert [sig.parameters[n].default for n in ("want_perm", "want_rank", "want_sorted")] == [True, False, False]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("want_perm", "want_rank", "want_sorted"))
    assert inspect.signature(_common.CutModel.rerank_order).parameters["by"].default == "rerank"
    assert models.MtAttnCut(num_tasks=3).head_names() == ("classi", "rerank", "decison_layer")
    assert models.MtAttnCut(num_tasks=2.1).head_names() == ("classi", "decison_layer")
    assert models.MtChoopy(num_tasks=2.2).head_names() == ("rerank", "decison_layer")
    assert models.MMOECut(num_tasks=2.2).head_names() == ("rerank", "decison_layer")
    assert models.PLECut().head_names() == ("classi", "rerank", "decison_layer")
    assert models.AttnCut().head_names() == ()
    import torch
    with pytest.raises(ValueError, match="no 'rerank' head"):
        models.AttnCut().rerank(torch.zeros(2, 8, 3))
    with pytest.raises(ValueError, match="no 'rerank' head"):
        models.MtAttnCut(num_tasks=2.1).rerank(torch.zeros(2, 8, 3))
    with pytest.raises(ValueError, match="by must be"):
        models.MtAttnCut().rerank(torch.zeros(2, 8, 3), by="decison_layer")


def test_run_parser_accepts_and_rejects_rerank_eval():
    import run
    parse = run.build_parser().parse_args
    assert parse([]).rerank_eval is None
    assert parse(["--rerank-eval", "rerank"]).rerank_eval == "rerank" and parse(["--rerank-eval", "classi"]).rerank_eval == "classi"
    for bad in ("cut", "decison_layer", ""):
        with pytest.raises(SystemExit):
            parse(["--rerank-eval", bad])
