"""ctypes binding of librlt_hip.so (the C ABI declared in include/rlt_hip.h).

There is NO CPU fallback: if the library is missing or a call fails, a RuntimeError is raised.
PyTorch is used only to own device memory and streams; every tensor is handed to the library as
a raw device pointer.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p  # noqa: F401  (ops.py and the tests use them as N.c_*)

import torch

from . import header

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RLT_HIP_LIB") or os.path.join(_PKG, "csrc", "librlt_hip.so")   # env override: kernel experiments
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "rlt_hip.h")

# the header is the one statement of the ABI: its integer #defines, the (restype, [argtypes]) of every prototype, its struct bodies
DEFINES, _SIGNATURES, STRUCTS = header.read(HEADER_PATH)
EXPORTS = tuple(_SIGNATURES)


def _rlt(prefix, names):
    return tuple(DEFINES[f"RLT_{prefix}_{n}"] for n in names.split())


ABI_VERSION = DEFINES["RLT_ABI_VERSION"]
METRIC_F1, METRIC_DCG = _rlt("METRIC", "F1 DCG")
LOSS_EXPECT, LOSS_CE, LOSS_KL, LOSS_JS = _rlt("LOSS", "EXPECT CE KL JS")
GEMM_RELU, GEMM_ACCUMULATE = _rlt("GEMM", "RELU ACCUMULATE")
HEAD_SOFTMAX, HEAD_SIGMOID, HEAD_IDENTITY = _rlt("HEAD", "SOFTMAX SIGMOID IDENTITY")
PROBE_BCE, PROBE_RERANK = _rlt("PROBE", "BCE RERANK")
CUT_ARGMAX, CUT_PAIR = _rlt("CUT", "ARGMAX PAIR")
SWEEP_QUANTILE, SWEEP_FIRST_BELOW, SWEEP_FIRST_ABOVE, SWEEP_COLS = _rlt("SWEEP", "QUANTILE FIRST_BELOW FIRST_ABOVE COLS")
SWEEP_MAX_T = 64                                                                          # rlt_cut_sweep: T <= 64, stated in words only
REWARD_FBETA, REWARD_GAIN, REWARD_MAX_GRADES = _rlt("REWARD", "FBETA GAIN MAX_GRADES")
PAIR_RANKNET, PAIR_LAMBDARANK = _rlt("PAIR", "RANKNET LAMBDARANK")
SEQ_MASK_NONE, SEQ_MASK_CAUSAL = _rlt("SEQ_MASK", "NONE CAUSAL")
PAIR_KINDS = {"ranknet": PAIR_RANKNET, "lambdarank": PAIR_LAMBDARANK}
SWEEP_ROWS = ("k", "f1", "dcg", "precision", "recall", "fbeta", "uncut", "n_lists")      # the rows of rlt_cut_sweep's curve
PRECISION_DEFAULT, PRECISION_FP32, PRECISION_BF16X3, PRECISION_BF16X6 = _rlt("PRECISION", "DEFAULT FP32 BF16X3 BF16X6")
_PRECISION_NAMES = {PRECISION_FP32: "fp32", PRECISION_BF16X3: "bf16x3", PRECISION_BF16X6: "bf16x6"}
OP_ENCODER_STASH, OP_ENCODER_FWD_WS, OP_ENCODER_BWD_WS, OP_BILSTM_STASH, OP_BILSTM_WS = _rlt(
    "OP", "ENCODER_STASH ENCODER_FWD_WS ENCODER_BWD_WS BILSTM_STASH BILSTM_WS")
ENCODER_FIELDS = ("in_proj_weight", "in_proj_bias", "out_proj_weight", "out_proj_bias", "norm1_weight", "norm1_bias",
                  "linear1_weight", "linear1_bias", "linear2_weight", "linear2_bias", "norm2_weight", "norm2_bias")


class EncoderPtrs(ctypes.Structure):
    """rlt_encoder_weights / rlt_encoder_grads: 12 device pointers in ENCODER_FIELDS order."""
    _fields_ = [(f, c_void_p) for f in ENCODER_FIELDS]


class LstmLayerPtrs(ctypes.Structure):
    """rlt_lstm_layer_weights / rlt_lstm_layer_grads: w_ih[2], w_hh[2], b_ih[2], b_hh[2] (0 = forward, 1 = reverse)."""
    _fields_ = [("w_ih", c_void_p * 2), ("w_hh", c_void_p * 2), ("b_ih", c_void_p * 2), ("b_hh", c_void_p * 2)]


SPARSE_CHUNK = DEFINES["RLT_SPARSE_CHUNK"]
SPARSE_POINTERS = ("dense", "ids", "perm", "indptr", "indices", "values", "col_ptr", "col_rows", "col_vals",
                   "chunk_col", "chunk_ptr", "multi_cols")
SPARSE_INTS = ("Dn", "n_docs", "V", "n_chunks", "n_multi")


class SparseBatchPtrs(ctypes.Structure):
    """rlt_sparse_batch: 12 device pointers in SPARSE_POINTERS order, then the five ints of SPARSE_INTS."""
    _fields_ = [(f, c_void_p) for f in SPARSE_POINTERS] + [(f, c_int) for f in SPARSE_INTS]


GEMM_FAMILIES = ("none", "gemm", "gemm3", "gemm3b", "gemm6", "gemm6b", "gemm6c", "gemm6e", "gemm6s")      # RLT_GEMM_NONE .. RLT_GEMM_6S
GEMM_DISPATCH_FIELDS = ("family", "ta", "tb", "fast", "persistent", "ns", "kchunk", "slab_xcd", "epilogue", "narrow")


class GemmDispatch(ctypes.Structure):
    """rlt_gemm_dispatch: what the calling thread's last rlt_gemm / rlt_gemm_ex / rlt_gemm_bits call launched."""
    _fields_ = [(f, c_int) for f in GEMM_DISPATCH_FIELDS]


def gemm_last_dispatch():
    """-> dict of GEMM_DISPATCH_FIELDS, `family` as its name in GEMM_FAMILIES."""
    d = GemmDispatch()
    check(load().rlt_gemm_last_dispatch(ctypes.byref(d)), "rlt_gemm_last_dispatch")
    out = {f: int(getattr(d, f)) for f in GEMM_DISPATCH_FIELDS}
    out["family"] = GEMM_FAMILIES[out["family"]]
    return out


GEMM_PTRS = ("A", "B", "C", "bias", "bias2", "bits_out", "bits_in", "relu_mask", "colsum")      # bits of RLT_GEMM_PTR_*
GEMM_CALL_INTS = ("ta", "tb", "M", "N", "K", "lda", "ldb", "ldc", "flags", "aligned16", "present", "drop", "ws_null")


class GemmCall(ctypes.Structure):
    """rlt_gemm_call: what the GEMM dispatch may depend on - no pointers."""
    _fields_ = [(f, c_int) for f in GEMM_CALL_INTS] + [("ws_bytes", c_size_t)]


def gemm_call(ta, tb, M, N, K, lda=None, ldb=None, ldc=None, flags=0, present=(), misaligned=(), drop=False, ws_bytes=None):
    """-> GemmCall.  Leading dimensions default to the packed ones; present / misaligned: names of GEMM_PTRS (A, B, C are always
    present); ws_bytes: None = no workspace (NULL, 0 bytes), else the bytes of a non-null one."""
    bit = lambda names: sum(1 << GEMM_PTRS.index(n) for n in names)
    return GemmCall(ta, tb, M, N, K, lda or (M if ta else K), ldb or (K if tb else N), ldc or N, flags,
                    bit(GEMM_PTRS[:7]) & ~bit(misaligned), bit(present), int(bool(drop)), int(ws_bytes is None), ws_bytes or 0)


def gemm_plan(call, precision=PRECISION_DEFAULT):
    """-> (return code of the real call before its launch, dict of GEMM_DISPATCH_FIELDS as gemm_last_dispatch gives it)."""
    d = GemmDispatch()
    rc = load().rlt_gemm_plan(ctypes.byref(call), precision, ctypes.byref(d))
    out = {f: int(getattr(d, f)) for f in GEMM_DISPATCH_FIELDS}
    out["family"] = GEMM_FAMILIES[out["family"]]
    return rc, out


ATTN_KERNELS = ("none", "f32", "f32_sb", "f32_occ1", "f32_hd16", "x3", "x6", "x6_img", "x6_pp", "x6_pp_img", "x6_dkv1", "x6_dq1",
                "x6n_2w", "x6n_2w_seeded", "x6n_pipe", "x6h_pipe")                  # RLT_ATTN_NONE .. RLT_ATTN_X6H_PIPE
ATTN_PREPARE = ("q", "k", "v", "do", "seeds", "delta")                              # bits of RLT_ATTN_PREP_*
ATTN_IMAGES = ("none", "x3_qkv", "x6_qkv", "x6n_kv", "x6h_kv")                      # RLT_ATTN_IMAGES_*
ATTN_WS = ("delta", "x3_do", "x6_do", "x6n_blocks")                                 # RLT_ATTN_WS_*
ATTN_PLAN_INTS = ("fwd", "fwd_fixup", "dkv", "dq", "fwd_prepare", "bwd_prepare", "dkv_prepare", "dq_prepare",
                  "images_kind", "images_retained", "ws_kind")
ATTN_PLAN_SIZES = ("images_bytes", "flags_offset", "flags_bytes", "delta_bytes", "ws_extra_bytes", "ws_bytes",
                   "ws_prepare_bytes", "ws_part_bytes")


class AttentionPlan(ctypes.Structure):
    """rlt_attention_plan: what the list-attention entry points decide for one call."""
    _fields_ = [(f, c_int) for f in ATTN_PLAN_INTS] + [(f, c_size_t) for f in ATTN_PLAN_SIZES]


def attention_plan(S, B, H, HD, drop_p, have_images, precision=PRECISION_DEFAULT):
    """-> dict of the plan's fields: kernels, image / workspace kinds as their names, prepare masks as tuples of ATTN_PREPARE names."""
    d = AttentionPlan()
    check(load().rlt_list_attention_plan(S, B, H, HD, drop_p, int(bool(have_images)), precision, ctypes.byref(d)), "rlt_list_attention_plan")
    out = {f: int(getattr(d, f)) for f in ATTN_PLAN_INTS + ATTN_PLAN_SIZES}
    for f in ("fwd", "fwd_fixup", "dkv", "dq"):
        out[f] = ATTN_KERNELS[out[f]]
    for f in ("fwd_prepare", "bwd_prepare", "dkv_prepare", "dq_prepare"):
        out[f] = tuple(n for i, n in enumerate(ATTN_PREPARE) if out[f] >> i & 1)
    out["images_kind"] = ATTN_IMAGES[out["images_kind"]]
    out["ws_kind"] = ATTN_WS[out["ws_kind"]]
    return out


LSTM_KERNELS = ("none", "f32", "x3", "x6", "x6w_single", "x6w_halves")            # RLT_LSTM_F32 .. RLT_LSTM_X6W_HALVES (0: unused)
LSTM_PLAN_FIELDS = ("fwd", "bwd", "fwd_lists", "bwd_lists")


class BilstmRecPlan(ctypes.Structure):
    """struct rlt_bilstm_rec_plan: what the BiLSTM recurrence entry points decide for one call."""
    _fields_ = [(f, c_int) for f in LSTM_PLAN_FIELDS]


def bilstm_rec_plan(B, xin, precision=PRECISION_DEFAULT):
    """-> dict of the plan's fields, the kernels as their names in LSTM_KERNELS."""
    d = BilstmRecPlan()
    check(load().rlt_bilstm_rec_plan(B, int(bool(xin)), precision, ctypes.byref(d)), "rlt_bilstm_rec_plan")
    out = {f: int(getattr(d, f)) for f in LSTM_PLAN_FIELDS}
    out["fwd"], out["bwd"] = LSTM_KERNELS[out["fwd"]], LSTM_KERNELS[out["bwd"]]
    return out


# rlt_opt_state as 13 int64 words (every member up to `coef` is 8 bytes wide); the float64 members through .view(torch.float64),
# word 11 = (coef, apply) and word 12 = (bc1, bc2_sqrt) through .view(torch.float32)
OPT_STATE_WORDS = 13
OPT_STEP, OPT_SKIPPED, OPT_CLIPPED, OPT_NONFINITE, OPT_NAN = 0, 1, 2, 3, 4
OPT_SUMSQ, OPT_NORM, OPT_MAX_ABS, OPT_NORM_SUM, OPT_NORM_MAX, OPT_NORM_STEPS = 5, 6, 7, 8, 9, 10
OPT_COEF_F32 = 22                                  # index of `coef` in the float32 view
GRAD_SEG_WORDS = 3                                 # rlt_grad_seg: sumsq (float64), nonfinite (int64), max_abs (float64)


# rlt_recipe_state as 4 int64 words: lr64 (float64 view) and ema_updates, then lr, ema_decay, coef through .view(torch.float32)
RECIPE_STATE_WORDS = 4
RECIPE_LR64, RECIPE_EMA_UPDATES = 0, 1
RECIPE_LR_F32, RECIPE_EMA_DECAY_F32, RECIPE_COEF_F32 = 4, 5, 6
SCHED_KINDS = ("constant", "linear", "cosine")                                      # RLT_SCHED_CONSTANT .. RLT_SCHED_COSINE
RECIPE_FIELDS = (("base_lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                 ("decoupled", c_int32), ("sched_kind", c_int32), ("ema_warmup", c_int32), ("warmup_steps", c_int64),
                 ("total_steps", c_int64), ("min_lr_ratio", c_float), ("ema_decay", c_float), ("skip_nonfinite", c_int32),
                 ("use_norm", c_int32))


class RecipeStruct(ctypes.Structure):
    """rlt_recipe of include/rlt_hip.h: a host struct, read by the library at call time."""
    _fields_ = list(RECIPE_FIELDS)


def recipe_struct(base_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, sched_kind="constant",
                  warmup_steps=0, total_steps=0, min_lr_ratio=0.0, ema_decay=0.0, ema_warmup=True, skip_nonfinite=False, use_norm=False):
    """-> RecipeStruct; sched_kind by its name in SCHED_KINDS or by its code."""
    kind = SCHED_KINDS.index(sched_kind) if sched_kind in SCHED_KINDS else int(sched_kind)
    return RecipeStruct(base_lr, beta1, beta2, eps, weight_decay, int(bool(decoupled)), kind, int(bool(ema_warmup)), int(warmup_steps),
                        int(total_steps), min_lr_ratio, ema_decay or 0.0, int(bool(skip_nonfinite)), int(bool(use_norm)))


def lr_at(recipe, t):
    """rlt_lr_at: the schedule's float64 value at applied step t >= 1, on the host (NaN for a recipe the step would refuse)."""
    return float(load().rlt_lr_at(ctypes.byref(recipe), int(t)))


# the record of rlt_paired_compare: CMP_WORDS 8-byte words per system (RLT_CMP_*), the float64 ones through .view(torch.float64)
(CMP_N, CMP_SUM_BASE, CMP_SUM_SYS, CMP_SUM_D, CMP_SSD, CMP_WINS, CMP_TIES, CMP_LOSSES, CMP_NONFINITE, CMP_T_OBS, CMP_RAND_GE,
 CMP_BOOT_LE0, CMP_BOOT_GE0, CMP_RESAMPLES, CMP_FORM, CMP_RESERVED, CMP_WORDS) = _rlt(
    "CMP", "N SUM_BASE SUM_SYS SUM_D SSD WINS TIES LOSSES NONFINITE T_OBS RAND_GE BOOT_LE0 BOOT_GE0 RESAMPLES FORM RESERVED WORDS")
CMP_F64_WORDS = (CMP_SUM_BASE, CMP_SUM_SYS, CMP_SUM_D, CMP_SSD, CMP_T_OBS)
CMP_FORMS = ("none", "resident", "chunked")                                         # RLT_COMPARE_RESIDENT, RLT_COMPARE_CHUNKED
CMP_MAX_Q, CMP_MAX_R = 1 << 26, 1 << 20                                             # limits the header states in words only
CMP_MAX_SYSTEMS = DEFINES["RLT_COMPARE_MAX_SYSTEMS"]
CMP_PLAN_FIELDS = ("form", "chunk", "resident_max_q", "chunks", "replicates_per_wave", "lds_bytes")


class PairedComparePlan(ctypes.Structure):
    """struct rlt_paired_compare_plan: what rlt_paired_compare decides for one call."""
    _fields_ = [(f, c_int) for f in CMP_PLAN_FIELDS]


def paired_compare_plan(Q, M, R):
    """-> dict of the plan's fields, the form as its name in CMP_FORMS."""
    d = PairedComparePlan()
    check(load().rlt_paired_compare_plan(Q, M, R, ctypes.byref(d)), "rlt_paired_compare_plan")
    out = {f: int(getattr(d, f)) for f in CMP_PLAN_FIELDS}
    out["form"] = CMP_FORMS[out["form"]]
    return out


def encoder_ptrs(tensors):
    return EncoderPtrs(*[t.data_ptr() for t in tensors])


def lstm_ptrs(layers):
    """layers: per layer (w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r) -> array of LstmLayerPtrs."""
    arr = (LstmLayerPtrs * len(layers))()
    for i, (wif, whf, bif, bhf, wir, whr, bir, bhr) in enumerate(layers):
        arr[i].w_ih[0], arr[i].w_ih[1] = wif.data_ptr(), wir.data_ptr()
        arr[i].w_hh[0], arr[i].w_hh[1] = whf.data_ptr(), whr.data_ptr()
        arr[i].b_ih[0], arr[i].b_ih[1] = bif.data_ptr(), bir.data_ptr()
        arr[i].b_hh[0], arr[i].b_hh[1] = bhf.data_ptr(), bhr.data_ptr()
    return arr


class RewardSpecStruct(ctypes.Structure):
    """rlt_reward_spec of include/rlt_hip.h: a host struct, read by the library at call time."""
    _fields_ = [("family", c_int), ("n_grades", c_int), ("normalize", c_int), ("beta", c_float),
                ("gain", c_float * REWARD_MAX_GRADES), ("discount", c_void_p)]


def reward_spec_struct(family, beta=1.0, gains=(), normalize=False, discount=None):
    """-> RewardSpecStruct.  `discount`: a device tensor of S floats, or None for the 1 / log2(j + 2) of the DCG table; the
    caller keeps it alive for the call."""
    s = RewardSpecStruct()
    s.family, s.n_grades, s.normalize, s.beta = int(family), len(gains), int(bool(normalize)), float(beta)
    for i, g in enumerate(gains[:REWARD_MAX_GRADES]):
        s.gain[i] = float(g)
    s.discount = None if discount is None else discount.data_ptr()
    return s


def byte_buffer(nbytes, device):
    """256-byte aligned device buffer of at least nbytes (torch's caching allocator aligns to 512)."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


_lib = None


def load():
    """Load librlt_hip.so (once) and declare every entry point; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python ranked-list-truncation_amd/rlt_hip/build.py` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP hot path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.rlt_abi_version() != ABI_VERSION:
        raise RuntimeError("librlt_hip.so ABI version mismatch")
    _lib = lib
    return lib


def precision_code(mode):
    """'fp32' | 'bf16x6' | 'bf16x3' | an RLT_PRECISION_* code -> the code."""
    code = {v: k for k, v in _PRECISION_NAMES.items()}.get(mode, mode)
    if code not in _PRECISION_NAMES:
        raise ValueError(f"unknown precision mode {mode!r}: one of {sorted(_PRECISION_NAMES.values())}")
    return int(code)


def set_precision(mode):
    """The PROCESS DEFAULT of the library: 'bf16x6' (fp32-faithful six-product split on the bf16 MFMA: the default), 'fp32'
    (exact fp32 products on the f32 MFMA) or 'bf16x3' (opt-in fast mode, 16 operand bits).  Calls that name their own mode
    (`ops.precision(...)`) do not read it."""
    check(load().rlt_set_precision(precision_code(mode)), "rlt_set_precision")


def get_precision():
    return _PRECISION_NAMES[load().rlt_get_precision()]


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != 0:
        msg = load().rlt_error_string(int(rc))
        raise RuntimeError(f"{what} failed: {msg.decode() if msg else rc} (code {rc})")


def call(name, *args):
    """Invoke an int-returning entry point and raise on a non-zero code."""
    check(getattr(load(), name)(*args), name)


def query(name, *args):
    """Invoke a size_t-returning workspace query."""
    return int(getattr(load(), name)(*args))


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("the HIP hot path needs tensors on the GPU (cuda device); there is no CPU fallback")


def f32c(t):
    """fp32 + contiguous view/copy of a tensor (glue only)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def workspace(nbytes, device):
    n = max(4, (int(nbytes) + 3) // 4)
    return torch.empty(n, dtype=torch.float32, device=device)


def pointer_array(tensors):
    """Host array of device pointers (const float* const*)."""
    arr = (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr
