"""Parity of the HIP hot path (through the C ABI, on a real MI355X) against the CPU oracle, torch
fp64 references and the golden vectors the reference produced.  `pytest -m gpu`.

The checks live in tools/gpu_probe.py (one section per kernel family, every case reports
|error| vs tolerance); each test runs a section and requires every case to be within tolerance:

    gemm        rlt_gemm all transpose modes, ragged sizes, K=3, split-K, bias/ReLU/accumulate; rlt_colsum
                (per-branch coverage - every kernel family, layout and epilogue with exact operands, the dispatch asserted:
                tests/test_gemm_dispatch_gpu.py)
    losses      every criterion x metric against the reference's golden losses and dL/dp (edge rows:
                no relevant doc, all relevant, single positive first/last), ragged S, MtCutLoss
    metrics     Metric.f1 / Metric.dcg known answers of the reference, argmax cut positions
    layernorm   residual+LayerNorm forward/backward vs fp64
    heads       softmax / sigmoid / identity heads forward/backward vs fp64
    attention   list-axis attention forward/backward vs fp64 (B not multiple of any tile, HD 16/32/64)
    lstm        2-layer BiLSTM forward/backward vs nn.LSTM
    lstm_generic  2-layer BiLSTM at hidden sizes other than 128 (MMOECut's encoding_size) vs nn.LSTM, and an
                MMOECut(encoding_size=64, d_model=128) against the oracle
    embed_mmoe  Choopy embedding, MMOE gates and mixture forward/backward vs fp64
    dropout     the four dropout sites of the encoder layer against references built with the kernels'
                own keep-masks; keep-rate statistics; eval() ignores dropout; reproducible under manual_seed
    optimizer_and_trainer  FusedAdam vs torch.optim.Adam on the oracle over 3 real steps; run.py Trainer on a
                synthetic robust04-format set for 4 models, checkpoints load into reference-shaped modules
    scale_models  whole models at benchmark batch sizes vs the CPU oracle: AttnCut 4096x16 and 512x300, Choopy 8192x8,
                MMOECut(4 experts, tasks 2.1) 1024x40 - outputs 1e-4, cut positions, loss 1e-4, per-parameter gradient rel-L2
    full_size_oracle  AttnCut 4096 x 300 (BASELINE configs[1]) forward + DivLoss + cut metrics against the CPU oracle's forward
                pass on the same batch: p 1e-4, cut positions, F1 / DCG / loss 1e-4
    full_size_oracle_choopy  Choopy 8192 x 300 (BASELINE configs[2]) forward against the oracle's logits on 24 of the 300 positions
                (no recurrence: positions meet only in the final softmax, which cancels in log-ratios): 1e-4 for all 8192 lists
    scale_ops   list attention at B=4096 (hd 64) / 8192 (hd 16), every GEMM layout at 1,228,800 rows (all elements vs
                fp64), split-K dW products over K=1,228,800 with the fused bias gradient, the 1-bit-mask FFN pair,
                BiLSTM at B=4096, LayerNorm at 1,228,800 rows
    full_size_kernels  BiLSTM 4096x300 and encoder layers 4096x300 (E256/H4), 8192x300 (E128/H8) at full size against
                list-/position-subset references with sparse upstream gradients
    scale_dropout  the TRAIN-MODE kernel variants at benchmark shapes: list attention with probability dropout at B=4096
                (hd 64, p 0.4) / 8192 (hd 16, p 0.2) fwd + dQ/dK/dV vs fp64 on the exported masks, the FFN-hidden dropout
                epilogue of rlt_gemm_bits and add_ln with branch dropout at 1,228,800 rows, full-size encoder layers in
                train mode (4096x300 p 0.4, 8192x300 p 0.2) vs position-subset fp64 references with all four masks
    flip_aligned_grads  whole-model gradients vs the oracle with knife-edge ReLU units following the device's branch
                (counted): per-parameter rel-L2 1e-4 (fp32 mode) / 1e-3 (bf16x3)
    trainer_bookkeeping  run.py's Trainer vs the same loop on the oracle: per-epoch means, best / best-5, checkpointed
                epoch and weights, scalar log
    trainer_buckets  run.py's Trainer on lists of 100 / 200 / 300 documents (length-bucketed batches, BASELINE configs[4]'s
                shape) vs the oracle loop over the same BatchLoader schedule: per-epoch means
    scale_mmoe  MMOE gates (K = 76,800) / mixture fwd+bwd at 2048 x 300 vs fp64, MtCutLoss terms at 4096 x 300 vs the oracle,
                the whole MMOECut(4 experts, tasks 2.1) at 1024 x 300 vs the oracle module in fp64 on the device
    path_level  rlt_encoder_layer_fwd/bwd (composed in the library) == the same launches driven from the host, bit for bit
    trainer_dp  run.py with two ranks on this GPU (gloo rehearsal) vs the shard-wise oracle: ragged and empty shards
    rccl_one_rank  bench.py and run.py as children of torch.distributed.run with ONE rank over RCCL (RLT_FORCE_DIST=1):
                init_process_group("nccl", device_id), broadcast, all-reduce(AVG) of the flat bucket, NCCL barrier execute;
                results equal the run without a process group
    trainer_dp_mt  the two configurations north_star shards (BASELINE configs[3], [4]) under two ranks: MMOECut(4 experts, tasks
                2.1 / 2.2) and MtAttnCut(3) on length buckets 100 / 200 / 300 vs the shard-wise oracle; replicas bitwise equal
    x6_adversarial  bf16x6 vs the f32 MFMA kernels on adversarial operands (low significand bits all ones / worst split, one
                sign; cancelling sums), K = 16 ... 1,228,800, GEMM and attention: err_x6 <= 1.25 err_f32 against fp64
    x6_fallbacks  the bf16x6 attention forms behind the default dispatch: two-workgroup head-dim-64 backward kernels without image
                staging, two-wavefront head-dim-16 kernels at scale (child process); the 24-bit row-offset switch-over at
                B = 21,760 / 21,888 against the exact-fp32 kernels
    precision_argument  two modes side by side in one process through the call argument == the same mode as process default
    determinism  the 4096 x 300 AttnCut and 8192 x 300 Choopy steps twice from one state in each mode: gradient bucket, p, k bitwise
    bench_two_ranks  bench.py --gpus 2 (its own torch.distributed.run child, two gloo ranks on this GPU): the N > 1 JSON line
    rccl_two_ranks  bench.py --gpus 2 with the REAL backend (nccl = RCCL), both ranks on this box's one GPU: either the N = 2 line, or
                RCCL's duplicate-GPU refusal reaching the parent as a non-zero exit inside the bounded wait - never a hang
    dp_four_ranks  the largest world the box's process guard admits beside the test process: bench.py --gpus 4 --batch 32 and
                run.py MMOECut(4e, 2.1) under four ranks with ragged and empty shards vs the shard-wise oracle, replicas bitwise equal
    trajectory  20 Adam steps, each side on its own gradients: per-step loss / F1 / p within 1e-4, cut positions
    models      all 22 golden model cases: outputs (1e-5), cut positions (identical), F1/DCG (1e-4),
                every criterion's loss (1e-4), per-parameter gradients (1e-3 of the gradient norm)
Tolerances are written next to each case in tools/gpu_probe.py; BASELINE.json asks for 1e-4.
"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
_SPEC = importlib.util.spec_from_file_location(
    "gpu_probe", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gpu_probe.py"))


@pytest.fixture(scope="module")
def probe():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    mod = importlib.util.module_from_spec(_SPEC)
    _SPEC.loader.exec_module(mod)
    from rlt_hip import native
    native.load()            # fails loudly if librlt_hip.so is missing: there is no fallback path
    return mod


MODE_DEPENDENT = ["gemm", "attention", "lstm", "dropout", "optimizer_and_trainer", "models", "bicut",
                  "scale_models", "scale_ops", "scale_dropout", "full_size_kernels", "flip_aligned_grads", "trajectory", "trainer_bookkeeping", "trainer_buckets", "scale_mmoe", "path_level", "lstm_generic", "trainer_dp"]
MODE_FREE = ["losses", "metrics", "layernorm", "heads", "embed_mmoe", "rccl_one_rank", "x6_image_staging", "x6_fallbacks",
             "x6_adversarial", "precision_argument", "determinism", "bench_two_ranks", "rccl_two_ranks", "dp_four_ranks", "trainer_dp_mt"]


def _run(probe, name):
    import torch
    probe.RESULTS.clear()
    getattr(probe, name)()
    torch.cuda.synchronize()
    assert probe.RESULTS, "section produced no checks"
    bad = [(n, e, t) for (n, e, t, ok) in probe.RESULTS if not ok]
    assert not bad, f"{len(bad)} of {len(probe.RESULTS)} checks out of tolerance: {bad[:8]}"


@pytest.mark.parametrize("name", MODE_FREE)
def test_section(probe, name):
    _run(probe, name)


@pytest.mark.parametrize("precision", ["bf16x6", "fp32", "bf16x3"])
@pytest.mark.parametrize("name", MODE_DEPENDENT)
def test_section_by_precision(probe, name, precision):
    """All three MFMA precision modes of the library: the default fp32-faithful six-product mode (bf16x6: GEMM family, list
    attention at head dims 16 / 32 / 64 and the BiLSTM recurrences on an EXACT three-way bf16 split of both operands), the
    exact-fp32 MFMA mode and the opt-in split-bf16 mode.  Model-level tolerances are identical in all three; op-level MFMA
    tolerances are 6x looser for bf16x3 ONLY (tools/gpu_probe.py: mfma_tol) - bf16x6 is held to the exact-fp32 tolerances
    everywhere.  The mode is set as the process DEFAULT here (what RLT_PRECISION_DEFAULT resolves to); the sections
    precision_argument / x6_adversarial pass it as the call argument instead."""
    from rlt_hip import native
    keep = native.get_precision()
    native.set_precision(precision)
    try:
        _run(probe, name)
    finally:
        native.set_precision(keep)


def test_full_size_oracle(probe):
    """BASELINE configs[1] (AttnCut 4096 x 300) at full size, default mode, directly against the CPU oracle's forward pass:
    p within 1e-4, cut positions identical outside knife-edge lists, F1 / DCG / loss within 1e-4 (tools/gpu_probe.py
    full_size_oracle)."""
    _run(probe, "full_size_oracle")


def test_full_size_oracle_choopy(probe):
    """BASELINE configs[2] (Choopy 8192 x 300) at full size, default mode, directly against the CPU oracle on a 24-position subset:
    the log-ratios of the device's cut probabilities between subset positions equal the oracle's logit differences within 1e-4 for
    all 8192 lists (tools/gpu_probe.py full_size_oracle_choopy)."""
    _run(probe, "full_size_oracle_choopy")


def test_full_size_models(probe):
    """BASELINE configs[1] (AttnCut 4096 x 300) and configs[2] (Choopy 8192 x 300) at full size, exact-fp32 mode vs
    bf16x3 mode: cut distributions within 1e-4, identical cut positions outside knife-edge lists, loss 1e-4.  The
    comparisons with independent references at these sizes are the sections scale_models (whole models vs the CPU
    oracle at batch 4096 / 8192 / 1024 / 512), scale_ops (attention, 1.2M-row GEMMs, BiLSTM vs fp64 / nn.LSTM) and
    full_size_kernels (full-size BiLSTM and encoder layers vs subset references), all above."""
    _run(probe, "full_size_models")
