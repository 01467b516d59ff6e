#!/usr/bin/env python3
"""Training loop of the truncation models on the HIP hot path - the mirror of the reference's
run.py `Trainer` (:26-240) and `main` (:301-369) for the five in-scope models.

Same flow per step (run.py:120-151): zero_grad -> model(X) -> criterion -> backward -> Adam ->
k = argmax+1 -> F1/DCG; same per-epoch bookkeeping (unweighted means over steps, best / best-5 test F1,
state_dict checkpoint on best test F1, run.py:153-232) and the same log lines.  What differs:
  * model / criterion / metrics / optimizer run through librlt_hip.so; inputs are fed by the
    pinned-memory loader in dataloader/ (the reference's pickle layout);
  * F1/DCG are evaluated on the device (no (B,S) round trip per step); one host sync per step for
    the three logged scalars;
  * launched under torch.distributed.run it is data-parallel: all ranks draw the same batch permutation (one seed
    broadcast from rank 0), every rank takes its contiguous shard of each batch (an exact partition, ragged tails
    included: shards are weighted by their list counts in the loss, the gradient and the logged means), one RCCL
    all-reduce of the flat gradient bucket per step (rlt_hip/parallel.py);
  * the scalars the reference sends to tensorboardX (run.py:146,154-156,196-198) go, under the same tags, to
    `<tensorboard-dir>/scalars.jsonl` (and to a SummaryWriter when tensorboard is installed);
  * --baselines 1: rank 0 first reports the truncation baselines of the reference's Baseline/ notebooks (Oracle, Fixed-k,
    Greedy-k) on the run's own labels, per list length, on the device (utils/baselines.py);
  * --report-out PATH: rank 0 runs a split through the trained (or loaded: --epochs 0 --ft 1 --model-path CKPT) model and writes
    what it does per query - cut, winning value, margin, F1 / DCG at the cut, the list's best, the count of better cuts - with
    the k histogram, the summary and the two curves below per list length, from one fused pass per batch (utils/report.py);
  * --draw 1: the arithmetic of the reference's figure (run.py:188,242-298) - the batch-mean softmax of the reward and the
    batch-mean sharpened softmax of the model's output - goes to scalars.jsonl under draw/reward and draw/prediction on the
    reference's condition (even epoch, a batch of more than 40 lists); no image is written;
  * --cut-sweep RULE:LO:HI:N [--sweep-out PATH]: rank 0 evaluates N thresholds of a cut rule (the predicted-mass quantile, the
    first output above tau, or the retrieval score falling below tau) on the train and test lists in one fused pass per batch,
    tunes tau* on train and reports test there beside the argmax cut (utils/sweep.py);
  * --rerank-loss ranknet|lambdarank [--rerank-sigma F]: the rerank head of a multi-task model is trained with a pairwise logistic
    loss over the documents of each list (utils.losses.PairwiseRankLoss, one O(S^2) kernel pass) in place of the reference's
    batch-wide hinge.  Towers that end in a softmax over positions (MMOE, PLE) have score gaps near 1/S and want a large sigma;
  * not carried over: rendering figures and the hyper-parameter random search.
"""
import argparse
import configparser
import contextlib
import json
import logging
import math
import os
import time

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
logging.basicConfig(level=logging.INFO)

from dataloader import at_dataloader, bicut_dataloader, cp_dataloader, mc_dataloader, write_synthetic_robust04  # noqa: E402
from models import AttnCut, BiCut, Choopy, MMOECut, MOECut, MtAttnCut, MtChoopy, PLECut  # noqa: E402
from utils import losses  # noqa: E402
from utils.metrics import Metric  # noqa: E402
from utils.rewards import RewardSpec  # noqa: E402
from rlt_hip import ops  # noqa: E402
from rlt_hip.parallel import FORCE_COLLECTIVES, FlatModel, FusedAdam, shard_bounds  # noqa: E402
from utils.recipe import add_recipe_arguments, recipe_kwargs  # noqa: E402


class ScalarLog:
    """add_scalar(tag, value, step) of the reference's tensorboardX writer (run.py:111): one JSON line per scalar in
    <dir>/scalars.jsonl, mirrored into torch.utils.tensorboard when that package is importable."""

    def __init__(self, log_dir):
        self.file = self.tb = None
        if not log_dir:
            return
        os.makedirs(log_dir, exist_ok=True)
        self.file = open(os.path.join(log_dir, "scalars.jsonl"), "w")
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.tb = SummaryWriter(log_dir=log_dir)
        except Exception:                      # tensorboard is not part of this image
            self.tb = None

    def add_scalar(self, tag, value, step):
        if self.file is not None:
            self.file.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
        if self.tb is not None:
            self.tb.add_scalar(tag, value, step)

    def add_curve(self, tag, values, step):
        """A whole curve under one tag (the --draw curves): one JSON line with `values`; not mirrored to tensorboard."""
        if self.file is not None:
            self.file.write(json.dumps({"tag": tag, "values": [float(v) for v in values], "step": int(step)}) + "\n")

    def close(self):
        if self.file is not None:
            self.file.close()
            self.file = None
        if self.tb is not None:
            self.tb.close()


class Trainer:
    attention_axis = "list"      # of a trainer a driver assembles by hand (verify_probe.py); __init__ sets the run's
    attention_mask = "none"      # likewise
    cut_head = "softmax"         # likewise
    hazard_prior = "uniform"     # likewise
    rerank_by = None             # --rerank-eval, likewise

    def __init__(self, args):
        self.args = args
        self.seq_len = 300 if args.retrieve_data == 'robust04' else 40
        self.model_name = args.model_name
        self.epochs, self.batch_size = args.epochs, args.batch_size
        self.model_persist, self.save_path, self.model_path = args.model_persist, args.save_path, args.model_path
        self.best_test_f1, self.best_test_dcg = -float('inf'), -float('inf')
        self.best_epoch = None                  # epoch whose weights were checkpointed (None: no test epoch has run)
        self.best5_f1 = self.best5_dcg = None
        self.f1_record, self.dcg_record = [], []
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        if not torch.cuda.is_available():
            raise RuntimeError("run.py trains on the GPU through librlt_hip.so; there is no CPU fallback")
        # RLT_RUN_DEVICE / RLT_DIST_BACKEND exist only to rehearse the data-parallel loop on a one-GPU box (several ranks
        # on cuda:0 over gloo, as bench.py's RLT_BENCH_DEVICE does); real runs use one GPU per rank over RCCL
        self.device = torch.device("cuda", int(os.environ.get("RLT_RUN_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
        torch.cuda.set_device(self.device)
        # --resume: the checkpoint of --save-state.  The data permutation and the dropout streams are not part of it: they restart
        # from --seed + the resumed epoch, so a resumed run is not bit-identical to an uninterrupted one (the optimizer is)
        resume = torch.load(args.resume, map_location="cpu") if getattr(args, "resume", None) else None
        self.start_epoch = resume["epoch"] + 1 if resume else 0
        seed = args.seed + self.start_epoch if resume and args.seed is not None else args.seed

        name = self.model_name
        if name in ('choopy', 'mtchoopy'):
            loader = cp_dataloader
        elif name in ('mmoecut', 'moecut', 'mtple') and args.retrieve_data != 'robust04':
            loader = mc_dataloader                                             # run.py:87-88: MQ2007 multi-task statistics
        else:
            loader = at_dataloader
        # --bicut-stats: BiCut at the width the reference declares it for, on the sparse bag-of-words table (the loader the
        # reference comments out, run.py:61-63)
        self.sparse_bicut = name == 'bicut' and bool(getattr(args, "bicut_stats", None))
        # a label-free report of a loaded model (--epochs 0 --report-out --report-labels 0) reads no label: gt.pkl may be missing
        need_labels = not (getattr(args, "report_out", None) and not getattr(args, "report_labels", 1) and args.epochs == 0)
        from dataloader import rank_data
        with rank_data.labels_optional(not need_labels):
            if self.sparse_bicut:
                self.train_loader, self.test_loader, data = bicut_dataloader(
                    args.retrieve_data, args.dataset_name, args.batch_size, device=self.device, base=args.dataset_base, seed=seed,
                    stats=args.bicut_stats, vocab=args.bicut_vocab)
            else:
                self.train_loader, self.test_loader, data = loader(args.retrieve_data, args.dataset_name, args.batch_size,
                                                                   device=self.device, base=args.dataset_base, seed=seed)
        # the reference hard-codes 3 / 25 / 47 input features and 300 / 40 positions (run.py:34,60,70,86); here both
        # come from the files, and a mismatch with the reference's numbers is reported instead of mis-striding the LSTM
        self.data = data
        feat = data.n_features
        if len(data.lengths) == 1:
            self.seq_len = data.lengths[0]
        if name not in ('bicut', 'attncut', 'mtattncut') and (len(data.lengths) != 1 or data.test_lengths != data.lengths):
            # Choopy's position encoding and the MMOE gates are sized by seq_len: a test list of another length would
            # only fail inside the model at the first test epoch
            raise ValueError(f"{name} is built for ONE list length; the data holds train lengths {data.lengths} and test "
                             f"lengths {data.test_lengths} (only the BiLSTM models bicut / attncut / mtattncut take "
                             "length-bucketed batches)")
        # --attention-axis: 'list' (the reference: lists attend to each other) or 'position' (every list over its own positions);
        # the weights do not depend on it, so it is recorded beside them and a mismatch on loading is a warning, not an error
        self.attention_axis = axis = getattr(args, "attention_axis", "list")
        # --attention-mask: 'none', or 'causal' on the position axis (position i attends to the positions <= i).  Recorded beside
        # the axis, but only when it is 'causal': the files of a default run are byte for byte what they were
        self.attention_mask = mask = getattr(args, "attention_mask", "none")
        mask_kw = {"attention_mask": mask} if mask != "none" else {}
        # --cut-head: 'softmax' (the reference's head), or 'hazard' (stop probabilities, ops.hazard_head) on the four models that
        # take it.  It changes no parameter; recorded like the mask, only when it is not the default
        self.cut_head = getattr(args, "cut_head", "softmax")
        self.hazard_prior = getattr(args, "hazard_prior", "uniform")
        if self.cut_head != "softmax":
            if name not in ('choopy', 'attncut', 'mtchoopy', 'mtattncut'):
                raise ValueError(f"--cut-head {self.cut_head}: {name} has the softmax cut head only (choopy, attncut, mtchoopy and "
                                 "mtattncut take a hazard head)")
            mask_kw.update(cut_head=self.cut_head, hazard_prior=self.hazard_prior)
            if (axis, mask) != ("position", "causal"):
                logging.warning('--cut-head hazard without --attention-axis position --attention-mask causal: the head reads ranks '
                                '<= i at rank i, but the encoder under it does not, so the stop probabilities are not online')
        # --rerank-loss: the loss of the rerank head inside MtCutLoss - the reference's batch-wide hinge, or a pairwise RankNet /
        # LambdaRank loss (utils.losses.PairwiseRankLoss); the default builds the criterion exactly as before
        rr_loss = getattr(args, "rerank_loss", "hinge")
        rr_kw = {} if rr_loss == "hinge" else {"rerank_loss": rr_loss, "rerank_sigma": getattr(args, "rerank_sigma", 1.0)}
        if rr_kw and (name not in ('mtchoopy', 'mtattncut', 'mmoecut', 'moecut', 'mtple') or args.num_tasks == 2.1):
            raise ValueError(f"--rerank-loss {rr_loss}: {name} with --num-tasks {args.num_tasks} has no rerank head to train "
                             "(the multi-task models with --num-tasks 3 or 2.2 have one)")
        if name == 'bicut':                                                    # run.py:59-64
            self.model = BiCut(input_size=feat, dropout=args.dropout, sparse_input=self.sparse_bicut)
            self.criterion = losses.BiCutLoss(metric=args.criterion)
        elif name == 'choopy':                                                 # run.py:65-68
            self.model = Choopy(seq_len=self.seq_len, dropout=args.dropout, attention_axis=axis, **mask_kw)
            self.criterion = losses.ChoopyLoss(metric=args.criterion)
        elif name == 'attncut':                                                # run.py:69-75
            self.model = AttnCut(input_size=feat, dropout=args.dropout, attention_axis=axis, **mask_kw)
            self.criterion = losses.DivLoss(metric=args.criterion, div_type=args.div_type,
                                            augmented=args.augmented_reward)
        elif name == 'mtchoopy':                                               # run.py:76-79
            self.model = MtChoopy(seq_len=self.seq_len, num_tasks=args.num_tasks, dropout=args.dropout, attention_axis=axis, **mask_kw)
            self.criterion = losses.MtCutLoss(metric=args.criterion, rerank_weight=args.rerank_weight,
                                              classi_weight=args.class_weight, num_tasks=args.num_tasks, **rr_kw)
        elif name == 'mtattncut':                                              # run.py:80-84
            self.model = MtAttnCut(input_size=feat, num_tasks=args.num_tasks, dropout=args.dropout, attention_axis=axis, **mask_kw)
            self.criterion = losses.MtCutLoss(metric=args.criterion, rerank_weight=args.rerank_weight,
                                              classi_weight=args.class_weight, num_tasks=args.num_tasks, **rr_kw)
        elif name == 'mmoecut':                                                # run.py:85-90 (num_experts exposed)
            self.model = MMOECut(seq_len=self.seq_len, num_tasks=args.num_tasks, input_size=feat,
                                 dropout=args.dropout, num_experts=args.num_experts, attention_axis=axis, **mask_kw)
            self.criterion = losses.MtCutLoss(metric=args.criterion, num_tasks=args.num_tasks, **rr_kw)
        elif name == 'moecut':                                                 # run.py:91-96
            self.model = MOECut(seq_len=self.seq_len, num_tasks=args.num_tasks, input_size=feat, dropout=args.dropout,
                                attention_axis=axis, **mask_kw)
            self.criterion = losses.MtCutLoss(metric=args.criterion, num_tasks=args.num_tasks, **rr_kw)
        elif name == 'mtple':                                                  # run.py:97-102
            self.model = PLECut(seq_len=self.seq_len, input_size=feat, dropout=args.dropout, num_experts=3, attention_axis=axis, **mask_kw)
            self.criterion = losses.MtCutLoss(metric=args.criterion, num_tasks=args.num_tasks, **rr_kw)
        else:
            raise ValueError(f"model {name!r} is outside the HIP hot path "
                             "(bicut, choopy, attncut, mtchoopy, mtattncut, mmoecut, moecut, mtple)")
        self.multi_task = name in ('mtchoopy', 'mtattncut', 'mmoecut', 'moecut', 'mtple')   # reference: `'m' in model_name`
        self.rerank_by = getattr(args, "rerank_eval", None)     # (drivers build their own Namespace)
        if self.rerank_by and self.rerank_by not in getattr(self.model, "head_names", tuple)():
            raise ValueError(f"--rerank-eval {self.rerank_by}: {name} with --num-tasks {args.num_tasks} has no such head")
        self.model = self.model.to(self.device)
        if args.ft and self.model_path and os.path.exists(self.model_path):
            self.load_model()
        self.flat = FlatModel(self.model)
        self.flat.broadcast_params()
        if resume:
            self._warn_axis(resume.get("attention_axis", "list"), args.resume, resume.get("attention_mask", "none"))
            self.model.load_state_dict(resume["model"])         # in place: into the views of the flat bucket
        total_steps = max(1, args.epochs * len(self.train_loader))
        self.optimizer = FusedAdam(self.flat, lr=args.lr, weight_decay=args.weight_decay, **grad_guard_kwargs(args),   # run.py:104
                                   **recipe_kwargs(args, self.flat.names, total_steps))
        self.ema_eval = bool(getattr(args, "ema_eval", 0))      # (drivers build their own Namespace)
        if resume:
            self.optimizer.load_state_dict(resume["optimizer"])
            for k in ("best_test_f1", "best_test_dcg", "best_epoch", "f1_record", "dcg_record", "history"):
                setattr(self, k, resume[k])
            if args.seed is not None:
                torch.manual_seed(seed)
        ops.set_seed_stream(self.rank)          # same torch seed on every rank, different dropout masks
        self.writer = ScalarLog(getattr(args, "tensorboard_dir", None) if self.rank == 0 else None)   # run.py:111
        if not resume:
            self.history = []                   # per epoch: train / test (loss, f1, dcg) means
        self.baseline_results = None            # --baselines 1: per list length, see baselines()

    @property
    def reward_stats(self):
        """A reward loss on a criterion beside f1 / dcg (utils/rewards.py): the epochs also log the reward at the cut, the list's
        best reward and the share of lists cut at their best reward, from the loss pass itself.  Read off the criterion, so it
        holds for a Trainer that was given one (verify_probe.py) as for one built from --criterion."""
        crit = getattr(self, "criterion", None)
        return hasattr(crit, "forward_with_metrics") and RewardSpec.is_spec(getattr(crit, "metric", None))

    # ------------------------------------------------------------------------------------------
    def _step(self, X, y, train):
        """One batch.  Data-parallel: every rank holds the SAME batch (shared permutation) and works on its contiguous
        shard; shards partition the batch exactly (a ragged tail gives unequal, possibly empty shards), so loss,
        gradient and logged means are weighted by the shards' list counts - what comes out is the batch mean of the
        shard-wise reference computation."""
        n_all = X.shape[0]
        lo, hi = shard_bounds(n_all, self.rank, self.world)
        n_own = hi - lo
        stats = torch.zeros(4, dtype=torch.float64, device=self.device)
        if n_own > 0:
            Xs, ys = (X, y) if self.world == 1 else (X[lo:hi], y[lo:hi])
            output = self.model(Xs)
            # loss and cut metrics (run.py:126,131-145) out of one pass over p and the labels; BiCut's (B,S,2) output goes
            # through its own criterion and Metric.evaluate's cut rule
            loss, _k, f1, dcg = Metric.step(self.criterion, output, ys)
            if train:
                # AVG all-reduce of sum_r (n_r * world / n) * grad_r / world = sum_r (n_r / n) * grad_r
                (loss if n_own * self.world == n_all else loss * (n_own * self.world / n_all)).backward()
            stats = torch.stack([loss.detach().double(), f1, dcg, torch.ones((), dtype=torch.float64, device=self.device)]) * n_own
        if self.reward_stats:                                   # sums over the shard's lists of r_k, r_best and [r_k == r_best]
            rs = self.criterion.last_reward_sums[:3] if n_own > 0 else torch.zeros(3, dtype=torch.float64, device=self.device)
            stats = torch.cat([stats, rs])
        if train:
            self.flat.all_reduce_grads()                        # an empty shard contributes its zeroed bucket
            self.optimizer.step()
        if self.world > 1 or (FORCE_COLLECTIVES and dist.is_initialized()):
            dist.all_reduce(stats, op=dist.ReduceOp.SUM)
        vals = stats.tolist()                                   # the step's only host sync
        return [v / vals[3] for v in vals[:3]] + [v / vals[3] for v in vals[4:]]

    def _log_reward(self, split, means, epoch):
        """The reward figures of an epoch under a criterion beside f1 / dcg: mean reward at the cut, mean best reward of the
        list, share of lists cut at their best reward."""
        r_k, r_best, share = means
        self.writer.add_scalar(split + '/reward_at_k_epoch', r_k, epoch)
        self.writer.add_scalar(split + '/reward_best_epoch', r_best, epoch)
        self.writer.add_scalar(split + '/cut_at_best_epoch', share, epoch)
        if self.rank == 0:
            logging.info('\t{}: reward@k = {:.6f} | best reward = {:.6f} | cut at best = {:.4f}  ({})\n'.format(
                split.capitalize(), r_k, r_best, share, self.args.criterion))
        return {"reward_at_k": r_k, "reward_best": r_best, "cut_at_best": share}

    def train_epoch(self, epoch):
        start = time.time()
        tot, step, num_itr = [0.0] * (6 if self.reward_stats else 3), 0, len(self.train_loader)
        logging.info('-' * 100)
        for X, y in self.train_loader:
            self.model.train()
            self.optimizer.zero_grad()
            vals = self._step(X, y, True)
            self.writer.add_scalar('train/loss_step', vals[0], step + num_itr * epoch)   # run.py:146
            tot = [a + b for a, b in zip(tot, vals)]
            step += 1
        loss, f1, dcg = [v / step for v in tot[:3]]             # unweighted over steps, run.py:153
        self.writer.add_scalar('train/loss_epoch', loss, epoch)
        self.writer.add_scalar('train/F1_epoch', f1, epoch)
        self.writer.add_scalar('train/DCG_epoch', dcg, epoch)
        self.history.append({"epoch": epoch, "train": (loss, f1, dcg)})
        if self.reward_stats:
            self.history[-1]["train_reward"] = self._log_reward('train', [v / step for v in tot[3:]], epoch)
        grad = log_grad_guard(self.writer, self.optimizer, epoch)
        if grad is not None:
            self.history[-1]["grad"] = grad
        if self.optimizer.recipe:                               # the learning rate of the epoch's last applied step
            lr = self.optimizer.epoch_stats(reset=False)["lr"]
            self.writer.add_scalar('train/lr', lr, epoch)
            self.history[-1]["lr"] = lr
        if self.rank == 0:
            logging.info('\nEpoch: {} | Epoch Time: {:.2f} s'.format(epoch, time.time() - start))
            logging.info('\tTrain: loss = {} | f1 = {:.6f} | dcg = {:.6f}\n'.format(loss, f1, dcg))
        return loss, f1, dcg

    def eval_weights(self):
        """--ema-eval 1: the block computes with the averaged weights (FusedAdam.ema_weights); otherwise with the raw iterate."""
        return self.optimizer.ema_weights() if getattr(self, "ema_eval", False) else contextlib.nullcontext()

    def test(self, epoch):
        with self.eval_weights():
            return self._test(epoch)

    def _test(self, epoch):
        tot, step = [0.0] * (6 if self.reward_stats else 3), 0
        for X, y in self.test_loader:
            self.model.eval()
            with torch.no_grad():
                vals = self._step(X, y, False)
            tot = [a + b for a, b in zip(tot, vals)]
            step += 1
        loss, f1, dcg = [v / step for v in tot[:3]]             # run.py:195
        self.writer.add_scalar('test/loss_epoch', loss, epoch)
        self.writer.add_scalar('test/F1_epoch', f1, epoch)
        self.writer.add_scalar('test/DCG_epoch', dcg, epoch)
        if self.history and self.history[-1]["epoch"] == epoch:
            self.history[-1]["test"] = (loss, f1, dcg)
        if self.reward_stats:
            rw = self._log_reward('test', [v / step for v in tot[3:]], epoch)
            if self.history and self.history[-1]["epoch"] == epoch:
                self.history[-1]["test_reward"] = rw
        self.f1_record.append(f1)
        self.dcg_record.append(dcg)
        if self.rank == 0:
            logging.info('\tTest: loss = {} | f1 = {:.6f} | dcg = {:.6f}\n'.format(loss, f1, dcg))
        if f1 > self.best_test_f1:                              # run.py:203-206
            self.best_test_f1, self.best_epoch = f1, epoch
            if self.model_persist and self.rank == 0:
                self.save_model()
        if dcg > self.best_test_dcg:
            self.best_test_dcg = dcg
        if self.rerank_by and self.rank == 0:
            self._test_reranked(epoch)
        return loss, f1, dcg

    def _forward_heads(self, x):
        """(the values of the --rerank-eval head, the cut distribution) of one batch, eval mode, no gradient."""
        self.model.eval()
        with torch.no_grad():
            out = self.model(x.to(self.device, non_blocking=True))
        return out[self.model.head_names().index(self.rerank_by)], out[-1]

    def _reranked_eval(self, L):
        from utils.rerank import RerankedEval
        ks = [int(k) for k in str(self.args.fixed_k).split(',') if k.strip()]
        return RerankedEval(L, by=self.rerank_by, metric=report_metric(self.args.criterion), reward=eval_reward_spec(self.args),
                            fixed_k=ks, device=self.device)

    def _test_reranked(self, epoch):
        """--rerank-eval: the test lists once more through the model, every figure in the retrieval order and in the head's
        order (utils/rerank.py).  No collective: rank 0 calls it."""
        from utils.rerank import mean_over_lengths
        evals = {}
        for X, y in self.test_loader:
            L = int(X.shape[1])
            if L not in evals:
                evals[L] = self._reranked_eval(L)
            head, cut = self._forward_heads(X)
            evals[L].update(head, cut, y)
        summ = {str(L): ev.summary() for L, ev in sorted(evals.items())}
        means = mean_over_lengths(summ)
        for m, tag in (("f1", "F1"), ("dcg", "DCG")):
            self.writer.add_scalar('test/{}_orig_epoch'.format(tag), means["orig"][m], epoch)
            self.writer.add_scalar('test/{}_rr_epoch'.format(tag), means["rr"][m], epoch)
        for L, s in summ.items():
            for name, v in s["rr"].items():
                self.writer.add_scalar('test_rr/{}'.format(name), v, epoch * 100000 + int(L))
        logging.info('\tTest, re-ranked by {}: f1 = {:.6f} -> {:.6f} | dcg = {:.6f} -> {:.6f}\n'.format(
            self.rerank_by, means["orig"]["f1"], means["rr"]["f1"], means["orig"]["dcg"], means["rr"]["dcg"]))
        if self.history and self.history[-1]["epoch"] == epoch:
            self.history[-1]["test_rr"] = {"by": self.rerank_by, "f1": means["orig"]["f1"], "f1_rr": means["rr"]["f1"],
                                           "dcg": means["orig"]["dcg"], "dcg_rr": means["rr"]["dcg"], "lengths": summ}
        return summ

    def _warn_axis(self, stored, path, stored_mask="none"):
        if stored != self.attention_axis:
            logging.warning('{} was written with --attention-axis {}; this run uses {} (the weights load, the model differs)'.format(
                path, stored, self.attention_axis))
        if stored_mask != self.attention_mask:
            logging.warning('{} was written with --attention-mask {}; this run uses {} (the weights load, the model differs)'.format(
                path, stored_mask, self.attention_mask))

    def _mask_record(self):
        """{'attention_mask': 'causal'} for a causal run, {'cut_head': 'hazard', 'hazard_prior': ...} for a hazard-head run, {}
        otherwise: a default run writes no new key"""
        rec = {"attention_mask": self.attention_mask} if self.attention_mask != "none" else {}
        if self.cut_head != "softmax":
            rec.update(cut_head=self.cut_head, hazard_prior=self.hazard_prior)
        return rec

    def save_model(self):
        os.makedirs(self.save_path, exist_ok=True)
        with open(os.path.join(self.save_path, '{}.pkl.meta.json'.format(self.model_name)), "w") as f:      # beside the state_dict
            json.dump({"attention_axis": self.attention_axis, **self._mask_record()}, f)
        # clone: parameters are views of the flat bucket
        state = {k: v.detach().clone().cpu() for k, v in self.model.state_dict().items()}
        torch.save(state, os.path.join(self.save_path, '{}.pkl'.format(self.model_name)))
        logging.info('The best model has beed updated and saved in {}\n'.format(self.save_path))

    def save_state(self, path, epoch):
        """--save-state: the training checkpoint after `epoch` - model, optimizer state_dict (moments, step count, ema, recipe
        state), the epoch, the best figures and the records.  --resume continues from it."""
        opt = {k: (v.detach().clone().cpu() if torch.is_tensor(v) else v) for k, v in self.optimizer.state_dict().items()}
        state = {"model": {k: v.detach().clone().cpu() for k, v in self.model.state_dict().items()}, "optimizer": opt, "epoch": epoch,
                 "best_test_f1": self.best_test_f1, "best_test_dcg": self.best_test_dcg, "best_epoch": self.best_epoch,
                 "f1_record": self.f1_record, "dcg_record": self.dcg_record, "history": self.history,
                 "attention_axis": self.attention_axis, **self._mask_record()}
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(state, path)

    def load_model(self):
        meta = self.model_path + '.meta.json'
        if os.path.exists(meta):
            with open(meta) as f:
                stored = json.load(f)
                self._warn_axis(stored.get("attention_axis", "list"), self.model_path, stored.get("attention_mask", "none"))
        self.model.load_state_dict(torch.load(self.model_path, map_location=self.device))
        logging.info('The best model has beed loaded from {}\n'.format(self.model_path))

    def baselines(self):
        """The reference's Baseline/ notebooks on this run's labels, for each list length of the test split: Oracle (each list's
        best cut) and Fixed-k on the test lists, Greedy-k with its k from the train lists of the same length.  Logged, written
        to the scalar log under baseline/... (step = the list length) and returned as {length: {...}}.  No collective."""
        from utils.baselines import TruncationCurves
        data = self.data
        ks = [int(k) for k in str(self.args.fixed_k).split(',') if k.strip()]
        single = len(data.lengths) == 1 and data.test_lengths == data.lengths
        out = {}
        for L in data.test_lengths:
            if single:
                y_train, y_test = data.gety_train(), data.gety_test()
            else:
                y_test = data.buckets['test'][L][1]
                y_train = data.buckets['train'][L][1] if L in data.buckets['train'] else None
            test = TruncationCurves(L, self.device).update(y_test)
            f1, dcg = test.best_cut()
            rec = {'n_test': test.n_lists, 'Oracle': {'f1': f1, 'dcg': dcg}, 'fixed_k': {}}
            logging.info('\tBaseline Oracle (S = {}): f1 = {:.6f} | dcg = {:.6f}'.format(L, f1, dcg))
            self.writer.add_scalar('baseline/Oracle_F1', f1, L)
            self.writer.add_scalar('baseline/Oracle_DCG', dcg, L)
            for k in ks:
                if not 0 <= k <= L:
                    logging.info('\tBaseline Fixed-k (S = {}, k = {}): k outside the list, skipped'.format(L, k))
                    continue
                f1, dcg = test.fixed_k(k)
                rec['fixed_k'][str(k)] = {'f1': f1, 'dcg': dcg}
                logging.info('\tBaseline Fixed-k (S = {}, k = {}): f1 = {:.6f} | dcg = {:.6f}'.format(L, k, f1, dcg))
                self.writer.add_scalar('baseline/Fixed_k{}_F1'.format(k), f1, L)
                self.writer.add_scalar('baseline/Fixed_k{}_DCG'.format(k), dcg, L)
            if y_train is not None:
                train = TruncationCurves(L, self.device).update(y_train)
                k_f1, k_dcg = train.best_k()
                f1, dcg = test.fixed_k((k_f1, k_dcg))
                rec['n_train'] = train.n_lists
                rec['greedy_k'] = {'k_f1': k_f1, 'k_dcg': k_dcg, 'f1': f1, 'dcg': dcg}
                logging.info('\tBaseline Greedy-k (S = {}, k_f1 = {}, k_dcg = {}): f1 = {:.6f} | dcg = {:.6f}'.format(
                    L, k_f1, k_dcg, f1, dcg))
                self.writer.add_scalar('baseline/Greedy_k_F1', f1, L)
                self.writer.add_scalar('baseline/Greedy_k_DCG', dcg, L)
                self.writer.add_scalar('baseline/Greedy_k_kF1', k_f1, L)
                self.writer.add_scalar('baseline/Greedy_k_kDCG', k_dcg, L)
            else:
                logging.info('\tBaseline Greedy-k (S = {}): no train lists of this length, skipped'.format(L))
            spec = eval_reward_spec(self.args)
            if spec is not None:                # --eval-reward: the same three rows in that reward
                rec['reward'] = self._reward_baselines(spec, L, y_train, y_test, ks)
            out[str(L)] = rec
        return out

    def _reward_baselines(self, spec, L, y_train, y_test, ks):
        """Oracle / Fixed-k / Greedy-k of one list length in the reward `spec` (utils.baselines.RewardCurves): logged, written
        to the scalar log under baseline/..._reward and returned as a dict."""
        from utils.baselines import RewardCurves
        test = RewardCurves(L, spec, self.device).update(y_test)
        rec = {'spec': eval_reward_text(spec), 'Oracle': test.best_cut(), 'fixed_k': {}}
        logging.info('\tBaseline Oracle (S = {}): reward = {:.6f} ({})'.format(L, rec['Oracle'], rec['spec']))
        self.writer.add_scalar('baseline/Oracle_reward', rec['Oracle'], L)
        for k in ks:
            if 0 <= k <= L:
                rec['fixed_k'][str(k)] = test.fixed_k(k)
                logging.info('\tBaseline Fixed-k (S = {}, k = {}): reward = {:.6f}'.format(L, k, rec['fixed_k'][str(k)]))
                self.writer.add_scalar('baseline/Fixed_k{}_reward'.format(k), rec['fixed_k'][str(k)], L)
        if y_train is not None:
            k = RewardCurves(L, spec, self.device).update(y_train).best_k()
            rec['greedy_k'] = {'k': k, 'reward': test.fixed_k(k)}
            logging.info('\tBaseline Greedy-k (S = {}, k = {}): reward = {:.6f}'.format(L, k, rec['greedy_k']['reward']))
            self.writer.add_scalar('baseline/Greedy_k_reward', rec['greedy_k']['reward'], L)
            self.writer.add_scalar('baseline/Greedy_k_kreward', k, L)
        return rec

    def _split_batches(self, split):
        """(length, qids, x, y) of every bucket of a split in file order (no shuffling); BicutData keeps the same buckets."""
        for L, (x, y, qids) in sorted(self.data.buckets[split].items()):
            yield L, qids, x, y

    def _forward_eval(self, x):
        """The cut distribution of one batch of a bucket, eval mode, no gradient (sparse BiCut: as SparseBatchLoader feeds it)."""
        x = x.to(self.device, non_blocking=True)
        if self.sparse_bicut:
            Dn = self.data.table.Dn
            x = ops.SparseBatch(x[..., :Dn].contiguous(), x[..., Dn].contiguous().view(torch.int32), self.data.table)
        self.model.eval()
        with torch.no_grad():
            out = self.model(x)
        return out[-1] if isinstance(out, (list, tuple)) else out

    def _forward_eval_stop(self, x):
        """(the cut distribution, the stop probabilities (B,S)) of one batch of a hazard-head model, eval mode, no gradient."""
        return self.model._eval_outputs(x.to(self.device, non_blocking=True))

    def report(self, path, split="test", labelled=True):
        """--report-out: every list of `split`, length bucket by length bucket, through the model and `CutReport`; one .npz with
        the per-query arrays (rows in the order of `qid`), and per list length the k histogram, the two curves and the summary
        (JSON).  Returns {length: summary}.  No collective: rank 0 calls it.  The model runs once per batch and `CutReport` takes
        k and p_k from that output in the same pass as the rest - what `model.truncate` returns for the batch, without the
        second forward pass a call of it would cost."""
        import numpy as np
        from utils.report import CutReport
        arrays, summaries, per_len = {}, {}, {}
        qid_all, len_all = [], []
        spec = eval_reward_spec(self.args) if labelled else None
        for L, qids, x, y in self._split_batches(split):
            rep = CutReport(L, metric=report_metric(self.args.criterion), device=self.device, reward=spec)
            rr = self._reranked_eval(L) if self.rerank_by and labelled else None
            for i in range(0, x.shape[0], self.batch_size):
                if rr is not None:              # one forward pass serves both
                    head, cut = self._forward_heads(x[i:i + self.batch_size])
                    rr.update(head, cut, y[i:i + self.batch_size])
                else:
                    cut = self._forward_eval(x[i:i + self.batch_size])
                rep.update(cut, y[i:i + self.batch_size] if labelled else None)
            for name, a in rep.per_query().items():
                arrays.setdefault(name, []).append(a)
            if rr is not None:
                for name, a in rr.per_query().items():
                    if name.endswith("_rr"):
                        arrays.setdefault(name, []).append(a)
            qid_all += [str(q) for q in qids]
            len_all += [L] * len(qids)
            reward, pred = rep.curves(tail_fix=True)
            summ = rep.summary()
            per_len[f"hist_{L}"] = np.asarray(summ.pop("hist"))
            per_len[f"pred_curve_{L}"] = pred
            if reward is not None:
                per_len[f"reward_curve_{L}"] = reward
            summaries[str(L)] = summ
            logging.info('\tReport ({} split, S = {}): {}'.format(split, L, json.dumps(summ)))
            for key, v in summ.items():
                if not isinstance(v, str):
                    self.writer.add_scalar('report/{}'.format(key), v, L)
        if spec is not None:                    # the reward the reward columns are in: compare_reports(metric='reward') checks it
            per_len["reward_spec"] = np.asarray(eval_reward_text(spec))
        per_len["attention_axis"] = np.asarray(self.attention_axis)
        if self.attention_mask != "none":
            per_len["attention_mask"] = np.asarray(self.attention_mask)
        if self.cut_head != "softmax":
            per_len["cut_head"] = np.asarray(self.cut_head)
            per_len["hazard_prior"] = np.asarray(self.hazard_prior)
        if self.rerank_by and labelled:
            per_len["rerank_by"] = np.asarray(self.rerank_by)
        np.savez(path, qid=np.asarray(qid_all), length=np.asarray(len_all, dtype=np.int32), lengths=np.asarray(sorted(map(int, summaries))),
                 summary=np.asarray(json.dumps(summaries)), **{k: np.concatenate(v) for k, v in arrays.items()}, **per_len)
        return summaries

    def compare(self, path, others):
        """--compare-to A.npz[,B.npz]: the report just written at `path` against the named ones (each of them the baseline of one
        comparison), on the run's criterion: one logged line per file."""
        from utils.compare import compare_reports
        fresh = path if path.endswith(".npz") else path + ".npz"
        lines = []
        for other in [o for o in others.split(",") if o]:
            cmp = compare_reports([other, fresh], metric=compare_metric(self.args), baseline=0,
                                  resamples=10000, seed=self.args.seed or 0, device=self.device)
            lines += cmp.lines()
        for line in lines:
            logging.info('\tCompare: {}'.format(line))
        return lines

    def cut_sweep(self, spec, out_path=None):
        """--cut-sweep RULE:LO:HI:N (or score:auto:N): per list length of the test split, the train and the test buckets go
        through one forward each and `CutSweep` (utils/sweep.py); tau* = the first threshold with the best mean of the run's
        criterion on the train lists.  Logs the test curve and the test figures at tau* beside the argmax cut's, writes
        everything to `out_path` (.npz, or .json) and returns {length: {...}}.  The 'score' rule reads feature 0 of X and runs no
        model.  No collective: rank 0 calls it."""
        import numpy as np
        from utils.report import CutReport
        from utils.sweep import CutSweep, score_quantiles
        rule, thresholds = spec if isinstance(spec, tuple) else parse_cut_sweep(spec)
        metric = argmax_metric = self.args.criterion if self.args.criterion in ("f1", "dcg") else "f1"
        reward = eval_reward_spec(self.args)
        if reward is not None:                  # --eval-reward: tau* on the mean reward of the cuts; the argmax report keeps F1 / DCG
            metric = "reward"
        buckets = {split: {L: (x, y) for L, _q, x, y in self._split_batches(split)} for split in ("train", "test")}
        results, arrays = {}, {}
        for L, (x_te, y_te) in buckets["test"].items():
            if L not in buckets["train"]:
                logging.info('\tCut sweep (S = {}): no train lists of this length, skipped'.format(L))
                continue
            x_tr, y_tr = buckets["train"][L]
            th = score_quantiles(x_tr[..., 0].cpu().numpy(), thresholds) if isinstance(thresholds, int) else thresholds
            sweeps = {}
            argmax = None if rule == "score" else CutReport(L, metric=argmax_metric, device=self.device, reward=reward)
            for split, (x, y) in (("train", (x_tr, y_tr)), ("test", (x_te, y_te))):
                sw = CutSweep(L, rule, th, device=self.device, reward=reward)
                for i in range(0, x.shape[0], self.batch_size):
                    xb, yb = x[i:i + self.batch_size], y[i:i + self.batch_size]
                    if rule == "above" and self.cut_head == "hazard":
                        # the rule's own input: the first rank whose STOP probability reaches tau (the argmax report keeps p)
                        v, stop = self._forward_eval_stop(xb)
                        sw.update(stop, yb)
                    else:
                        v = xb[..., 0].to(self.device, non_blocking=True) if rule == "score" else self._forward_eval(xb)
                        sw.update(v, yb)
                    if argmax is not None and split == "test":
                        argmax.update(v, yb)
                sweeps[split] = sw
            tau, idx, _ = sweeps["train"].best(metric)
            rec = {"rule": rule, "metric": metric, "tau": tau, "index": idx, "n_train": sweeps["train"].n_lists,
                   "n_test": sweeps["test"].n_lists, "train": sweeps["train"].at(tau), "test": sweeps["test"].at(tau)}
            if argmax is not None:
                summ = argmax.summary()
                rec["argmax"] = {"f1": summ["f1"], "dcg": summ["dcg"], "k": summ["mean_k"],
                                 **({"reward": summ["reward"]} if reward is not None else {})}
            for split, sw in sweeps.items():
                c = sw.curve()
                arrays[f"thresholds_{L}"] = c["thresholds"]
                for name in ("k", "f1", "dcg", "precision", "recall", "fbeta", "uncut") + (("reward",) if reward is not None else ()):
                    arrays[f"{split}_{name}_{L}"] = c[name]
                if split == "test":
                    for t, kk, f1, dcg in zip(c["thresholds"], c["k"], c["f1"], c["dcg"]):
                        logging.info('\tCut sweep ({} S = {}): tau = {:.6g} | mean k = {:.3f} | f1 = {:.6f} | dcg = {:.6f}'.format(
                            rule, L, t, kk, f1, dcg))
            logging.info('\tCut sweep ({} S = {}) at the train-tuned tau* = {:.6g}: test {}{}'.format(
                rule, L, tau, json.dumps(rec["test"]), ' | argmax cut: {}'.format(json.dumps(rec["argmax"])) if argmax is not None else ''))
            results[str(L)] = rec
        if out_path:
            if out_path.endswith(".json"):
                with open(out_path, "w") as f:
                    json.dump({"results": results, "curves": {k: v.tolist() for k, v in arrays.items()}}, f)
            else:
                np.savez(out_path, summary=np.asarray(json.dumps(results)), lengths=np.asarray(sorted(map(int, results))), **arrays)
        return results

    def stream_eval(self, page, tau, compact=0, compact_below=1.0):
        """--stream-eval: the test split once more, a page of `page` ranks at a time through model.stream; the lists of a
        bucket whose length is not the model's seq_len cannot be streamed and are an error.  Means over the lists: the streamed
        cut, F1 and DCG at it (ops.cut_metrics with k_in) and the ranks read (whole pages up to the stop).  No collective: rank
        0 calls it.  One host read per batch, after its last page.  compact (--stream-compact N): the stopped lists leave the batch
        after every N-th page (one 4-byte read more per compaction); then also the mean rows computed per list, beside the
        seq_len rounded up to pages that every list costs without it."""
        n, tot, rows = 0, [0.0, 0.0, 0.0, 0.0], 0
        for X, y in self.test_loader:
            B, S = int(X.shape[0]), int(X.shape[1])
            if S != self.model.seq_len:
                raise ValueError(f"--stream-eval: a test bucket of length {S} does not match the model's seq_len {self.model.seq_len}")
            st = self.model.stream(tau, B, compact_every=compact or None, compact_below=compact_below)
            scores = X.to(self.device, non_blocking=True)[..., :1].contiguous()
            for t0 in range(0, S, page):
                st.push(scores[:, t0:t0 + page].contiguous())
            k = st.k
            _, f1, dcg, _ = ops.cut_metrics(None, y.to(self.device, non_blocking=True).float().contiguous(), k_in=k)
            vals = torch.stack([k.double().sum(), f1.sum(), dcg.sum(), st.documents_read().double().sum()]).tolist()
            tot = [a + b for a, b in zip(tot, vals)]
            n += B
            rows += st.rows_computed()
        res = {"stream_page": int(page), "stream_tau": float(tau), "stream_lists": n, "stream_k": tot[0] / n, "stream_f1": tot[1] / n,
               "stream_dcg": tot[2] / n, "stream_read": tot[3] / n}
        logging.info('\tStreamed test (pages of {}, tau = {}): cut = {:.3f} | f1 = {:.6f} | dcg = {:.6f} | ranks read = {:.3f}\n'.format(
            page, tau, res["stream_k"], res["stream_f1"], res["stream_dcg"], res["stream_read"]))
        if compact:
            res.update(stream_compact=int(compact), stream_compact_below=float(compact_below), stream_rows=rows / n,
                       stream_rows_full=float((self.model.seq_len + page - 1) // page * page))
            logging.info('\tCompacted every {} pages (live fraction <= {}): rows computed per list = {:.3f} of {:.0f}\n'.format(
                compact, compact_below, res["stream_rows"], res["stream_rows_full"]))
        return res

    def draw(self, epoch):
        """--draw 1 (run.py:188): for every test batch of more than 40 lists, the two curves `Trainer.plot` draws (run.py:262-283,
        tau = 0.9) into the scalar log.  The batches are the test buckets in file order."""
        from utils.report import CutReport
        step = 0
        for L, _qids, x, y in self._split_batches("test"):
            for i in range(0, x.shape[0], self.batch_size):
                if x[i:i + self.batch_size].shape[0] <= 40:
                    continue
                rep = CutReport(L, metric=report_metric(self.args.criterion), tau=0.9, device=self.device)
                rep.update(self._forward_eval(x[i:i + self.batch_size]), y[i:i + self.batch_size])
                reward, pred = rep.curves(tail_fix=False)      # the figure's norm_s[-3:] overwrite is presentation: not logged
                self.writer.add_curve('draw/reward', reward, epoch * 100000 + step)
                self.writer.add_curve('draw/prediction', pred, epoch * 100000 + step)
                step += 1

    def run(self):
        if self.args.baselines and self.rank == 0:
            self.baseline_results = self.baselines()
        if self.rank == 0:
            logging.info('\nTrain the {} model: \n'.format(self.model_name))
        for epoch in range(getattr(self, "start_epoch", 0), self.epochs):
            self.train_epoch(epoch)
            self.test(epoch)
            if getattr(self.args, "draw", 0) and epoch % 2 == 0 and self.rank == 0:      # (drivers build their own Namespace)
                self.draw(epoch)
            if getattr(self.args, "save_state", None) and self.rank == 0:
                self.save_state(self.args.save_state, epoch)
        with self.eval_weights():
            if getattr(self.args, "report_out", None) and self.rank == 0:
                self.report_results = self.report(self.args.report_out, getattr(self.args, "report_split", "test"),
                                                  bool(getattr(self.args, "report_labels", 1)))
                if getattr(self.args, "compare_to", None):
                    self.compare_lines = self.compare(self.args.report_out, self.args.compare_to)
            if getattr(self.args, "cut_sweep", None) and self.rank == 0:
                self.sweep_results = self.cut_sweep(self.args.cut_sweep, getattr(self.args, "sweep_out", None))
            if getattr(self.args, "stream_eval", 0) and self.rank == 0:
                self.stream_results = self.stream_eval(self.args.stream_eval, getattr(self.args, "stream_tau", 0.5),
                                                          getattr(self.args, "stream_compact", 0), getattr(self.args, "stream_compact_below", 1.0))
        top = sorted(self.f1_record, reverse=True)[:5]
        topd = sorted(self.dcg_record, reverse=True)[:5]
        best5_f1, best5_dcg = sum(top) / 5, sum(topd) / 5       # run.py:229-230 divides by 5 regardless
        self.best5_f1, self.best5_dcg = best5_f1, best5_dcg
        self.writer.close()
        if self.rank == 0:
            logging.info('the best metric of this model: f1: {} | dcg: {}'.format(self.best_test_f1, self.best_test_dcg))
            logging.info('the best-5 metric of this model: f1: {} | dcg: {}'.format(best5_f1, best5_dcg))
        return self.best_test_f1, self.best_test_dcg


GRAD_GUARD_TAGS = ('train/grad_norm_epoch', 'train/grad_norm_max_epoch', 'train/clipped_steps', 'train/skipped_steps')


def add_grad_guard_arguments(p):
    """--clip-grad-norm / --skip-nonfinite of run.py, verify_probe.py and verify_BMT.py: FusedAdam's guarded step."""
    p.add_argument('--clip-grad-norm', type=float, default=0.0,
                   help="F > 0: clip the gradient's global L2 norm to F before every Adam step (torch's clip_grad_norm_ rule, on the "
                        "device, after the gradient all-reduce) and log train/grad_norm_epoch, train/grad_norm_max_epoch, "
                        "train/clipped_steps, train/skipped_steps per epoch; 0: off")
    p.add_argument('--skip-nonfinite', type=int, default=0, choices=(0, 1),
                   help="1: a step whose gradient holds a NaN or an Inf leaves parameters and Adam moments untouched and is counted "
                        "in train/skipped_steps")


def grad_guard_kwargs(args):
    """FusedAdam's keyword arguments for the two flags; empty with both at their defaults (the plain rlt_adam_step path).  The norm
    is taken inside step(), i.e. after FlatModel.all_reduce_grads(): every rank forms the same coefficient from the same bucket."""
    clip, skip = float(getattr(args, "clip_grad_norm", 0) or 0), bool(getattr(args, "skip_nonfinite", 0))   # (drivers build their own Namespace)
    return dict(max_grad_norm=clip if clip > 0 else None, skip_nonfinite=skip) if clip > 0 or skip else {}


def log_grad_guard(writer, optimizer, epoch):
    """The epoch's one read of the optimizer state, under GRAD_GUARD_TAGS; returns the same values for --history-json (None, and
    nothing logged, when the guarded step is off)."""
    if not optimizer.guarded:
        return None
    gs = optimizer.epoch_stats(reset=True)
    vals = (gs["grad_norm_mean"], gs["grad_norm_max"], gs["clipped_steps"], gs["skipped_steps"])
    for tag, v in zip(GRAD_GUARD_TAGS, vals):
        writer.add_scalar(tag, v, epoch)
    # an epoch without one finite gradient has no mean norm (JSON has no NaN)
    return {tag.split('/', 1)[1]: (v if math.isfinite(v) else None) for tag, v in zip(GRAD_GUARD_TAGS, vals)}


def eval_reward_spec(args):
    """--eval-reward -> the RewardSpec the baselines, the report, the comparison and the sweep also evaluate in, or None (off,
    the default).  'criterion' is the run's own reward and an error under f1 / dcg, which those tools already speak."""
    text = getattr(args, "eval_reward", None)       # (drivers build their own Namespace)
    if not text:
        return None
    if text == "criterion":
        if not RewardSpec.is_spec(args.criterion):
            raise ValueError("--eval-reward criterion needs a --criterion beside f1 / dcg (fbeta:<beta>, ndcg, gain:...); "
                             "F1 and DCG are reported as they are")
        text = args.criterion
    return RewardSpec.parse(text)


def eval_reward_text(spec):
    try:
        return str(spec)
    except ValueError:                              # a reward with its own discounts has no text form
        return repr(spec)


def compare_metric(args):
    """The column --compare-to compares: 'reward' under --eval-reward, otherwise report_metric's."""
    return 'reward' if eval_reward_spec(args) is not None else report_metric(args.criterion)


def report_metric(criterion):
    """The metric of the cut report, the comparison and --draw, which know F1 and DCG: the run's criterion, or F1 under a reward
    beside those two (utils/rewards.py)."""
    return 'f1' if RewardSpec.is_spec(criterion) else criterion


def parse_cut_sweep(spec):
    """argparse type of --cut-sweep: 'RULE:LO:HI:N' or 'score:auto:N' -> (rule, thresholds or N) (utils/sweep.py)."""
    from utils.sweep import parse_sweep
    try:
        return parse_sweep(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def build_parser():
    p = argparse.ArgumentParser(description="Truncation Model Trainer Args (HIP hot path)")
    p.add_argument('--retrieve-data', type=str, default='robust04')
    p.add_argument('--dataset-name', type=str, default='drmm_tks')
    p.add_argument('--batch-size', type=int, default=63)
    p.add_argument('--model-name', type=str, default='mmoecut')
    p.add_argument('--augmented-reward', type=int, default=1)
    p.add_argument('--div-type', type=str, default='js')
    p.add_argument('--criterion', type=str, default='dcg')
    p.add_argument('--model-path', type=str, default=None)
    p.add_argument('--ft', type=int, default=0)
    p.add_argument('--model-persist', type=int, default=0)
    p.add_argument('--save-path', type=str, default=os.path.join(HERE, 'best_model'))
    p.add_argument('--epochs', type=int, default=80)
    p.add_argument('--lr', type=float, default=3e-5)
    p.add_argument('--weight-decay', type=float, default=0.005)
    p.add_argument('--dropout', type=float, default=0.1)
    p.add_argument('--num-tasks', type=float, default=3)       # 2.1: class + cut | 2.2: rerank + cut
    p.add_argument('--rerank-weight', type=float, default=0.3)
    p.add_argument('--class-weight', type=float, default=0.4)
    # additions
    p.add_argument('--num-experts', type=int, default=3, help="MMOECut experts (the reference hard-codes 3, run.py:89)")
    p.add_argument('--dataset-base', type=str, default=None, help="directory holding <retrieve_data>/*.pkl")
    p.add_argument('--synthetic', type=int, default=0, help="write a robust04-shaped synthetic set into --dataset-base first")
    p.add_argument('--use-conf', type=int, default=1, help="override lr/batch/dropout/wd/task weights from hyper_parameter_<dataset>.conf")
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--attention-axis', type=str, default='list', choices=('list', 'position'),
                   help="axis the encoder layers attend over: 'list' = the lists of a mini-batch attend to each other at every position "
                        "(the reference); 'position' = every list attends over its own positions (the papers' model; a list's cut "
                        "then does not depend on its batch).  Recorded in --history-json, --report-out and --save-state")
    p.add_argument('--attention-mask', type=str, default='none', choices=('none', 'causal'),
                   help="'causal' (needs --attention-axis position): position i attends to the positions <= i of its list, so the "
                        "encoder's output at rank i does not look below rank i (Choopy's logits are then prefix-only; AttnCut's "
                        "BiLSTM and every softmax over positions stay global).  Recorded beside the axis when it is 'causal'")
    p.add_argument('--cut-head', type=str, default='softmax', choices=('softmax', 'hazard'),
                   help="'hazard' (choopy, attncut, mtchoopy, mtattncut): the cut head emits a stop probability per position and "
                        "the cut distribution is p_s = h_s prod_{j<s} (1 - h_j), the last position taking the rest; its value at "
                        "rank i reads ranks <= i only, so with --attention-axis position --attention-mask causal Choopy's stop "
                        "probabilities are online and --cut-sweep above:... sweeps them.  Same parameters: checkpoints load across "
                        "heads.  Recorded in checkpoints and reports when it is 'hazard'")
    p.add_argument('--hazard-prior', type=str, default='uniform', choices=('uniform', 'none'),
                   help="fixed offset of the hazard head's logits: 'uniform' = -log(S-1-s), under which zero weights give the uniform "
                        "cut distribution (without it they give a geometric one with mean 2, which cannot reach long cuts)")
    p.add_argument('--stream-eval', type=int, default=0, metavar='C',
                   help="choopy with --attention-axis position --attention-mask causal --cut-head hazard only: after the last epoch "
                        "walk the test split in pages of C ranks through model.stream (utils/stream.py) and log the mean cut, F1 and "
                        "DCG at the streamed cut and the mean ranks read; `stream_*` keys in --history-json.  0 = off")
    p.add_argument('--stream-tau', type=float, default=0.5, help="the stop threshold of --stream-eval (truncate's rule 'above')")
    p.add_argument('--stream-compact', type=int, default=0, metavar='N',
                   help="with --stream-eval: take the stopped lists out of the batch after every N-th page (StreamingTruncator.compact), so "
                        "that the pages behind a stop cost no GEMM rows; `stream_compact`, `stream_rows`, `stream_rows_full` in "
                        "--history-json.  0 = off")
    p.add_argument('--stream-compact-below', type=float, default=1.0, metavar='F',
                   help="--stream-compact moves the caches only when at most this fraction of the batch's slots is still live")
    p.add_argument('--history-json', type=str, default=None, help="rank 0 writes the per-epoch train / test means and the best / best-5 figures here")
    p.add_argument('--param-dump-dir', type=str, default=None,
                   help="every rank saves its final flat parameter bucket as flat_param_rank<r>.npy here (data-parallel checks: the "
                        "replicas must stay bitwise identical)")
    p.add_argument('--baselines', type=int, default=0, choices=(0, 1),
                   help="1: rank 0 first reports the Oracle / Fixed-k / Greedy-k truncation baselines of the run's labels "
                        "(the reference's Baseline/ notebooks), per list length")
    p.add_argument('--fixed-k', type=str, default='5,10,30', help="comma-separated cut positions of the Fixed-k baseline")
    p.add_argument('--report-out', type=str, default=None,
                   help="rank 0 writes a per-query cut report of the final model (.npz: k, winning value, margin, F1 / DCG at the cut, "
                        "each list's best and the count of better cuts, keyed by query id; per list length the k histogram, the "
                        "reward / prediction curves and the summary); with --epochs 0 --ft 1 --model-path CKPT it reports a checkpoint")
    p.add_argument('--compare-to', type=str, default=None,
                   help="A.npz[,B.npz]: after --report-out, rank 0 compares the fresh report with each named one query by query "
                        "(paired randomization test, bootstrap interval, sign and t statistics) and logs one line per file")
    p.add_argument('--eval-reward', type=str, default=None, metavar='criterion|SPEC',
                   help="also evaluate in a cut reward beside F1 / DCG: 'criterion' (the run's own --criterion, which must then be a "
                        "reward spec) or a spec (fbeta:<beta>, ndcg[:<penalty>], gain:<g0>,<g1>,...[:norm]).  --baselines 1 adds "
                        "Oracle / Fixed-k / Greedy-k in that reward, --report-out writes reward, best_reward, best_reward_k and "
                        "better_reward per query, --compare-to and --cut-sweep use the reward.  Default: off")
    p.add_argument('--report-split', type=str, default='test', choices=('train', 'test'))
    p.add_argument('--report-labels', type=int, default=1, choices=(0, 1), help="0: label-free report (k, winning value, margin only)")
    p.add_argument('--cut-sweep', type=parse_cut_sweep, default=None, metavar='RULE:LO:HI:N',
                   help="after training (or with --epochs 0 --ft 1 --model-path CKPT) rank 0 evaluates N thresholds from LO to HI of a "
                        "cut rule on the train and test lists in one pass each: quantile (the smallest cut whose predicted mass "
                        "reaches the share tau), above (the first position whose output is >= tau) or score (cut where feature 0 of "
                        "X, the retrieval score, falls below tau; no model; score:auto:N takes N quantiles of the train scores); "
                        "logs the test curve and the test figures at the train-tuned tau* beside the argmax cut's")
    p.add_argument('--sweep-out', type=str, default=None, help="--cut-sweep writes its curves and the tuned figures here (.npz or .json)")
    p.add_argument('--rerank-loss', type=str, default='hinge', choices=('hinge', 'ranknet', 'lambdarank'),
                   help="loss of the rerank head in the multi-task criterion: 'hinge' (the reference's batch-wide hinge between "
                        "the mean irrelevant and the mean relevant score; the default, nothing changes), 'ranknet' (mean pairwise "
                        "logistic loss per list) or 'lambdarank' (pairs weighted by their nDCG swap gain); weighted by "
                        "--rerank-weight.  A model without a rerank head rejects a non-default value")
    p.add_argument('--rerank-sigma', type=float, default=1.0,
                   help="slope of the pairwise logistic loss, x = sigma (s_i - s_j).  Towers that end in a softmax over positions "
                        "(MMOE, PLE) have score gaps near 1/S and want a large sigma (of the order of S)")
    p.add_argument('--rerank-eval', type=str, default=None, choices=('rerank', 'classi'),
                   help="a multi-task model's auxiliary head: every test pass also re-ranks each test list by that head's values "
                        "(stable, descending) and logs F1 / DCG at the model's k and the best-cut figures in both orders (test/..._rr "
                        "scalars, `test_rr` in --history-json); --report-out gains *_rr per-query arrays and rerank_by")
    p.add_argument('--draw', type=int, default=0, choices=(0, 1),
                   help="1: on even epochs, the reward and prediction curves of the reference's figure for every test batch of more "
                        "than 40 lists go to scalars.jsonl (draw/reward, draw/prediction); no image is written")
    p.add_argument('--bicut-stats', type=str, default=None,
                   help="path of the reference's statics/bicut_stats.pkl (dict[doc_id] -> [token count, distinct count, [(term, "
                        "count), ...]]): --model-name bicut then trains on its bag-of-words input, kept sparse, at input width "
                        "(dense columns) + (dictionary size); without it bicut reads the three attncut columns as before")
    p.add_argument('--bicut-vocab', type=int, default=None,
                   help="dictionary size V of --bicut-stats (the reference: 231448); default 1 + the largest term id of the file")
    add_grad_guard_arguments(p)
    add_recipe_arguments(p)
    p.add_argument('--save-state', type=str, default=None,
                   help="rank 0 writes a training checkpoint here after every epoch: model, optimizer state (moments, step count, "
                        "averaged weights, schedule state), epoch, best figures and records")
    p.add_argument('--resume', type=str, default=None,
                   help="continue from a --save-state checkpoint at the epoch after it.  The data permutation and the dropout streams "
                        "are not restored - they restart from --seed + that epoch - so the run is not bit-identical to an "
                        "uninterrupted one; the optimizer state is")
    p.add_argument('--tensorboard-dir', type=str, default=os.path.join(HERE, 'Tensorboard_summary', 'Truncation'),
                   help="scalars.jsonl (+ tensorboard event files when tensorboard is installed); '' disables")
    return p


def apply_conf(args):
    """run.py:338-347: the .conf section of the model overrides the CLI values."""
    conf = configparser.ConfigParser()
    path = os.path.join(HERE, 'hyper_parameter_{}.conf'.format(args.dataset_name))
    sec = '{}_conf'.format(args.model_name)
    if not conf.read(path) or not conf.has_section(sec):
        # the reference dies with configparser.NoSectionError here (run.py:340); running on silently with the CLI
        # defaults would train a different model than the user asked for
        raise configparser.NoSectionError(f"{sec} (in {path}; pass --use-conf 0 to train with the command-line values)")
    args.lr = conf.getfloat(sec, 'lr')
    if args.retrieve_data == 'robust04':
        args.batch_size = conf.getint(sec, 'batch_size')
    args.dropout = conf.getfloat(sec, 'dropout')
    args.weight_decay = conf.getfloat(sec, 'weight_decay')
    if 'm' in args.model_name:
        args.rerank_weight = conf.getfloat(sec, 'rerank_weight')
        args.class_weight = conf.getfloat(sec, 'class_weight')
    return args


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        eval_reward_spec(args)
    except ValueError as e:
        parser.error(str(e))
    if args.stream_eval < 0:
        parser.error("--stream-eval takes a positive page size (0 = off)")
    if args.stream_eval and not (args.model_name == "choopy" and args.attention_axis == "position" and args.attention_mask == "causal"
                                 and args.cut_head == "hazard"):
        parser.error("--stream-eval needs --model-name choopy --attention-axis position --attention-mask causal --cut-head hazard "
                     "(only that model computes rank i from the ranks above it)")
    if args.stream_compact < 0 or not 0.0 <= args.stream_compact_below <= 1.0:
        parser.error("--stream-compact takes a positive number of pages (0 = off), --stream-compact-below a fraction in [0, 1]")
    if args.stream_compact and not args.stream_eval:
        parser.error("--stream-compact needs --stream-eval (it compacts the batch of the streamed test pass)")
    if args.attention_mask == "causal" and args.attention_axis != "position":
        parser.error("--attention-mask causal needs --attention-axis position (the list axis attends across lists, not positions)")
    # RLT_FORCE_DIST=1: initialise the process group (and run the step's collectives) even with one rank - the RCCL
    # rehearsal on a one-GPU box (rlt_hip/parallel.py)
    if (int(os.environ.get("WORLD_SIZE", "1")) > 1 or (FORCE_COLLECTIVES and "RANK" in os.environ)) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("RLT_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    if args.use_conf:
        args = apply_conf(args)
    if args.model_path is None:
        args.model_path = os.path.join(args.save_path, '{}.pkl'.format(args.model_name))
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.synthetic:
        if not args.dataset_base:
            raise SystemExit("--synthetic needs --dataset-base")
        if (not dist.is_initialized()) or dist.get_rank() == 0:
            write_synthetic_robust04(args.dataset_base, args.retrieve_data, args.dataset_name)
        if dist.is_initialized():
            dist.barrier()
    logging.info('{}'.format(vars(args)))
    trainer = Trainer(args)
    result = trainer.run()
    if args.history_json and trainer.rank == 0:
        with open(args.history_json, "w") as f:
            fin = lambda v: v if v is not None and math.isfinite(v) else None     # -inf (no test epoch) is not valid JSON
            json.dump({"history": trainer.history, "best_f1": fin(trainer.best_test_f1), "best_dcg": fin(trainer.best_test_dcg),
                       "best5_f1": fin(trainer.best5_f1), "best5_dcg": fin(trainer.best5_dcg), "best_epoch": trainer.best_epoch,
                       "world": trainer.world, "attention_axis": trainer.attention_axis, **trainer._mask_record(), **getattr(trainer, "stream_results", {}), **({"baselines": trainer.baseline_results} if args.baselines else {}),
                       **({"eval_reward": {"spec": eval_reward_text(eval_reward_spec(args)),
                                           "report": getattr(trainer, "report_results", None),
                                           "cut_sweep": getattr(trainer, "sweep_results", None)}} if eval_reward_spec(args) else {})}, f)
    if args.param_dump_dir:
        import numpy as np
        os.makedirs(args.param_dump_dir, exist_ok=True)
        np.save(os.path.join(args.param_dump_dir, f"flat_param_rank{trainer.rank}.npy"), trainer.flat.flat_param.detach().cpu().numpy())
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    return result


if __name__ == '__main__':
    main()
