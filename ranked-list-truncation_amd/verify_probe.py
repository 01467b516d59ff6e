#!/usr/bin/env python3
"""The MMOE probing study on the HIP hot path - the mirror of the reference's verify_probe.py.

ProbeBase (MMOECut with its intermediates returned) is trained with MtCutLoss for --epochs-base (--ft 0: run.py's own
Trainer step, epoch, test, best-F1 checkpoint and best-5 lines) or loaded from --model-path (--ft 1).  Then six probes train
for --epochs-probe on its frozen features: c1 / r1 on the BiLSTM output (experts_in), ce1 / re1 on expert 0, ce2 / re2 on
expert 1.  That is one fused rlt_probe_heads pass per feature tensor - three per step - and one FusedAdam step over all six
probes.  The six metrics (ROC AUC for the classification probes, DCG of the re-ranked list for the rerank probes) go under
the reference's probe/... tags, with a step counter that counts (the reference never increments it), and their epoch means
into --history-json.

Decisions where the reference is broken or silent:
  * `self.model.cuda()` (verify_probe.py:86) names a model that does not exist; here everything runs on the GPU.
  * The conf section [probe_base_conf] is read only if it exists (no hyper_parameter_*.conf has one); otherwise the CLI
    defaults apply.
  * The probe gradients are zeroed every step.  The reference never zeroes its six optimizers, so its gradients accumulate
    over the whole run; --accumulate-grads 1 reproduces that exactly.
  * One FusedAdam over the six probes is the reference's six Adam optimizers: Adam works element by element and all six
    share lr and weight decay.
  * Only --num-tasks 3 is accepted for training the base: with 2.1 or 2.2 the reference hands the rerank tower's output to
    MtCutLoss as the cut.
  * The base draws the probes' features in eval mode.  The reference's mode depends on the run: test_base leaves the model
    in eval after --ft 0 training, while a model loaded with --ft 1 stays in train mode with its dropout active.
  * Inputs are always (B,S): the reference's `.squeeze()` would also drop the batch axis at B = 1.
Additions: --dataset-base, --synthetic, --seed, --history-json, --tensorboard-dir, --accumulate-grads.
"""
import argparse
import configparser
import json
import logging
import math
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

import run  # noqa: E402  (loaders, ScalarLog, Trainer)
from models import MMOECut, Probe, ProbeBase  # noqa: E402
from rlt_hip.parallel import FlatModel, FusedAdam  # noqa: E402
from utils import losses  # noqa: E402
from utils.metrics import Metric  # noqa: E402

# probe name -> (the reference's tag, classification probe?)
TAGS = {"c1": ("probe/pre_encoding_classification", True), "r1": ("probe/pre_encoding_rerank", False),
        "ce1": ("probe/expert0_classification", True), "re1": ("probe/expert0_rerank", False),
        "ce2": ("probe/expert1_classification", True), "re2": ("probe/expert1_rerank", False)}


class _ProbeBaseCut(ProbeBase):
    """ProbeBase seen as a cut model by run.py's Trainer: forward gives the towers only (MMOECut.forward); the state_dict is
    ProbeBase's."""
    forward = MMOECut.forward


def base_trainer(args, model, loaders, device):
    """run.py's Trainer around ProbeBase: its _step / train_epoch / test / save_model / run, not a second training loop."""
    t = run.Trainer.__new__(run.Trainer)
    t.args, t.device, t.rank, t.world = args, device, 0, 1
    t.model_name, t.epochs, t.batch_size = args.model_name, args.epochs_base, args.batch_size
    t.model_persist, t.save_path, t.model_path = 1, args.save_path, args.model_path
    t.best_test_f1, t.best_test_dcg, t.best_epoch = -float('inf'), -float('inf'), None
    t.best5_f1 = t.best5_dcg = None
    t.f1_record, t.dcg_record, t.history, t.baseline_results = [], [], [], None
    t.train_loader, t.test_loader = loaders
    t.model = model
    t.criterion = losses.MtCutLoss(metric=args.criterion, num_tasks=args.num_tasks)
    t.multi_task = True
    t.flat = FlatModel(model)
    t.optimizer = FusedAdam(t.flat, lr=args.lr, weight_decay=args.weight_decay, **run.grad_guard_kwargs(args),
                            **run.recipe_kwargs(args, t.flat.names, max(1, args.epochs_base * len(t.train_loader))))
    t.writer = run.ScalarLog(os.path.join(args.tensorboard_dir, 'base') if args.tensorboard_dir else None)
    return t


class Trainer:
    def __init__(self, args):
        if not torch.cuda.is_available():
            raise RuntimeError("verify_probe.py trains on the GPU through librlt_hip.so; there is no CPU fallback")
        self.args = args
        self.device = torch.device("cuda", 0)
        loader = run.at_dataloader if args.retrieve_data == 'robust04' else run.mc_dataloader
        self.train_loader, self.test_loader, data = loader(args.retrieve_data, args.dataset_name, args.batch_size,
                                                           device=self.device, base=args.dataset_base, seed=args.seed)
        if len(data.lengths) != 1 or data.test_lengths != data.lengths:
            raise ValueError("ProbeBase is built for ONE list length (its gates are sized by it)")
        self.seq_len = data.lengths[0]
        if not args.ft and args.num_tasks != 3:
            raise ValueError("--num-tasks {} with --ft 0: the reference would train MtCutLoss on the rerank tower's output as "
                             "the cut; only --num-tasks 3 trains the base".format(args.num_tasks))
        self.model_base = _ProbeBaseCut(seq_len=self.seq_len, num_tasks=args.num_tasks, input_size=data.n_features,
                                        dropout=args.dropout, num_experts=2).to(self.device)
        self.probe = Probe().to(self.device)
        self.flat = FlatModel(self.probe)
        self.optimizer = FusedAdam(self.flat, lr=args.lr, weight_decay=args.weight_decay, **run.grad_guard_kwargs(args),
                                   **run.recipe_kwargs(args, self.flat.names, max(1, args.epochs_probe * len(self.train_loader))))
        self.writer = run.ScalarLog(args.tensorboard_dir)
        self.base_history, self.history = None, []
        self.step = 0

    def load_model(self):
        self.model_base.load_state_dict(torch.load(self.args.model_path, map_location=self.device))
        logging.info('The best model has beed loaded from {}\n'.format(self.args.model_path))

    def train_probe(self, epoch):
        logging.info('-' * 100)
        self.model_base.eval()
        tot, n = {k: 0.0 for k in TAGS}, 0
        for X, y in self.train_loader:
            B, S = y.shape
            with torch.no_grad():
                h, experts, _ = self.model_base.forward_pm(X)
            if not self.args.accumulate_grads:
                self.optimizer.zero_grad()
            res = self.probe.losses([h, experts[0], experts[1]], y, S, B)
            torch.stack([loss for loss, _ in res.values()]).sum().backward()   # each probe's own loss reaches only it
            self.optimizer.step()
            for name, (_, out) in res.items():
                tag, cls = TAGS[name]
                p = out.detach().squeeze(2)
                v = Metric.taskc_metric(y, p) if cls else Metric.taskr_metric(y, p)
                self.writer.add_scalar(tag, v, self.step)
                tot[name] += v
            self.step += 1
            n += 1
        means = {name: tot[name] / n for name in TAGS}
        self.history.append({"epoch": epoch, **means})
        grad = run.log_grad_guard(self.writer, self.optimizer, epoch)
        if grad is not None:
            self.history[-1]["grad"] = grad
        logging.info('\tProbe epoch {}: '.format(epoch) + ' | '.join('{} = {:.6f}'.format(k, v) for k, v in means.items()))

    def run(self):
        a = self.args
        if a.ft:
            self.load_model()
        else:
            logging.info('\nTrain the Base model: \n')
            bt = base_trainer(a, self.model_base, (self.train_loader, self.test_loader), self.device)
            bt.run()                                   # train / test per epoch, checkpoint on the best test F1, best-5 lines
            self.base_history = bt.history
        self.model_base.eval()                         # features in eval mode (see the module docstring)
        for epoch in range(a.epochs_probe):
            self.train_probe(epoch)
        self.writer.close()
        return self.history


def build_parser():
    p = argparse.ArgumentParser(description="Probe Trainer Args (HIP hot path)")
    p.add_argument('--retrieve-data', type=str, default='robust04')
    p.add_argument('--dataset-name', type=str, default='drmm_tks')
    p.add_argument('--batch-size', type=int, default=20)
    p.add_argument('--num-workers', type=int, default=8, help="accepted for the reference's command lines; unused")
    p.add_argument('--model-name', type=str, default='probe_base')
    p.add_argument('--criterion', type=str, default='f1')
    p.add_argument('--model-path', type=str, default=None)
    p.add_argument('--ft', type=int, default=1)
    p.add_argument('--save-path', type=str, default=os.path.join(HERE, 'best_model'))
    p.add_argument('--epochs-base', type=int, default=20)
    p.add_argument('--epochs-probe', type=int, default=180)
    p.add_argument('--lr', type=float, default=1e-5)
    p.add_argument('--weight-decay', type=float, default=0.005)
    p.add_argument('--dropout', type=float, default=0.1)
    p.add_argument('--parameter-record', type=str, default=None, help="accepted for the reference's command lines; unused")
    p.add_argument('--parameter-search', type=int, default=0, help="accepted; the hyper-parameter search is not carried over")
    p.add_argument('--regularizer-search', type=int, default=0, help="accepted; not carried over")
    p.add_argument('--mt-search', type=int, default=0, help="accepted; not carried over")
    p.add_argument('--search-times', type=int, default=80, help="accepted; not carried over")
    p.add_argument('--num-tasks', type=float, default=3)  # 2.1: classification + truncation | 2.2: rerank + truncation
    p.add_argument('--rerank-weight', type=float, default=0.5)
    p.add_argument('--class-weight', type=float, default=0.8)
    # additions
    p.add_argument('--accumulate-grads', type=int, default=0, choices=(0, 1),
                   help="1: never zero the probes' gradients, as the reference does")
    p.add_argument('--dataset-base', type=str, default=None, help="directory holding <retrieve_data>/*.pkl")
    p.add_argument('--synthetic', type=int, default=0, help="write a robust04-shaped synthetic set into --dataset-base first")
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--history-json', type=str, default=None, help="the base's per-epoch history and the probes' epoch means")
    run.add_grad_guard_arguments(p)
    run.add_recipe_arguments(p, ema_eval=False)
    p.add_argument('--tensorboard-dir', type=str, default=os.path.join(HERE, 'Tensorboard_summary', 'Probe'),
                   help="scalars.jsonl (+ tensorboard event files when tensorboard is installed); '' disables")
    return p


def apply_conf(args):
    """verify_probe.py:300-307, but only if the section exists."""
    conf = configparser.ConfigParser()
    sec = '{}_conf'.format(args.model_name)
    if conf.read(os.path.join(HERE, 'hyper_parameter_{}.conf'.format(args.dataset_name))) and conf.has_section(sec):
        args.lr = conf.getfloat(sec, 'lr')
        if args.retrieve_data == 'robust04':
            args.batch_size = conf.getint(sec, 'batch_size')
        args.dropout = conf.getfloat(sec, 'dropout')
        args.weight_decay = conf.getfloat(sec, 'weight_decay')
        args.rerank_weight = conf.getfloat(sec, 'rerank_weight')
        args.class_weight = conf.getfloat(sec, 'class_weight')
        logging.info('hyper-parameters read from [{}]'.format(sec))
    return args


def main(argv=None):
    args = apply_conf(build_parser().parse_args(argv))
    args.baselines = 0                                # run.Trainer.run reads it
    if args.model_path is None:
        args.model_path = os.path.join(args.save_path, '{}.pkl'.format(args.model_name))
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.synthetic:
        if not args.dataset_base:
            raise SystemExit("--synthetic needs --dataset-base")
        run.write_synthetic_robust04(args.dataset_base, args.retrieve_data, args.dataset_name)
    logging.info('{}'.format(vars(args)))
    trainer = Trainer(args)
    hist = trainer.run()
    if args.history_json:
        fin = lambda v: v if v is not None and math.isfinite(v) else None     # noqa: E731
        with open(args.history_json, "w") as f:
            json.dump({"base": trainer.base_history, "tags": {k: v[0] for k, v in TAGS.items()},
                       "probe": [{k: (fin(v) if k != "epoch" else v) for k, v in h.items()} for h in hist]}, f)
    return hist


if __name__ == '__main__':
    main()
