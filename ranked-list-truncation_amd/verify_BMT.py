#!/usr/bin/env python3
"""Probing a cut model's representation on the HIP hot path - the mirror of the reference's verify_BMT.py.

A probe (TaskC: Linear -> Sigmoid -> nn.BCELoss, or TaskR: Linear -> Softmax over positions -> RerankLoss) is trained on
frozen features: the raw inputs (--ft 0) or the representation of a trained cut model (--ft 1, a checkpoint written by
`run.py --model-persist 1`):
  AttnCut  attention_layer(encoding_layer(X)), E = 256;
  Choopy   attention_layer(cat(X, PE)),        E = 128.
Each step is one fused probe pass (rlt_probe_heads: activations, loss and weight gradients from one read of the features),
one FusedAdam step and the metric on the device (ROC AUC per list for c, DCG of the re-ranked list for r: utils/metrics.py
taskc_metric / taskr_metric).  Per epoch the train and test means of loss and metric go to the reference's log lines; at the
end the list of train metrics is printed (verify_BMT.py:145) and written into --history-json.

Decisions where the reference is broken or silent:
  * `from utils import Metric` fails in the reference (its utils/__init__.py is empty); here the device metrics are used.
  * The reference never calls eval() on the cut model, so the trunk's dropout is active while the features are drawn.  That
    stays the default; --trunk-eval 1 draws them in eval mode.
  * Inputs are always (B,S): the reference's `.squeeze()` would also drop the batch axis at B = 1.
Additions: --dataset-base, --synthetic, --seed, --history-json, --tensorboard-dir, --trunk-eval.
"""
import argparse
import json
import logging
import math
import os
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

import run  # noqa: E402  (the loaders, ScalarLog and the synthetic set)
from models import AttnCut, Choopy, TaskC, TaskR  # noqa: E402
from models import _common as C  # noqa: E402
from rlt_hip import ops  # noqa: E402
from rlt_hip.parallel import FlatModel, FusedAdam  # noqa: E402
from utils.metrics import Metric  # noqa: E402


class Trainer:
    def __init__(self, args):
        if not torch.cuda.is_available():
            raise RuntimeError("verify_BMT.py trains on the GPU through librlt_hip.so; there is no CPU fallback")
        self.args = args
        self.device = torch.device("cuda", 0)
        self.verify_type, self.model_name, self.ft = args.verify_type, args.model_name, args.ft
        if self.verify_type not in ("c", "r"):
            raise ValueError("--verify-type must be c (classification) or r (rerank)")
        self.metric_name = 'auc' if self.verify_type == 'c' else 'DCG'
        self.metric = []
        self.history = []
        if self.model_name == 'choopy':
            loader = run.cp_dataloader
        elif self.model_name == 'attncut':
            loader = run.at_dataloader
        else:
            raise ValueError("--model-name must be attncut or choopy")
        self.train_loader, self.test_loader, data = loader(args.retrieve_data, args.dataset_name, args.batch_size,
                                                           device=self.device, base=args.dataset_base, seed=args.seed)
        feat = data.n_features
        if self.model_name == 'choopy':
            if len(data.lengths) != 1 or data.test_lengths != data.lengths:
                raise ValueError("choopy is built for ONE list length")
            self.seq_len = data.lengths[0]
            self.cut_model = Choopy(seq_len=self.seq_len, dropout=args.dropout)
            width = 128
        else:
            self.cut_model = AttnCut(input_size=feat, dropout=args.dropout)
            width = 256
        self.cut_model = self.cut_model.to(self.device)
        if self.ft:
            self.load_model()
        if args.trunk_eval:
            self.cut_model.eval()
        E = width if self.ft else feat
        self.model = (TaskC if self.verify_type == 'c' else TaskR)(d_model=E).to(self.device)
        self.flat = FlatModel(self.model)
        self.optimizer = FusedAdam(self.flat, lr=args.lr, weight_decay=args.weight_decay, **run.grad_guard_kwargs(args),
                                   **run.recipe_kwargs(args, self.flat.names, max(1, args.epochs * len(self.train_loader))))
        self.writer = run.ScalarLog(args.tensorboard_dir)

    def features(self, X):
        """Frozen position-major features (S*B, E) of a batch X (B,S,F)."""
        B, S, _ = X.shape
        with torch.no_grad():
            if not self.ft:
                return ops.to_position_major(C.check_input(X))
            m = self.cut_model
            drop_p = C.check_dropout(m, m.dropout)
            if self.model_name == 'attncut':
                h = C.bilstm(ops.to_position_major(C.check_input(X)), m.encoding_layer, S, B)
            else:
                h = ops.choopy_embed(C.check_input(X), m.position_encoding)
            return C.encoder(h, m.attention_layer, m.n_head, S, B, drop_p)

    def _metric(self, y, out):
        return Metric.taskc_metric(y, out) if self.verify_type == 'c' else Metric.taskr_metric(y, out)

    def _epoch(self, loader, train):
        tot_loss, tot_metric, step = 0.0, 0.0, 0
        for X, y in loader:
            B, S = y.shape
            x_pm = self.features(X)
            if train:
                self.model.train()
                self.optimizer.zero_grad()
                loss, outs = self.model.loss(x_pm, y, S, B)
                loss.sum().backward()
                self.optimizer.step()
            else:
                self.model.eval()
                with torch.no_grad():
                    loss, outs = self.model.loss(x_pm, y, S, B)
            tot_metric += self._metric(y, outs[0].detach().squeeze(2))
            tot_loss += float(loss[0])
            step += 1
        return tot_loss / step, tot_metric / step

    def train_epoch(self, epoch):
        start = time.time()
        logging.info('-' * 100)
        loss, metric = self._epoch(self.train_loader, True)
        self.metric.append(metric)
        self.writer.add_scalar('train/loss_epoch', loss, epoch)
        self.writer.add_scalar('train/{}_epoch'.format(self.metric_name), metric, epoch)
        self.history.append({"epoch": epoch, "train": (loss, metric)})
        grad = run.log_grad_guard(self.writer, self.optimizer, epoch)
        if grad is not None:
            self.history[-1]["grad"] = grad
        logging.info('\nEpoch: {} | Epoch Time: {:.2f} s'.format(epoch, time.time() - start))
        logging.info('\tTrain: loss = {} | {} = {:.6f}\n'.format(loss, self.metric_name, metric))

    def test(self, epoch):
        loss, metric = self._epoch(self.test_loader, False)
        self.writer.add_scalar('test/loss_epoch', loss, epoch)
        self.writer.add_scalar('test/{}_epoch'.format(self.metric_name), metric, epoch)
        self.history[-1]["test"] = (loss, metric)
        logging.info('\tTest: loss = {} | {} = {:.6f}\n'.format(loss, self.metric_name, metric))

    def load_model(self):
        self.cut_model.load_state_dict(torch.load(self.args.model_path, map_location=self.device))
        logging.info('The best model has beed loaded from {}\n'.format(self.args.model_path))

    def run(self):
        for epoch in range(self.args.epochs):
            self.train_epoch(epoch)
            self.test(epoch)
        print(self.metric)
        self.writer.close()
        return self.metric


def build_parser():
    p = argparse.ArgumentParser(description="Verification Trainer Args (HIP hot path)")
    p.add_argument('--retrieve-data', type=str, default='robust04')
    p.add_argument('--dataset-name', type=str, default='drmm_tks')
    p.add_argument('--batch-size', type=int, default=20)
    p.add_argument('--num-workers', type=int, default=8, help="accepted for the reference's command lines; unused")
    p.add_argument('--model-name', type=str, default='attncut')
    p.add_argument('--verify-type', type=str, default='r')  # c: classification, r: rerank
    p.add_argument('--model-path', type=str, default=None)
    p.add_argument('--save-path', type=str, default=os.path.join(HERE, 'best_model'))
    p.add_argument('--ft', type=int, default=0)
    p.add_argument('--epochs', type=int, default=100)
    p.add_argument('--lr', type=float, default=3e-5)
    p.add_argument('--weight-decay', type=float, default=0.0015)
    p.add_argument('--dropout', type=float, default=0.1)
    # additions
    p.add_argument('--trunk-eval', type=int, default=0, choices=(0, 1),
                   help="1: draw the features with the cut model in eval mode (the reference leaves its dropout active)")
    p.add_argument('--dataset-base', type=str, default=None, help="directory holding <retrieve_data>/*.pkl")
    p.add_argument('--synthetic', type=int, default=0, help="write a robust04-shaped synthetic set into --dataset-base first")
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--history-json', type=str, default=None, help="per-epoch train / test means and the train metric list")
    run.add_grad_guard_arguments(p)
    run.add_recipe_arguments(p, ema_eval=False)
    p.add_argument('--tensorboard-dir', type=str, default=os.path.join(HERE, 'Tensorboard_summary', 'Verify'),
                   help="scalars.jsonl (+ tensorboard event files when tensorboard is installed); '' disables")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
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
    metrics = trainer.run()
    if args.history_json:
        fin = lambda v: v if math.isfinite(v) else None     # noqa: E731  (nan is not valid JSON)
        with open(args.history_json, "w") as f:
            json.dump({"metric_name": trainer.metric_name, "train_metrics": [fin(v) for v in metrics],
                       "history": [{"epoch": h["epoch"], "train": [fin(v) for v in h["train"]],
                                    "test": [fin(v) for v in h["test"]]} for h in trainer.history]}, f)
    return metrics


if __name__ == '__main__':
    main()
