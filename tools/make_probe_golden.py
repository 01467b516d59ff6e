#!/usr/bin/env python3
"""Generate tests/golden/probe_*.npz by RUNNING THE REFERENCE'S own probing-study modules on the CPU.

CPU only; run in the build container, where the reference is mounted read-only (RLT_REFERENCE, default /root/reference).
Its models/Classification.py (TaskC), models/Rerank.py (TaskR), models/Probe.py (ProbeBase, Probe) and utils/losses.py
(RerankLoss) are imported at run time; nothing from the reference is written into this repository: the fixtures hold seeds,
shapes, key lists and what those modules returned (data).  Features, labels and weights are not stored: the features and
labels come from tests/probe_restate.py's probe_data(seed, ...), the weights from oracle/weights.py's
fill_state_dict(model, seed).

    python tools/make_probe_golden.py        # regenerates every tests/golden/probe_*.npz

probe_heads_s40.npz / probe_heads_s300.npz, per case tag (c|r)_e<E>: <tag>/seed, <tag>/shape (B, S, E), <tag>/out (B,S),
<tag>/loss, <tag>/dw (E), <tag>/db - TaskC with nn.BCELoss() / TaskR with RerankLoss(), one forward and backward.
The s40 file also holds adam_<tag>/w (5,E), adam_<tag>/b (5,), adam_<tag>/loss (5,): the probe's weights after each of five
torch.optim.Adam(lr=1e-3) steps on the same batch (the losses before each step), adam/lr.
probe_models_s40.npz: keys/<Class> and shapes/<Class> (state_dict of TaskC(), TaskR(), ProbeBase(seq_len=40), Probe());
pb/seed, pb/shape; the ProbeBase(seq_len=40, dropout=0) outputs as pb/<name>/norm plus pb/<name>/idx, pb/<name>/val
(probed elements) for experts_in, expert0, expert1, tower0..2.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("RLT_REFERENCE", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle.weights import fill_state_dict, synthetic_lists  # noqa: E402
import probe_restate as R  # noqa: E402
from golden_util import probe_index  # noqa: E402

HEAD_CASES = {40: (16, [3, 256]), 300: (8, [3, 256])}
ADAM_STEPS, ADAM_LR = 5, 1e-3


def ref_module(rel):
    spec = importlib.util.spec_from_file_location("reference_" + rel.replace("/", "_")[:-3], os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def head_case(cls, crit, kind, B, S, E, seed):
    model = cls(d_model=E)
    fill_state_dict(model, seed)
    x, y = R.probe_data(seed + 1, B, S, E)
    out = model(torch.from_numpy(x))
    loss = crit(out.squeeze(2) if kind == "c" else out, torch.from_numpy(y))     # nn.BCELoss wants (B,S) like the labels
    loss = loss if torch.is_tensor(loss) else torch.tensor(loss)
    loss.backward()
    lin = next(m for m in model.modules() if isinstance(m, torch.nn.Linear))
    return model, x, y, {"seed": np.int64(seed), "shape": np.array([B, S, E]), "out": out.detach().squeeze(2).numpy(),
                         "loss": np.float32(loss.item()), "dw": lin.weight.grad.reshape(-1).numpy().copy(),
                         "db": lin.bias.grad.reshape(-1).numpy().copy()}


def main():
    C, Rr, P = (ref_module(p) for p in ("models/Classification.py", "models/Rerank.py", "models/Probe.py"))
    # utils/losses.py imports its package's metrics relatively; utils/metrics.py:3 imports numpy.lib.financial (unused,
    # dropped by modern numpy): an empty stand-in, as tools/make_golden.py does
    sys.modules.setdefault("numpy.lib.financial", types.ModuleType("numpy.lib.financial")).irr = None
    sys.path.insert(0, REF)
    L = importlib.import_module("utils.losses")
    sys.path.remove(REF)
    kinds = {"c": (C.TaskC, lambda: torch.nn.BCELoss()), "r": (Rr.TaskR, lambda: L.RerankLoss())}
    for S, (B, Es) in HEAD_CASES.items():
        rec = {}
        for E in Es:
            for k, (cls, crit) in kinds.items():
                tag = f"{k}_e{E}"
                seed = 1000 + S + E + (0 if k == "c" else 7)
                _, x, y, r = head_case(cls, crit(), k, B, S, E, seed)
                for n, v in r.items():
                    rec[f"{tag}/{n}"] = v
                if S == 40:          # five Adam steps of the same probe on the same batch
                    model = cls(d_model=E)
                    fill_state_dict(model, seed)
                    opt = torch.optim.Adam(model.parameters(), lr=ADAM_LR)
                    lin = next(m for m in model.modules() if isinstance(m, torch.nn.Linear))
                    ws, bs, ls = [], [], []
                    for _ in range(ADAM_STEPS):
                        opt.zero_grad()
                        out = model(torch.from_numpy(x))
                        loss = crit()(out.squeeze(2) if k == "c" else out, torch.from_numpy(y))
                        loss = loss if torch.is_tensor(loss) else torch.tensor(loss)
                        loss.backward()
                        opt.step()
                        ls.append(loss.item())
                        ws.append(lin.weight.detach().reshape(-1).numpy().copy())
                        bs.append(float(lin.bias.detach()[0]))
                    rec[f"adam_{tag}/w"] = np.array(ws, np.float32)
                    rec[f"adam_{tag}/b"] = np.array(bs, np.float32)
                    rec[f"adam_{tag}/loss"] = np.array(ls, np.float32)
        if S == 40:
            rec["adam/lr"] = np.float32(ADAM_LR)
        np.savez_compressed(os.path.join(OUT, f"probe_heads_s{S}.npz"), **rec)

    rec = {}
    for name, ctor in (("TaskC", lambda: C.TaskC()), ("TaskR", lambda: Rr.TaskR()),
                       ("ProbeBase", lambda: P.ProbeBase(seq_len=40)), ("Probe", lambda: P.Probe())):
        sd = ctor().state_dict()
        rec[f"keys/{name}"] = np.array(list(sd.keys()))
        rec[f"shapes/{name}"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    seed, B, S = 4040, 6, 40
    torch.manual_seed(0)
    pb = P.ProbeBase(seq_len=40, dropout=0.0).eval()
    fill_state_dict(pb, seed)
    x, _ = synthetic_lists(B, S, 3, seed + 1)
    with torch.no_grad():
        experts_in, experts_o, towers = pb(x)
    rec["pb/seed"], rec["pb/shape"] = np.int64(seed), np.array([B, S, 3])
    for name, t in [("experts_in", experts_in), ("expert0", experts_o[0]), ("expert1", experts_o[1])] + \
            [(f"tower{i}", t) for i, t in enumerate(towers)]:
        a = t.numpy().reshape(-1)
        idx = probe_index(a.size, "pb/" + name)
        rec[f"pb/{name}/norm"] = np.float64(np.linalg.norm(a.astype(np.float64)))
        rec[f"pb/{name}/idx"] = idx
        rec[f"pb/{name}/val"] = a[idx]
    np.savez_compressed(os.path.join(OUT, "probe_models_s40.npz"), **rec)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("probe_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
