"""Independent restatement of BiCut on its sparse bag-of-words input (torch, CPU, float64), for the tests of
rlt_sparse_inproj_fwd / _bwd and models.BiCut(sparse_input=True).

Layer 0's input projection is an EXPLICIT sparse sum - per token row: bias, the dense columns, then one weight column per
nonzero of the document's table row - and everything after it is stock torch: an nn.LSTM that receives those pre-activations
through identity input weights (so that its own layer-0 projection is the identity), nn.Linear, ReLU, softmax, and the
criterion of oracle/losses.py.  Autograd differentiates the sparse sum, so the layer-0 weight gradient is the sum over the
nonzeros too; nothing here densifies the input."""
import numpy as np
import torch
from torch import nn

L0 = ("bilstm.weight_ih_l0", "bilstm.weight_ih_l0_reverse")


def state_dict_for(input_size, seed):
    """The case's weights by the shared recipe (oracle/weights.py), float64, as leaves."""
    from oracle import models as om
    from oracle.weights import fill_state_dict
    m = om.BiCut(input_size=input_size, dropout=0.0)
    fill_state_dict(m, seed)
    return {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}


def layer0_gates(sd, dense, ids, indptr, indices, values):
    """(B, S, 1024) pre-activations [forward 512 | reverse 512] of layer 0: b_ih + b_hh + dense W[:, :Dn]^T + the sparse sum."""
    B, S, Dn = dense.shape
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    n = (indptr[ids + 1] - indptr[ids]).astype(np.int64)
    tok = torch.from_numpy(np.repeat(np.arange(B * S), n))
    j = np.concatenate([np.arange(indptr[d], indptr[d + 1]) for d in ids]) if n.sum() else np.zeros(0, np.int64)
    term = torch.from_numpy(indices[j].astype(np.int64))
    val = torch.from_numpy(values[j].astype(np.float64))
    x = torch.from_numpy(np.asarray(dense, dtype=np.float64)).reshape(B * S, Dn)
    halves = []
    for sfx in ("", "_reverse"):
        W = sd["bilstm.weight_ih_l0" + sfx]
        g = sd["bilstm.bias_ih_l0" + sfx] + sd["bilstm.bias_hh_l0" + sfx] + x @ W[:, :Dn].t()
        g = g.index_add(0, tok, val[:, None] * W[:, Dn + term].t())
        halves.append(g)
    return torch.cat(halves, dim=1).reshape(B, S, 1024)


def forward(sd, dense, ids, indptr, indices, values):
    """(B, S, 2) float64 output of models/Bicut.py:18-21 with dropout 0."""
    gates = layer0_gates(sd, dense, ids, indptr, indices, values)
    lstm = nn.LSTM(input_size=1024, hidden_size=128, num_layers=2, batch_first=True, bidirectional=True).double()
    eye = torch.eye(512, dtype=torch.float64)
    zero = torch.zeros(512, 512, dtype=torch.float64)
    own = {"weight_ih_l0": torch.cat([eye, zero], 1), "weight_ih_l0_reverse": torch.cat([zero, eye], 1),
           "bias_ih_l0": torch.zeros(512, dtype=torch.float64), "bias_ih_l0_reverse": torch.zeros(512, dtype=torch.float64),
           "bias_hh_l0": torch.zeros(512, dtype=torch.float64), "bias_hh_l0_reverse": torch.zeros(512, dtype=torch.float64)}
    params = {k: own[k] if k in own else sd["bilstm." + k] for k, _ in lstm.named_parameters()}
    h, _ = torch.func.functional_call(lstm, params, (gates,))
    h = torch.relu(h @ sd["fc.weight"].t() + sd["fc.bias"])
    z = h @ sd["softmax.1.weight"].t() + sd["softmax.1.bias"]
    return torch.softmax(z, dim=2)


def cut_positions(out):
    """run.py:131-136: the first position whose argmax is class 0, 1-based; S when every position says continue."""
    pred = np.argmax(out, axis=2)
    S = out.shape[1]
    return np.array([S if r.sum() == S else np.argmin(r) + 1 for r in pred], dtype=np.int64)


def run(d, grad_crit="nci"):
    """Fixture arrays -> dict(out0, k_s, loss/{nci,f1}, grads {name: float64 tensor} of `grad_crit`)."""
    from oracle.losses import BiCutLoss
    Dn, V = d["dense"].shape[2], int(d["V"])
    sd = state_dict_for(Dn + V, int(d["seed"]))
    y = torch.from_numpy(d["y"])
    res = {}
    out = forward(sd, d["dense"], d["ids"], d["indptr"], d["indices"], d["values"])
    res["out0"] = out.detach().numpy()
    res["k_s"] = cut_positions(res["out0"])
    for metric in ("nci", "f1"):
        loss = BiCutLoss(metric=metric)(out, y)
        res["loss/" + metric] = float(loss.detach())
        if metric == grad_crit:
            names = list(sd)
            grads = torch.autograd.grad(loss, [sd[k] for k in names], retain_graph=True)
            res["grads"] = dict(zip(names, grads))
    return res
