"""BiCut on the HIP hot path - drop-in for the reference's models/Bicut.py:5-21:
BiLSTM (2 layers, 128 hidden) -> Linear(256, fc) -> ReLU -> Linear(fc, 2) -> Dropout -> softmax over the two classes
{0: truncate, 1: continue} at every position.  Same constructor, state_dict keys and (B,S,2) output.

`sparse_input=True` is the model at the width the reference declares it for (input_size=231449, models/Bicut.py:6) but could
not afford to feed (run.py:61-63 comments its loader out): the input is an `ops.SparseBatch` - `Dn` dense columns and one row
of a device-resident bag-of-words table per ranked document (dataloader/bicut_data.py) - and the two layer-0 input weights
are stored column-major, shape (512, input_size) with strides (1, 512), so that one nonzero reads and one gradient column
writes contiguous memory.  state_dict keys and shapes stay the reference's; load_state_dict copies whatever the source
strides are."""
import torch
from torch import nn

from rlt_hip import ops
from . import _common as C


class BiCut(C.CutModel):
    def __init__(self, input_size=231449, lstm_hiden_size=128, lstm_layers=2, fc_dimensions=256, dropout=0.4, sparse_input=False):
        super().__init__()
        if lstm_hiden_size != 128 or lstm_layers != 2:
            raise ValueError("the HIP BiLSTM kernel is specialised for 2 layers of hidden size 128 (the reference's defaults)")
        self.dropout = dropout
        self.bilstm = C.bilstm_params(input_size, lstm_hiden_size)
        self.sparse_input = bool(sparse_input)
        if self.sparse_input:
            for name in ("weight_ih_l0", "weight_ih_l0_reverse"):           # same values, column-major memory
                p = getattr(self.bilstm, name)
                p.data = p.data.t().contiguous().t()
        self.fc = C.ParamTree(nn.Linear(in_features=lstm_hiden_size * 2, out_features=fc_dimensions))
        self.softmax = C.ParamTree(nn.Sequential(nn.ReLU(), nn.Linear(in_features=fc_dimensions, out_features=2),
                                                 nn.Dropout(dropout), nn.Softmax(dim=2)))

    def forward(self, x):
        if self.sparse_input != isinstance(x, ops.SparseBatch):
            if self.sparse_input:
                raise TypeError("this BiCut was built with sparse_input=True: it expects an ops.SparseBatch (dense columns, table rows, "
                                f"table), got {'a dense tensor' if torch.is_tensor(x) else type(x).__name__}")
            raise TypeError("this BiCut was built with sparse_input=False: it expects a dense (B, S, input_size) tensor, got an "
                            "ops.SparseBatch")
        drop_p = C.check_dropout(self, self.dropout)
        if self.sparse_input:
            B, S = x.ids.shape
            h = ops.bilstm_sparse(x, self.bilstm, S, B)                                   # (S*B, 256)
        else:
            x = C.check_input(x)
            B, S, _ = x.shape
            h = C.bilstm(ops.to_position_major(x), self.bilstm, S, B)                     # (S*B, 256)
        h = ops.linear(h, self.fc.weight, self.fc.bias, relu=True)                        # fc + the Sequential's ReLU
        head = getattr(self.softmax, "1")
        z = ops.linear(h, head.weight, head.bias)                                         # (S*B, 2)
        return ops.pair_softmax(z, S, B, drop_p)                                          # (B, S, 2)
