"""The BiLSTM recurrence of include/rlt_hip.h (rlt_bilstm_rec_fwd / _fwd_x / _bwd) restated in float64, and the rule of
rlt_bilstm_rec_plan restated in Python - both independently of csrc/lstm.hip and csrc/lstm6w.hip.

The recurrence is a plain time loop over torch float64 tensors (any device), in the header's layout:
    gate order i, f, g, o; rows gate * 128 + unit of W_hh (512, 128) and W_ih (512, I)
    gates  (S*B, 2, 512)  position-major, row = s * B + b; direction 0 runs s = 0 .. S-1, direction 1 runs s = S-1 .. 0
    h_out  (S*B, 256) = [forward | reverse];  c (S*B, 2, 128);  h0 = c0 = 0
tests/test_lstm_restate.py pins it to float64 torch.nn.LSTM; tests/test_lstm_dispatch_gpu.py compares every kernel with it."""
import torch

HID = 128
PRECISIONS = ("fp32", "bf16x3", "bf16x6")


# ---------------------------------------------------------------------------------------------------------------- the plan
def _flag(sw, name):
    return True if name not in sw else int(sw[name]) != 0


def plan(B, xin, precision, sw=None):
    """-> dict(fwd, bwd, fwd_lists, bwd_lists), the kernels by their names in native.LSTM_KERNELS.  precision: one of PRECISIONS
    (the process default is bf16x6).  sw: the environment switches of the family as a dict of their string values."""
    sw = sw or {}
    assert xin in (0, 1)            # selects the forward kernel's instantiation, not the kernel
    p = dict(fwd="f32", bwd="f32", fwd_lists=32, bwd_lists=32)
    if precision == "bf16x3":
        p["fwd"] = p["bwd"] = "x3"
    if precision != "bf16x6":
        return p
    # bf16x6: lstm6w.hip's kernels below 2^20 lists (their buffer bounds are 32-bit byte counts), one 16-list half per workgroup
    # up to 16 * 128 lists, two halves beyond
    w6 = ("x6w_single", 16) if _flag(sw, "RLT_LSTM6W_SINGLE") and B <= 16 * 128 else ("x6w_halves", 32)
    small = B < 2 ** 20
    if not _flag(sw, "RLT_LSTM6"):
        pass                                            # forward on the f32 kernel
    elif _flag(sw, "RLT_LSTM6W") and small:
        p["fwd"], p["fwd_lists"] = w6
    else:
        p["fwd"] = "x6"                                 # the two-phase forward; its backward is the f32 kernel
    if _flag(sw, "RLT_LSTM6W") and _flag(sw, "RLT_LSTM6W_BWD") and small:      # (RLT_LSTM6 does not govern the backward)
        p["bwd"], p["bwd_lists"] = w6
    return p


# ---------------------------------------------------------------------------------------------------------- the recurrence
def preactivations(x, w_ih, b_ih, b_hh):
    """x (S*B, I), w_ih / b_ih / b_hh: per direction (512, I) / (512,) / (512,) -> (S*B, 2, 512) float64"""
    x = x.double()
    return torch.stack([x @ w_ih[d].double().T + b_ih[d].double() + b_hh[d].double() for d in (0, 1)], 1)


def _steps(S, d):
    return range(S) if d == 0 else range(S - 1, -1, -1)


def forward(pre, w_hh, S, B):
    """pre (S*B, 2, 512), w_hh: per direction (512, 128) -> activated gates (S*B, 2, 512), c (S*B, 2, 128), h (S*B, 256)"""
    pre = pre.double().reshape(S, B, 2, 4, HID)
    act = torch.empty_like(pre)
    c_out = pre.new_empty(S, B, 2, HID)
    h_out = pre.new_empty(S, B, 2, HID)
    for d in (0, 1):
        w = w_hh[d].double()
        h = pre.new_zeros(B, HID)
        c = pre.new_zeros(B, HID)
        for s in _steps(S, d):
            a = pre[s, :, d] + (h @ w.T).reshape(B, 4, HID)
            i, f, o = torch.sigmoid(a[:, 0]), torch.sigmoid(a[:, 1]), torch.sigmoid(a[:, 3])
            g = torch.tanh(a[:, 2])
            c = f * c + i * g
            h = o * torch.tanh(c)
            act[s, :, d] = torch.stack([i, f, g, o], 1)
            c_out[s, :, d] = c
            h_out[s, :, d] = h
    return act.reshape(S * B, 2, 4 * HID), c_out.reshape(S * B, 2, HID), h_out.reshape(S * B, 2 * HID)


def backward(act, c, w_hh, d_hout, S, B):
    """activated gates, c (the forward's stashes), d_hout (S*B, 256) -> d(pre-activation gates) (S*B, 2, 512)"""
    act = act.double().reshape(S, B, 2, 4, HID)
    c = c.double().reshape(S, B, 2, HID)
    d_hout = d_hout.double().reshape(S, B, 2, HID)
    dpre = torch.empty_like(act)
    for d in (0, 1):
        w = w_hh[d].double()
        order = list(_steps(S, d))
        dh = act.new_zeros(B, HID)          # what the later step hands back through W_hh
        dc = act.new_zeros(B, HID)          # ... and through its forget gate
        for t in range(S - 1, -1, -1):
            s = order[t]
            i, f, g, o = (act[s, :, d, k] for k in range(4))
            c_prev = c[order[t - 1], :, d] if t > 0 else torch.zeros_like(dc)
            tc = torch.tanh(c[s, :, d])
            dh = dh + d_hout[s, :, d]
            dc = dc + dh * o * (1 - tc * tc)
            da = torch.stack([dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], 1)
            dpre[s, :, d] = da
            dh = da.reshape(B, 4 * HID) @ w
            dc = dc * f
    return dpre.reshape(S * B, 2, 4 * HID)
