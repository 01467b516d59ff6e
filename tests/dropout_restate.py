"""Numpy integer restatement of the counter-based dropout generator (csrc/common.h: rlt_mix32 .. rlt_keep; csrc/attention_common.h:
pair_seed) and of the masks the library exports (csrc/attention.hip: rlt_dropout_mask, rlt_attention_dropout_mask[_range]).
uint32 arithmetic is carried in uint64 and masked; every argument broadcasts.  tests/test_dropout_restate.py pins it to values
printed by the C functions themselves and to the statistics of independent draws; tests/test_dropout_gpu.py builds every float64
reference of a train-mode kernel from these masks, never from the library's own."""
import numpy as np

from compare_restate import MASK, _u, mix32, row_hash          # one copy of the mixer and the row hash for all restatements

__all__ = ["mix32", "row_hash", "col_hash", "drop_threshold", "keep_rc", "keep", "pair_seed", "keep_bits", "keep_scale", "mask", "attention_mask"]


def col_hash(seed, col):
    """rlt_col_hash: mix32((seed ^ 0x85EBCA6B) + mix32(col + 0x7F4A7C15)) | 1"""
    return mix32(((_u(seed) ^ np.uint64(0x85EBCA6B)) + mix32((_u(col) + np.uint64(0x7F4A7C15)) & MASK)) & MASK) | np.uint64(1)


def drop_threshold(p):
    """rlt_drop_threshold: the float32 p widened to double, times 2^32 (exact: a power of two), truncated; 0xFFFFFFFF from
    4294967295.0 on."""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def keep_rc(rh, ch, thr):
    """rlt_keep_rc: row_hash * col_hash (mod 2^32) >= thr"""
    return ((_u(rh) * _u(ch)) & MASK) >= np.uint64(thr)


def keep(seed, row, col, thr):
    return keep_rc(row_hash(seed, row), col_hash(seed, col), thr)


def pair_seed(seed, pair):
    """pair_seed: mix32(seed ^ (pair * 0x9E3779B9)) - the stream of one (position, head) pair"""
    return mix32(_u(seed) ^ ((_u(pair) * np.uint64(0x9E3779B9)) & MASK))


def keep_bits(seed, rows, cols, p):
    """(rows, cols) bool: keep(seed, r, c) at the threshold of p"""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    return keep(seed, r, c, drop_threshold(p))


def keep_scale(p):
    """1.f / (1.f - p) as the exporter rounds it: fp32 subtraction and fp32 division of fp32 operands"""
    p = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p)


def mask(seed, rows, cols, p):
    """rlt_dropout_mask: (rows, cols) float32, keep ? 1 / (1 - p) : 0"""
    return np.where(keep_bits(seed, rows, cols, p), keep_scale(p), np.float32(0.0)).astype(np.float32)


def attention_mask(seed, S, B, H, p, pair0=0, npair=None):
    """rlt_attention_dropout_mask (pair0 = 0, npair = S * H) / _range: (npair, B, B) float32 over (pair, query, key); pair =
    position * H + head draws from pair_seed(seed, pair)"""
    npair = S * H - pair0 if npair is None else npair
    out = np.empty((npair, B, B), dtype=np.float32)
    for i in range(npair):
        out[i] = mask(int(pair_seed(seed, pair0 + i)), B, B, p)
    return out
