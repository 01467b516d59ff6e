"""Pins tests/dropout_restate.py - the numpy restatement of the dropout keep-stream that tests/test_dropout_gpu.py builds its
float64 references from - to things that do not depend on it: a table printed by the C functions of csrc/common.h themselves, the
statistics of independent Bernoulli draws at the size the header names, and the properties `ops.next_seed` promises.  No GPU.

C_VALUES was printed by tools/dropout_table.cpp, a stand-alone host program compiled from csrc/common.h with RLT_HOST_ONLY
(`hipcc -O1 -o dropout_table tools/dropout_table.cpp && ./dropout_table`); one test compiles it again and compares, so the table
follows the header.  pair_seed is a __device__ function of csrc/attention_common.h; that program restates its single line on top
of the header's rlt_mix32 (the header is unchanged; the same test holds the two texts equal), and tests/test_dropout_gpu.py
closes the gap to the device function through the attention mask exporters, bit for bit.

A note on the corners: the float32 just below 1 gives the threshold (1 - 2^-24) * 2^32 = 0xFFFFFF00; the clamp at 0xFFFFFFFF is
reached from p = 1 on only (two rows of the table), which every entry point refuses."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dropout_restate as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, row, col, pair, p as float32 bits) -> col_hash(seed, col), pair_seed(seed, pair), drop_threshold(p), keep(seed, row, col),
# keep(pair_seed(seed, pair), row, col)
C_VALUES = (
    ((0x00000000, 0x00000000, 0x00000000, 0, 0x00000000), 0x66BE48EB, 0x00000000, 0x00000000, 1, 1),
    ((0x00003039, 0x00000000, 0x00000000, 3, 0x00000000), 0x3940BF25, 0xEA9B83AB, 0x00000000, 1, 1),
    ((0x00000000, 0x00000000, 0x00000000, 0, 0x3F000000), 0x66BE48EB, 0x00000000, 0x80000000, 0, 0),
    ((0x00003039, 0x00000000, 0x00000000, 3, 0x3F000000), 0x3940BF25, 0xEA9B83AB, 0x80000000, 0, 0),
    ((0x00000000, 0x00000000, 0x00000000, 0, 0x3F7FFFFF), 0x66BE48EB, 0x00000000, 0xFFFFFF00, 0, 0),
    ((0x00003039, 0x00000000, 0x00000000, 3, 0x3F7FFFFF), 0x3940BF25, 0xEA9B83AB, 0xFFFFFF00, 0, 0),
    ((0x00000000, 0x00000000, 0xFFFFFFFF, 1, 0x00000000), 0x42DB672F, 0x01FCE552, 0x00000000, 1, 1),
    ((0x00003039, 0x00000000, 0xFFFFFFFF, 2, 0x00000000), 0x6B5A8241, 0x4545BE4D, 0x00000000, 1, 1),
    ((0x00000000, 0x00000000, 0xFFFFFFFF, 1, 0x3F000000), 0x42DB672F, 0x01FCE552, 0x80000000, 0, 1),
    ((0x00003039, 0x00000000, 0xFFFFFFFF, 2, 0x3F000000), 0x6B5A8241, 0x4545BE4D, 0x80000000, 0, 1),
    ((0x00000000, 0x00000000, 0xFFFFFFFF, 1, 0x3F7FFFFF), 0x42DB672F, 0x01FCE552, 0xFFFFFF00, 0, 0),
    ((0x00003039, 0x00000000, 0xFFFFFFFF, 2, 0x3F7FFFFF), 0x6B5A8241, 0x4545BE4D, 0xFFFFFF00, 0, 0),
    ((0x00000000, 0xFFFFFFFF, 0x00000000, 2, 0x00000000), 0x66BE48EB, 0x04F8D29E, 0x00000000, 1, 1),
    ((0x00003039, 0xFFFFFFFF, 0x00000000, 1, 0x00000000), 0x3940BF25, 0x6F6344E1, 0x00000000, 1, 1),
    ((0x00000000, 0xFFFFFFFF, 0x00000000, 2, 0x3F000000), 0x66BE48EB, 0x04F8D29E, 0x80000000, 1, 1),
    ((0x00003039, 0xFFFFFFFF, 0x00000000, 1, 0x3F000000), 0x3940BF25, 0x6F6344E1, 0x80000000, 1, 1),
    ((0x00000000, 0xFFFFFFFF, 0x00000000, 2, 0x3F7FFFFF), 0x66BE48EB, 0x04F8D29E, 0xFFFFFF00, 0, 0),
    ((0x00003039, 0xFFFFFFFF, 0x00000000, 1, 0x3F7FFFFF), 0x3940BF25, 0x6F6344E1, 0xFFFFFF00, 0, 0),
    ((0x00000000, 0xFFFFFFFF, 0xFFFFFFFF, 3, 0x00000000), 0x42DB672F, 0x0F8C1DBD, 0x00000000, 1, 1),
    ((0x00003039, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0x00000000), 0x6B5A8241, 0x912EFCF7, 0x00000000, 1, 1),
    ((0x00000000, 0xFFFFFFFF, 0xFFFFFFFF, 3, 0x3F000000), 0x42DB672F, 0x0F8C1DBD, 0x80000000, 0, 1),
    ((0x00003039, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0x3F000000), 0x6B5A8241, 0x912EFCF7, 0x80000000, 1, 0),
    ((0x00000000, 0xFFFFFFFF, 0xFFFFFFFF, 3, 0x3F7FFFFF), 0x42DB672F, 0x0F8C1DBD, 0xFFFFFF00, 0, 0),
    ((0x00003039, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0x3F7FFFFF), 0x6B5A8241, 0x912EFCF7, 0xFFFFFF00, 0, 0),
    ((0x00000001, 0x00000001, 0x0000003F, 0, 0x3DCCCCCD), 0x20E7FDD5, 0x688990C0, 0x199999A0, 1, 0),
    ((0x000010E1, 0x00000203, 0x000007FF, 1, 0x3E99999A), 0xC8EAFF8B, 0x8830F533, 0x4CCCCD00, 1, 1),
    ((0xFFFFFFFF, 0x000007FF, 0x00000203, 3, 0x3F666666), 0x4C5965D9, 0x8F424829, 0xE6666600, 0, 0),
    ((0x80000000, 0x0000003F, 0x00000001, 4095, 0x00000001), 0x474A378D, 0x73F79CD8, 0x00000000, 1, 1),
    ((0x00000000, 0x7FFFFFFF, 0x80000000, 2147483647, 0x3F7FF000), 0x84311F63, 0xC7B4F160, 0xFFF00000, 0, 0),
    ((0x00000309, 0x00000000, 0x00000040, 0, 0x3F000000), 0x62A55F11, 0xF398BFE7, 0x80000000, 0, 1),
    ((0x00000001, 0x00000040, 0x00000000, 1, 0x3E800000), 0x6C4F139F, 0xA4F7896C, 0x40000000, 0, 0),
    ((0x000010E1, 0x80000000, 0x7FFFFFFF, 3, 0x3F000001), 0x719FB4AD, 0x38C6F089, 0x80000100, 0, 1),
    ((0xFFFFFFFF, 0x00000001, 0x0000003F, 4095, 0x3DCCCCCD), 0xD444D23D, 0x2809C907, 0x199999A0, 1, 1),
    ((0x80000000, 0x00000203, 0x000007FF, 2147483647, 0x3E99999A), 0x242C61F1, 0x7ED47951, 0x4CCCCD00, 1, 1),
    ((0x00000000, 0x000007FF, 0x00000203, 0, 0x3F666666), 0x17E60FA1, 0x00000000, 0xE6666600, 0, 0),
    ((0x00000309, 0x0000003F, 0x00000001, 1, 0x00000001), 0x1B314F55, 0xF0B86E91, 0x00000000, 1, 1),
    ((0x00000001, 0x7FFFFFFF, 0x80000000, 3, 0x3F7FF000), 0x57275059, 0x705F7037, 0xFFF00000, 0, 0),
    ((0x000010E1, 0x00000000, 0x00000040, 4095, 0x3F000000), 0xC3C4A283, 0xECD71551, 0x80000000, 0, 1),
    ((0xFFFFFFFF, 0x00000040, 0x00000000, 2147483647, 0x3E800000), 0x87A6AB87, 0xD7FA9978, 0x40000000, 1, 1),
    ((0x80000000, 0x80000000, 0x7FFFFFFF, 0, 0x3F000001), 0xA7446703, 0xCC4B4124, 0x80000100, 0, 0),
    ((0x00003039, 0x00000005, 0x00000007, 1, 0x3F800000), 0x346217ED, 0x6F6344E1, 0xFFFFFFFF, 0, 0),
    ((0x000010E1, 0xFFFFFFFF, 0x00000000, 2, 0x40000000), 0x08C973AB, 0x4C83BAD9, 0xFFFFFFFF, 0, 0),
)
C_ROW_HASH_12345_999 = 0xDA7F2DF8


def _p(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def test_generator_matches_values_computed_by_the_c_functions():
    assert len(C_VALUES) == 42
    for (seed, row, col, pair, pbits), ch, ps, thr, kept, kept_pair in C_VALUES:
        p = _p(pbits)
        assert int(D.col_hash(seed, col)) == ch, (seed, col)
        assert int(D.pair_seed(seed, pair)) == ps, (seed, pair)
        assert D.drop_threshold(p) == thr, pbits
        assert bool(D.keep(seed, row, col, thr)) == bool(kept), (seed, row, col, pbits)
        assert bool(D.keep(ps, row, col, thr)) == bool(kept_pair), (seed, pair, row, col, pbits)
        assert bool(D.keep_rc(D.row_hash(seed, row), ch, thr)) == bool(kept)
    assert int(D.row_hash(12345, 999)) == C_ROW_HASH_12345_999
    # the corners the table must hold
    ps = {c[0][4] for c in C_VALUES}
    assert {0x00000000, 0x3F000000, 0x3F7FFFFF} <= ps
    assert {c[3] for c in C_VALUES if c[0][4] == 0x3F000000} == {1 << 31}
    assert {c[3] for c in C_VALUES if c[0][4] == 0x3F7FFFFF} == {0xFFFFFF00}
    assert {c[3] for c in C_VALUES if c[0][4] >= 0x3F800000} == {0xFFFFFFFF}
    assert all(c[4] == 1 and c[5] == 1 for c in C_VALUES if c[3] == 0)          # p = 0 keeps everything
    for i in (0, 1, 2):
        assert {0, 0xFFFFFFFF} <= {c[0][i] for c in C_VALUES}


def test_header_still_prints_the_table(tmp_path):
    """The committed table is what csrc/common.h computes NOW: tools/dropout_table.cpp, compiled for the host alone against the
    header, prints exactly the rows of C_VALUES.  A changed constant of rlt_mix32 / rlt_col_hash / rlt_row_hash or a changed
    threshold fails here.  And the one line the program restates - pair_seed - is the text of csrc/attention_common.h."""
    from rlt_hip import build
    exe = str(tmp_path / "dropout_table")
    cmd = [build.HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-O1", "-o", exe, os.path.join(REPO, "tools", "dropout_table.cpp")]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = [eval(line.strip().rstrip(","), {"__builtins__": {}}) for line in out.splitlines() if line.startswith("    ((")]
    assert tuple(rows) == C_VALUES
    assert f"rlt_row_hash(12345, 999) = 0x{C_ROW_HASH_12345_999:08X}" in out
    body = r"uint32_t pair_seed\(uint32_t seed, int pair\) (\{.*\})"
    with open(os.path.join(REPO, "ranked-list-truncation_amd", "csrc", "attention_common.h")) as f:
        device = re.findall(body, f.read())
    with open(os.path.join(REPO, "tools", "dropout_table.cpp")) as f:
        host = re.findall(body, f.read())
    assert len(device) == 1 and device == host, (device, host)
    assert device[0] == "{ return rlt_mix32(seed ^ ((uint32_t)pair * 0x9E3779B9U)); }"          # what D.pair_seed restates


def test_generator_broadcasts_and_masks_to_32_bits():
    """The array forms equal the scalar forms element by element, also where the uint32 sums and products wrap."""
    seeds = np.array([0, 1, 0xFFFFFFFF, 12345], dtype=np.uint64)
    idx = np.array([0, 1, 63, 0x7FFFFFFF, 0xFFFFFFFF], dtype=np.uint64)
    ch = D.col_hash(seeds[:, None], idx[None, :])
    ps = D.pair_seed(seeds[:, None], idx[None, :])
    assert ch.shape == (4, 5) and int(ch.max()) <= 0xFFFFFFFF and bool((ch & np.uint64(1)).all())
    for i, s in enumerate(seeds.tolist()):
        for j, c in enumerate(idx.tolist()):
            assert int(ch[i, j]) == int(D.col_hash(s, c)) and int(ps[i, j]) == int(D.pair_seed(s, c))
    thr = D.drop_threshold(0.3)
    k = D.keep(7, idx[:, None], idx[None, :], thr)
    for i, r in enumerate(idx.tolist()):
        for j, c in enumerate(idx.tolist()):
            want = (int(D.row_hash(7, r)) * int(D.col_hash(7, c)) & 0xFFFFFFFF) >= thr
            assert bool(k[i, j]) == want


def test_mask_builders():
    """mask: 0 or fp32(1 / fp32(1 - p)); attention_mask: pair i of the range is mask(pair_seed(seed, pair0 + i)), (npair, B, B)."""
    for p in (0.0, 0.1, 0.3, 0.5, float(np.nextafter(np.float32(1), np.float32(0)))):
        m = D.mask(12345, 37, 19, p)
        scale = np.float32(1) / (np.float32(1) - np.float32(p))
        assert m.dtype == np.float32 and m.shape == (37, 19)
        assert np.array_equal(m > 0, D.keep_bits(12345, 37, 19, p)) and set(np.unique(m).tolist()) <= {0.0, float(scale)}
    assert bool((D.mask(5, 8, 8, 0.0) == 1.0).all())
    assert float(np.unique(D.mask(5, 64, 64, 0.1)).max()) == float(np.float32(1) / np.float32(0.9))       # not the double 1 / 0.9
    assert float(D.mask(5, 999, 64, float(np.nextafter(np.float32(1), np.float32(0)))).max()) in (0.0, 2.0 ** 24)
    full = D.attention_mask(4321, 2, 9, 3, 0.3)
    assert full.shape == (6, 9, 9)
    assert np.array_equal(D.attention_mask(4321, 2, 9, 3, 0.3, pair0=3, npair=2), full[3:5])
    for i in range(6):
        assert np.array_equal(full[i], D.mask(int(D.pair_seed(4321, i)), 9, 9, 0.3))
    assert not np.array_equal(full[0], full[1])


# ------------------------------------------------------------------------------------------------ independence
SIZE = 2048          # the size csrc/common.h names


def _standardized(seed, n, p):
    q = 1.0 - float(np.float32(p))
    return (D.keep_bits(seed, n, n, p).astype(np.float64) - q) / math.sqrt(q * (1.0 - q))


@pytest.mark.parametrize("seed", (12345, 4321, 1))
@pytest.mark.parametrize("p", (0.1, 0.3, 0.5))
def test_mask_is_indistinguishable_from_independent_draws(p, seed):
    """2048 x 2048 keep decisions, standardized to x = (keep - q) / sqrt(q (1 - q)), q = 1 - p.  Under independent Bernoulli(q)
    draws every x has mean 0 and variance 1, and so has every product of distinct x; products over different index sets are
    uncorrelated.  Hence each sum below, divided by the square root of its number of terms, is a z value:
      global      the sum of all x; the lag-1 products x[r, c] x[r, c + 1] and x[r, c] x[r + 1, c]; the product of the four x of
                  every disjoint 2 x 2 rectangle                                                                     |z| <= 4
      means       the sum of every row and of every column                                                       max |z| <= 5
      row pairs   the inner product of every pair of distinct rows (2,096,128 of them)        max |z| <= 7, std within 1 +- 0.01
    The bounds are conditions on the generator (for 2 million Gaussian z the largest is about 5.3; the products at p = 0.1 are
    skewed, which the bound of 7 allows for), not measurements."""
    n = SIZE
    x = _standardized(seed, n, p)
    z = {"keep fraction": x.sum() / n,
         "lag-1 along rows": (x[:, :-1] * x[:, 1:]).sum() / math.sqrt(n * (n - 1)),
         "lag-1 along columns": (x[:-1, :] * x[1:, :]).sum() / math.sqrt(n * (n - 1)),
         "2 x 2 rectangles": (x[0::2, 0::2] * x[0::2, 1::2] * x[1::2, 0::2] * x[1::2, 1::2]).sum() / (n / 2)}
    rows, cols = x.sum(axis=1) / math.sqrt(n), x.sum(axis=0) / math.sqrt(n)
    g = (x @ x.T)[np.triu_indices(n, 1)] / math.sqrt(n)
    figures = dict(z, row_mean=float(np.abs(rows).max()), col_mean=float(np.abs(cols).max()), pair_max=float(np.abs(g).max()),
                   pair_std=float(g.std()))
    print(p, seed, {k: round(float(v), 3) for k, v in figures.items()})
    for name, v in z.items():
        assert abs(v) <= 4.0, (name, v)
    assert figures["row_mean"] <= 5.0 and figures["col_mean"] <= 5.0, figures
    assert figures["pair_max"] <= 7.0, figures
    assert abs(figures["pair_std"] - 1.0) <= 0.01, figures


@pytest.mark.parametrize("seed", (12345, 4321, 1))
def test_pairs_draw_independent_masks(seed):
    """The masks of pair_seed(seed, 0) and pair_seed(seed, 1) at 512 x 512, p = 0.3: the sum of the products of their
    standardized decisions over 512 is a z value, |z| <= 4 (a pair_seed that ignored the pair would give z = 512).  And
    pair_seed(seed, .) is injective over the 4096 pairs of the largest list count the project runs."""
    a, b = (_standardized(int(D.pair_seed(seed, pair)), 512, 0.3) for pair in (0, 1))
    z = float((a * b).sum() / 512)
    print(seed, round(z, 3))
    assert abs(z) <= 4.0
    assert np.unique(D.pair_seed(seed, np.arange(4096))).size == 4096


# ------------------------------------------------------------------------------------------------ ops.next_seed
@pytest.fixture
def seeding():
    """ops with its counter and stream id, and torch's seed, put back afterwards"""
    import torch
    from rlt_hip import ops
    saved = (torch.initial_seed(), ops._SEED_COUNTER[0], ops._SEED_STREAM[0])
    yield ops
    torch.manual_seed(saved[0])
    ops._SEED_COUNTER[0], ops._SEED_STREAM[0] = saved[1], saved[2]


def _sequence(ops, torch_seed, stream_id, n):
    import torch
    torch.manual_seed(torch_seed)
    ops._SEED_COUNTER[0] = 0
    ops.set_seed_stream(stream_id)
    return [ops.next_seed() for _ in range(n)]


@pytest.mark.parametrize("torch_seed", (0, 12345))
def test_next_seed_gives_distinct_32_bit_seeds(seeding, torch_seed):
    s = _sequence(seeding, torch_seed, 0, 10000)
    assert all(isinstance(v, int) and 0 <= v <= 0xFFFFFFFF for v in s)
    assert len(set(s)) == 10000


def test_next_seed_streams_differ(seeding):
    """Stream ids 0..7 (the ranks of a data-parallel run) under one torch seed: pairwise different sequences - and, stronger, no
    position at which two of them agree in 1000 draws (28 pairs x 1000 positions of 32-bit values: 6.5e-6 by chance)."""
    seqs = [_sequence(seeding, 77, sid, 1000) for sid in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert seqs[a] != seqs[b]
            assert not any(u == v for u, v in zip(seqs[a], seqs[b])), (a, b)


def test_next_seed_is_reproducible_under_manual_seed(seeding):
    first = _sequence(seeding, 2024, 3, 500)
    seeding.next_seed()
    assert _sequence(seeding, 2024, 3, 500) == first
    assert _sequence(seeding, 2025, 3, 500) != first          # and a function of torch's seed
