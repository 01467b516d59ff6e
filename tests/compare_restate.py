"""Numpy float64 restatement of the paired comparison pass (csrc/compare.hip, include/rlt_hip.h): the generator in uint64
arithmetic masked to 32 bits, the signs, the bootstrap indices, the record, T_r and B_r, and the host-side figures drawn from them.
tests/test_compare_restate.py pins it to exhaustive enumeration, to the statistics of its draws and to scipy."""
import math

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
WORDS = 16
(N_, SUM_BASE, SUM_SYS, SUM_D, SSD, WINS, TIES, LOSSES, NONFINITE, T_OBS, RAND_GE, BOOT_LE0, BOOT_GE0, RESAMPLES, FORM,
 RESERVED) = range(16)
F64_WORDS = (SUM_BASE, SUM_SYS, SUM_D, SSD, T_OBS)


def _u(x):
    return np.asarray(x, dtype=np.uint64) & MASK


def mix32(x):
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & MASK
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & MASK
    return x ^ (x >> np.uint64(16))


def row_hash(seed, row):
    return mix32((_u(seed) + mix32((_u(row) + np.uint64(0x9E3779B9)) & MASK)) & MASK)


def draw(seed, r, c):
    """draw(seed, r, c) = mix32(row_hash(seed, r) ^ mix32(c + 0x7F4A7C15)); r and c broadcast."""
    return mix32(row_hash(seed, r) ^ mix32((_u(c) + np.uint64(0x7F4A7C15)) & MASK))


def boot_seed(seed):
    return int(mix32(_u(seed) ^ np.uint64(0xA511E9B3)))


def signs(seed, r, Q):
    """(len(r), Q) float64 of +-1: -1 where bit (q & 31) of draw(seed, r, q >> 5) is set."""
    r = np.atleast_1d(np.asarray(r, dtype=np.uint64))
    q = np.arange(Q, dtype=np.uint64)
    w = draw(seed, r[:, None], (q >> np.uint64(5))[None, :])
    bit = (w >> (q & np.uint64(31))[None, :]) & np.uint64(1)
    return 1.0 - 2.0 * bit.astype(np.float64)


def indices(seed, r, Q):
    """(len(r), Q) int64: idx(r, j) = (draw(seed', r, j) * Q) >> 32."""
    r = np.atleast_1d(np.asarray(r, dtype=np.uint64))
    j = np.arange(Q, dtype=np.uint64)
    u = draw(boot_seed(seed), r[:, None], j[None, :])
    return ((u * np.uint64(Q)) >> np.uint64(32)).astype(np.int64)


def differences(base, sys):
    """d (M, Q) float64 with 0 where a member of the pair is not finite, and the mask of the finite pairs."""
    base = np.asarray(base, dtype=np.float32)
    sys = np.atleast_2d(np.asarray(sys, dtype=np.float32))
    ok = np.isfinite(base)[None, :] & np.isfinite(sys)
    with np.errstate(invalid="ignore"):
        d = np.where(ok, sys.astype(np.float64) - base.astype(np.float64)[None, :], 0.0)
    return d, ok


def replicate_stats(d, seed, R, block=1 << 21):
    """rand (M, R) and boot (M, R) float64."""
    M, Q = d.shape
    rand, boot = np.zeros((M, R)), np.zeros((M, R))
    step = max(1, block // Q)
    for r0 in range(0, R, step):
        r = np.arange(r0, min(R, r0 + step))
        s = signs(seed, r, Q)
        idx = indices(seed, r, Q)
        for m in range(M):
            rand[m, r] = (s * d[m][None, :]).sum(axis=1)
            boot[m, r] = d[m][idx].sum(axis=1)
    return rand, boot


def compare(base, sys, R, seed):
    """-> (records: list of M dicts keyed like the record's words, rand (M, R), boot (M, R))."""
    d, ok = differences(base, sys)
    base64 = np.asarray(base, dtype=np.float32).astype(np.float64)
    sys64 = np.atleast_2d(np.asarray(sys, dtype=np.float32)).astype(np.float64)
    rand, boot = replicate_stats(d, seed, R)
    recs = []
    for m in range(d.shape[0]):
        k = ok[m]
        n = int(k.sum())
        dm = d[m][k]
        sum_d = float(dm.sum())
        mean = sum_d / n if n else 0.0
        t_obs = float(d[m].sum())
        recs.append({N_: n, SUM_BASE: float(base64[k].sum()), SUM_SYS: float(sys64[m][k].sum()), SUM_D: sum_d,
                     SSD: float(((dm - mean) ** 2).sum()), WINS: int((dm > 0).sum()), TIES: int((dm == 0).sum()),
                     LOSSES: int((dm < 0).sum()), NONFINITE: int((~k).sum()), T_OBS: t_obs,
                     RAND_GE: int((np.abs(rand[m]) >= abs(t_obs)).sum()), BOOT_LE0: int((boot[m] <= 0).sum()),
                     BOOT_GE0: int((boot[m] >= 0).sum()), RESAMPLES: int(R), RESERVED: 0})
    return recs, rand, boot


# ------------------------------------------------------------------------------------------ host-side figures
def randomization_p(rand_ge, R):
    return (rand_ge + 1) / (R + 1)


def sign_test_p(wins, losses):
    n, k = wins + losses, min(wins, losses)
    if n == 0:
        return 1.0
    return min(1.0, 2.0 * sum(math.comb(n, i) for i in range(k + 1)) / 2.0 ** n)


def t_statistic(d):
    """(t, df) of a vector of differences; zero variance: 0 when the mean is 0, +-inf otherwise."""
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    mean = d.sum() / n
    ssd = ((d - mean) ** 2).sum()
    if n < 2 or ssd == 0.0:
        return (0.0 if mean == 0 else math.copysign(math.inf, mean)), max(n - 1, 0)
    return float(mean / math.sqrt(ssd / (n - 1) / n)), n - 1


def holm(p):
    order = np.argsort(np.asarray(p, dtype=np.float64), kind="stable")
    out, running = np.zeros(len(p)), 0.0
    for rank, i in enumerate(order):
        running = max(running, min(1.0, (len(p) - rank) * p[i]))
        out[i] = running
    return out.tolist()


def percentile_interval(boot_row, Q, level):
    s = np.sort(np.asarray(boot_row, dtype=np.float64)) / Q
    R, a = s.size, 1.0 - level
    lo = min(max(int(math.floor(R * a / 2)), 0), R - 1)
    hi = min(max(int(math.ceil(R * (1 - a / 2))) - 1, 0), R - 1)
    return float(s[lo]), float(s[hi])


def exact_operands(Q, M, seed):
    """base (Q,), sys (M, Q) float32: integers in [-512, 512] times 2^-10, adjusted so that every system's sum of differences is a
    multiple of Q * 2^-10 - the mean difference is then a multiple of 2^-10 and every sum of the record, the squared deviations
    included, is exact in float64 in any order."""
    rng = np.random.RandomState(seed)
    kb = rng.randint(-512, 513, size=Q)
    ks = rng.randint(-512, 513, size=(M, Q))
    for m in range(M):
        rho = int((ks[m] - kb).sum() % Q)
        room = np.flatnonzero(ks[m] > -512)[:rho]
        assert room.size == rho
        ks[m, room] -= 1
        assert (ks[m] - kb).sum() % Q == 0
    return (kb / 1024.0).astype(np.float32), (ks / 1024.0).astype(np.float32)
