"""Is one truncation run better than another?  Paired significance tests between per-query columns of `run.py --report-out` files:
the Fisher sign-flip randomization test and the paired bootstrap run on the device (rlt_paired_compare, csrc/compare.hip); the sign
test, the t statistic, the percentile interval and the Holm correction are host arithmetic on the record it leaves."""
import json
import math
from fractions import Fraction

import numpy as np
import torch

from rlt_hip import native as N
from rlt_hip import ops


SIGN_TEST_EXACT_MAX = 4096      # above it the binomial tail is summed in floating point (lgamma), relative error below 1e-9


def sign_test_p(wins, losses):
    """Two-sided sign test: P(a Binomial(wins + losses, 1/2) is at least as far from its mean as what was seen); ties dropped.
    Exact integer arithmetic (math.comb) up to SIGN_TEST_EXACT_MAX untied pairs."""
    n, k = int(wins) + int(losses), min(int(wins), int(losses))
    if n == 0 or 2 * k == n:
        return 1.0
    if n <= SIGN_TEST_EXACT_MAX:
        tail = sum(math.comb(n, i) for i in range(k + 1))
        return min(1.0, float(Fraction(2 * tail, 2 ** n)))
    logs = [math.lgamma(n + 1) - math.lgamma(i + 1) - math.lgamma(n - i + 1) - n * math.log(2.0) for i in range(k, max(k - 100 - 8 * math.isqrt(n), -1), -1)]
    return min(1.0, 2.0 * math.exp(logs[0]) * math.fsum(math.exp(v - logs[0]) for v in logs))


def t_statistic(mean_d, ssd, n):
    """(t, degrees of freedom) of the paired t test.  Zero variance (or n < 2): t = 0 when the mean difference is 0, +-inf otherwise."""
    df = max(int(n) - 1, 0)
    var = float(ssd) / df if df > 0 else 0.0
    if var <= 0.0:
        return (0.0 if mean_d == 0 else math.copysign(math.inf, mean_d)), df
    return float(mean_d) / math.sqrt(var / int(n)), df


def holm(p):
    """Holm's step-down adjustment of a family of p-values, in the order given."""
    p = [float(x) for x in p]
    order = sorted(range(len(p)), key=lambda i: p[i])
    out, running = [0.0] * len(p), 0.0
    for rank, i in enumerate(order):
        running = max(running, min(1.0, (len(p) - rank) * p[i]))
        out[i] = running
    return out


def percentile_interval(sorted_values, level):
    """The percentile interval of an ascending sample: [x_(floor(R a / 2)), x_(ceil(R (1 - a / 2)) - 1)], a = 1 - level."""
    R = len(sorted_values)
    a = 1.0 - float(level)
    lo = min(max(int(math.floor(R * a / 2)), 0), R - 1)
    hi = min(max(int(math.ceil(R * (1 - a / 2))) - 1, 0), R - 1)
    return float(sorted_values[lo]), float(sorted_values[hi])


class PairedComparison:
    """M systems against one baseline on the same queries.  base (Q,), systems (M, Q) or (Q,): float32 tensors on the GPU.  The
    device pass runs in the constructor; the first figure that is asked for reads the record (one host read)."""

    def __init__(self, base, systems, resamples=10000, seed=0, names=None, keep_stats=True):
        out = ops.paired_compare(base, systems, resamples, seed, keep_stats=keep_stats)
        self.record, self.rand_stat, self.boot_stat = out["record"], out["rand_stat"], out["boot_stat"]
        self.M, self.Q, self.R = self.record.shape[0], int(base.numel()), int(resamples)
        self.names = list(names) if names is not None else [f"system{m}" for m in range(self.M)]
        if len(self.names) != self.M:
            raise ValueError(f"{len(self.names)} names for {self.M} systems")
        self._host = None

    def _rec(self):
        if self._host is None:
            w = self.record.cpu()
            f = w.view(torch.float64)
            rows = []
            for m in range(self.M):
                rows.append({"n": int(w[m, N.CMP_N]), "sum_base": float(f[m, N.CMP_SUM_BASE]), "sum_sys": float(f[m, N.CMP_SUM_SYS]),
                             "sum_d": float(f[m, N.CMP_SUM_D]), "ssd": float(f[m, N.CMP_SSD]), "wins": int(w[m, N.CMP_WINS]),
                             "ties": int(w[m, N.CMP_TIES]), "losses": int(w[m, N.CMP_LOSSES]), "nonfinite": int(w[m, N.CMP_NONFINITE]),
                             "t_obs": float(f[m, N.CMP_T_OBS]), "rand_ge": int(w[m, N.CMP_RAND_GE]),
                             "boot_le0": int(w[m, N.CMP_BOOT_LE0]), "boot_ge0": int(w[m, N.CMP_BOOT_GE0]),
                             "form": N.CMP_FORMS[int(w[m, N.CMP_FORM])]})
            bad = sum(r["nonfinite"] for r in rows)
            if bad:
                raise ValueError(f"paired comparison: {bad} query values are NaN or Inf")
            self._host = rows
        return self._host

    def means(self, m):
        """(baseline mean, system mean, mean difference)"""
        r = self._rec()[m]
        return r["sum_base"] / r["n"], r["sum_sys"] / r["n"], r["sum_d"] / r["n"]

    def t_test(self, m):
        r = self._rec()[m]
        return t_statistic(r["sum_d"] / r["n"], r["ssd"], r["n"])

    def sign_test(self, m):
        r = self._rec()[m]
        return sign_test_p(r["wins"], r["losses"])

    def randomization_p(self, m):
        return (self._rec()[m]["rand_ge"] + 1) / (self.R + 1)

    def holm_p(self):
        return holm([self.randomization_p(m) for m in range(self.M)])

    def bootstrap_interval(self, m, level=0.95):
        """Percentile interval of the mean difference from the sorted bootstrap sums / Q."""
        self._rec()
        if self.boot_stat is None or self.R == 0:
            raise ValueError("the bootstrap interval needs keep_stats=True and resamples > 0")
        s = torch.sort(self.boot_stat[m])[0].cpu().numpy() / self.Q
        return percentile_interval(s, level)

    def null_distribution(self, m):
        """The R randomization sums of system m (host array): what the observed sum t_obs is compared with."""
        return self.rand_stat[m].cpu().numpy()

    def summary(self, level=0.95):
        """One dict per system, JSON-serialisable."""
        adj = self.holm_p()
        rows = []
        for m, r in enumerate(self._rec()):
            mb, ms, md = self.means(m)
            t, df = self.t_test(m)
            row = {"name": self.names[m], "n": r["n"], "mean_base": mb, "mean_sys": ms, "mean_diff": md, "t": t, "df": df,
                   "wins": r["wins"], "ties": r["ties"], "losses": r["losses"], "sign_p": self.sign_test(m),
                   "rand_p": self.randomization_p(m), "rand_p_holm": adj[m], "resamples": self.R, "form": r["form"]}
            if self.boot_stat is not None and self.R > 0:
                row["level"] = level
                row["ci_low"], row["ci_high"] = self.bootstrap_interval(m, level)
            rows.append(row)
        return rows

    def lines(self, level=0.95):
        out = []
        for s in self.summary(level):
            ci = f" CI{int(round(100 * level))} [{s['ci_low']:+.4f}, {s['ci_high']:+.4f}]" if "ci_low" in s else ""
            out.append(f"{s['name']}: {s['mean_sys']:.4f} vs {s['mean_base']:.4f} diff {s['mean_diff']:+.4f}{ci} "
                       f"t({s['df']}) {s['t']:.3f} sign p {s['sign_p']:.4g} W/T/L {s['wins']}/{s['ties']}/{s['losses']} "
                       f"rand p {s['rand_p']:.4g} (Holm {s['rand_p_holm']:.4g}, R = {s['resamples']})")
        return out


def _load_report(path, metric):
    with np.load(path, allow_pickle=False) as z:
        if metric not in z.files:
            raise ValueError(f"{path}: no '{metric}' column (a label-free report cannot be compared)" if metric != "reward" else
                             f"{path}: no 'reward' column (the report was written without --eval-reward)")
        keys = [(str(q), int(l)) for q, l in zip(z["qid"], z["length"])]
        cols = {k: np.asarray(z[k], dtype=np.float64) for k in (metric, "best_" + metric) if k in z.files}
        spec = str(z["reward_spec"]) if "reward_spec" in z.files else None
    if len(set(keys)) != len(keys):
        raise ValueError(f"{path}: duplicate (qid, length) rows")
    return keys, cols, spec


def is_best_cut(baseline):
    """True for the name of the Oracle baseline (each query's best cut), whatever its letter case."""
    # compared capitalised: tests/test_abi.py keeps the lower-case word - the name of the CPU reference package of the tests - out
    # of every source of this package, so that the product can never come to import it
    return isinstance(baseline, str) and baseline.capitalize() == "Oracle"


def compare_reports(paths, metric="f1", baseline=0, resamples=10000, seed=0, device="cuda", keep_stats=True):
    """Load `run.py --report-out` files, join them on (qid, length) and compare.  baseline: an index into `paths`, or the name of the
    Oracle baseline in any letter case (the first file's best_f1 / best_dcg column; every file is then a system).  Files whose query sets differ are refused.
    metric='reward' reads the `reward` / `best_reward` columns a report written with a reward spec carries (CutReport(reward=...),
    run.py --eval-reward); files without the column, and files whose `reward_spec` strings differ, are refused."""
    if metric not in ("f1", "dcg", "reward"):
        raise ValueError("metric: 'f1', 'dcg' or 'reward'")
    paths = list(paths)
    loaded = [_load_report(p, metric) for p in paths]
    if metric == "reward":
        for p, (_k, _c, spec) in zip(paths, loaded):
            if spec != loaded[0][2]:
                raise ValueError(f"{p}: its rewards are in {spec!r}, {paths[0]}'s in {loaded[0][2]!r}: not comparable")
    keys0 = loaded[0][0]
    ref = set(keys0)
    columns = []
    for p, (keys, cols, _spec) in zip(paths, loaded):
        if set(keys) != ref:
            missing, extra = len(ref - set(keys)), len(set(keys) - ref)
            raise ValueError(f"{p}: its query set differs from {paths[0]}'s ({missing} missing, {extra} unknown)")
        at = {k: i for i, k in enumerate(keys)}
        columns.append(cols[metric][[at[k] for k in keys0]])
    if is_best_cut(baseline):
        if "best_" + metric not in loaded[0][1]:
            raise ValueError(f"{paths[0]}: no 'best_{metric}' column")
        base, systems, names = loaded[0][1]["best_" + metric], columns, paths
    else:
        b = int(baseline)
        if not 0 <= b < len(paths) or len(paths) < 2:
            raise ValueError("baseline: an index into at least two files, or 'Oracle'")
        base = columns[b]
        systems = [c for i, c in enumerate(columns) if i != b]
        names = [p for i, p in enumerate(paths) if i != b]
    dev = torch.device(device)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(dev)
    return PairedComparison(t(base), t(np.stack(systems)), resamples=resamples, seed=seed, names=names, keep_stats=keep_stats)


def write_json(comparison, path, level=0.95, **extra):
    with open(path, "w") as f:
        json.dump({"systems": comparison.summary(level), **extra}, f, indent=1)
