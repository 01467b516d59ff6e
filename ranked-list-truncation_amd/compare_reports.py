"""Compare `run.py --report-out` files query by query: paired randomization test, paired bootstrap interval, sign and t statistics.

    python compare_reports.py A.npz B.npz [...] --metric f1 --baseline 0 --resamples 10000 --seed 0 --level 0.95 --out cmp.json

The first file (or --baseline N, or --baseline Oracle, in any letter case: the first file's best cut per query) is the baseline; one line per system."""
import argparse

from utils.compare import compare_reports, is_best_cut, write_json


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("reports", nargs="+", help=".npz files written by run.py --report-out")
    p.add_argument("--metric", choices=("f1", "dcg", "reward"), default="f1",
                   help="reward: the columns of a report written with run.py --eval-reward (the files must share one reward)")
    p.add_argument("--baseline", default="0", help="index of the baseline file, or Oracle")
    p.add_argument("--resamples", type=int, default=10000)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--level", type=float, default=0.95)
    p.add_argument("--out", default=None, help="write the per-system figures as JSON")
    args = p.parse_args(argv)
    baseline = args.baseline if is_best_cut(args.baseline) else int(args.baseline)
    cmp = compare_reports(args.reports, metric=args.metric, baseline=baseline, resamples=args.resamples, seed=args.seed)
    for line in cmp.lines(args.level):
        print(line)
    if args.out:
        write_json(cmp, args.out, args.level, metric=args.metric, baseline=args.baseline, seed=args.seed)
    return cmp


if __name__ == "__main__":
    main()
