#!/usr/bin/env python3
"""Write AttnCut's input statistics `<base>/<retrieve_data>/attncut/<name>_{train,test}.pkl` from the ranked lists and the two
document tables - what the reference does in data_prep/data_review.ipynb (simi_list) over hours of Python loops, here one
kernel pass per list length (dataloader/doc_features.py, rlt_neighbor_features).

    python prepare_features.py --dataset-base DIR --retrieve-data robust04 --dataset-name bm25 \\
        --tfidf DIR/robust04/statics/tfidf.pkl --doc2vec DIR/robust04/statics/doc2vec.pkl
    python run.py --dataset-base DIR --retrieve-data robust04 --dataset-name bm25 --model-name attncut

Reads  <base>/<retrieve_data>/<name>_{train,test}.pkl   dict[qid] -> dict[doc_id -> score], rank order
       --tfidf    dict[doc_id] -> list[(term_id, weight)], term ids ascending (gensim bag-of-words)
       --doc2vec  dict[doc_id] -> float32 vector
Writes dict[qid] -> list[S][2]: column 0 the tf-idf similarity, column 1 the doc2vec one.  With only one of --tfidf / --doc2vec
the lists have that one column."""
import argparse
import os
import pickle
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def build_parser():
    p = argparse.ArgumentParser(description="neighbour-similarity statistics of the AttnCut family, computed on the GPU")
    p.add_argument('--dataset-base', type=str, required=True, help="directory holding <retrieve_data>/*.pkl")
    p.add_argument('--retrieve-data', type=str, default='robust04')
    p.add_argument('--dataset-name', type=str, default='bm25')
    p.add_argument('--tfidf', type=str, default=None, help="pickle: dict[doc_id] -> [(term_id, weight)]")
    p.add_argument('--doc2vec', type=str, default=None, help="pickle: dict[doc_id] -> float32 vector")
    p.add_argument('--out-dir', type=str, default='attncut', help="sub-directory of <base>/<retrieve_data> to write into")
    p.add_argument('--device', type=str, default='cuda:0')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.tfidf and not args.doc2vec:
        raise SystemExit("give --tfidf, --doc2vec or both")
    import torch
    from dataloader.doc_features import DocTable, neighbor_stats
    if not torch.cuda.is_available():
        raise SystemExit("prepare_features.py needs a GPU: the statistics are computed by a HIP kernel, there is no CPU path")
    root = os.path.join(args.dataset_base, args.retrieve_data)
    raws = {}
    for split in ("train", "test"):
        with open(os.path.join(root, f"{args.dataset_name}_{split}.pkl"), "rb") as f:
            raws[split] = pickle.load(f)
    t0 = time.time()
    table = DocTable.from_pickles(args.tfidf, args.doc2vec, *raws.values()).to(args.device)
    t1 = time.time()
    os.makedirs(os.path.join(root, args.out_dir), exist_ok=True)
    for split, raw in raws.items():
        stats = neighbor_stats(raw, table)
        path = os.path.join(root, args.out_dir, f"{args.dataset_name}_{split}.pkl")
        with open(path, "wb") as f:
            pickle.dump(stats, f)
        print(f"{path}: {len(stats)} lists, {table.n_columns} columns")
    print(f"{table.n_docs} documents packed in {t1 - t0:.1f} s, statistics in {time.time() - t1:.1f} s")


if __name__ == "__main__":
    main()
