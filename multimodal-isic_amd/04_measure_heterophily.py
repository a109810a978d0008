"""Drop-in for the numeric part of the reference's ``04_measure_heterophily.py``: the master summary of the
heterophily measures over all images, folds and graph variants (`build_master_summary`, 04:188-226), computed on
the MI355X (``measure_heterophily.py``): each chunk of images is summarised on the device
(``heterophily_summary_device``) and copied to the host once.  The reference's plotting / aggregation section
(04:229-589) and its hard-coded cluster paths (04:23,560-561) are out of scope: paths are flags here and the output
is one CSV.

    python 04_measure_heterophily.py --graph-outputs-root graph_outputs --patch-stats-root patch_stats --out-csv h.csv

``--lesion-flags PATH...`` (the patch-level frames ``05_train_gnns.py --lesion-flags`` takes) measures the subgraph that every
image's lesion flags induce -- the graphs the GNNs are then trained on -- and adds a ``num_nodes`` column after ``num_edges``.
``--lesion-knn`` (with ``--lesion-flags``): a ``knn<k>`` variant is measured on the k-NN graph rebuilt AMONG the lesion patches
of every image, k clamped per image as the reference clamps it on a lesion-only frame; other variants keep the induced subgraph.
``--lesion-random`` (with ``--lesion-flags``): a ``random<r>`` variant is measured on the reference's random graph rebuilt AMONG
the lesion patches of every image (r clamped per image; the image's seed is ``--graph-seed`` + fold * 10000 + its row in the
fold's patch-statistics frame, `03_build_graphs.py:136`); other variants keep the induced subgraph.
"""
import argparse
import os
import pickle

import numpy as np
import pandas as pd
import torch

import measure_heterophily as mh
from lesion_flags import _keep_flags, load_lesion_flags


def build_master_summary(graph_root, patch_root, images_per_launch=64, device="cuda:0", lesion_flags=None, lesion_knn=False,
                         lesion_random=False, graph_seed=42):
    """``lesion_flags`` (``lesion_flags.load_lesion_flags``): summarise the induced subgraphs
    (``heterophily_summary_lesion_only``); an image id without flags is a ``ValueError`` that names it.
    ``lesion_knn``: knn<k> variants are rebuilt among the lesion patches (``heterophily_summary_lesion_knn``).
    ``lesion_random``: random<r> variants are rebuilt among the lesion patches (``heterophily_summary_lesion_random``), an
    image seeded with ``graph_seed`` + fold * 10000 + its index label in the patch-statistics frame (`03_build_graphs.py:136`)."""
    if lesion_knn and lesion_flags is None:
        raise ValueError("lesion_knn rebuilds the k-NN graph among the lesion patches: it needs lesion_flags")
    if lesion_random and lesion_flags is None:
        raise ValueError("lesion_random rebuilds the random graph among the lesion patches: it needs lesion_flags")
    rows = []
    for model in sorted(os.listdir(graph_root)):
        gpath = os.path.join(graph_root, model, "graph_dataset.pkl")
        if not os.path.exists(gpath):
            continue
        gdf = pd.DataFrame(pickle.load(open(gpath, "rb")))
        for (fold, split), grp in gdf.groupby(["fold", "split"]):
            ppath = os.path.join(patch_root, model, f"patch_stats_fold_{int(fold)}_{split}.pkl")
            pdf = pd.DataFrame(pickle.load(open(ppath, "rb")))
            row_idx = dict(zip(pdf["image_id"], pdf.index))
            merged = grp.merge(pdf, on="image_id", how="inner", suffixes=("", "_patch"))        # 04:80-85
            if merged.empty:
                continue
            first = merged.iloc[0]
            variants = ["grid4", "grid8"] + [f"knn{int(k)}" for k in first["knn_edge_indices"]] + \
                       [f"random{int(r)}" for r in first["random_edge_indices"]]
            for variant in variants:
                for lo in range(0, len(merged), images_per_launch):
                    chunk = merged.iloc[lo:lo + images_per_launch]
                    recs = chunk.to_dict("records")
                    dev = torch.device(device)
                    x = torch.as_tensor(np.stack([np.asarray(r["patch_embeddings"], dtype=np.float32) for r in recs])).to(dev)
                    pp = torch.as_tensor(np.stack([np.asarray(r["patch_probs"], dtype=np.float32) for r in recs])).to(dev)
                    dom = torch.as_tensor(np.stack([np.asarray(r["dominant_class"], dtype=np.int32) for r in recs])).to(dev)
                    eis = [torch.as_tensor(np.asarray(mh.edge_index_from_variant(r, variant), dtype=np.int64)).to(dev)
                           for r in recs]
                    if lesion_flags is not None:
                        keep = torch.as_tensor(np.stack([_keep_flags(lesion_flags, str(r["image_id"]), int(x.shape[1]))
                                                         for r in recs])).to(dev)
                        if lesion_knn and variant.startswith("knn"):
                            summary = mh.heterophily_summary_lesion_knn(x, pp, dom, keep, int(variant[3:]))
                        elif lesion_random and variant.startswith("random"):
                            seeds = [int(graph_seed) + int(fold) * 10_000 + int(row_idx[r["image_id"]]) for r in recs]
                            summary = mh.heterophily_summary_lesion_random(x, pp, dom, keep, int(variant[6:]), seeds)
                        else:
                            summary = mh.heterophily_summary_lesion_only(x, pp, dom, eis, keep)
                    else:
                        summary = mh.heterophily_summary_device(x, pp, dom, eis)      # one copy to the host per chunk
                    kind = "grid" if variant.startswith("grid") else ("knn" if variant.startswith("knn") else "random")
                    metas = [{"model_name": r.get("model_name", model), "fold": int(fold), "split": split,
                              "image_id": r["image_id"], "label": r.get("label"), "graph_variant": variant,
                              "graph_type": kind,
                              "graph_param": None if kind == "grid" else int(variant[len(kind):])}      # 04:211-222
                             for r in recs]
                    rows.extend(mh.summary_records(summary, metas))
    return pd.DataFrame.from_records(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph-outputs-root", default="graph_outputs")
    ap.add_argument("--patch-stats-root", default="patch_stats")
    ap.add_argument("--out-csv", default="heterophily_summary.csv")
    ap.add_argument("--images-per-launch", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--lesion-flags", nargs="+", default=None, metavar="PATH",
                    help="patch-level frames with patch_in_mask: measure the subgraph the lesion patches induce")
    ap.add_argument("--lesion-knn", action="store_true",
                    help="with --lesion-flags: measure knn<k> variants on the k-NN graph rebuilt among the lesion patches "
                         "(k clamped per image) instead of the induced subgraph")
    ap.add_argument("--lesion-random", action="store_true",
                    help="with --lesion-flags: measure random<r> variants on the reference's random graph rebuilt among the "
                         "lesion patches (r clamped per image) instead of the induced subgraph")
    ap.add_argument("--graph-seed", type=int, default=42,
                    help="the --seed 03_build_graphs.py was run with (--lesion-random seeds an image as it did)")
    a = ap.parse_args()
    if a.lesion_knn and not a.lesion_flags:
        ap.error("--lesion-knn needs --lesion-flags")
    if a.lesion_random and not a.lesion_flags:
        ap.error("--lesion-random needs --lesion-flags")
    flags = load_lesion_flags(a.lesion_flags) if a.lesion_flags else None
    df = build_master_summary(a.graph_outputs_root, a.patch_stats_root, a.images_per_launch, a.device, lesion_flags=flags,
                              lesion_knn=a.lesion_knn, lesion_random=a.lesion_random, graph_seed=a.graph_seed)
    df.drop(columns=["H_compat_matrix"]).to_csv(a.out_csv, index=False)
    print(f"wrote {len(df)} rows ({df['graph_variant'].nunique() if len(df) else 0} graph variants) to {a.out_csv}")


if __name__ == "__main__":
    main()
