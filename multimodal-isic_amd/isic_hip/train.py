"""Host-side train / eval loops of the MIL teacher (`01_train_mil_teacher.py:170-305`)
and of the patch-graph GNN (`05_train_gnns.py:273-358`) over the HIP path, with the two
things the reference does not have: several bags / graphs per optimizer step in one
launch, and bag-sharded data parallelism (one process per GPU, RCCL gradient all-reduce
through ``ddp.GradSync``).

Step semantics (SURVEY.md §7 "Batch-vs-per-bag"): with ``per_step=1, world=1`` these loops
ARE the reference loops (one optimizer step per bag / graph); with B bags per step the loss
is the mean of the per-bag reference losses and the gradient the mean of the per-bag
gradients.
"""
from __future__ import annotations

import copy
import os
from collections import Counter

import numpy as np
import torch
import torch.distributed as dist

from . import ddp, ops, optim
from .bags import BagOffsets
from .graph import GraphBatch
from .lib import call


def dist_info():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def init_distributed():
    """One process per GPU under torchrun / torch.distributed.run; no-op otherwise."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return dist_info()


def weighted_sample_indices(labels, generator):
    """`01_train_mil_teacher.py:189-193`: WeightedRandomSampler(1/class_count, n, replacement=True)."""
    labels = np.asarray(labels)
    counts = Counter(labels.tolist())
    w = torch.tensor([1.0 / counts[int(l)] for l in labels], dtype=torch.float64)
    return torch.multinomial(w, len(labels), replacement=True, generator=generator).tolist()


class BagStore:
    """Bags resident in HBM: uniform bags as one [n, K, D] tensor (gathered by index per step),
    ragged bags as a list of device tensors concatenated per step."""

    def __init__(self, bags, device):
        self.device = device
        lens = {int(b.shape[0]) for b in bags}
        self.uniform = len(lens) == 1
        self.lengths = [int(b.shape[0]) for b in bags]

        def dev(b):            # numpy latents (`01_train_mil_teacher.py:51-67`) or tensors already resident in HBM
            if isinstance(b, torch.Tensor):
                return b.to(device=device, dtype=torch.float32)
            return torch.as_tensor(np.asarray(b, dtype=np.float32)).to(device)
        if self.uniform and not any(isinstance(b, torch.Tensor) for b in bags):
            self.data = torch.as_tensor(np.stack([np.asarray(b, dtype=np.float32) for b in bags])).to(device)
        elif self.uniform:
            self.data = torch.stack([dev(b) for b in bags])
        else:
            self.data = [dev(b) for b in bags]

    def batch(self, idx):
        if self.uniform:
            x = self.data[torch.as_tensor(idx, device=self.device)]
            return x.reshape(-1, x.shape[-1]), BagOffsets.uniform(len(idx), x.shape[1], self.device)
        xs = [self.data[i] for i in idx]
        return torch.cat(xs), BagOffsets.from_lengths([self.lengths[i] for i in idx], self.device)


def _make_optimizer(model, name, lr, wd):
    cls = optim.AdamW if name.lower() == "adamw" else optim.Adam if name.lower() == "adam" else None
    if cls is None:
        raise ValueError(f"Unknown optimizer: {name}")
    return cls(model.parameters(), lr=lr, weight_decay=wd)


def _sync_step(opt, sync, world):
    sync.finish()
    opt.step(grad_scale=1.0 / world)


# ----------------------------------------------------------------------------- validation scored on the device
class _DeviceScores:
    """The ``device_metrics=True`` side of the evaluations below: every chunk's probabilities and per-sample losses are
    copied device-to-device into ``[n, C]`` / ``[n]`` buffers allocated once, the labels are on the device once, and ONE
    ``metrics.class_counts`` call (one launch pair, one read-back, one sync) ends the evaluation -- instead of two ``.cpu()``
    per chunk and scikit-learn on the host (`01:111-113,266-272`, `05:284-302`)."""

    def __init__(self, labels, device):
        self.y = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels), device=device)
        self.y = self.y.to(device=device, dtype=torch.int64)
        self.scores = self.loss = None

    def put(self, lo, probs, loss):
        if self.scores is None:
            n = self.y.shape[0]
            self.scores = torch.empty((n, probs.shape[1]), device=probs.device, dtype=torch.float32)
            self.loss = torch.empty((n,), device=probs.device, dtype=torch.float32)
        self.scores[lo:lo + probs.shape[0]].copy_(probs)
        self.loss[lo:lo + probs.shape[0]].copy_(loss)

    def finish(self):
        from .metrics import class_counts
        return class_counts(self.scores, self.y, self.loss)


# ----------------------------------------------------------------------------- MIL teacher
@torch.no_grad()
def eval_teacher(model, store, labels, chunk=64, device_metrics=False):
    """bag_probs + mean per-bag CE over all bags (`01:247-260`).  ``device_metrics``: -> (``metrics.ClassMetrics``, loss)
    from counts formed on the device; the probabilities never leave it."""
    model.eval()
    probs, losses = [], []
    n = len(labels)
    acc = _DeviceScores(labels, store.device) if device_metrics and n else None
    for lo in range(0, n, chunk):
        idx = list(range(lo, min(n, lo + chunk)))
        x, offs = store.batch(idx)
        out = model(x, offs)
        if acc is not None:
            acc.put(lo, out["bag_probs"], ops.CrossEntropyFn.apply(out["bag_logits"], acc.y[lo:lo + len(idx)], 0)[1])
            continue
        y = torch.as_tensor(np.asarray(labels)[idx], device=x.device)
        losses.append(ops.CrossEntropyFn.apply(out["bag_logits"], y, 0)[1].cpu())
        probs.append(out["bag_probs"].cpu())
    if acc is not None:
        cm = acc.finish()
        return cm, cm.loss
    return torch.cat(probs).numpy(), float(torch.cat(losses).mean()) if losses else float("nan")


def train_teacher_fold(model, train_bags, train_labels, val_bags, val_labels, *, optimizer="adamw", lr=2.2e-4,
                       weight_decay=8.6e-4, epochs=200, patience=8, bags_per_step=1, seed=42, device=None, log=print,
                       metric_fn=None, device_metrics=False):
    """`01_train_mil_teacher.py:203-290` for one fold.  Returns dict(best_state_bacc, best_state_loss,
    history).  Every rank draws the same sampler stream and takes its slice of each step's bags.
    ``device_metrics``: the validation is scored on the device (``eval_teacher``); ``metric_fn`` then receives the
    ``ClassMetrics`` in place of the probabilities."""
    from sklearn.metrics import balanced_accuracy_score
    rank, world = dist_info()
    device = device or next(model.parameters()).device
    tr, va = BagStore(train_bags, device), BagStore(val_bags, device)
    opt = _make_optimizer(model, optimizer, lr, weight_decay)
    ddp.broadcast_parameters(opt.flat.data)
    sync = ddp.GradSync(opt.flat.grad, world_size=world)
    gen = torch.Generator().manual_seed(seed)
    best = {"bacc": -np.inf, "loss": float("inf"), "state_bacc": None, "state_loss": None, "no_improve": 0}
    history = []
    per_step = bags_per_step * world
    for epoch in range(1, epochs + 1):
        model.train()
        order = weighted_sample_indices(train_labels, gen)
        for s in range(0, len(order), per_step):
            glob = order[s:s + per_step]
            lo, hi = ddp.shard_range(len(glob), rank, world)
            mine = glob[lo:hi]
            opt.zero_grad()
            sync.reset()
            if mine:
                x, offs = tr.batch(mine)
                out = model(x, offs)
                y = torch.as_tensor(np.asarray(train_labels)[mine], device=device)
                # mean over the GLOBAL step: local mean * (local / global count), summed by the all-reduce
                loss = ops.cross_entropy(out["bag_logits"], y) * (len(mine) * world / len(glob))
                ops.backward(loss)
            _sync_step(opt, sync, world)
        probs, val_loss = eval_teacher(model, va, val_labels, device_metrics=device_metrics)
        if len(val_labels) == 0:
            break
        if device_metrics:
            bacc = probs.bacc
        else:
            pred = probs.argmax(axis=1)
            bacc = balanced_accuracy_score(np.asarray(val_labels), pred)
        if bacc > best["bacc"] + 1e-6:
            best["bacc"], best["state_bacc"] = bacc, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        if val_loss < best["loss"] - 1e-6:
            best["loss"], best["no_improve"] = val_loss, 0
            best["state_loss"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        else:
            best["no_improve"] += 1
        extra = metric_fn(np.asarray(val_labels), probs) if metric_fn else {}
        history.append({"epoch": epoch, "val_bacc": bacc, "val_loss": val_loss, **extra})
        if rank == 0 and log:
            log(f"    Epoch {epoch:03d}: Val BAcc: {bacc:.4f} (best: {best['bacc']:.4f})  | Val Loss: {val_loss:.4f} "
                f"(best: {best['loss']:.4f} ) | Epochs no improve: {best['no_improve']}/{patience}")
        if best["no_improve"] >= patience:
            break
    return {"best_state_bacc": best["state_bacc"], "best_state_loss": best["state_loss"], "history": history}


@torch.no_grad()
def collect_teacher_outputs(model, bags, labels, image_ids, device, chunk=64):
    """`01_train_mil_teacher.py:69-87`: rows {image_id, label, patch_probs, attention, patch_embeddings}."""
    import pandas as pd
    model.eval()
    store = BagStore(bags, device)
    rows = []
    for lo in range(0, len(bags), chunk):
        idx = list(range(lo, min(len(bags), lo + chunk)))
        x, offs = store.batch(idx)
        out = model(x, offs)
        pp, att = out["patch_probs"].cpu().numpy(), out["attention"].cpu().numpy()
        for j, i in enumerate(idx):
            a, b = int(offs.host[j]), int(offs.host[j + 1])
            rows.append({"image_id": image_ids[i], "label": int(labels[i]), "patch_probs": pp[a:b], "attention": att[a:b],
                         "patch_embeddings": np.asarray(bags[i], dtype=np.float32)})
    return pd.DataFrame(rows)


# ----------------------------------------------------------------------------- configs[1]: bags of image patches
class ImageBagStore:
    """Bags of K image patches + one radiomic vector per bag, resident in HBM (images as bf16: what the encoder's
    first kernel rounds to anyway)."""

    def __init__(self, images, radiomics, labels, device):
        images = torch.as_tensor(images)
        if images.dim() != 5:
            raise ValueError(f"expected images[n, K, 3, H, W], got {tuple(images.shape)}")
        self.images = images.to(device=device, dtype=torch.bfloat16)
        self.radiomics = torch.as_tensor(radiomics, dtype=torch.float32).to(device)
        self.labels = np.asarray(labels)
        self.y_dev = torch.as_tensor(self.labels, device=device)
        self.device = device

    def __len__(self):
        return len(self.labels)

    def batch(self, idx):
        sel = torch.as_tensor(list(idx), device=self.device)
        return self.images[sel], self.radiomics[sel], self.y_dev[sel]


@torch.no_grad()
def eval_milnet(model, store, chunk=64, device_metrics=False):
    """Fused-logit class probabilities and mean per-bag CE over all bags, eval mode (running BatchNorm statistics,
    no dropout) -- the evaluation of `01_train_mil_teacher.py:247-260` for the composed model.  ``device_metrics``:
    -> (``metrics.ClassMetrics``, loss) from counts formed on the device."""
    model.eval()
    probs, losses = [], []
    acc = _DeviceScores(store.y_dev, store.device) if device_metrics and len(store) else None
    for lo in range(0, len(store), chunk):
        img, rad, y = store.batch(range(lo, min(len(store), lo + chunk)))
        out = model(img, rad)
        if acc is not None:
            acc.put(lo, ops.softmax_rows(out["logits"]), ops.CrossEntropyFn.apply(out["logits"], y, 0)[1])
            continue
        losses.append(ops.CrossEntropyFn.apply(out["logits"], y, 0)[1].cpu())
        probs.append(ops.softmax_rows(out["logits"]).cpu())
    if acc is not None:
        cm = acc.finish()
        return cm, cm.loss
    if not probs:
        return np.zeros((0, 0), np.float32), float("nan")
    return torch.cat(probs).numpy(), float(torch.cat(losses).mean())


def train_milnet_fold(model, train_set, val_set, *, optimizer="adamw", lr=2.2e-4, weight_decay=8.6e-4, epochs=200,
                      patience=8, bags_per_step=8, seed=42, num_classes=7, device=None, log=print, device_metrics=False):
    """The 01 loop (`01_train_mil_teacher.py:203-290`) for BASELINE.json configs[1]: ``model.MultiModalMILNet`` (ResNet-18
    patch encoder -> attention-MIL head -> radiomic fusion) trained end to end on bags of image patches.  Class-balanced
    sampler stream (`01:189-193`), ``bags_per_step`` bags per optimizer step and rank (bag-sharded DDP: every rank draws
    the same stream and takes its slice; gradients all-reduced through ``ddp.GradSync`` overlapped with the encoder's
    backward), validation after every epoch -> macro one-vs-rest AUROC / balanced accuracy / loss of the fused logits,
    best states by balanced accuracy and by loss, early stop on the loss (`01:265-290`).
    ``train_set`` / ``val_set`` = (images[n, K, 3, H, W], radiomics[n, R], labels[n]).
    ``device_metrics``: the validation is scored on the device; a history entry then holds the ``ClassMetrics`` under
    ``"metrics"`` and no ``"probs"``."""
    from sklearn.metrics import balanced_accuracy_score
    rank, world = dist_info()
    device = device or next(model.parameters()).device
    tr, va = ImageBagStore(*train_set, device), ImageBagStore(*val_set, device)
    opt = _make_optimizer(model, optimizer, lr, weight_decay)
    ddp.broadcast_parameters(opt.flat.data)
    sync = ddp.GradSync(opt.flat.grad, world_size=world)
    ddp.attach(model.encoder, opt.flat, sync)
    gen = torch.Generator().manual_seed(seed)
    best = {"bacc": -np.inf, "loss": float("inf"), "state_bacc": None, "state_loss": None, "no_improve": 0}
    history = []
    per_step = bags_per_step * world
    snapshot = lambda: {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for epoch in range(1, epochs + 1):
        model.train()
        order = weighted_sample_indices(tr.labels, gen)
        step_losses = []                          # device scalars: read back once per epoch (no sync inside the loop)
        for s in range(0, len(order), per_step):
            glob = order[s:s + per_step]
            lo, hi = ddp.shard_range(len(glob), rank, world)
            mine = glob[lo:hi]
            opt.zero_grad()
            sync.reset()
            if mine:
                img, rad, y = tr.batch(mine)
                with ops.fused_grad_accumulation():
                    out = model(img, rad)
                    loss = model.loss(out, y)
                    step_losses.append(loss.detach())
                    (loss * (len(mine) * world / len(glob))).backward()
            _sync_step(opt, sync, world)
        ddp.average_buffers(model)               # BatchNorm running statistics are per rank during the epoch
        probs, val_loss = eval_milnet(model, va, device_metrics=device_metrics)
        if len(va) == 0:
            break
        if device_metrics:
            m, bacc = {"auc": probs.auc}, probs.bacc
        else:
            m = gnn_metrics(va.labels, probs, num_classes)
            bacc = balanced_accuracy_score(va.labels, probs.argmax(axis=1))
        if bacc > best["bacc"] + 1e-6:
            best["bacc"], best["state_bacc"] = bacc, snapshot()
        if val_loss < best["loss"] - 1e-6:
            best["loss"], best["no_improve"], best["state_loss"] = val_loss, 0, snapshot()
        else:
            best["no_improve"] += 1
        history.append({"epoch": epoch, "val_auc": m["auc"], "val_bacc": bacc, "val_loss": val_loss,
                        **({"metrics": probs} if device_metrics else {"probs": probs}),
                        "train_losses": [float(v) for v in torch.stack(step_losses).cpu()] if step_losses else []})
        if rank == 0 and log:
            log(f"    Epoch {epoch:03d}: Val AUROC: {m['auc']:.4f} | Val BAcc: {bacc:.4f} (best: {best['bacc']:.4f})  | "
                f"Val Loss: {val_loss:.4f} (best: {best['loss']:.4f} ) | Epochs no improve: {best['no_improve']}/{patience}")
        if best["no_improve"] >= patience:
            break
    model.encoder.grad_ready_hook = None
    return {"best_state_bacc": best["state_bacc"], "best_state_loss": best["state_loss"], "history": history}


# ----------------------------------------------------------------------------- patch-graph GNN
# Whether GraphStore(lesion_only=True) assembles its batches out of a ragged stack when the caller does not say
# (DESIGN.md §4 "Lesion-only patch graphs": the measurement behind the value).
RAGGED_STACK_DEFAULT_LESION_ONLY = True


H2_MODE = "h2"                                 # gnn_models._GRAPH_MODE["h2gcn"]: a batch's graph is a graph.TwoHopGraph


class GraphStore:
    """Graph records resident in HBM with their normalised CSR built once (graphs are static across
    epochs; the reference re-uploads x and edge_index every step, `05:340-343`)."""

    def __init__(self, records, device, needs_graph=True, mode="gcn", lesion_only=False, ragged_stack=None, lesion_knn=None,
                 lesion_random=None):
        """``mode``: aggregation of the CSR the model's layers need (``gnn_models._GRAPH_MODE``: 'gcn' =
        self loops + symmetric normalisation, 'sum' = GINConv, 'mean' = SAGEConv), or 'h2' for H2GCN: every batch's graph is a
        ``graph.TwoHopGraph`` (the 1-hop and the exact 2-hop operator).  The pair is built ONCE over the whole record set from a
        'sum'-mode CSR (``graph.two_hop``) and a step is assembled by two ``isic_csr_batch_assemble_ragged`` launches, one per
        operator -- the 2-hop entry count differs from graph to graph, so the equal-size stack does not apply and the ragged
        stack is the default; where it cannot be built (a record of more than 256 or of no nodes) a step builds its pair from
        the concatenated batch.
        ``lesion_only``: every record carries ``"keep"`` (bool [n], the lesion flag of each patch) and the store holds the
        subgraph induced by the kept patches of every record (``graph.induced_subgraphs``: one call over the whole record
        set, ``x`` gathered once; a record without a kept patch keeps all of them).
        ``ragged_stack``: graphs of unequal size are assembled per step by ONE launch out of one CSR built over the whole
        record set (``isic_csr_batch_assemble_ragged``) instead of being rebuilt from concatenated edge lists.  ``None`` =
        ``RAGGED_STACK_DEFAULT_LESION_ONLY`` for a lesion-only store and off otherwise; with ``True`` an equal-size store
        assembles through the ragged entry too.
        ``lesion_knn``: with ``lesion_only``, the records' own ``edge_index`` is ignored and the store holds the k-NN graph
        (k = ``lesion_knn``) built AMONG the kept patches of every record, as the reference builds it on a lesion-only frame
        (`03_build_graphs.py:37-54`: k clamped by the record's own number of kept patches, no edge below 2 of them) -- the
        induced subgraph of a k-NN graph over all patches loses every edge to a background patch.  One top-k launch and one
        edge-list launch over the whole record set (``graph.knn_indices_ragged`` / ``knn_edges_ragged``).
        ``lesion_random``: with ``lesion_only`` (and not together with ``lesion_knn``), the records' own ``edge_index`` is
        ignored and the store holds the reference's random graph (r = ``lesion_random``) built AMONG the kept patches of
        every record, ``_random_edge_index(kept patches, r, record["graph_seed"])`` bit for bit (`03_build_graphs.py:57-78`:
        r clamped by the record's own number of kept patches, no edge below 2 of them) -- of the random graph over all
        patches the induced subgraph keeps a neighbour with probability (kept - 1) / (all - 1) only, so it is no control of
        the same density.  Every record carries ``"graph_seed"`` (int) next to ``"keep"``; two launches over the whole
        record set (``graph.random_graphs_ragged``)."""
        if mode not in GraphBatch.MODES and mode != H2_MODE:
            raise ValueError(f"unknown graph mode '{mode}'")
        if lesion_knn is not None and not lesion_only:
            raise ValueError("GraphStore(lesion_knn=k) rebuilds the k-NN graph among the lesion patches: it needs lesion_only=True")
        if lesion_knn is not None and int(lesion_knn) < 1:
            raise ValueError("GraphStore(lesion_knn=k): k must be >= 1")
        self.lesion_knn = int(lesion_knn) if lesion_knn is not None else None
        if lesion_random is not None and not lesion_only:
            raise ValueError("GraphStore(lesion_random=r) rebuilds the random graph among the lesion patches: it needs lesion_only=True")
        if lesion_random is not None and lesion_knn is not None:
            raise ValueError("GraphStore: lesion_random and lesion_knn exclude each other (one graph per record)")
        if lesion_random is not None and int(lesion_random) < 1:
            raise ValueError("GraphStore(lesion_random=r): r must be >= 1")
        self.lesion_random = int(lesion_random) if lesion_random is not None else None
        self.device, self.records, self.mode = device, records, mode
        def dev_tensor(v, dtype, np_dtype):      # records hold numpy arrays (05:248-270) or tensors already in HBM
            if isinstance(v, torch.Tensor):
                return v.to(device=device, dtype=dtype)
            return torch.as_tensor(np.asarray(v, dtype=np_dtype)).to(device)

        self.x = [dev_tensor(r["x"], torch.float32, np.float32) for r in records]
        self.y = np.asarray([int(r["y"]) for r in records])
        self.ei = [dev_tensor(r["edge_index"], torch.int64, np.int64)
                   if needs_graph and self.lesion_knn is None and self.lesion_random is None and r.get("edge_index") is not None
                   else None for r in records]
        self.needs_graph = needs_graph
        self.lesion_only = bool(lesion_only)
        self._ragged, self._xcat = None, None
        if self.lesion_only and self.lesion_knn is not None:
            self._rebuild_knn_among_lesion()
        elif self.lesion_only and self.lesion_random is not None:
            self._rebuild_random_among_lesion()
        elif self.lesion_only:
            self._restrict_to_lesion(dev_tensor)
        self._want_ragged = ((self.lesion_only and RAGGED_STACK_DEFAULT_LESION_ONLY) or mode == H2_MODE) if ragged_stack is None \
            else bool(ragged_stack)
        # equal-sized graphs (the reference's case): one [G, n, D] tensor, a step's batch is ONE index_select
        self.y_dev = torch.as_tensor(self.y, device=device)
        self._xstack = torch.stack(self.x) if self.x and len({tuple(t.shape) for t in self.x}) == 1 else None
        self._single = {}
        self._chunks = {}          # evaluation chunks (sequential index ranges) repeat every epoch: cached whole
        self._stack = None
        self._build_stack()
        if self._want_ragged:
            self._build_ragged()

    def _make_graph(self, ei, n_nodes, offs):
        """The graph of one batch from its concatenated edge list: a ``GraphBatch`` of the store's mode, or for 'h2' the
        ``TwoHopGraph`` of its 'sum'-mode CSR."""
        if self.mode != H2_MODE:
            return GraphBatch(ei, n_nodes, mode=self.mode)
        from .graph import two_hop
        return two_hop(GraphBatch(ei, n_nodes, mode="sum"), offs)

    def _keep_flags(self, ns):
        """The ``keep`` flags of every record as host bool arrays, checked against the records' node counts ``ns``."""
        keeps = []
        for i, (r, n) in enumerate(zip(self.records, ns)):
            if r.get("keep") is None:
                raise ValueError(f"GraphStore(lesion_only=True): record {i} has no 'keep' flags")
            k = np.asarray(r["keep"].cpu() if isinstance(r["keep"], torch.Tensor) else r["keep"]).reshape(-1) != 0
            if k.size != n:
                raise ValueError(f"GraphStore(lesion_only=True): record {i} has {n} nodes but {k.size} 'keep' flags")
            keeps.append(k)
        return keeps

    def _gather_kept(self):
        """``x`` gathered by ``keep`` once (a record without a kept patch keeps all): fills ``self.x`` / ``self.rows`` /
        ``self._xcat`` as ``_restrict_to_lesion`` fills them and returns (xcat, offsets of the kept patches), or None for
        an empty record set."""
        from .bags import BagOffsets
        dev = self.device
        ns = [int(t.shape[0]) for t in self.x]
        keeps = [k if k.any() else np.ones_like(k) for k in self._keep_flags(ns)]
        if not self.x:
            return None
        noff = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        local = [np.flatnonzero(k) for k in keeps]                            # old local id of every kept node, per record
        n2 = [int(r.size) for r in local]
        rows = torch.as_tensor(np.concatenate(local).astype(np.int64)).to(dev)
        pick = torch.as_tensor(np.concatenate([r + o for r, o in zip(local, noff[:-1])]).astype(np.int64)).to(dev)
        xcat = self._xcat = torch.cat(self.x)[pick]
        self.rows = list(torch.split(rows, n2))
        self.x = list(torch.split(xcat, n2))
        return xcat, BagOffsets.from_lengths(n2, dev)

    def _rebuild_knn_among_lesion(self):
        """Replace every record's graph by the k-NN graph among its kept patches (a record without a kept patch keeps
        all): ``x`` is gathered by ``keep`` once, the neighbours of all records come from one top-k launch over the kept
        rows and the edge lists from one more.  ``self.x`` / ``self.ei`` / ``self.rows`` are filled as
        ``_restrict_to_lesion`` fills them, so every path of the store sees the rebuilt records."""
        from .graph import knn_edges_ragged, knn_indices_ragged
        kept = self._gather_kept()
        if kept is None or not self.needs_graph:
            return
        xcat, offs = kept
        n2 = np.diff(offs.host)
        k = self.lesion_knn
        nn = knn_indices_ragged(xcat, offs, max(1, min(k, offs.max_bag - 1)))
        ei2, eoff = knn_edges_ragged(nn, offs, [k])[k]
        self.ei = [ei2[:, int(eoff[g]):int(eoff[g + 1])] for g in range(len(n2))]

    def _rebuild_random_among_lesion(self):
        """Replace every record's graph by the reference's random graph among its kept patches, seeded by the record's
        ``"graph_seed"`` (a record without a kept patch keeps all): ``x`` is gathered by ``keep`` once and the edge lists
        of all records come from ``graph.random_graphs_ragged``.  ``self.x`` / ``self.ei`` / ``self.rows`` are filled as
        ``_rebuild_knn_among_lesion`` fills them, so every path of the store sees the rebuilt records."""
        from .graph import random_graphs_ragged
        seeds = []
        for i, r in enumerate(self.records):
            if r.get("graph_seed") is None:
                raise ValueError(f"GraphStore(lesion_random=r): record {i} has no 'graph_seed'")
            seeds.append(int(r["graph_seed"]))
        kept = self._gather_kept()
        if kept is None or not self.needs_graph:
            return
        _, offs = kept
        r = self.lesion_random
        ei2, eoff = random_graphs_ragged(seeds, offs, [r])[r]
        self.ei = [ei2[:, int(eoff[g]):int(eoff[g + 1])] for g in range(offs.num_bags)]

    def _restrict_to_lesion(self, dev_tensor):
        """Replace every record's graph by the subgraph its ``keep`` flags induce: the edge lists of all records go through
        ``induced_subgraphs`` in one call, the node features are gathered by its ``rows`` once.  ``self.x`` / ``self.ei``
        become views of the two results, so every path of the store (single graph, slow path, stacks) sees induced records."""
        from .graph import induced_subgraphs
        dev = self.device
        ns = [int(t.shape[0]) for t in self.x]
        keeps = self._keep_flags(ns)
        if not self.x:
            return
        es = [int(e.shape[1]) if e is not None else 0 for e in self.ei]
        noff = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        eoff = np.concatenate([[0], np.cumsum(es)]).astype(np.int64)
        have = [e for e in self.ei if e is not None]
        ei = torch.cat(have, dim=1) if have else torch.empty((2, 0), device=dev, dtype=torch.int64)
        keep = torch.as_tensor(np.concatenate(keeps).astype(np.uint8)).to(dev)
        ei2, eoff2, noff2, rows = induced_subgraphs(ei, eoff, noff, keep)
        sizes = torch.stack([noff2, eoff2]).cpu().numpy()                    # per-graph sizes of the induced records
        n2, e2 = np.diff(sizes[0]).tolist(), np.diff(sizes[1]).tolist()
        start = torch.as_tensor(noff[:-1], device=dev).repeat_interleave(torch.as_tensor(n2, device=dev))
        xcat = self._xcat = torch.cat(self.x)[rows + start]
        self.rows = list(torch.split(rows, n2))                              # old local id of every kept node, per record
        self.x = list(torch.split(xcat, n2))
        parts = torch.split(ei2, e2, dim=1)
        self.ei = [p if e is not None else None for p, e in zip(parts, self.ei)]

    def _build_ragged(self):
        """One ``GraphBatch`` over the whole record set, graphs of any size: graph g owns rows ``node_off[g]:node_off[g+1]``
        and -- rows being stored in order, in both orientations -- slots ``nnz_off[g]:nnz_off[g+1]``, ``nnz_off[g] =
        rowptr[node_off[g]]``.  The CSR keeps its GLOBAL ids; a step's batch is cut out and rebased by one launch.  The
        per-graph sizes are read back once, here; a step computes its prefix sums from them on the host."""
        if not self.needs_graph or not self.x or any(e is None for e in self.ei):
            return
        dev, G = self.device, len(self.x)
        ns = np.asarray([int(t.shape[0]) for t in self.x], dtype=np.int64)
        es = np.asarray([int(e.shape[1]) for e in self.ei], dtype=np.int64)
        noff_h = np.concatenate([[0], np.cumsum(ns)])
        if noff_h[-1] + es.sum() >= 2 ** 31 - 16 or ns.min() < 1:
            return
        noff = torch.as_tensor(noff_h, device=dev)
        ei = torch.cat([e + int(o) for e, o in zip(self.ei, noff_h[:-1])], dim=1)
        def feature_store():                   # the concatenation of all records' x: formed only where a stack is kept
            if self._xstack is not None:
                return self._xstack.view(-1, self._xstack.shape[-1])
            return self._xcat if self._xcat is not None else torch.cat(self.x)

        if self.mode == H2_MODE:
            # the two operators of the whole record set, built once; an operator is symmetric, so its two orientations share
            # their segments by construction
            from .graph import H2_MAX_NODES, two_hop
            if ns.max() > H2_MAX_NODES:
                return
            pair = two_hop(GraphBatch(ei, int(noff_h[-1]), mode="sum"), BagOffsets(noff_h, dev))
            nnz_off = torch.stack([pair.a1.rowptr[noff], pair.a2.rowptr[noff]]).to(torch.int64)
            self._ragged = {"G": G, "pair": pair, "node_off": noff, "nnz_off": nnz_off, "n": ns, "edges": es,
                            "nnz": np.diff(nnz_off.cpu().numpy(), axis=1), "x": feature_store()}
            return
        full = GraphBatch(ei, int(noff_h[-1]), mode=self.mode)
        nnz_off = full.rowptr[noff].to(torch.int64)
        if not bool((full.rowptr_t[noff].to(torch.int64) == nnz_off).all()):
            return                             # the two orientations do not share their segments: no ragged stack
        self._ragged = {"G": G, "graph": full, "node_off": noff, "nnz_off": nnz_off, "n": ns, "edges": es,
                        "nnz": np.diff(nnz_off.cpu().numpy()), "x": feature_store()}

    def _ragged_graph(self, key, want_rows):
        """The batch of the graphs ``key`` (host indices, repeats allowed) out of the ragged stack: ``sel`` and the batch's two
        prefix arrays go up in one copy, one launch writes the seven CSR arrays and the row index.
        -> (offsets, GraphBatch, rows int32 padded for ``ops.linear_rows`` or None)"""
        rg = self._ragged
        sel = np.asarray(key, dtype=np.int64)
        if sel.size and (sel.min() < 0 or sel.max() >= rg["G"]):
            raise IndexError("GraphStore.batch: graph index out of range")
        B = int(sel.size)
        if self.mode == H2_MODE:
            return self._ragged_pair(sel, want_rows)
        up = np.empty(3 * B + 2, dtype=np.int64)                              # sel | node_base [B+1] | nnz_base [B+1]
        up[:B] = sel
        up[B] = up[2 * B + 1] = 0
        np.cumsum(rg["n"][sel], out=up[B + 1:2 * B + 1])
        np.cumsum(rg["nnz"][sel], out=up[2 * B + 2:])
        tn, tz = int(up[2 * B]), int(up[3 * B + 1])
        i32, dev = torch.int32, self.device
        d = torch.from_numpy(up).to(dev)
        full = rg["graph"]
        parts = {"rowptr": torch.empty(tn + 1, device=dev, dtype=i32), "rowptr_t": torch.empty(tn + 1, device=dev, dtype=i32),
                 "col": torch.empty(tz, device=dev, dtype=i32), "col_t": torch.empty(tz, device=dev, dtype=i32),
                 "val": torch.empty(tz, device=dev, dtype=torch.float32), "val_t": torch.empty(tz, device=dev, dtype=torch.float32),
                 "perm_t": torch.empty(tz, device=dev, dtype=i32)}
        rows = torch.empty((tn + 7) // 8 * 8 + 8, device=dev, dtype=i32) if want_rows else None
        call("isic_csr_batch_assemble_ragged", d[:B], d[B:2 * B + 1], d[2 * B + 1:], B, rg["G"], tn, tz, rg["node_off"],
             rg["nnz_off"], full.rowptr, full.rowptr_t, full.col, full.col_t, full.val, full.val_t, full.perm_t,
             parts["rowptr"], parts["rowptr_t"], parts["col"], parts["col_t"], parts["val"], parts["val_t"], parts["perm_t"], rows)
        offs = BagOffsets.from_uploaded(up[B:2 * B + 1], d[B:2 * B + 1])
        return offs, GraphBatch.from_parts(tn, int(rg["edges"][sel].sum()), self.mode, parts), rows

    def _ragged_pair(self, sel, want_rows):
        """``_ragged_graph`` for the 'h2' store: ``sel`` and the batch's three prefix arrays (nodes, entries of A1, entries of
        A2) go up in one copy, and one launch per operator cuts it out of the record set's pair and rebases it.  The store's
        ``_t`` arrays alias its forward ones (an operator is symmetric); the batch's are written as arrays of their own with
        the same content, because the entry's outputs may not overlap."""
        from .graph import SYM_MODE, TwoHopGraph
        rg = self._ragged
        B = int(sel.size)
        up = np.empty(4 * B + 3, dtype=np.int64)                              # sel | node_base | nnz_base of A1 | of A2, [B+1] each
        up[:B] = sel
        up[B] = up[2 * B + 1] = up[3 * B + 2] = 0
        np.cumsum(rg["n"][sel], out=up[B + 1:2 * B + 1])
        np.cumsum(rg["nnz"][0][sel], out=up[2 * B + 2:3 * B + 2])
        np.cumsum(rg["nnz"][1][sel], out=up[3 * B + 3:])
        tn = int(up[2 * B])
        i32, dev = torch.int32, self.device
        d = torch.from_numpy(up).to(dev)
        rows = torch.empty((tn + 7) // 8 * 8 + 8, device=dev, dtype=i32) if want_rows else None
        ops_out = []
        for q, full in enumerate((rg["pair"].a1, rg["pair"].a2)):
            zb = d[(2 + q) * B + 1 + q:(3 + q) * B + 2 + q]
            tz = int(up[(3 + q) * B + 1 + q])
            parts = {"rowptr": torch.empty(tn + 1, device=dev, dtype=i32), "rowptr_t": torch.empty(tn + 1, device=dev, dtype=i32),
                     "col": torch.empty(tz, device=dev, dtype=i32), "col_t": torch.empty(tz, device=dev, dtype=i32),
                     "val": torch.empty(tz, device=dev, dtype=torch.float32),
                     "val_t": torch.empty(tz, device=dev, dtype=torch.float32), "perm_t": torch.empty(tz, device=dev, dtype=i32)}
            call("isic_csr_batch_assemble_ragged", d[:B], d[B:2 * B + 1], zb, B, rg["G"], tn, tz, rg["node_off"], rg["nnz_off"][q],
                 full.rowptr, full.rowptr_t, full.col, full.col_t, full.val, full.val_t, full.perm_t, parts["rowptr"],
                 parts["rowptr_t"], parts["col"], parts["col_t"], parts["val"], parts["val_t"], parts["perm_t"],
                 rows if q == 0 else None)
            ops_out.append(GraphBatch.from_parts(tn, tz, SYM_MODE, parts))
        offs = BagOffsets.from_uploaded(up[B:2 * B + 1], d[B:2 * B + 1])
        return offs, TwoHopGraph(*ops_out), rows

    def _build_stack(self):
        """Graphs are static across epochs, so their normalised CSR is built ONCE: one ``GraphBatch`` launch over
        the whole record set.  When every graph has the same node and edge count (the reference's case: 196
        nodes, k-NN / grid edges) the per-graph pieces are kept as [G, ...] stacks with LOCAL ids, and a step's
        batch is six ``index_select``s plus offsets -- no per-step sort / scan / Python loop over graphs."""
        if not self.needs_graph or not self.x or any(e is None for e in self.ei) or self.mode == H2_MODE:
            return
        ns = {int(t.shape[0]) for t in self.x}
        es = {int(e.shape[1]) for e in self.ei}
        if len(ns) != 1 or len(es) != 1:
            return
        n, G = ns.pop(), len(self.x)
        noff = torch.arange(G, device=self.device, dtype=torch.int64) * n
        ei = (torch.stack(self.ei) + noff.view(G, 1, 1)).permute(1, 0, 2).reshape(2, -1)
        full = GraphBatch(ei, G * n, mode=self.mode)
        rp = full.rowptr.to(torch.int64)
        rpt = full.rowptr_t.to(torch.int64)
        used = int(rp[-1])                     # stored entries (the arrays are allocated for E + n)
        nnz = used // G
        if used != G * nnz or int(rpt[-1]) != used:
            return
        # graph g owns rows [g*n, (g+1)*n) and, because every graph has the same number of stored entries,
        # slots [g*nnz, (g+1)*nnz) of both the CSR and its transpose
        if not (bool((rp[::n] == torch.arange(G + 1, device=self.device) * nnz).all())
                and bool((rpt[::n] == torch.arange(G + 1, device=self.device) * nnz).all())):
            return
        eoff = (torch.arange(G, device=self.device, dtype=torch.int64) * nnz).view(G, 1)
        i32 = torch.int32
        self._stack = {
            "n": n, "nnz": nnz,
            "rowptr": (rp[:-1].view(G, n) - eoff).to(i32), "rowptr_t": (rpt[:-1].view(G, n) - eoff).to(i32),
            "col": (full.col[:used].view(G, nnz).to(torch.int64) - noff.view(G, 1)).to(i32),
            "col_t": (full.col_t[:used].view(G, nnz).to(torch.int64) - noff.view(G, 1)).to(i32),
            "val": full.val[:used].view(G, nnz).clone(), "val_t": full.val_t[:used].view(G, nnz).clone(),
            "perm_t": (full.perm_t[:used].view(G, nnz).to(torch.int64) - eoff).to(i32),
        }

    def _stacked_graph(self, sel, rows_out=None):
        """``sel``: device int64 tensor of graph indices.  ``rows_out``: int32 [>= B*n] that receives, for every node row of the
        batch, its row in the stacked record store (``batch_rows``)."""
        st = self._stack
        n, nnz, B = st["n"], st["nnz"], int(sel.numel())
        i32, dev = torch.int32, self.device
        parts = {"rowptr": torch.empty(B * n + 1, device=dev, dtype=i32), "rowptr_t": torch.empty(B * n + 1, device=dev, dtype=i32),
                 "col": torch.empty(B * nnz, device=dev, dtype=i32), "col_t": torch.empty(B * nnz, device=dev, dtype=i32),
                 "val": torch.empty(B * nnz, device=dev, dtype=torch.float32),
                 "val_t": torch.empty(B * nnz, device=dev, dtype=torch.float32),
                 "perm_t": torch.empty(B * nnz, device=dev, dtype=i32)}
        # ONE launch (graph.hip: csr_batch_assemble_kernel) instead of seven index_selects + offset adds + concatenations
        call("isic_csr_batch_assemble", sel, B, n, nnz, st["rowptr"], st["rowptr_t"], st["col"], st["col_t"], st["val"],
             st["val_t"], st["perm_t"], parts["rowptr"], parts["rowptr_t"], parts["col"], parts["col_t"], parts["val"],
             parts["val_t"], parts["perm_t"], rows_out)
        return GraphBatch.from_parts(B * n, B * (nnz - (n if self.mode == "gcn" else 0)), self.mode, parts)

    def batch_rows(self, idx):
        """The batch WITHOUT gathering its node features: (x_store[G*n, D], rows int32, n_rows, offsets, GraphBatch) with
        batch node row i = x_store[rows[i]] -- for ``GraphMIL(x_store, x_rows=(rows, n_rows), ...)``, whose input projection
        reads through the index (``ops.linear_rows``).  Equal-sized graphs with a stacked CSR and a device index, or a
        ragged stack (graphs of any size, host or device index; x_store[sum n_g, D]); ``None`` otherwise (use ``batch``)."""
        if self._ragged is not None:           # graphs of any size: the feature store is the concatenation of all records' x
            key = idx.tolist() if isinstance(idx, torch.Tensor) else [int(i) for i in idx]      # (a host list costs no read-back)
            offs, graph, rows = self._ragged_graph(key, True)
            return self._ragged["x"], rows, offs.total, offs, graph
        if not (isinstance(idx, torch.Tensor) and idx.is_cuda) or self._xstack is None or self._stack is None or not self.needs_graph:
            return None
        sel = idx.to(torch.int64)
        B, n, D = int(sel.numel()), int(self._xstack.shape[1]), int(self._xstack.shape[2])
        rows = torch.empty((B * n + 7) // 8 * 8 + 8, device=self.device, dtype=torch.int32)
        graph = self._stacked_graph(sel, rows_out=rows)
        return self._xstack.view(-1, D), rows, B * n, BagOffsets.uniform(B, n, self.device), graph

    def batch(self, idx, cache=False):
        """(x[sum n, D], offsets, GraphBatch) of the graphs ``idx`` (a list, or an int64 tensor already on the device:
        no host -> device copy then); ``cache=True`` keeps the result (evaluation chunks, which repeat every epoch)."""
        on_dev = isinstance(idx, torch.Tensor) and idx.is_cuda
        key = None if on_dev else tuple(int(i) for i in idx)
        if cache and key is not None and key in self._chunks:
            return self._chunks[key]
        if not on_dev and len(key) == 1:
            i = key[0]
            n = int(self.x[i].shape[0])
            if self.needs_graph and i not in self._single:
                self._single[i] = self._make_graph(self.ei[i], n, BagOffsets.single(n, self.device))
            return self.x[i], BagOffsets.single(n, self.device), self._single.get(i)
        uniform = self._xstack is not None and (not self.needs_graph or self._stack is not None)
        if self._ragged is not None:
            if on_dev:
                key = tuple(int(i) for i in idx.tolist())
            offs, graph, rows = self._ragged_graph(key, True)
            x = self._ragged["x"].index_select(0, rows[:offs.total])
        elif uniform:
            sel = idx.to(torch.int64) if on_dev else torch.as_tensor(key, device=self.device)
            n, D = int(self._xstack.shape[1]), int(self._xstack.shape[2])
            x = self._xstack[sel].reshape(-1, D)
            offs = BagOffsets.uniform(int(sel.numel()), n, self.device)
            graph = self._stacked_graph(sel) if self.needs_graph else None
        else:
            if on_dev:
                key = tuple(int(i) for i in idx.tolist())
            xs = [self.x[i] for i in key]
            x = torch.cat(xs)
            offs = BagOffsets.from_lengths([int(t.shape[0]) for t in xs], self.device)
            graph = None
            if self.needs_graph:
                ei = torch.cat([self.ei[i] + int(o) for i, o in zip(key, offs.host[:-1])], dim=1)
                graph = self._make_graph(ei, offs.total, offs)
        out = (x, offs, graph)
        if cache and key is not None:
            self._chunks[key] = out
        return out


def gnn_metrics(labels, scores, num_classes):
    """`05_train_gnns.py:284-302` metric set (sklearn, as the reference)."""
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, precision_recall_fscore_support, roc_auc_score
    pred = scores.argmax(axis=1)
    try:
        auc = roc_auc_score(labels, scores, multi_class="ovr", labels=np.arange(num_classes))
    except ValueError:
        auc = float("nan")
    f1 = precision_recall_fscore_support(labels, pred, average="macro", zero_division=0)[2]
    return {"accuracy": accuracy_score(labels, pred), "bacc": balanced_accuracy_score(labels, pred), "auc": auc,
            "macro_f1": f1}


@torch.no_grad()
def evaluate_gnn(model, store, num_classes, chunk=32, device_metrics=False):
    """`05_train_gnns.py:273-302`.  ``device_metrics``: the same keys from counts formed on the device (one read-back per
    evaluation; the AUROC is NaN when a class has no validation sample, where ``gnn_metrics`` gives sklearn's NaN).
    ``store`` decides what is scored: a ``GraphStore(lesion_only=True)`` evaluates the induced graphs, through its ragged stack
    when it has one."""
    model.eval()
    n = len(store.x)
    if n == 0:
        return {k: float("nan") for k in ("loss", "accuracy", "bacc", "auc", "macro_f1")}
    scores, losses = [], []
    acc = _DeviceScores(store.y_dev, store.device) if device_metrics else None
    for lo in range(0, n, chunk):
        idx = list(range(lo, min(n, lo + chunk)))
        x, offs, g = store.batch(idx, cache=True)
        probs, _ = model(x, offsets=offs, graph=g)
        if acc is not None:
            acc.put(lo, probs, ops.CrossEntropyFn.apply(probs, acc.y[lo:lo + len(idx)], 1)[1])
            continue
        y = torch.as_tensor(store.y[idx], device=x.device)
        losses.append(ops.CrossEntropyFn.apply(probs, y, 1)[1].cpu())      # CE(log(p + 1e-9)), 05:282
        scores.append(probs.cpu())
    if acc is not None:
        if probs.shape[1] != num_classes:
            raise ValueError(f"evaluate_gnn: the model scores {probs.shape[1]} classes, num_classes is {num_classes}")
        return acc.finish().as_dict()
    scores = torch.cat(scores).numpy()
    return {"loss": float(torch.cat(losses).mean()), **gnn_metrics(store.y, scores, num_classes)}


def train_gnn_fold(model, train_records, val_records, test_records, *, lr=1e-4, weight_decay=1e-4, epochs=1,
                   patience=16, min_delta=1e-6, graphs_per_step=1, num_classes=7, device=None, rng=None,
                   device_metrics=False, history=None, lesion_only=False, ragged_stack=None, lesion_knn=None,
                   lesion_random=None):
    """`05_train_gnns.py:305-358`: AdamW, epoch order = np.random.permutation, best state by validation
    balanced accuracy.  The class weights of `05:328-331` cancel for single-sample CE and
    batched steps keep the unweighted per-graph mean.  Returns (val_metrics, test_metrics, best_epoch).
    ``device_metrics``: every evaluation is scored on the device (``evaluate_gnn``).  ``history``: a list that receives one
    ``{"epoch", "val_bacc", "val_loss"}`` per epoch.
    ``lesion_only`` / ``ragged_stack``: as ``GraphStore`` takes them, for all three record sets (every record carries
    ``"keep"``; ``lesion_knn=k`` rebuilds the k-NN graph among the kept patches instead of inducing the records' graphs and
    needs ``lesion_only``; ``lesion_random=r`` rebuilds the reference's random graph among them from every record's
    ``"graph_seed"``, needs ``lesion_only`` and excludes ``lesion_knn``).  A ragged batch changes its shapes from step to step, so a captured step (``graphs.CapturedStep``) is not offered
    for it: ragged steps run eagerly."""
    rank, world = dist_info()
    device = device or next(model.parameters()).device
    needs = model.gnn_type != "mlp"
    mode = model.graph_mode or "gcn"
    tr, va, te = (GraphStore(r, device, needs, mode=mode, lesion_only=lesion_only, ragged_stack=ragged_stack,
                             lesion_knn=lesion_knn, lesion_random=lesion_random)
                  for r in (train_records, val_records, test_records))
    ragged = tr._ragged is not None            # its steps index the store with the host list: the batch's sizes are host facts
    opt = optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)
    ddp.broadcast_parameters(opt.flat.data)
    sync = ddp.GradSync(opt.flat.grad, world_size=world)
    rng = rng or np.random
    best_state, best_bacc, no_imp, best_epoch = None, -np.inf, 0, 0
    per_step = graphs_per_step * world
    for epoch in range(1, epochs + 1):
        model.train()
        order = rng.permutation(len(train_records)).tolist()
        order_dev = torch.as_tensor(order, device=device)        # ONE upload per epoch; steps slice it on the device
        for s in range(0, len(order), per_step):
            glob = order[s:s + per_step]
            lo, hi = ddp.shard_range(len(glob), rank, world)
            mine = glob[lo:hi]
            opt.zero_grad()
            sync.reset()
            if mine:
                mine_dev = order_dev[s + lo:s + hi]
                br = tr.batch_rows(mine if ragged else mine_dev) if len(mine) > 1 and hasattr(model, "classifier_light") else None
                if br is not None:                           # stacked graphs: no gather, the projection reads through the index
                    x, rows, n_rows, offs, g = br
                    xr = (rows, n_rows)
                else:
                    x, offs, g = tr.batch(mine_dev if len(mine) > 1 and not ragged else mine)
                    xr = None
                with ops.fused_grad_accumulation():          # zero_grad -> backward -> step: gradients go straight into the flat buffer
                    y = tr.y_dev[mine_dev]
                    w = len(mine) * world / len(glob)
                    if hasattr(model, "classifier_light"):      # GraphMIL: head + loss as one autograd node (two launches)
                        _probs, _att, loss = model(x, offsets=offs, graph=g, labels=y, x_rows=xr)
                    else:
                        probs, _ = model(x, offsets=offs, graph=g)
                        loss = ops.cross_entropy_from_probs(probs, y)
                    ops.backward(loss if w == 1.0 else loss * w)
            _sync_step(opt, sync, world)
        vm = evaluate_gnn(model, va, num_classes, device_metrics=device_metrics)
        if history is not None:
            history.append({"epoch": epoch, "val_bacc": vm["bacc"], "val_loss": vm["loss"]})
        if vm["bacc"] > best_bacc + min_delta:
            best_bacc, no_imp, best_epoch = vm["bacc"], 0, epoch
            best_state = copy.deepcopy(model.state_dict())
        else:
            no_imp += 1
        if no_imp >= patience:
            break
    if best_state is not None:
        model.load_state_dict(best_state)
    return (evaluate_gnn(model, va, num_classes, device_metrics=device_metrics),
            evaluate_gnn(model, te, num_classes, device_metrics=device_metrics), best_epoch)
