"""Training driver: the counterpart of the reference's train.py on the MI355X path -- its epoch loop (train.py:98-143), its
checkpoint / resume convention (:137-141, :330-339) and its loaders (:353-362), as ONE PROCESS PER GPU instead of nn.DataParallel (:351).

    python -m diffmvs_amd.train_driver --logdir ./ckpt --epochs 16 --batch_size 4 --trainviews 9 --lr 1e-3 --lr_sche onecycle \\
        [--trainpath <tree> --trainlist scans.txt | --synthetic 256] [--resume] [--loadckpt model.ckpt] [--method casdiffmvs]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m diffmvs_amd.train_driver ...

What changes against the reference when the batch is spread over processes instead of DataParallel replicas:
  * `shuffle=True` (train.py:359-360) becomes a RANK-STRIDED sampler: one permutation of the sample indices per epoch, the same on every
    rank (seeded by --seed + epoch), rank r takes elements r, r + world, ...; drop_last like the reference's train loader -- the ranks
    see disjoint samples and the same number of steps;
  * the draws that a single process made from one global RNG must DIFFER between ranks: the source views of a training sample
    (`random.sample(src_views, nviews - 1)`, datasets/dtu.py:125) come from a per-(rank, epoch) `random.Random`, the diffusion step `t` and
    the noise of every refinement stage (models/update.py:432-433) from per-(rank, epoch) torch generators, injected through the model's
    t_source / noise_source hooks;
  * gradients: ONE all-reduce of the flat bucket per step (diffmvs_amd.trainer.Trainer), then the identical clip + AdamW on every rank --
    parameters stay bit-identical across ranks; BatchNorm running statistics stay per rank, rank 0's are saved (DataParallel keeps
    replica 0's, train.py:139 saves model.module);
  * rank 0 writes `<logdir>/model_{epoch:06d}.ckpt` = {'epoch', 'model', 'optimizer'} every --save_freq epochs; --resume loads the
    highest-numbered one on every rank (train.py:330-339) and continues the LR schedule where it stopped.
Samples follow the dict contract of the reference's training datasets (datasets/dtu.py:196-210: imgs, proj_matrices, depth_values, depth
and mask per stage); `TreeTrainSet` reads them from an MVS tree with ground-truth depth maps, `SyntheticTrainSet` renders them.

Validation (train.py:144-162, :234-291): with --valpath / --vallist or --val_synthetic N a held-out pass runs after the checkpoint step of every
--eval_freq-th epoch and of the last one (`validate`): model.eval(), no_grad, the eval forward of the current weights, the initial depth scored
against stage1 (`init_abs_depth_error`) and the final depth against stage4 (`final_depth_error`, plus abs-rel, RMSE and inlier shares) by
diffmvs_amd.depth_eval -- integer rows per sample.  Determinism rules: samples are dealt rank-strided in index order, nothing is dropped, the source
views are the first val_views - 1 of the pair list (no draw), the diffusion noise of sample i comes from a host generator seeded by (seed, i)
alone and the batch tensor is assembled item by item, the ranks all_gather (sample index, integer rows) and the summary is computed from the rows
sorted by index: the record is the same for any world size and any --val_batch_size.  Rank 0 appends it to <logdir>/val.jsonl (with
`best_epoch`, the epoch of the lowest final_depth_error so far; no extra *.ckpt is written -- --resume parses every *.ckpt name as an epoch).
The pass uses its own generators, leaves the global RNG alone, keeps HIP graphs off, and puts model.train() and the epoch's stream hooks back.
The reference also reports the LOSS of the held-out batch.  This pass does not, although it could: the eval forward of a `test=False` model
returns every iterate in "depth" and the Unet confidences in "conf" (diffmvs_amd.engine.Engine.forward), which is what compute_inverse_loss
takes.  It is left out because that loss is an fp32 mean over the batch: to keep the record independent of --val_batch_size and of the
world size it would have to be evaluated sample by sample and reduced like the rows, which nobody has asked for yet."""
from __future__ import annotations

import argparse
import json
import os
import random
import time
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import formats as IO
from . import shard, synth

_STAGES = (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1))


# ------------------------------------------------------------------------------------------ datasets
class SyntheticTrainSet:
    """`n` rendered scenes (diffmvs_amd.synth: one slanted textured plane seen from `pool` + 1 cameras, ground-truth depth of the reference
    view per stage).  A sample = the reference view + nviews - 1 source views DRAWN from the pool by the caller's generator."""

    def __init__(self, n: int, H: int, W: int, nviews: int, pool: int | None = None, seed: int = 0, numdepth: int = 384):
        self.n, self.H, self.W, self.nviews, self.numdepth, self.seed = n, H, W, nviews, numdepth, seed
        self.pool = max(pool or (nviews + 1), nviews - 1)
        self._cache: Dict[int, tuple] = {}

    def __len__(self):
        return self.n

    def get(self, idx: int, rng: random.Random) -> dict:
        if idx not in self._cache:
            if len(self._cache) > 64:
                self._cache.clear()
            self._cache[idx] = synth.synth_inputs(self.H, self.W, self.pool, B=1, seed=self.seed + idx, numdepth=self.numdepth, with_gt=True)
        imgs, proj, dv, gt, mask = self._cache[idx]
        # datasets/dtu.py:125; rng None (validation): no draw, the first nviews - 1 source views
        ids = [0] + (list(range(1, self.nviews)) if rng is None else sorted(rng.sample(range(1, self.pool + 1), self.nviews - 1)))
        return {"imgs": [imgs[v][0] for v in ids], "proj_matrices": {k: p[0, ids] for k, p in proj.items()}, "depth_values": dv[0],
                "depth": {k: g[0] for k, g in gt.items()}, "mask": {k: m[0] for k, m in mask.items()}, "index": idx, "view_ids": ids}


class TreeTrainSet:
    """An MVS tree in the evaluation layout (diffmvs_amd.formats.MVSDataset: <root>/<scan>/{images, cams_1 | cams, pair.txt}) that also holds
    `depth_gt/%08d.pfm` (and optionally `mask/%08d.png`) for its reference views.  Multi-scale ground truth like datasets/dtu.py:100-112:
    nearest-neighbour subsampling by 8 / 4 / 2 / 1; the mask defaults to `depth_min < depth < depth_max`."""

    def __init__(self, root: str, scans: Sequence[str], nviews: int, numdepth: int = 384, dataset: str = "general"):
        self.ds = IO.MVSDataset(root, nviews, numdepth, dataset=dataset, scan=list(scans))
        self.root, self.nviews = root, nviews
        self.items = []
        for i, (scan, ref, srcs) in enumerate(self.ds.metas):
            base = os.path.join(root, scan) if dataset != "general" else root
            if os.path.exists(os.path.join(base, "depth_gt", f"{ref:08d}.pfm")) and len(srcs) >= nviews - 1:
                self.items.append((i, base))

    def __len__(self):
        return len(self.items)

    def get(self, idx: int, rng: random.Random) -> dict:
        i, base = self.items[idx]
        scan, ref, srcs = self.ds.metas[i]
        # datasets/dtu.py:125; rng None (validation): no draw, the first nviews - 1 of the pair list
        ids = [ref] + (list(srcs)[:self.nviews - 1] if rng is None else rng.sample(list(srcs), self.nviews - 1))
        loaded = [self.ds.load_view(scan, v) for v in ids]
        s = IO.make_sample([x[0] for x in loaded], [x[1] for x in loaded], [x[2] for x in loaded], loaded[0][3], loaded[0][4], self.ds.numdepth)
        depth = np.ascontiguousarray(IO.read_pfm(os.path.join(base, "depth_gt", f"{ref:08d}.pfm"))[0]).astype(np.float32)
        H, W = loaded[0][0].shape[:2]
        if depth.shape != (H, W):
            raise ValueError(f"{base}/depth_gt/{ref:08d}.pfm: {depth.shape} does not match the image {(H, W)}")
        mfile = os.path.join(base, "mask", f"{ref:08d}.png")
        if os.path.exists(mfile):
            from PIL import Image
            m = (np.array(Image.open(mfile).convert("L")) > 10).astype(np.float32)
        else:
            m = ((depth > loaded[0][3]) & (depth < loaded[0][4])).astype(np.float32)
        out = {"imgs": [torch.from_numpy(a) for a in s["imgs"]], "proj_matrices": {k: torch.from_numpy(p) for k, p in s["proj_matrices"].items()},
               "depth_values": torch.from_numpy(s["depth_values"]), "depth": {}, "mask": {}, "index": idx, "view_ids": ids}
        for name, f in _STAGES:
            out["depth"][name] = torch.from_numpy(np.ascontiguousarray(depth[::f, ::f]))
            out["mask"][name] = torch.from_numpy(np.ascontiguousarray(m[::f, ::f]))
        return out


def collate_train(samples: Sequence[dict], device) -> dict:
    """what default_collate makes of a list of training samples (train.py:359), moved to the device (tocuda, train.py:184)"""
    V = len(samples[0]["imgs"])
    st = lambda xs: torch.stack(list(xs)).to(device)  # noqa: E731
    return {"imgs": [st(s["imgs"][v] for s in samples) for v in range(V)],
            "proj_matrices": {k: st(s["proj_matrices"][k] for s in samples) for k in samples[0]["proj_matrices"]},
            "depth_values": st(s["depth_values"] for s in samples),
            "depth": {k: st(s["depth"][k] for s in samples) for k in samples[0]["depth"]},
            "mask": {k: st(s["mask"][k] for s in samples) for k in samples[0]["mask"]}}


# ------------------------------------------------------------------------------------------ sampler and per-rank streams
class RankStridedSampler:
    """DistributedSampler semantics for the reference's `shuffle=True, drop_last=True` train loader (train.py:359-360): the permutation of
    an epoch is a function of (seed, epoch) only -- identical on every rank -- and rank r owns positions r, r + world, ... of its first
    `world * (n // world)` entries, so the ranks' samples are disjoint and equally many."""

    def __init__(self, n: int, rank: int, world: int, seed: int = 0, shuffle: bool = True):
        if not (0 <= rank < world):
            raise ValueError(f"rank {rank} outside world {world}")
        self.n, self.rank, self.world, self.seed, self.shuffle = n, rank, world, seed, shuffle

    def indices(self, epoch: int) -> List[int]:
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + epoch)
            perm = torch.randperm(self.n, generator=g).tolist()
        else:
            perm = list(range(self.n))
        return perm[self.rank:self.world * (self.n // self.world):self.world]

    def batches(self, epoch: int, batch_size: int) -> List[List[int]]:
        idx = self.indices(epoch)
        return [idx[i:i + batch_size] for i in range(0, len(idx) - batch_size + 1, batch_size)]      # drop_last


class RankStreams:
    """The random draws of one (rank, epoch): source views (python), diffusion step t (host generator), stage noise (device generator).
    Distinct per rank -- under the reference's single process they all came from one global stream -- and re-creatable on resume."""

    def __init__(self, seed: int, rank: int, epoch: int, device):
        base = (seed * 1000003 + rank * 7919 + epoch * 104729) & 0x7FFFFFFF
        self.views = random.Random(base + 1)
        self.t_gen = torch.Generator().manual_seed(base + 2)
        self.noise_gen = torch.Generator(device=device).manual_seed(base + 3)
        self.device = torch.device(device)
        self.t_log: List[List[int]] = []

    def t_source(self, B, T, device):
        t = torch.randint(0, T, (B,), generator=self.t_gen)
        self.t_log.append(t.tolist())
        return t.to(device).long()

    def noise_source(self, shape, device):
        return torch.randn(shape, generator=self.noise_gen, device=self.device).to(device)

    def install(self, model):
        model.t_source, model.noise_source = self.t_source, self.noise_source


# ------------------------------------------------------------------------------------------ validation
VAL_THRESHOLDS = (2.0, 4.0, 8.0)


class SampleNoise:
    """The diffusion noise of a validation batch: item b of every draw comes from a HOST generator seeded by (seed, sample index) alone, so
    a sample sees the same noise in any batch, on any rank and on any device."""

    def __init__(self, seed: int, idxs: Sequence[int]):
        self.gens = [torch.Generator().manual_seed(((seed * 1000003 + i * 7919 + 5) ^ 0x5DEECE66D) & 0x7FFFFFFFFFFF) for i in idxs]

    def __call__(self, shape, device):
        if shape[0] != len(self.gens):
            raise ValueError(f"noise for a batch of {shape[0]} asked of {len(self.gens)} sample streams")
        return torch.stack([torch.randn(tuple(shape[1:]), generator=g) for g in self.gens]).to(device)


def validate(model, ds, ops, device, seed: int = 0, batch_size: int = 1, rank: int = 0, world: int = 1, thresholds=VAL_THRESHOLDS) -> dict:
    """One held-out pass over `ds` with the model's CURRENT weights (train.py:144-162, :234-291) -> the validation record without its
    epoch / step / seconds, identical on every rank and for every (world, batch_size): see the module docstring.  Collective when world > 1.
    Leaves the model as it found it: training flag, noise / t hooks, graph switch."""
    from . import depth_eval
    was_training, hooks, graphs = model.training, (model.noise_source, model.t_source), model.hip_graphs
    width = depth_eval.HEAD + depth_eval.SLOTS + len(thresholds)
    mine = list(range(rank, len(ds), world))                                               # rank-strided, in order, nothing dropped
    rows, kept = [], []
    try:
        if world > 1:
            # BatchNorm running statistics stay per rank while training and rank 0's are the ones saved: every rank validates the model
            # the checkpoint holds, then takes its own statistics back
            import torch.distributed as dist
            for b in model.buffers():
                kept.append(b.detach().clone())
                dist.broadcast(b, src=0)
        model.eval()
        model.hip_graphs = False
        with torch.no_grad():
            for i0 in range(0, len(mine), batch_size):
                idxs = mine[i0:i0 + batch_size]
                batch = collate_train([ds.get(i, None) for i in idxs], device)
                model.noise_source = SampleNoise(seed, idxs)
                out = model(batch["imgs"], batch["proj_matrices"], batch["depth_values"])      # through model.engine(): re-packed after a step
                big = (1.0 / batch["depth_values"][:, 0].double()).tolist()                 # the sample's depth_max
                init = depth_eval.score(ops, out["depth"][0], batch["depth"]["stage1"], batch["mask"]["stage1"], thresholds, big=big)
                final = depth_eval.score(ops, out["depth"][-1], batch["depth"]["stage4"], batch["mask"]["stage4"], thresholds, big=big)
                index = torch.tensor(idxs, dtype=torch.int64, device=init.device)[:, None]
                rows.append(torch.cat([index, init, final], 1))
    finally:
        with torch.no_grad():
            for b, k in zip(model.buffers(), kept):
                b.copy_(k)
        model.noise_source, model.t_source = hooks
        model.hip_graphs = graphs
        model.train(was_training)
    per_rank = (len(ds) + world - 1) // world
    table = torch.full((per_rank, 1 + 2 * width), -1, dtype=torch.int64, device=ops.device)    # padded with index -1: equal sizes for the gather
    if rows:
        got = torch.cat(rows)
        table[:got.shape[0]] = got
    if world > 1:
        import torch.distributed as dist
        parts = [torch.empty_like(table) for _ in range(world)]
        dist.all_gather(parts, table)
        table = torch.cat(parts)
    host = sorted((r for r in table.cpu().tolist() if r[0] >= 0), key=lambda r: r[0])          # the one readback; sample order
    init = depth_eval.summarise([r[1:1 + width] for r in host], thresholds)
    final = depth_eval.summarise([r[1 + width:] for r in host], thresholds)
    rec = {"samples": len(host), "init_abs_depth_error": init["abs_err"], "final_depth_error": final["abs_err"], "final_abs_rel": final["abs_rel"],
           "final_rmse": final["rmse"]}
    rec.update({"final_" + k: v for k, v in final.items() if k.startswith("inlier_")})
    rec.update(init=init, final=final)
    return rec


def build_val_dataset(a):
    """the held-out set of --valpath / --vallist or --val_synthetic (None: no validation)"""
    views = a.val_views or a.trainviews
    if a.valpath:
        scans = [""]
        if a.vallist:
            with open(a.vallist) as f:
                scans = [ln.strip() for ln in f if ln.strip()]
        return TreeTrainSet(a.valpath, scans, views, a.numdepth, dataset=a.dataset)
    if a.val_synthetic:
        # scene i of a synthetic set is rendered from seed + i: the held-out scenes start right past the last training scene
        return SyntheticTrainSet(a.val_synthetic, a.height, a.width, views, pool=a.view_pool, seed=a.seed + max(a.synthetic, 0), numdepth=a.numdepth)
    return None


def _read_val_log(path: str, before_epoch: int) -> List[dict]:
    if not os.path.exists(path):
        return []
    with open(path) as f:
        recs = [json.loads(ln) for ln in f if ln.strip()]
    return [r for r in recs if r.get("epoch", 0) < before_epoch]


# ------------------------------------------------------------------------------------------ the loop
def latest_checkpoint(logdir: str):
    """train.py:330-335: the highest-numbered *.ckpt of the log directory"""
    if not os.path.isdir(logdir):
        return None
    saved = sorted((fn for fn in os.listdir(logdir) if fn.endswith(".ckpt")), key=lambda x: int(x.split("_")[-1].split(".")[0]))
    return os.path.join(logdir, saved[-1]) if saved else None


def build_dataset(a):
    if a.trainpath:
        scans = [""]
        if a.trainlist:
            with open(a.trainlist) as f:
                scans = [ln.strip() for ln in f if ln.strip()]
        return TreeTrainSet(a.trainpath, scans, a.trainviews, a.numdepth, dataset=a.dataset)
    return SyntheticTrainSet(a.synthetic, a.height, a.width, a.trainviews, pool=a.view_pool, seed=a.seed, numdepth=a.numdepth)


def run(a, device=None, ops=None) -> dict:
    from models import CasDiffMVS
    from .trainer import Trainer, parse_lrepochs
    rank, world, local = shard.env_rank_world()
    if device is None:
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    if world > 1:
        shard.init_distributed(a.backend, device if str(device).startswith("cuda") else None)
    margs = synth.make_args("casdiffmvs" if a.method == "casdiffmvs" else "diffmvs", numdepth_initial=a.numdepth_initial, numdepth=a.numdepth)
    model = CasDiffMVS(margs, test=False)
    if a.loadckpt:
        model.load_state_dict(torch.load(a.loadckpt, map_location="cpu")["model"])             # train.py:340-344 (strict)
    elif a.init == "synthetic":
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), 123 + (0 if a.same_init else rank)), strict=True)
    # (--init default: the modules' own initialisation, like the reference's train.py; the Trainer broadcasts rank 0's)
    model.to(device)
    ds = build_dataset(a)
    if a.eval_freq < 1 or a.val_batch_size < 1:
        raise SystemExit(f"train_driver: --eval_freq {a.eval_freq} and --val_batch_size {a.val_batch_size} must be at least 1")
    val_ds = build_val_dataset(a)
    if val_ds is not None and len(val_ds) == 0:
        raise SystemExit("train_driver: the validation set is empty (no reference view with depth_gt/ and enough source views)")
    sampler = RankStridedSampler(len(ds), rank, world, seed=a.seed)
    steps_per_epoch = len(sampler.batches(0, a.batch_size))
    if steps_per_epoch == 0:
        raise SystemExit(f"train_driver: {len(ds)} samples are fewer than one batch of {a.batch_size} on each of {world} ranks")
    kw = {}
    if a.lr_sche == "onecycle":
        kw["total_steps"] = steps_per_epoch * a.epochs + 100                                   # train.py:374
    elif a.lr_sche == "mslr":
        ms, gamma = parse_lrepochs(a.lrepochs)
        kw.update(milestones=ms, lr_gamma=gamma, steps_per_epoch=steps_per_epoch)
    tr = Trainer(model, margs, ops=ops, lr=a.lr, wd=a.wd, **kw)                                # broadcasts rank 0's weights and buffers
    start_epoch = 0
    if a.resume:
        ck = latest_checkpoint(a.logdir)
        if ck is None:
            raise SystemExit(f"--resume: no *.ckpt in {a.logdir}")
        start_epoch = tr.load_checkpoint(torch.load(ck, map_location=device))
        tr.step_count = steps_per_epoch * start_epoch                                          # the schedule continues where the epoch count says
    log = {"rank": rank, "world": world, "steps_per_epoch": steps_per_epoch, "start_epoch": start_epoch, "seen": [], "view_draws": [],
           "t_draws": [], "loss": [], "lr": []}
    val_file = os.path.join(a.logdir, "val.jsonl")
    if val_ds is not None:
        log["val"] = []
        # rank 0 owns the file (the other ranks may not even see it): it alone reads the earlier records and names the best epoch.  On
        # --resume the records of epochs that are trained again are dropped, so the file holds every epoch once
        earlier = _read_val_log(val_file, start_epoch) if a.resume and rank == 0 else []
        if a.resume and rank == 0 and os.path.exists(val_file):
            with open(val_file, "w") as f:
                f.writelines(json.dumps(r) + "\n" for r in earlier)
    for epoch in range(start_epoch, a.epochs):
        streams = RankStreams(a.seed, rank, epoch, device)
        streams.install(model)
        seen, draws = [], []
        for bi, idxs in enumerate(sampler.batches(epoch, a.batch_size)):
            t0 = time.time()
            samples = [ds.get(i, streams.views) for i in idxs]
            seen += idxs
            draws += [s["view_ids"] for s in samples]
            lr = tr.current_lr()
            loss, parts, gnorm, _ = tr.train_sample(collate_train(samples, device))
            log["loss"].append(float(loss))
            log["lr"].append(lr)
            if rank == 0 and not a.quiet:
                print("Epoch {}/{}, Iter {}/{}, lr {:.6f}, train loss = {:.3f}, grad norm = {:.3f}, time = {:.3f}".format(
                    epoch, a.epochs, bi, steps_per_epoch, lr, float(loss), float(gnorm), time.time() - t0), flush=True)
        log["seen"].append(seen)
        log["view_draws"].append(draws)
        log["t_draws"].append(streams.t_log)
        if (epoch + 1) % a.save_freq == 0 and rank == 0:                                       # train.py:136-141
            os.makedirs(a.logdir, exist_ok=True)
            torch.save(tr.checkpoint(epoch), os.path.join(a.logdir, "model_{:0>6}.ckpt".format(epoch)))
        if val_ds is not None and (epoch % a.eval_freq == 0 or epoch == a.epochs - 1):         # train.py:145
            t0 = time.time()
            rec = validate(model, val_ds, tr.ops, device, seed=a.seed, batch_size=a.val_batch_size, rank=rank, world=world)
            streams.install(model)                                                             # (validate restored them; the epoch's hooks stay)
            rec = {"epoch": epoch, "step": tr.step_count, **rec, "seconds": time.time() - t0}
            best = None
            if rank == 0:
                known = [r for r in earlier + log["val"] + [rec] if r["final_depth_error"] is not None]
                best = min(known, key=lambda r: (r["final_depth_error"], r["epoch"]))["epoch"] if known else None
            if world > 1:
                import torch.distributed as dist
                box = [best]
                dist.broadcast_object_list(box, src=0)
                best = box[0]
            rec["best_epoch"] = best
            log["val"].append(rec)
            if rank == 0:
                os.makedirs(a.logdir, exist_ok=True)
                with open(val_file, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                fin = rec["final"]
                hidden = "".join(f", {k} {v}" for k, v in (("left_out", rec["init"]["left_out"] + fin["left_out"]),
                                                          ("saturated", rec["init"]["saturated"] + fin["saturated"]),
                                                          ("empty_items", rec["init"]["empty_items"] + fin["empty_items"])) if v)
                fmt = lambda v: "nan" if v is None else "{:.4f}".format(v)  # noqa: E731
                print("Epoch {}/{}, validation on {} samples: init_abs_depth_error = {}, final_depth_error = {}, abs_rel = {}, best epoch {}{}, "
                      "time = {:.3f}".format(epoch, a.epochs, rec["samples"], fmt(rec["init_abs_depth_error"]), fmt(rec["final_depth_error"]),
                                             fmt(rec["final_abs_rel"]), rec["best_epoch"], hidden, rec["seconds"]), flush=True)
    flat = tr.flat.data.detach().double().cpu()
    log["weights_sum"], log["weights_abs_sum"], log["steps_done"] = float(flat.sum()), float(flat.abs().sum()), tr.step_count
    if world > 1:
        import torch.distributed as dist
        gathered = [torch.zeros_like(tr.flat.data) for _ in range(world)]
        dist.all_gather(gathered, tr.flat.data)
        log["weights_identical_across_ranks"] = bool(all(torch.equal(gathered[0], g) for g in gathered))
        dist.barrier()
    return log


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--logdir", default="./checkpoints/debug", help="checkpoint directory (train.py --logdir)")
    ap.add_argument("--resume", action="store_true", help="continue from the highest-numbered checkpoint of --logdir (train.py:330-339)")
    ap.add_argument("--loadckpt", default=None, help="initial weights: a reference checkpoint ({'model': state_dict})")
    ap.add_argument("--method", default="casdiffmvs", choices=["casdiffmvs", "diffmvs"])
    ap.add_argument("--trainpath", default=None, help="MVS tree with depth_gt/ (TreeTrainSet); default: --synthetic scenes")
    ap.add_argument("--trainlist", default=None)
    ap.add_argument("--dataset", default="general", choices=["dtu", "tank", "eth3d", "general"])
    ap.add_argument("--synthetic", type=int, default=64, help="number of rendered scenes when no --trainpath is given")
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--view_pool", type=int, default=None, help="source views rendered per synthetic scene (the draw picks trainviews - 1 of them)")
    ap.add_argument("--trainviews", type=int, default=9, help="images per sample: 1 reference + trainviews - 1 sources (scripts/train/*.sh)")
    ap.add_argument("--numdepth", type=int, default=384)
    ap.add_argument("--numdepth_initial", type=int, default=48)
    ap.add_argument("--epochs", type=int, default=16)
    ap.add_argument("--batch_size", type=int, default=4, help="per GPU (the reference's DataParallel split its batch ACROSS the GPUs)")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--wd", type=float, default=1e-3)
    ap.add_argument("--lr_sche", default="onecycle", choices=["onecycle", "mslr", "const"])
    ap.add_argument("--lrepochs", default="10,12,14:2")
    ap.add_argument("--save_freq", type=int, default=1)
    ap.add_argument("--init", default="synthetic", choices=["synthetic", "default"],
                    help="initial weights without --loadckpt.  synthetic (default): synth.synth_state_dict, the seeded weights of this package's tests and "
                         "benchmarks; default: the modules' own initialisation, as the reference's train.py -- what a REAL training run wants")
    ap.add_argument("--valpath", default=None, help="held-out MVS tree with depth_gt/ (the layout of --trainpath): validate during training")
    ap.add_argument("--vallist", default=None, help="scans of --valpath, one per line")
    ap.add_argument("--val_synthetic", type=int, default=0, help="validate on this many rendered scenes (seeds disjoint from the training scenes')")
    ap.add_argument("--eval_freq", type=int, default=1, help="validate every N-th epoch and after the last (train.py --eval_freq); needs a validation set")
    ap.add_argument("--val_batch_size", type=int, default=1, help="per GPU; the validation record does not depend on it")
    ap.add_argument("--val_views", type=int, default=None, help="images per validation sample (default: --trainviews); the first val_views - 1 of the pair list")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--same_init", type=int, default=1, help=argparse.SUPPRESS)       # 0: per-rank initial weights (test of the broadcast)
    ap.add_argument("--backend", default="nccl", help=argparse.SUPPRESS)
    ap.add_argument("--quiet", action="store_true")
    return ap.parse_args(argv)


def main(argv=None):
    log = run(parse_args(argv))
    print("TRAIN_DRIVER " + json.dumps({k: v for k, v in log.items() if k not in ("view_draws", "t_draws")}), flush=True)
    return log


if __name__ == "__main__":
    main()
