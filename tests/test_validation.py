"""The held-out pass of diffmvs_amd.train_driver (reference train.py:144-162, :234-291): it leaves training bit for bit alone, scores the
CURRENT weights, and its record does not depend on the validation batch size or on the number of ranks; --resume still finds its checkpoint.
Smallest model and image the driver's own tests train at (DiffMVS, 32 x 64, 2 views, 8 initial depths), on the host emulation; one gpu-marked
test repeats the first two checks on the real library."""
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, emu_ops
from diffmvs_amd import train_driver as TD

BASE = ["--method", "diffmvs", "--synthetic", "1", "--height", "32", "--width", "64", "--trainviews", "2", "--view_pool", "4",
        "--numdepth_initial", "8", "--batch_size", "1", "--lr_sche", "onecycle", "--quiet", "--seed", "11"]
VAL = ["--val_synthetic", "3", "--eval_freq", "1"]
TIMELESS = lambda rec: {k: v for k, v in rec.items() if k not in ("seconds", "epoch", "step", "best_epoch")}  # noqa: E731


def _run(argv, device=None, ops=None):
    return TD.run(TD.parse_args(argv), device=device, ops=ops)


def _same_training(a, b):
    for k in ("loss", "lr", "t_draws", "weights_sum", "weights_abs_sum", "seen", "view_draws", "steps_done"):
        assert a[k] == b[k], k


def _same_checkpoint(fa, fb):
    ca, cb = torch.load(fa, map_location="cpu"), torch.load(fb, map_location="cpu")
    assert ca["epoch"] == cb["epoch"] and list(ca["model"]) == list(cb["model"])
    for k in ca["model"]:
        assert torch.equal(ca["model"][k], cb["model"][k]), k
    for i, st in ca["optimizer"]["state"].items():
        assert torch.equal(st["exp_avg"], cb["optimizer"]["state"][i]["exp_avg"]) and torch.equal(st["exp_avg_sq"], cb["optimizer"]["state"][i]["exp_avg_sq"])


def _fresh_validate(ckpt, ops, device, batch_size=1, extra=()):
    """the record of a NEW model loaded from a checkpoint file, on the samples and noise of `--val_synthetic 3 --seed 11`"""
    from diffmvs_amd import synth
    from models import CasDiffMVS
    a = TD.parse_args(BASE + VAL + list(extra))
    model = CasDiffMVS(synth.make_args("diffmvs", numdepth_initial=a.numdepth_initial, numdepth=a.numdepth), test=False)
    model.load_state_dict(torch.load(ckpt, map_location="cpu")["model"])
    model.to(device)
    return TD.validate(model, TD.build_val_dataset(a), ops, device, seed=a.seed, batch_size=batch_size)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the same 2 epochs x 1 step three times on the host emulation: without validation, with it at batch 1, with it at batch 2"""
    from diffmvs_amd.ops import Ops
    old = Ops.__dict__["for_device"]
    Ops.for_device = classmethod(lambda cls, device: emu_ops())
    try:
        root = tmp_path_factory.mktemp("val")
        cpu = torch.device("cpu")
        out = {"root": root}
        for name, extra in (("plain", []), ("val1", VAL + ["--val_batch_size", "1"]), ("val2", VAL + ["--val_batch_size", "2"])):
            out[name] = _run(BASE + ["--epochs", "2", "--logdir", str(root / name)] + extra, cpu, emu_ops())
        yield out
    finally:
        Ops.for_device = old


def test_validation_leaves_training_untouched(runs):
    plain, val = runs["plain"], runs["val1"]
    assert "val" not in plain and len(val["val"]) == 2 and len(plain["loss"]) == 2
    _same_training(plain, val)
    for e in (0, 1):
        _same_checkpoint(runs["root"] / "plain" / f"model_{e:06d}.ckpt", runs["root"] / "val1" / f"model_{e:06d}.ckpt")
    assert not os.path.exists(runs["root"] / "plain" / "val.jsonl")


def test_the_pass_scores_the_current_weights(runs, monkeypatch):
    from conftest import pin_ops
    pin_ops(monkeypatch, emu_ops())
    r0, r1 = runs["val1"]["val"]
    assert (r0["epoch"], r1["epoch"]) == (0, 1) and (r0["step"], r1["step"]) == (1, 2) and r0["samples"] == r1["samples"] == 3
    assert TIMELESS(r0) != TIMELESS(r1) and r0["final"]["scored"] == r1["final"]["scored"] > 0
    for r in (r0, r1):
        assert r["final_depth_error"] == r["final"]["abs_err"] > 0 and r["init_abs_depth_error"] == r["init"]["abs_err"] > 0
        assert 0 < r["final_abs_rel"] < 1 and 0 <= r["final_inlier_2"] <= r["final_inlier_4"] <= r["final_inlier_8"] <= 1
        assert 0 < r["init"]["scored"] <= 3 * 4 * 8 and 0 < r["final"]["scored"] <= 3 * 32 * 64      # stage1 is 1/8 of stage4 per side
    assert r1["best_epoch"] == min((r0, r1), key=lambda r: r["final_depth_error"])["epoch"]
    fresh = _fresh_validate(runs["root"] / "val1" / "model_000001.ckpt", emu_ops(), torch.device("cpu"))
    assert fresh == TIMELESS(r1)
    lines = [json.loads(ln) for ln in open(runs["root"] / "val1" / "val.jsonl")]
    assert lines == runs["val1"]["val"]


def test_the_record_does_not_depend_on_the_validation_batch(runs):
    """3 samples at batch 2: the last batch is partial"""
    _same_training(runs["val1"], runs["val2"])
    assert [TIMELESS(r) for r in runs["val1"]["val"]] == [TIMELESS(r) for r in runs["val2"]["val"]]
    assert [r["best_epoch"] for r in runs["val1"]["val"]] == [r["best_epoch"] for r in runs["val2"]["val"]]


def test_resume_still_finds_the_highest_checkpoint(runs, monkeypatch):
    from conftest import pin_ops
    pin_ops(monkeypatch, emu_ops())
    logdir = runs["root"] / "val1"
    assert sorted(os.listdir(logdir)) == ["model_000000.ckpt", "model_000001.ckpt", "val.jsonl"]
    assert TD.latest_checkpoint(str(logdir)).endswith("model_000001.ckpt")
    log = _run(BASE + VAL + ["--epochs", "3", "--logdir", str(logdir), "--resume"], torch.device("cpu"), emu_ops())
    assert log["start_epoch"] == 2 and len(log["loss"]) == 1 and [r["epoch"] for r in log["val"]] == [2]
    assert sorted(os.listdir(logdir)) == ["model_000000.ckpt", "model_000001.ckpt", "model_000002.ckpt", "val.jsonl"]
    lines = [json.loads(ln) for ln in open(logdir / "val.jsonl")]
    assert [r["epoch"] for r in lines] == [0, 1, 2]
    assert lines[2]["best_epoch"] == min(lines, key=lambda r: (r["final_depth_error"], r["epoch"]))["epoch"]      # the earlier records count


def test_init_default_keeps_the_modules_own_weights(monkeypatch):
    """--init default: no synthetic state dict is loaded (the reference's train.py starts like this); synthetic stays the default"""
    from diffmvs_amd import synth
    assert TD.parse_args([]).init == "synthetic" and TD.parse_args(["--init", "default"]).init == "default"
    calls = []
    real = synth.synth_state_dict
    monkeypatch.setattr(synth, "synth_state_dict", lambda *a, **k: calls.append(1) or real(*a, **k))

    class Stop(Exception):
        pass

    def stop(a):
        raise Stop
    monkeypatch.setattr(TD, "build_dataset", stop)                  # the weights are set before the dataset is built: stop there
    for init, n in (("default", 0), ("synthetic", 1)):
        calls.clear()
        with pytest.raises(Stop):
            _run(BASE + ["--init", init], torch.device("cpu"), emu_ops())
        assert len(calls) == n, init


_WORKER = r"""
import os, sys, json, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
from conftest import emu_ops
from diffmvs_amd.ops import Ops
Ops.for_device = classmethod(lambda cls, device: emu_ops())      # this CPU worker runs the package on the host emulation
from diffmvs_amd import train_driver as TD
torch.set_num_threads(2)
log = TD.run(TD.parse_args({argv!r}), device=torch.device("cpu"), ops=emu_ops())
print("RESULT " + json.dumps({{"rank": log["rank"], "val": log["val"], "identical": log["weights_identical_across_ranks"]}}), flush=True)
import torch.distributed as dist
dist.destroy_process_group()
"""


def test_the_record_does_not_depend_on_the_world_size(tmp_path, monkeypatch):
    """two ranks over gloo on the host emulation (the pattern of test_train_driver): one epoch of one step per rank, then the pass over 3
    samples dealt 2 + 1.  Both ranks hold the same record, rank 0 alone wrote val.jsonl, and ONE process validating the checkpoint that
    run saved (at batch 2: another split again) gets the same record."""
    from conftest import pin_ops
    logdir = tmp_path / "ckpt"
    argv = BASE + VAL + ["--synthetic", "2", "--epochs", "1", "--logdir", str(logdir), "--backend", "gloo", "--same_init", "0"]
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, argv=argv))
    port = 29500 + (os.getpid() % 2000) + 11
    procs = [subprocess.Popen([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                                       OMP_NUM_THREADS="2")) for r in range(2)]
    res = {}
    for p in procs:
        try:
            out, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        assert p.returncode == 0, out[-3000:]
        r = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res[r["rank"]] = r
    assert res[0]["identical"] and len(res[0]["val"]) == 1
    assert TIMELESS(res[0]["val"][0]) == TIMELESS(res[1]["val"][0]) and res[0]["val"][0]["samples"] == 3
    assert sorted(os.listdir(logdir)) == ["model_000000.ckpt", "val.jsonl"]
    lines = [json.loads(ln) for ln in open(logdir / "val.jsonl")]
    assert len(lines) == 1 and lines[0] == res[0]["val"][0]                                # one writer
    pin_ops(monkeypatch, emu_ops())
    assert _fresh_validate(logdir / "model_000000.ckpt", emu_ops(), torch.device("cpu"), batch_size=2, extra=["--synthetic", "2"]) == TIMELESS(res[0]["val"][0])


@pytest.mark.gpu
def test_validation_on_the_device_leaves_training_untouched_and_scores_the_current_weights(tmp_path, monkeypatch):
    """the first two checks on the real library, 2 epochs x 2 steps.  Two training runs on the device do not agree to the last bit with or
    without validation -- the warp backward scatters with fp32 atomics (tests/test_trainer.py allows 1e-3 on the gradient norm of two
    identical steps) -- so "untouched" is checked where it is decidable: everything a pass could disturb (parameters, gradients, Adam
    moments, step count, buffers, the epoch's generators, the global CPU and device RNG, the training flag, the stream hooks) is bit for
    bit the same after every pass as before it, and against a run without the pass the quantities that are deterministic on the device
    (learning rates, samples, view and diffusion-step draws, the loss of the first step) are equal."""
    from conftest import hip_ops
    from diffmvs_amd import trainer as TR
    trainers, passes = [], []

    class Recording(TR.Trainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            trainers.append(self)
    monkeypatch.setattr(TR, "Trainer", Recording)
    real = TD.validate

    def snapshot(model):
        tr = trainers[-1]
        ts = [tr.flat.data, tr.flat.grad, tr.exp_avg, tr.exp_avg_sq, tr.sumsq] + list(model.buffers())
        return ([t.detach().clone() for t in ts], tr.step_count, torch.get_rng_state(), torch.cuda.get_rng_state(0), model.training,
                model.noise_source, model.t_source, model.noise_source.__self__.noise_gen.get_state(), model.t_source.__self__.t_gen.get_state(),
                model.hip_graphs)

    def checked(model, *a, **k):
        before = snapshot(model)
        rec = real(model, *a, **k)
        torch.cuda.synchronize()
        after = snapshot(model)
        assert all(torch.equal(x, y) for x, y in zip(before[0], after[0])) and before[1] == after[1]
        assert torch.equal(before[2], after[2]) and torch.equal(before[3], after[3]) and after[4] is True and before[4] is True
        assert after[5] is not None and before[5] == after[5] and before[6] == after[6]
        assert torch.equal(before[7], after[7]) and torch.equal(before[8], after[8]) and before[9] == after[9]
        passes.append(rec)
        return rec
    monkeypatch.setattr(TD, "validate", checked)
    argv = BASE + ["--synthetic", "2", "--epochs", "2"]
    plain = _run(argv + ["--logdir", str(tmp_path / "plain")])
    val = _run(argv + VAL + ["--val_batch_size", "2", "--logdir", str(tmp_path / "val")])
    assert len(passes) == 2 and "val" not in plain
    for k in ("lr", "t_draws", "seen", "view_draws", "steps_done"):
        assert plain[k] == val[k], k
    assert plain["loss"][0] == val["loss"][0] and len(val["loss"]) == 4
    assert sorted(os.listdir(tmp_path / "val")) == ["model_000000.ckpt", "model_000001.ckpt", "val.jsonl"]
    r0, r1 = val["val"]
    assert TIMELESS(r0) != TIMELESS(r1) and r1["samples"] == 3 and r1["final_depth_error"] > 0 and r1["step"] == 4
    monkeypatch.setattr(TD, "validate", real)
    for bs in (1, 3):
        assert _fresh_validate(tmp_path / "val" / "model_000001.ckpt", hip_ops(), torch.device("cuda", 0), batch_size=bs, extra=["--synthetic", "2"]) == TIMELESS(r1), bs


def test_eval_freq_below_one_is_refused():
    for flag in ("--eval_freq", "--val_batch_size"):
        with pytest.raises(SystemExit, match="at least 1"):
            _run(BASE + VAL + [flag, "0"], torch.device("cpu"), emu_ops())
