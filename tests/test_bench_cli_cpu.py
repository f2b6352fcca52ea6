"""bench.py's command line and its --dump-outputs writer, on the CPU: a plain run is the headline
alone (--full is off by default), and dump_outputs writes losses, gradients and parameters as .npy
within its byte budget, with the same seeded sample every time."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    args = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert args.full and args.dump_outputs == "somewhere"


def _step_state():
    torch.manual_seed(0)
    model = torch.nn.Linear(8, 4)
    item_matrix = torch.nn.Parameter(torch.randn(300, 128))
    (model(torch.randn(3, 8)).sum() + item_matrix[:7].square().sum()).backward()
    model.bias.grad = None  # a parameter the step left without a gradient
    return model, item_matrix


def test_dump_outputs_writes_losses_params_and_grads(tmp_path):
    model, item_matrix = _step_state()
    bench.dump_outputs(str(tmp_path / "out"), model, item_matrix, (torch.tensor(3.5), torch.tensor(3.0), 0.5))
    names = sorted(os.listdir(tmp_path / "out"))
    assert names == sorted(["losses.npy"] + [f"{k}.{n}.npy" for k in ("param", "grad")
                                             for n in ("weight", "bias", "item_matrix")])
    losses = np.load(tmp_path / "out" / "losses.npy")
    assert losses.dtype == np.float64 and losses.tolist() == [3.5, 3.0, 0.5]
    w = np.load(tmp_path / "out" / "param.weight.npy")
    assert w.dtype == np.float32 and np.array_equal(w, model.weight.detach().numpy())
    assert np.array_equal(np.load(tmp_path / "out" / "grad.item_matrix.npy"), item_matrix.grad.numpy())
    assert not np.load(tmp_path / "out" / "grad.bias.npy").any()


def test_dump_outputs_samples_large_arrays_into_the_budget(tmp_path, monkeypatch):
    model, item_matrix = _step_state()
    monkeypatch.setattr(bench, "DUMP_SMALL_BYTES", 1024)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)  # the two 153,600-byte arrays do not fit
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, item_matrix, (1.0, 1.0, 0.0))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 100_000
    a, b = (np.load(tmp_path / d / "param.item_matrix.npy") for d in ("a", "b"))
    assert a.ndim == 1 and 0 < a.size < item_matrix.numel() and np.array_equal(a, b)
    keep = np.sort(np.random.default_rng(0).choice(item_matrix.numel(), a.size, replace=False))
    assert np.array_equal(a, item_matrix.detach().numpy().reshape(-1)[keep])
    # small arrays stay whole
    assert np.load(tmp_path / "a" / "param.weight.npy").shape == (4, 8)
