"""CPU, bench.py --dump-outputs: file set, dtypes, the seeded sample of large arrays (logical element order) and the size budget."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bench


class _Trainer:
    """the two state_dict accessors dump_outputs reads, with an integer buffer that must be left out"""

    def __init__(self):
        self.sd = OrderedDict(w=torch.arange(6.0).reshape(2, 3), n=torch.tensor(3), b=torch.tensor([7.0]))

    def state_dict(self):
        return self.sd

    def teacher_state_dict(self):
        return OrderedDict((k, -v) for k, v in self.sd.items())


def _out():
    g = torch.Generator().manual_seed(0)
    return {"loss": torch.tensor(1.5), "grad_sumsq": torch.tensor([2.0], dtype=torch.float64), "beta": 5.0, "skipped": False,
            "s_logits": torch.randn(2, 5, 3, 4, generator=g).bfloat16().permute(0, 3, 1, 2),      # non-contiguous bf16
            "mask": torch.tensor([[0, 1], [1, 1]], dtype=torch.uint8)}


def test_dump_outputs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP", 16)
    out = _out()
    bench.dump_outputs(out, _Trainer(), str(tmp_path / "a"))
    bench.dump_outputs(out, _Trainer(), str(tmp_path / "b"))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(k + ".npy" for k in list(out) + ["student_weights", "teacher_weights"])
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    ld = lambda n: np.load(tmp_path / "a" / (n + ".npy"))      # noqa: E731
    assert ld("loss").dtype == np.float32 and ld("loss") == 1.5
    assert ld("grad_sumsq").dtype == np.float64 and ld("beta").dtype == np.float64 and ld("skipped") == 0.0
    assert ld("mask").dtype == np.float32 and ld("mask").shape == (2, 2)
    np.testing.assert_array_equal(ld("student_weights"), [0, 1, 2, 3, 4, 5, 7])
    np.testing.assert_array_equal(ld("teacher_weights"), [0, -1, -2, -3, -4, -5, -7])
    logits = out["s_logits"].float().reshape(-1).numpy()                                   # 40 elements > DUMP_CAP
    pos = np.sort(np.random.default_rng(0).choice(logits.size, 16, replace=False))
    assert ld("s_logits").dtype == np.float32
    np.testing.assert_array_equal(ld("s_logits"), logits[pos])


def test_dump_outputs_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64)
    with pytest.raises(SystemExit):
        bench.dump_outputs(_out(), _Trainer(), str(tmp_path / "d"))
    assert not (tmp_path / "d").exists()
