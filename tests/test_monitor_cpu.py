"""utils.monitor without a GPU: the workspace query is host-only and linear in B*N; CPU tensors are refused with a clear error."""
import pytest
import torch

from dycon_paper_replication_amd import _lib


def test_simhist_workspace_is_linear():
    lib = _lib.load()
    w = lib.dycon_simhist_workspace(2, 15680, 256, 50)
    assert 2 * 15680 * 4 <= w <= 2 * 15680 * 4 + 64          # inverse norms + the min / max slots: no N^2 term
    assert lib.dycon_simhist_workspace(2, 2 * 15680, 256, 50) - w == 2 * 15680 * 4
    assert lib.dycon_simhist_workspace(1, 1, 16, 1) > 0


def test_monitor_refuses_cpu_tensors(tmp_path):
    from dycon_paper_replication_amd.utils import monitor
    from dycon_paper_replication_amd import ops
    feat, mask = torch.randn(2, 8, 16), torch.zeros(2, 1, 8)
    with pytest.raises(ValueError, match="CUDA"):
        monitor.monitor_similarity_distributions(feat, mask, 0, str(tmp_path))
    with pytest.raises(ValueError, match="CUDA"):
        ops.similarity_histograms(feat, mask)
    assert not list(tmp_path.iterdir())
