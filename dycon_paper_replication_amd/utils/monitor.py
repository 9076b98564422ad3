"""utils.monitor of the reference (code/utils/monitor.py): the positive- / negative-pair similarity histograms its training loops
draw every 200 iterations (train_DyCON_BraTS19.py:333-343, train_DyCON_Pancreas.py:240).

The histograms come from ops.similarity_histograms: Gram tiles recomputed on the GPU and binned on chip, so neither the (B, N, N)
similarity matrix nor its masks exist and only 2 x bins counts reach the host.  Drawing uses a matplotlib Figure on the Agg canvas
directly, so the caller's pyplot state and backend are left alone.
"""
from __future__ import annotations

import os

from .. import ops


def monitor_similarity_distributions(feat, mask, epoch, path_prefix="../misc/similarity_plots/", tau=0.6, bins=50, plot=True):
    """feat (B, N, D) embeddings, mask (B, 1, N) or (B, N) labels (monitor.py:7-50).  Saves
    `{path_prefix}/epoch_{epoch}_similarity_distributions.png` (positive pairs left in green, negative right in red) when `plot`,
    and returns numpy (counts[2, bins] int64, edges[2, bins + 1] float32), row 0 positive, row 1 negative."""
    counts, edges, _ = ops.similarity_histograms(feat, mask, tau=tau, bins=bins)
    counts, edges = counts.cpu().numpy(), edges.cpu().numpy()
    if plot:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure

        fig = Figure(figsize=(10, 4))
        FigureCanvasAgg(fig)
        for k, (title, color) in enumerate((("Positive Pair Similarities", "green"), ("Negative Pair Similarities", "red"))):
            ax = fig.add_subplot(1, 2, k + 1)
            ax.hist(edges[k][:-1], bins=edges[k], weights=counts[k], alpha=0.7, color=color)
            ax.set_title(title)
            ax.set_xlabel("Similarity")
            ax.set_ylabel("Frequency")
        fig.tight_layout()
        os.makedirs(path_prefix, exist_ok=True)
        fig.savefig(os.path.join(path_prefix, f"epoch_{epoch}_similarity_distributions.png"))
    return counts, edges
