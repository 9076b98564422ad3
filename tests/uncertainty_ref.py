"""fp64 numpy restatement of the uncertainty maps and the calibration counts (utils/uncertainty.py, csrc/uncertainty.hip), written
from their definitions; windows, entries, flips and tables are tests/sw_blend_ref.py's.  It shares no code with the package.

A MEMBER is one forward of one model (one Monte-Carlo pass of it) over every entry of the case: its logits are (n, p0, p1, p2, C), the
windows as they went through the network (flipped by their entry's mask).  Per voxel, every covering entry of every member is one
element e of the ensemble, with its own softmax p_e and the blend weight w_e:

    prob = sum w_e p_e / sum w_e        entropy = H(prob)        expected_entropy = sum w_e H(p_e) / sum w_e
    mutual_info = max(0, entropy - expected_entropy)             variance = sum_k max(0, sum w_e p_e[k]^2 / sum w_e - prob[k]^2)
with H(p) = -sum_k p_k ln p_k and 0 ln 0 = 0."""
import numpy as np
import torch

import sw_blend_ref as BR

MAPS = ("label", "prob", "entropy", "expected_entropy", "mutual_info", "variance")


def entropy(p):
    """(C, ...) -> H over axis 0, a zero probability adding nothing"""
    p = np.asarray(p, np.float64)
    return -(p * np.log(np.where(p > 0, p, 1.0))).sum(0)


def moments(members, ents, patch_size, vol_shape, tabs):
    """(score (C, ...), cnt, hsum, sq (C, ...)) in fp64: what dycon_sw_accumulate_moments adds to zeroed maps over all members"""
    W = BR.weight_volume(tabs)
    C = np.asarray(members[0]).shape[-1]
    score, sq = np.zeros((C,) + tuple(vol_shape)), np.zeros((C,) + tuple(vol_shape))
    cnt, hsum = np.zeros(vol_shape), np.zeros(vol_shape)
    for logits in members:
        logits = np.asarray(logits, np.float64)
        for n, (x, y, z, mask) in enumerate(ents):
            p = BR.softmax64(np.moveaxis(logits[n], -1, 0))
            p = np.flip(p, tuple(1 + a for a in range(3) if mask >> a & 1))          # back to the volume's orientation
            sl = (slice(x, x + patch_size[0]), slice(y, y + patch_size[1]), slice(z, z + patch_size[2]))
            score[(slice(None),) + sl] += W * p
            sq[(slice(None),) + sl] += W * p * p
            hsum[sl] += W * entropy(p)
            cnt[sl] += W
    return score, cnt, hsum, sq


def finalize(score, cnt, hsum, sq):
    """the six maps as a dict; voxels with cnt == 0 give nan"""
    with np.errstate(invalid="ignore", divide="ignore"):
        prob = score / cnt
        h, ee = entropy(prob), hsum / cnt
        var = np.maximum(0.0, sq / cnt - prob * prob).sum(0)
    return {"label": prob.argmax(0), "prob": prob, "entropy": h, "expected_entropy": ee, "mutual_info": np.maximum(0.0, h - ee),
            "variance": var}


def maps_from_members(members, ents, patch_size, vol_shape, tabs):
    return finalize(*moments(members, ents, patch_size, vol_shape, tabs))


def single_case(nets, image, stride_xy, stride_z, patch_size, weighting="constant", sigma_scale=0.125, mirror_axes=()):
    """The six maps of one case, cropped to the image.  nets: callables, one per member, each mapping a (1, 1, p0, p1, p2) float32
    tensor to (1, C, p0, p1, p2) logits.  Pad, windows and entries as sw_blend_ref.single_case."""
    image = np.asarray(image, np.float32)
    shape = image.shape
    pads = [(max(p - s, 0) // 2, max(p - s, 0) - max(p - s, 0) // 2) for s, p in zip(shape, patch_size)]
    padded = np.pad(image, pads, mode="constant", constant_values=0)
    ents = BR.entries(BR.windows(padded.shape, patch_size, stride_xy, stride_z), mirror_axes)
    members = [[] for _ in nets]
    for x, y, z, mask in ents:
        win = padded[x:x + patch_size[0], y:y + patch_size[1], z:z + patch_size[2]]
        t = torch.from_numpy(np.ascontiguousarray(np.flip(win, tuple(a for a in range(3) if mask >> a & 1)))[None, None])
        with torch.no_grad():
            for m, net in zip(members, nets):
                m.append(np.moveaxis(net(t)[0].double().cpu().numpy(), 0, -1))
    out = maps_from_members([np.asarray(m) for m in members], ents, patch_size, padded.shape,
                            BR.tables(patch_size, weighting, sigma_scale))
    sl = tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, shape))
    return {k: v[(Ellipsis,) + sl] for k, v in out.items()}


# ---------------------------------------------------------------- calibration
def bin_index(x, K):
    """min(K - 1, (int)(x * (float)K)) with the product in float32; x float32"""
    t = np.asarray(x, np.float32) * np.float32(K)
    assert t.dtype == np.float32
    return np.minimum(K - 1, t.astype(np.int64))


def unc_bin_index(u, u_max, K):
    """min(K - 1, (int)(u / u_max * (float)K)): float32 division, then float32 multiplication"""
    t = (np.asarray(u, np.float32) / np.float32(u_max)) * np.float32(K)
    assert t.dtype == np.float32
    return np.minimum(K - 1, t.astype(np.int64))


def calibration_counts(prob, label, K, mask=None, unc=None, u_max=None):
    """The outputs of dycon_calibration_counts as a dict: int64 n[K], correct[K], n_scored, unc_hist[2][K] (correct, wrong), fp64
    conf_sum[K], brier_sum, nll_sum.  prob (C, ...) float32, label (...) in [0, C)."""
    prob = np.asarray(prob, np.float32)
    C = prob.shape[0]
    p = prob.reshape(C, -1)
    g = np.asarray(label).reshape(-1).astype(np.int64)
    keep = np.ones(g.shape, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    assert ((g[keep] >= 0) & (g[keep] < C)).all()
    p, g = p[:, keep], g[keep]
    c, pred = p.max(0), p.argmax(0)
    b = bin_index(c, K)
    ok = pred == g
    p64 = p.astype(np.float64)
    brier = np.zeros(p.shape[1])
    for k in range(C):
        d = p64[k] - (g == k)
        brier = brier + d * d
    nll = -np.log(np.maximum(p64[g, np.arange(p.shape[1])], 1e-12))
    out = {"n": np.bincount(b, minlength=K), "correct": np.bincount(b[ok], minlength=K), "n_scored": int(keep.sum()),
           "conf_sum": np.bincount(b, weights=c.astype(np.float64), minlength=K), "brier_sum": float(brier.sum()), "nll_sum": float(nll.sum())}
    if unc is not None:
        ub = unc_bin_index(np.asarray(unc, np.float32).reshape(-1)[keep], u_max, K)
        out["unc_hist"] = np.stack([np.bincount(ub[ok], minlength=K), np.bincount(ub[~ok], minlength=K)])
    return out


def ece_mce(n, correct, conf_sum):
    """expected and maximum calibration error of a reliability table (counts, correct counts, confidence sums per bin)"""
    n, correct, conf_sum = (np.asarray(a, np.float64) for a in (n, correct, conf_sum))
    gaps = [(n[b], abs(correct[b] / n[b] - conf_sum[b] / n[b])) for b in range(len(n)) if n[b] > 0]
    total = sum(w for w, _ in gaps)
    return sum(w / total * g for w, g in gaps), max(g for _, g in gaps)


def error_auroc(unc_hist):
    """P(u_wrong > u_right) + P(u_wrong == u_right) / 2 over the binned uncertainties: the area under the ROC curve of 'wrong'"""
    right, wrong = (np.asarray(a, np.float64) for a in unc_hist)
    below = np.concatenate([[0.0], np.cumsum(right)[:-1]])
    return float((wrong * (below + right / 2)).sum() / (right.sum() * wrong.sum()))
