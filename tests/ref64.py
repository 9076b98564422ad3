"""fp64 references of the convolutions and normalisations of the step, for the element-wise parity tests.

The convolutions take channels-last (B, D, H, W, C) tensors, as the engine does, and form y, gx, gw and gb explicitly as sums over
the taps of one matmul / einsum each (no autograd graph): at 96^3 with B = 8 that keeps the memory at a few GB, and the same code
runs on the GPU (the parity tests) and on the CPU (test_parity_helpers_cpu.py holds it to F.conv3d / F.conv_transpose3d autograd).
Weights keep torch's layouts: Conv3d (Co, Ci, k, k, k), ConvTranspose3d (Ci, Co, 2, 2, 2).
"""
import torch
import torch.nn.functional as F

KSIZE = {"k3": 3, "k2s2": 2, "deconv": 2, "1x1": 1}


def _taps(k):
    return [(i, j, l) for i in range(k) for j in range(k) for l in range(k)]


def _mm(a, b):
    """(..., K) @ (K, N) over the leading dimensions"""
    return (a.reshape(-1, a.shape[-1]) @ b).reshape(a.shape[:-1] + (b.shape[-1],))


def _k2_view(t):
    """(B, 2D, 2H, 2W, C) -> (B, D, 2, H, 2, W, 2, C)"""
    B, D, H, W, C = t.shape
    assert D % 2 == 0 and H % 2 == 0 and W % 2 == 0, "k2s2 / transposed k2s2 need even extents"
    return t.reshape(B, D // 2, 2, H // 2, 2, W // 2, 2, C)


def conv_ref64(kind, x, w, b, gy):
    """y = conv(x) + b and its gradients for the output gradient gy, all in float64.  Returns (y, gx, gw, gb)."""
    x, w, b, gy = x.double(), w.double(), b.double(), gy.double()
    B, D, H, W, Ci = x.shape
    if kind == "k3":                            # y[p] = sum_t x[p + t - 1] W_t^T ; gx[q] = sum_t gy[q - t + 1] W_t
        Co = w.shape[0]
        xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
        gp = F.pad(gy, (0, 0, 1, 1, 1, 1, 1, 1))
        y = b.expand(B, D, H, W, Co).clone()
        gx = torch.zeros_like(x)
        gw = torch.empty_like(w)
        for i, j, l in _taps(3):
            wt = w[:, :, i, j, l]                                   # (Co, Ci)
            xs = xp[:, i:i + D, j:j + H, l:l + W, :]
            y += _mm(xs, wt.t())
            gx += _mm(gp[:, 2 - i:2 - i + D, 2 - j:2 - j + H, 2 - l:2 - l + W, :], wt)
            gw[:, :, i, j, l] = torch.einsum("bdhwo,bdhwc->oc", gy, xs)
    elif kind == "k2s2":                        # y[m] = sum_t x[2m + t] W_t^T
        Co = w.shape[0]
        xv = _k2_view(x)
        y = b.expand(B, D // 2, H // 2, W // 2, Co).clone()
        gxv = torch.zeros_like(xv)
        gw = torch.empty_like(w)
        for i, j, l in _taps(2):
            wt = w[:, :, i, j, l]
            xs = xv[:, :, i, :, j, :, l, :]
            y += _mm(xs, wt.t())
            gxv[:, :, i, :, j, :, l, :] = _mm(gy, wt)
            gw[:, :, i, j, l] = torch.einsum("bdhwo,bdhwc->oc", gy, xs)
        gx = gxv.reshape(x.shape)
    elif kind == "deconv":                      # y[2m + t] = x[m] W_t (W_t: (Ci, Co))
        Co = w.shape[1]
        y = b.expand(B, 2 * D, 2 * H, 2 * W, Co).clone()
        yv = _k2_view(y)
        gv = _k2_view(gy)
        gx = torch.zeros_like(x)
        gw = torch.empty_like(w)
        for i, j, l in _taps(2):
            wt = w[:, :, i, j, l]                                   # (Ci, Co)
            yv[:, :, i, :, j, :, l, :] += _mm(x, wt)
            gs = gv[:, :, i, :, j, :, l, :]
            gx += _mm(gs, wt.t())
            gw[:, :, i, j, l] = torch.einsum("bdhwc,bdhwo->co", x, gs)
    elif kind == "1x1":
        wt = w[:, :, 0, 0, 0]
        y = _mm(x, wt.t()) + b
        gx = _mm(gy, wt)
        gw = torch.einsum("bdhwo,bdhwc->oc", gy, x).reshape(w.shape)
    else:
        raise ValueError(kind)
    gb = gy.reshape(-1, gy.shape[-1]).sum(0)
    return y, gx, gw, gb


def norm_ref64(kind, z, gy, gamma=None, beta=None, relu=True, skip=None, chan_scale=None, running=None, training=True, groups=16,
               eps=1e-5, momentum=0.1):
    """norm -> [ReLU] -> [x chan_scale per (sample, channel)] -> [+ skip] in float64 through torch autograd, channels-last in and out.
    kind: gn (GroupNorm(groups)) | in (InstanceNorm, no affine) | bn (BatchNorm; `running` = (mean, var) is updated in place when
    training, read when not).  Returns (y, gz, dgamma, dbeta, gskip)."""
    z = z.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    g64 = gamma.double().requires_grad_(True) if gamma is not None else None
    b64 = beta.double().requires_grad_(True) if beta is not None else None
    if kind == "gn":
        n = F.group_norm(z, groups, g64, b64, eps)
    elif kind == "in":
        n = F.instance_norm(z, eps=eps)
    elif kind == "bn":
        rm, rv = running if running is not None else (None, None)
        n = F.batch_norm(z, rm, rv, g64, b64, training, momentum, eps)
    else:
        raise ValueError(kind)
    y = F.relu(n) if relu else n
    if chan_scale is not None:
        y = y * chan_scale.double().reshape(z.shape[0], z.shape[1], 1, 1, 1)
    if skip is not None:
        y = y + skip.double().permute(0, 4, 1, 2, 3)
    y.backward(gy.double().permute(0, 4, 1, 2, 3))
    cl = lambda t: t.permute(0, 2, 3, 4, 1)     # noqa: E731
    gskip = gy.double() if skip is not None else None
    return (cl(y.detach()), cl(z.grad), g64.grad if g64 is not None else None, b64.grad if b64 is not None else None, gskip)
