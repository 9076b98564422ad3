"""CPU tests of the host side: C-ABI surface, state_dict contract, schedules, loud failure without a GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.engine import param_spec, projection_buffers
from dycon_paper_replication_amd.networks import net_factory_3d
from dycon_paper_replication_amd.trainer import TrainConfig
from dycon_paper_replication_amd.utils import dycon_losses, ramps
from oracle import nets as ON


def test_abi_surface_matches_header():
    """every function declared in include/dycon_hip.h is exported by the library and bound with a prototype"""
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    declared = set(re.findall(r"\b(dycon_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.dycon_version() >= 100
    assert lib.dycon_last_error() is not None
    # pure host-side queries are callable without a GPU
    assert lib.dycon_bfrag_bytes(_lib.BF16, 27, 16, 16) == 14 * 1 * 64 * 16
    assert lib.dycon_bfrag_bytes(_lib.F32, 27, 16, 16) == 27 * 1 * 64 * 16
    assert lib.dycon_fecl_workspace(4, 1728, 256) >= 5 * 4 * 1728 * 4
    assert lib.dycon_conv_gemm_workspace(_lib.BF16, _lib.CONV_K3, 0, 4, 96, 96, 96, 16, 16) == 0       # big level: no split-K
    assert lib.dycon_conv_gemm_workspace(_lib.BF16, _lib.CONV_K3, 0, 4, 6, 6, 6, 256, 256) > 0        # 6^3 level: split-K slabs


@pytest.mark.parametrize("kind", ["vnet", "unet"])
def test_state_dict_contract(kind):
    """parameter names / order / shapes equal the reference modules' (names recorded from the reference in the fixtures)"""
    net_type = "vnet" if kind == "vnet" else "unet_3D"
    ref_names = list(load_golden(f"step_{kind}")["param_names"])      # from reference named_parameters()
    spec = param_spec(net_type)
    assert list(spec) == ref_names
    oracle = (ON.make_vnet_params if kind == "vnet" else ON.make_unet_params)(0)
    m = net_factory_3d(net_type, 1, 2, 2)
    sd = m.state_dict()
    assert list(sd) == list(oracle)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(oracle[k].shape), k
    assert [k for k, _ in m.named_parameters()] == ref_names
    n = sum(p.numel() for p in m.parameters())
    head = sum(int(np.prod(s)) for k, s in spec.items() if k.startswith("projection."))
    assert (n - head == 9448866) if kind == "vnet" else (n == 6148532)
    m.load_state_dict(oracle)                                               # reference-shaped checkpoint loads
    assert list(projection_buffers()) == [k for k in oracle if k not in spec]


def test_no_cpu_fallback():
    m = net_factory_3d("vnet", 1, 2, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 16, 16, 16))
    assert net_factory_3d("nope") is None
    with pytest.raises(NotImplementedError):
        net_factory_3d("unet_3D", use_aspp=True)


def test_schedules_match_reference_tables():
    tab = json.load(open(os.path.join(GOLDEN, "schedules.json")))
    for e, tot, mx, mn, v in tab["adaptive_beta"]:
        assert dycon_losses.adaptive_beta(e, tot, mx, mn) == pytest.approx(v, rel=1e-12)
    for e, R, lo, hi, v in tab["threshold_rampup"]:
        assert dycon_losses.sigmoid_rampup(e, R, lo, hi) == pytest.approx(v, rel=1e-12)
    for c, R, v in tab["consistency_rampup"]:
        assert ramps.sigmoid_rampup(c, R) == pytest.approx(v, rel=1e-12)


def test_train_config_defaults_are_the_reference_flags():
    c = TrainConfig()
    assert (c.max_iterations, c.batch_size, c.labeled_bs, c.base_lr, c.ema_decay) == (20000, 8, 4, 0.01, 0.99)
    assert (c.consistency, c.consistency_type, c.consistency_rampup, c.gamma) == (0.1, "mse", 200.0, 2.0)
    assert (c.beta_min, c.beta_max, c.s_beta, c.temp, c.l_weight, c.u_weight) == (0.5, 5.0, None, 0.6, 1.0, 0.5)
    assert (c.use_focal, c.use_teacher_loss, c.feature_scaler, c.seed) == (1, 1, 2, 1337)


@pytest.mark.parametrize("norm", ["groupnorm", "instancenorm", "batchnorm", "none"])
def test_vnet_param_spec_all_normalizations(norm):
    """state_dict keys / shapes / order of the V-Net for each of the reference's normalisation options (VNet.py:17-24: the
    nn.Sequential index step is 3 with a norm module, 2 without; InstanceNorm3d has no affine parameters) -- against the
    oracle's builder, which test_oracle_golden pins to the reference modules."""
    from dycon_paper_replication_amd.engine import net_buffers
    spec = param_spec("vnet", normalization=norm)
    ref = ON.trainable(ON.make_vnet_params(1, normalization=norm))
    assert list(spec) == list(ref)
    assert all(tuple(spec[k]) == tuple(ref[k].shape) for k in spec)
    net = net_factory_3d("vnet", 1, 2, 2, normalization=norm)
    assert [k for k, _ in net.named_parameters()] == list(spec)
    bufs = [k for k, _ in net.named_buffers()]
    assert bufs == list(net_buffers("vnet", norm))
    assert ("block_one.conv.1.running_mean" in bufs) == (norm == "batchnorm")


def test_step_has_no_outside_switches():
    """Nothing in a step can be changed from outside the process: the package reads the environment in ONE place (DYCON_LIB in _lib.py:
    which shared library is loaded, not what a step does), and the switches TrainConfig offers are exactly the ones written down here."""
    import dataclasses
    pkg = os.path.join(ROOT, "dycon_paper_replication_amd")
    hits = []
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                path = os.path.join(d, f)
                hits += [(os.path.relpath(path, pkg), line.strip()) for line in open(path) if "environ" in line or "getenv" in line]
    assert len(hits) == 1 and hits[0][0] == "_lib.py" and hits[0][1].startswith('LIB_PATH = os.environ.get("DYCON_LIB"'), hits
    bools = {f.name for f in dataclasses.fields(TrainConfig) if isinstance(f.default, bool)}
    assert bools == {"poly_lr", "strict_nan_check", "global_batch_losses", "overlap_teacher", "overlap_wgrad", "overlap_features",
                     "use_aspp", "ddp_force", "replay"}, bools


def test_conv_dispatch_is_decided_in_one_place():
    """The forward convolution's kernel choice lives in conv_fwd_plan (csrc/conv.hip) alone: the 24^3 threshold is one named constant
    there and appears in no Python file of the package, the statistics buffer is an argument and not thread-local state, and ops no
    longer restates the LDS-halo predicate."""
    from dycon_paper_replication_amd import ops
    pkg = os.path.join(ROOT, "dycon_paper_replication_amd")
    hits = []
    for d, _, files in os.walk(pkg):
        hits += [os.path.join(d, f) for f in files if f.endswith(".py") and "13824" in open(os.path.join(d, f)).read()]
    assert not hits, hits
    conv = open(os.path.join(pkg, "csrc", "conv.hip")).read()
    assert conv.count("13824") == 1
    assert "thread_local" not in conv
    assert not hasattr(ops, "conv_uses_lds")
